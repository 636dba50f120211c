"""The elastic deformation of the patch crop on the device (medicalseg_amd/csrc/msk_elastic.hip, msk_affine_patch_elastic,
preprocess.elastic_field_device, transforms.RandomElasticAffinePatchCrop3D) against the numpy statement of
tests/elastic_reference.py.  Fields, images and labels are compared with np.array_equal; the only tolerance is the training
loss being finite.  Every buffer is red-zoned (tests/helpers.py): a store outside it fails by name, a load outside it pulls in
a NaN."""
import ctypes as C
import functools
import os
import random
import re

import numpy as np
import pytest

import affine_reference as A
import elastic_reference as E
import patch_reference as P
from helpers import SENTINEL_BITS, dev, dfree, dmalloc, redzone_check, vec  # noqa: F401  (redzone_check: autouse here)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = C.c_void_p
PAD, LABEL_PAD = np.float32(-3.5), 255
SEED = 0xC0FFEE1234567891
# (roi, sigma): two ordinary patches; every operand of every line is padding; r = 2; a row past one workgroup's segment with an
# odd tail; lines longer than 2r+1 along each axis, several segments along W
FIELDS = [((12, 16, 20), 9.0), ((8, 8, 64), 13.0), ((4, 4, 4), 16.0), ((4, 5, 7), 0.5), ((2, 8, 300), 9.0),
          ((140, 3, 5), 16.0), ((3, 140, 5), 16.0), ((2, 3, 1100), 16.0)]
AXES = [(0, 1, 2), (1, 2), (0,)]
ALPHA = 900.0


def _mask(axes):
    return sum(1 << a for a in axes)


@functools.lru_cache(maxsize=None)
def _want_field(k, axes, alpha=ALPHA, seed=SEED):
    roi, sigma = FIELDS[k]
    f = E.field(roi, seed + k, sigma, alpha, axes)
    f.setflags(write=False)
    return f


def _up(a, offset=0):
    """4-byte elements -> (pointer to the first element, pointer to free); offset 4: one SENTINEL word in front, so the data
    are only 4-byte aligned"""
    a = np.ascontiguousarray(a).reshape(-1)
    assert a.dtype.itemsize == 4
    host = np.empty(a.size + offset // 4, np.uint32)
    host[:offset // 4] = SENTINEL_BITS
    host[offset // 4:] = a.view(np.uint32)
    p = vec(host.view(np.float32))
    return p + offset, p


def _out(words, offset=0):
    """an output of `words` 4-byte elements -> (pointer to the first element, pointer to free)"""
    p = dmalloc(4 * words + offset)
    return p + offset, p


def _record(origin):
    return vec(np.array(list(origin) + [-1, -1, -1, -1, 0], np.int32).view(np.float32))


def _field_call(roi, sigma, alpha, seed, axes, field, scratch):
    w = E.taps(sigma)
    dev().call("msk_elastic_field", C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), *roi, w.ctypes.data_as(V), (len(w) - 1) // 2,
               C.c_float(alpha), _mask(axes), V(field), V(scratch))


def _same_bits(got, want):
    return np.array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32))


# ---- msk_elastic_field -------------------------------------------------------------------------------------------------------
def test_cases_cover_what_they_are_there_for():
    r = [int(4 * s + 0.5) for _, s in FIELDS]
    assert min(r) == 2 and max(r) == 64
    assert any(all(e <= rr for e in roi) for (roi, _), rr in zip(FIELDS, r))          # every operand but one's own is padding
    for axis in range(3):
        assert any(roi[axis] > 2 * rr + 1 for (roi, _), rr in zip(FIELDS, r))        # a line with interior outputs
    assert any(roi[2] > 256 and roi[2] % 8 for roi, _ in FIELDS)                      # several W segments, an odd tail
    assert any(roi[2] > 1024 for roi, _ in FIELDS)
    assert any(roi[0] % 8 and roi[1] % 8 for roi, _ in FIELDS)                        # column segments that end early


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("axes", AXES, ids=["dhw", "hw", "d"])
@pytest.mark.parametrize("k", range(len(FIELDS)))
def test_field_equals_the_statement(k, axes, offset):
    roi, sigma = FIELDS[k]
    want = _want_field(k, axes)
    n3 = 3 * int(np.prod(roi))
    d = dev()
    field, field_base = _out(n3, offset)
    scratch, scratch_base = _out(n3, offset)
    _field_call(roi, sigma, ALPHA, SEED + k, axes, field, scratch)
    got = d.d2h(field, (3,) + roi, np.float32)
    assert _same_bits(got, want), (int((got.view(np.uint32) != want.view(np.uint32)).sum()), float(np.nanmax(np.abs(got - want))))
    for a in range(3):
        if a not in axes:
            assert not got[a].view(np.uint32).any()                                  # +0.0
    if offset:
        assert d.d2h(field_base, (1,), np.uint32)[0] == SENTINEL_BITS and d.d2h(scratch_base, (1,), np.uint32)[0] == SENTINEL_BITS
    dfree(field_base)
    dfree(scratch_base)


def test_two_calls_equal_bits_and_two_seeds_differ():
    roi, sigma = FIELDS[0]
    n3 = 3 * int(np.prod(roi))
    d = dev()
    bufs = [dmalloc(4 * n3) for _ in range(4)]
    _field_call(roi, sigma, ALPHA, SEED, (0, 1, 2), bufs[0], bufs[1])
    first = d.d2h(bufs[0], (3,) + roi, np.float32)
    _field_call(roi, sigma, ALPHA, SEED, (0, 1, 2), bufs[0], bufs[1])                # over its own result and a used scratch
    _field_call(roi, sigma, ALPHA, SEED, (0, 1, 2), bufs[2], bufs[3])
    assert _same_bits(d.d2h(bufs[0], (3,) + roi, np.float32), first) and _same_bits(d.d2h(bufs[2], (3,) + roi, np.float32), first)
    _field_call(roi, sigma, ALPHA, SEED + 1, (0, 1, 2), bufs[2], bufs[3])
    other = d.d2h(bufs[2], (3,) + roi, np.float32)
    assert np.isfinite(other).all() and (other != first).mean() > 0.99
    assert _same_bits(other, E.field(roi, SEED + 1, sigma, ALPHA))
    for p in bufs:
        dfree(p)


# ---- msk_affine_patch_elastic ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(k):
    """affine_reference.GPU_CASES[k] sampled through a field of elastic_reference.FIELD_CASES[k] / ALPHAS[k], computed once"""
    shape, roi, origin, angles, scale = A.GPU_CASES[k]
    assert E.FIELD_CASES[k][0] == roi
    img, label = A.image_for(shape, 100 + k), A.label_for(shape, 200 + k)
    m = A.matrix(angles, scale)
    f = E.field(roi, SEED + k, E.FIELD_CASES[k][1], E.ALPHAS[k])
    want_i, want_l = E.elastic(img, label, roi, origin, m, f, PAD, LABEL_PAD)
    for a in (img, label, m, f, want_i, want_l):
        a.setflags(write=False)
    return shape, roi, origin, img, label, m, f, want_i, want_l


def _elastic(img, label, shape, sel, m, field, out_i, out_l, roi, name="msk_affine_patch_elastic"):
    m = np.ascontiguousarray(np.asarray(m, np.float32).reshape(9))
    extra = (V(field),) if name == "msk_affine_patch_elastic" else ()
    dev().call(name, V(img), V(label) if label else None, *shape, V(sel), m.ctypes.data_as(V), *extra, V(out_i),
               V(out_l) if out_l else None, *roi, C.c_float(float(PAD)), LABEL_PAD)


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("with_label", [True, False], ids=["label", "image only"])
@pytest.mark.parametrize("k", range(len(A.GPU_CASES)))
def test_sampling_equals_the_statement(k, with_label, offset):
    shape, roi, origin, img, label, m, f, want_i, want_l = _case(k)
    d = dev()
    n = int(np.prod(roi))
    assert np.abs(f).max() > (1.0 if k in (0, 2) else 0.0)                            # the sampling moves, twice by voxels
    ip, ip_base = _up(img, offset)
    fp, fp_base = _up(f, offset)
    lp = _up(label)[0] if with_label else None
    sel = _record(origin)
    try:
        for amap in (1, 0):                                                         # both thread -> voxel maps
            d.set_option("affine_map", amap)
            out_i, out_i_base = _out(n, offset)
            out_l = dmalloc(4 * n) if with_label else None
            _elastic(ip, lp, shape, sel, m, fp, out_i, out_l, roi)
            got_i = d.d2h(out_i, roi, np.float32)
            assert _same_bits(got_i, want_i), (amap, int((got_i.view(np.uint32) != want_i.view(np.uint32)).sum()))
            if with_label:
                assert np.array_equal(d.d2h(out_l, roi, np.int32), want_l), amap
                dfree(out_l)
            dfree(out_i_base)
    finally:
        d.set_option("affine_map", 1)
    assert np.array_equal(d.d2h(ip, shape, np.float32), img) and _same_bits(d.d2h(fp, (3,) + roi, np.float32), f)
    for p in (ip_base, fp_base, sel) + ((lp,) if with_label else ()):
        dfree(p)


@pytest.mark.parametrize("k", [0, 5])
def test_zero_field_gives_the_affine_patch(k):
    shape, roi, origin, img, label, m, f, want_i, want_l = _case(k)
    d = dev()
    n = int(np.prod(roi))
    ip, lp, sel = _up(img)[0], _up(label)[0], _record(origin)
    zero = _up(np.zeros(3 * n, np.float32))[0]
    outs = [dmalloc(4 * n) for _ in range(4)]
    _elastic(ip, lp, shape, sel, m, None, outs[0], outs[1], roi, name="msk_affine_patch")
    _elastic(ip, lp, shape, sel, m, zero, outs[2], outs[3], roi)
    plain_i, plain_l = A.affine(img, label, roi, origin, m, PAD, LABEL_PAD)
    assert _same_bits(d.d2h(outs[0], roi, np.float32), plain_i) and np.array_equal(d.d2h(outs[1], roi, np.int32), plain_l)
    assert _same_bits(d.d2h(outs[2], roi, np.float32), plain_i) and np.array_equal(d.d2h(outs[3], roi, np.int32), plain_l)
    for p in [ip, lp, sel, zero] + outs:
        dfree(p)


# ---- the preprocess wrappers, the transform, training ------------------------------------------------------------------------
def _counting(monkeypatch):
    from medicalseg_amd.device import Device
    calls = []
    real = Device.call

    def counting(self, name, *args):
        calls.append(name)
        return real(self, name, *args)
    monkeypatch.setattr(Device, "call", counting)
    return calls


def _pool_balance(monkeypatch):
    from medicalseg_amd import preprocess as pp
    balance = [0]
    alloc, release = pp._pool_alloc, pp._pool_release
    monkeypatch.setattr(pp, "_pool_alloc", lambda dev_, nbytes: (balance.__setitem__(0, balance[0] + 1), alloc(dev_, nbytes))[1])
    monkeypatch.setattr(pp, "_pool_release", lambda dev_, ptr, nbytes: (balance.__setitem__(0, balance[0] - 1), release(dev_, ptr, nbytes))[1])
    return balance


def test_preprocess_wrappers_download_nothing(monkeypatch):
    import inspect

    from medicalseg_amd import preprocess as pp
    from medicalseg_amd._lib import MskError
    for fn in (pp.elastic_field_device, pp.affine_patch_device):
        assert not re.search(r"d2h|\.numpy\(|\.sync\(", inspect.getsource(fn))
    shape, roi, origin, img, label, m, f, want_i, want_l = _case(0)
    sigma, alpha = E.FIELD_CASES[0][1], E.ALPHAS[0]
    iv, lv = pp.upload_pooled(img), pp.upload_pooled(label)
    sel = pp._pooled_volume(iv.dev, (1, 8), np.int32)
    iv.dev.h2d(sel.ptr, np.array([list(origin) + [-1, -1, -1, -1, 0]], np.int32))
    balance = _pool_balance(monkeypatch)
    calls = _counting(monkeypatch)
    field = pp.elastic_field_device(iv.dev, roi, sigma, alpha, SEED)
    out_i, out_l = pp.affine_patch_device(iv, lv, sel, roi, m, PAD, LABEL_PAD, field=field)
    only = pp.affine_patch_device(iv, None, sel, roi, m, PAD, field=field)
    assert [c for c in calls if c != "msk_malloc"] == ["msk_elastic_field", "msk_affine_patch_elastic", "msk_affine_patch_elastic"], calls
    del calls[:]
    assert balance[0] == 4                                                          # the scratch went back, the results are out
    assert field.pooled and field.shape == (3,) + roi and field.dtype == np.float32
    assert _same_bits(field.numpy(), f)
    assert _same_bits(out_i.numpy(), want_i) and np.array_equal(out_l.numpy(), want_l) and _same_bits(only.numpy(), want_i)
    part = pp.elastic_field_device(iv.dev, roi, sigma, alpha, SEED, axes=(1, 2))
    assert _same_bits(part.numpy(), E.field(roi, SEED, sigma, alpha, (1, 2)))
    for v in (out_i, out_l, only, part):
        v.free()
    assert balance[0] == 1
    # a refused call hands its buffers back to the pool
    with pytest.raises(MskError, match="msk_elastic_field"):
        pp.elastic_field_device(iv.dev, roi, sigma, 5000.0, SEED)
    with pytest.raises(MskError, match="msk_affine_patch_elastic"):
        pp.affine_patch_device(iv, lv, sel, roi, m * np.float32(100.0), PAD, LABEL_PAD, field=field)
    for bad in (dict(sigma=0.4), dict(sigma=16.5), dict(axes=(0, 3)), dict(axes=(1, 1))):
        with pytest.raises(ValueError):
            pp.elastic_field_device(iv.dev, roi, **{**dict(sigma=sigma, alpha=alpha, seed=1), **bad})
    with pytest.raises(TypeError):
        pp.affine_patch_device(iv, lv, sel, roi, m, field=lv)
    with pytest.raises(TypeError):
        pp.affine_patch_device(iv, lv, sel, (4, 4, 4), m, field=field)
    assert balance[0] == 1
    for v in (field, sel, iv, lv):
        v.free()


def _draws(seed):
    """(rotate coin, scale coin, elastic coin) of the class's first call under this seed"""
    random.seed(seed)
    random.random()
    [random.getrandbits(32) for _ in range(5)]
    u = [random.random() for _ in range(9)]
    return u[0], u[4], random.random()


@pytest.mark.parametrize("shape,roi", [((9, 70, 67), (12, 16, 20)), ((20, 33, 130), (8, 8, 64))])
def test_transform_device_path_equals_host_path(shape, roi, monkeypatch):
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    label = P.blobs(shape, 3, 21)
    img = np.abs(A.image_for(shape, 22)) + np.float32(0.5)
    op = T.RandomElasticAffinePatchCrop3D(roi, 3, fg_prob=0.5, pad_value=-3.5, label_pad=255, rotate_prob=0.5, scale_prob=0.5,
                                          elastic_prob=0.5, elastic_alpha=(300.0, 900.0))
    parent = T.RandomAffinePatchCrop3D(roi, 3, fg_prob=0.5, pad_value=-3.5, label_pad=255, rotate_prob=0.5, scale_prob=0.5)
    seeds = {"elastic and matrix": next(s for s in range(400) if _draws(s)[2] < 0.5 and min(_draws(s)[:2]) < 0.5),
             "elastic alone": next(s for s in range(400) if _draws(s)[2] < 0.5 and min(_draws(s)[:2]) >= 0.5),
             "matrix alone": next(s for s in range(400) if _draws(s)[2] >= 0.5 and min(_draws(s)[:2]) < 0.5),
             "neither": next(s for s in range(400) if min(_draws(s)) >= 0.5)}
    balance = _pool_balance(monkeypatch)
    calls = _counting(monkeypatch)
    new = {"msk_elastic_field", "msk_affine_patch_elastic"}
    for what, seed in seeds.items():
        hit = what.startswith("elastic")
        random.seed(seed)
        h_img, h_lab = op(img, label)
        state = random.getstate()
        random.seed(seed)
        p_img, p_lab = parent(img, label)
        assert (np.array_equal(h_img, p_img) and np.array_equal(h_lab, p_lab)) != hit, what   # the coin did what the seed was chosen for
        d_in, l_in = pp.upload_pooled(img), pp.upload_pooled(label)
        del calls[:]
        random.seed(seed)
        d_img, d_lab = op(d_in, l_in)
        ran = list(calls)
        assert random.getstate() == state
        # back to back, nothing downloaded, nothing synchronised; without an elastic hit neither new kernel is launched
        want = {"elastic and matrix": ["msk_patch_select", "msk_elastic_field", "msk_affine_patch_elastic"],
                "elastic alone": ["msk_patch_select", "msk_elastic_field", "msk_affine_patch_elastic"],
                "matrix alone": ["msk_patch_select", "msk_affine_patch"],
                "neither": ["msk_patch_select", "msk_patch_crop", "msk_patch_crop"]}[what]
        assert [c for c in ran if c.startswith("msk_patch") or c.startswith("msk_affine") or c in new] == want, (what, ran)
        assert not any(c in ("msk_sync", "msk_d2h") for c in ran), (what, ran)
        assert d_img.shape == roi and d_lab.shape == roi and d_img.dtype == np.float32 and d_lab.dtype == np.int32
        assert _same_bits(d_img.numpy(), np.asarray(h_img, np.float32)), what
        assert np.array_equal(d_lab.numpy(), h_lab), what
        d_img.free()
        d_lab.free()
        assert balance[0] == 0, what
        # without a label
        random.seed(seed)
        h_only, none = op(img, None)
        random.seed(seed)
        d_only, none_d = op(pp.upload_pooled(img), None)
        assert none is None and none_d is None and _same_bits(d_only.numpy(), np.asarray(h_only, np.float32))
        d_only.free()
        assert balance[0] == 0, what


def test_elastic_patch_training_end_to_end(tmp_path, capsys):
    """configs/synthetic/vnet_synthetic_ct_patch_elastic_96.yml shrunk to a 32^3 patch of 40 x 44 x 52 volumes and two
    iterations, with every coin certain so that both kernels are in the loop"""
    from medicalseg_amd.core import train
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd import transforms as T
    src = open(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_elastic_96.yml")).read()
    for old, new in (("'../_base_/global_configs.yml'", "'%s'" % os.path.join(ROOT, "configs", "_base_", "global_configs.yml")),
                     ("iters: 100", "iters: 2"), ("num_samples: 16", "num_samples: 4"), ("size: [96, 96, 96]", "size: [32, 32, 32]"),
                     ("rotate_prob: 0.2", "rotate_prob: 1.0"), ("scale_prob: 0.2", "scale_prob: 1.0"),
                     ("elastic_prob: 0.2", "elastic_prob: 1.0")):
        assert old in src, old
        src = src.replace(old, new)
    assert src.count("shape: [144, 128, 160]") == 2
    src = src.replace("shape: [144, 128, 160]", "shape: [40, 44, 52]")
    p = tmp_path / "elastic_32.yml"
    p.write_text(src)
    cfg = Config(str(p))
    ds = cfg.train_dataset
    assert type(ds.transforms.transforms[0]) is T.RandomElasticAffinePatchCrop3D and ds.transforms.device
    random.seed(0)
    train(cfg.model, ds, optimizer=cfg.optimizer, save_dir=str(tmp_path / "o"), iters=cfg.iters, batch_size=cfg.batch_size,
          save_interval=10, log_iters=1, losses=cfg.loss)
    logged = [float(v) for v in re.findall(r"\[TRAIN\].*? loss: ([^,]+),", capsys.readouterr().out)]
    assert len(logged) == 2 and np.isfinite(logged).all() and all(v > 0 for v in logged), logged


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def _refused(name, bad, outputs):
    """every argument tuple of `bad` returns an error, raises through Device.call and enqueues nothing"""
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import MskError
    d = dev()
    d.set_option("prof_only_halo", 0)
    d.prof_reset()
    d.prof_enable(True)
    try:
        for keep, args in bad:
            rc = getattr(d.lib, name)(d.ctx, *args)
            assert rc != 0, args
            assert _lib.last_error(d.ctx)
            with pytest.raises(MskError, match=name):
                d.call(name, *args)
        d.sync()
        assert d.prof_report() == {}                                                 # the launch counter: nothing was enqueued
        for p, words in outputs:                                                     # ... and the outputs hold the sentinel
            assert (d.d2h(p, (words,), np.uint32) == SENTINEL_BITS).all()
    finally:
        d.prof_enable(False)
        d.prof_reset()


def test_field_argument_errors_launch_nothing():
    d = dev()
    roi, sigma = (4, 5, 7), 9.0
    n3 = 3 * 4 * 5 * 7
    w = E.taps(sigma)
    r = (len(w) - 1) // 2
    field, scratch, big = dmalloc(4 * n3), dmalloc(4 * n3), dmalloc(8 * n3)
    wide = np.zeros(2 * 65 + 1, np.float32)

    def a(seed=1, rd=4, rh=5, rw=7, taps=w, r_=r, alpha=100.0, mask=7, field=field, scratch=scratch):
        return (taps, (C.c_uint64(seed), rd, rh, rw, taps.ctypes.data_as(V) if taps is not None else None, r_, C.c_float(alpha), mask,
                       V(field) if field else None, V(scratch) if scratch else None))
    bad = [a(taps=None), a(field=None), a(scratch=None),                                                  # null pointers
           a(r_=1), a(r_=0), a(r_=-3), a(r_=65, taps=wide),                                               # r outside [2, 64]
           a(alpha=-1.0), a(alpha=4096.5), a(alpha=float("nan")), a(alpha=float("inf")),                  # alpha
           a(mask=-1), a(mask=8),
           a(rd=0), a(rh=-2), a(rw=0), a(rd=8193), a(rh=8193), a(rw=8193),                                # extents
           a(rd=1024, rh=1024, rw=683),                                                                   # 3 N >= 2^31
           a(field=field + 2), a(scratch=scratch + 1),                                                    # not 4-byte aligned
           a(scratch=field), a(field=big, scratch=big + 4 * n3 - 4), a(field=big + 4, scratch=big)]       # overlapping
    _refused("msk_elastic_field", bad, ((field, n3), (scratch, n3), (big, 2 * n3)))
    # ... and the same call with valid arguments runs; alpha = 4096 and r = 64 are allowed
    d.prof_reset()
    d.prof_enable(True)
    try:
        d.call("msk_elastic_field", *a()[1])
        d.sync()
        report = d.prof_report()
        assert list(report) == ["elastic_field"] and report["elastic_field"][0] == 1, report
    finally:
        d.prof_enable(False)
        d.prof_reset()
    assert _same_bits(d.d2h(field, (3,) + roi, np.float32), E.field(roi, 1, sigma, 100.0))
    w16 = E.taps(16.0)
    d.call("msk_elastic_field", *a(taps=w16, r_=64, alpha=4096.0)[1])
    assert _same_bits(d.d2h(field, (3,) + roi, np.float32), E.field(roi, 1, 16.0, 4096.0))
    for p in (field, scratch, big):
        dfree(p)


def test_sampling_argument_errors_launch_nothing():
    d = dev()
    shape, roi = (5, 7, 9), (4, 4, 4)
    n, nv = 64, 5 * 7 * 9
    img, label = A.image_for(shape, 1), A.label_for(shape, 2)
    f = E.field(roi, 3, 0.5, 2.0)
    ip, lp, fp, sel = _up(img)[0], _up(label)[0], _up(f)[0], _record((0, 1, 2))
    out_i, out_l = dmalloc(4 * n), dmalloc(4 * n)
    eye = np.eye(3, dtype=np.float32)

    def a(img=ip, label=lp, d_=5, h=7, w=9, sel=sel, m=eye, field=fp, out_i=out_i, out_l=out_l, rd=4, rh=4, rw=4):
        keep = np.ascontiguousarray(np.asarray(m, np.float32).reshape(9)) if m is not None else None
        return (keep, (V(img) if img else None, V(label) if label else None, d_, h, w, V(sel) if sel else None,
                       keep.ctypes.data_as(V) if keep is not None else None, V(field) if field else None,
                       V(out_i) if out_i else None, V(out_l) if out_l else None, rd, rh, rw, C.c_float(-3.5), 255))
    bad = [a(img=None), a(sel=None), a(m=None), a(out_i=None), a(field=None),                             # null pointers
           a(label=None), a(out_l=None),                                                                  # only one of the pair
           a(img=ip + 2), a(field=fp + 2), a(out_i=out_i + 2), a(out_l=out_l + 3),                        # not 4-byte aligned
           a(d_=0), a(rd=0), a(rw=8193), a(w=8193), a(rd=2048, rh=1024, rw=1024),                         # extents, 2^31 voxels
           a(rd=1024, rh=1024, rw=683),                                                                   # 3 N >= 2^31
           a(m=eye * np.float32(4.5)), a(m=eye * np.float32(np.nan)),                                     # the matrix
           a(out_i=ip), a(out_l=lp), a(out_l=out_i),                                                      # msk_affine_patch's overlaps
           a(out_i=fp), a(out_i=fp + 4 * (3 * n - 1)), a(out_l=fp + 4 * n), a(out_l=fp + 8 * n + 16)]     # outputs over the field
    _refused("msk_affine_patch_elastic", bad, ((out_i, n), (out_l, n)))
    d.call("msk_affine_patch_elastic", *a()[1])
    want_i, want_l = E.elastic(img, label, roi, (0, 1, 2), eye, f, PAD, LABEL_PAD)
    assert _same_bits(d.d2h(out_i, roi, np.float32), want_i) and np.array_equal(d.d2h(out_l, roi, np.int32), want_l)
    assert _same_bits(d.d2h(fp, (3,) + roi, np.float32), f) and np.array_equal(d.d2h(ip, shape, np.float32), img)
    for p in (ip, lp, fp, sel, out_i, out_l):
        dfree(p)

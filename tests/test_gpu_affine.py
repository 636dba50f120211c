"""The rotated and scaled patch crop on the device (medicalseg_amd/csrc/msk_affine.hip, preprocess.affine_patch_device,
transforms.RandomAffinePatchCrop3D) against the numpy statement of tests/affine_reference.py.  Image and label are compared
with np.array_equal; the only tolerance is the training loss being finite.  Every buffer is red-zoned (tests/helpers.py): a
store outside it fails by name, a load outside it pulls in a NaN."""
import ctypes as C
import functools
import os
import random
import re

import numpy as np
import pytest

import affine_reference as R
import patch_reference as P
from helpers import SENTINEL_BITS, dev, dfree, dmalloc, redzone_check, vec  # noqa: F401  (redzone_check: autouse here)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = C.c_void_p
PAD, LABEL_PAD = np.float32(-3.5), 255


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


def _record(origin):
    return vec(np.array(list(origin) + [-1, -1, -1, -1, 0], np.int32).view(np.float32))


def _mat(m):
    m = np.ascontiguousarray(np.asarray(m, np.float32).reshape(9))
    return m, m.ctypes.data_as(V)


def _affine(img, label, shape, sel, m, out_i, out_l, roi, pad=PAD, label_pad=LABEL_PAD):
    keep, mp = _mat(m)
    dev().call("msk_affine_patch", V(img), V(label) if label else None, *shape, V(sel), mp, V(out_i), V(out_l) if out_l else None,
               *roi, C.c_float(float(pad)), int(label_pad))


@functools.lru_cache(maxsize=None)
def _case(k):
    """the statement of one case, computed once and shared"""
    shape, roi, origin, angles, scale = R.GPU_CASES[k]
    img, label = R.image_for(shape, 100 + k), R.label_for(shape, 200 + k)
    m = R.matrix(angles, scale)
    want_i, want_l = R.affine(img, label, roi, origin, m, PAD, LABEL_PAD)
    for a in (img, label, m, want_i, want_l):
        a.setflags(write=False)
    return shape, roi, origin, img, label, m, want_i, want_l


# ---- msk_affine_patch --------------------------------------------------------------------------------------------------------
def test_cases_cover_what_they_are_there_for():
    rws = [c[1][2] for c in R.GPU_CASES]
    assert any(rw % 2 for rw in rws)                                          # an odd row length: the row-linear map's div / mod
    assert any(rw % 16 for rw in rws)                                         # rows that end inside a box of the tile map
    assert any(rw % 4 == 0 for rw in rws) and any(rw >= 256 for rw in rws)    # a row as wide as one workgroup
    assert any(min(c[2]) < 0 for c in R.GPU_CASES)                            # a negative origin
    assert any(any(r % t for r, t in zip(c[1], (4, 4, 16))) for c in R.GPU_CASES)


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("with_label", [True, False], ids=["label", "image only"])
@pytest.mark.parametrize("k", range(len(R.GPU_CASES)))
def test_kernel_equals_the_statement(k, with_label, offset):
    shape, roi, origin, img, label, m, want_i, want_l = _case(k)
    d = dev()
    n = int(np.prod(roi))
    ip, ip_base = _up(img, offset)
    lp = _up(label)[0] if with_label else None
    sel = _record(origin)
    try:
        for amap in (1, 0):                                                         # both thread -> voxel maps
            d.set_option("affine_map", amap)
            out_i = dmalloc(4 * n)
            out_l = dmalloc(4 * n) if with_label else None
            _affine(ip, lp, shape, sel, m, out_i, out_l, roi)
            got_i = d.d2h(out_i, roi, np.float32)
            assert np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32)), \
                (amap, int((got_i.view(np.uint32) != want_i.view(np.uint32)).sum()), float(np.nanmax(np.abs(got_i - want_i))))
            if with_label:
                assert np.array_equal(d.d2h(out_l, roi, np.int32), want_l), amap
                dfree(out_l)
            dfree(out_i)
    finally:
        d.set_option("affine_map", 1)
    assert np.array_equal(d.d2h(ip, shape, np.float32), img)
    if with_label:
        assert np.array_equal(d.d2h(lp, shape, np.int32), label)
        dfree(lp)
    dfree(ip_base)
    dfree(sel)


@pytest.mark.parametrize("shape,roi,origin", [((9, 70, 67), (12, 16, 20), (-1, 20, 11)), ((5, 6, 7), (8, 8, 8), (-1, -1, 0)),
                                              ((20, 33, 130), (8, 8, 64), (12, 25, 66)), ((6, 10, 21), (4, 5, 7), (2, 5, 14))])
def test_identity_equals_patch_crop(shape, roi, origin):
    d = dev()
    n = int(np.prod(roi))
    img, label = R.image_for(shape, 7), R.label_for(shape, 8)
    assert not (np.signbit(img) & (img == 0)).any()
    ip, lp, sel = _up(img)[0], _up(label)[0], _record(origin)
    crop_i, crop_l, out_i, out_l = (dmalloc(4 * n) for _ in range(4))
    pad_bits = int(np.array([PAD], np.float32).view(np.uint32)[0])
    d.call("msk_patch_crop", V(ip), *shape, V(sel), V(crop_i), *roi, C.c_uint32(pad_bits))
    d.call("msk_patch_crop", V(lp), *shape, V(sel), V(crop_l), *roi, C.c_uint32(LABEL_PAD))
    _affine(ip, lp, shape, sel, np.eye(3), out_i, out_l, roi)
    want_i, want_l = d.d2h(crop_i, roi, np.uint32), d.d2h(crop_l, roi, np.int32)
    assert np.array_equal(want_i.view(np.float32), P.crop(img, origin, roi, PAD))
    assert np.array_equal(d.d2h(out_i, roi, np.uint32), want_i) and np.array_equal(d.d2h(out_l, roi, np.int32), want_l)
    for p in (ip, lp, sel, crop_i, crop_l, out_i, out_l):
        dfree(p)


def test_record_is_read_on_the_device(monkeypatch):
    """select and the affine crop enqueued back to back: the origin never visits the host, and no synchronising entry point
    is called in between"""
    from medicalseg_amd.device import Device
    shape, roi = (9, 70, 67), (12, 16, 20)
    d = dev()
    n = int(np.prod(roi))
    img, label = R.image_for(shape, 31), P.blobs(shape, 3, 32)
    words = np.ascontiguousarray(np.array([1] + [int(w) for w in P.mixed_words(1, 33)[0, 1:]], np.uint32))
    rec = P.select(label, roi, 3, [1, 2], words)
    assert rec[3] in (1, 2)                                                         # a foreground patch: the label is searched
    m = R.matrix((17, -23, 29), 1.1)
    want_i, want_l = R.affine(img, label, roi, rec[:3], m, PAD, LABEL_PAD)
    nbytes = C.c_size_t(0)
    assert d.lib.msk_patch_workspace(C.c_long(int(np.prod(shape))), 3, C.byref(nbytes)) == 0
    ip, lp, ws, sel = _up(img)[0], _up(label)[0], dmalloc(nbytes.value), dmalloc(32)
    out_i, out_l = dmalloc(4 * n), dmalloc(4 * n)
    classes = np.array([1, 2], np.int32)
    calls = []
    real = Device.call

    def counting(self, name, *args):
        calls.append(name)
        return real(self, name, *args)
    monkeypatch.setattr(Device, "call", counting)
    d.call("msk_patch_select", V(lp), *shape, 3, classes.ctypes.data_as(V), 2, *roi, words.ctypes.data_as(V), 1, V(ws), V(sel), None)
    _affine(ip, lp, shape, sel, m, out_i, out_l, roi)
    monkeypatch.setattr(Device, "call", real)
    assert calls == ["msk_patch_select", "msk_affine_patch"]
    assert sum(c in ("msk_sync", "msk_d2h") for c in calls) == 0
    assert np.array_equal(d.d2h(sel, (8,), np.int32), np.array(rec, np.int32))
    assert np.array_equal(d.d2h(out_i, roi, np.float32).view(np.uint32), want_i.view(np.uint32))
    assert np.array_equal(d.d2h(out_l, roi, np.int32), want_l)
    for p in (ip, lp, ws, sel, out_i, out_l):
        dfree(p)


# ---- the preprocess wrapper, the transform, training -------------------------------------------------------------------------
def test_preprocess_wrapper_downloads_nothing(monkeypatch):
    import inspect

    from medicalseg_amd import preprocess as pp
    from medicalseg_amd._lib import MskError
    assert not re.search(r"d2h|\.numpy\(|\.sync\(", inspect.getsource(pp.affine_patch_device))
    shape, roi, origin, img, label, m, want_i, want_l = _case(0)
    iv, lv = pp.upload_pooled(img), pp.upload_pooled(label)
    sel = pp._pooled_volume(iv.dev, (2, 8), np.int32)
    iv.dev.h2d(sel.ptr, np.array([[0] * 8, list(origin) + [-1, -1, -1, -1, 0]], np.int32))
    out_i, out_l = pp.affine_patch_device(iv, lv, sel, roi, m, PAD, LABEL_PAD, index=1)
    assert out_i.pooled and out_l.pooled and out_i.dtype == np.float32 and out_l.dtype == np.int32
    assert np.array_equal(out_i.numpy().view(np.uint32), want_i.view(np.uint32)) and np.array_equal(out_l.numpy(), want_l)
    only = pp.affine_patch_device(iv, None, sel, roi, m.reshape(3, 3), PAD, index=1)
    assert isinstance(only, pp.DeviceVolume) and np.array_equal(only.numpy().view(np.uint32), want_i.view(np.uint32))
    for v in (out_i, out_l, only):
        v.free()
    # a refused call hands both outputs back to the pool
    balance = [0]
    alloc, release = pp._pool_alloc, pp._pool_release
    monkeypatch.setattr(pp, "_pool_alloc", lambda dev_, nbytes: (balance.__setitem__(0, balance[0] + 1), alloc(dev_, nbytes))[1])
    monkeypatch.setattr(pp, "_pool_release", lambda dev_, ptr, nbytes: (balance.__setitem__(0, balance[0] - 1), release(dev_, ptr, nbytes))[1])
    with pytest.raises(MskError, match="msk_affine_patch"):
        pp.affine_patch_device(iv, lv, sel, roi, m * np.float32(100.0), PAD, LABEL_PAD)
    assert balance[0] == 0
    with pytest.raises(ValueError):
        pp.affine_patch_device(iv, lv, sel, roi, m, index=2)
    with pytest.raises(TypeError):
        pp.affine_patch_device(lv, None, sel, roi, m)
    assert balance[0] == 0
    for v in (sel, iv, lv):
        v.free()


def _coins(seed):
    """(rotate coin, scale coin) of the class's first call under this seed: the parent's six draws, then nine"""
    random.seed(seed)
    random.random()
    [random.getrandbits(32) for _ in range(5)]
    u = [random.random() for _ in range(9)]
    return u[0], u[4]


@pytest.mark.parametrize("shape,roi", [((9, 70, 67), (12, 16, 20)), ((20, 33, 130), (8, 8, 64))])
def test_transform_device_path_equals_host_path(shape, roi, monkeypatch):
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    label = P.blobs(shape, 3, 21)
    img = np.abs(R.image_for(shape, 22)) + np.float32(0.5)
    op = T.RandomAffinePatchCrop3D(roi, 3, fg_prob=0.5, pad_value=-3.5, label_pad=255, rotate_prob=0.5, scale_prob=0.5)
    both = next(s for s in range(200) if max(_coins(s)) < 0.5)
    neither = next(s for s in range(200) if min(_coins(s)) >= 0.5)
    balance = [0]
    alloc, release = pp._pool_alloc, pp._pool_release

    def counted_alloc(dev_, nbytes):
        balance[0] += 1
        return alloc(dev_, nbytes)

    def counted_release(dev_, ptr, nbytes):
        balance[0] -= 1
        return release(dev_, ptr, nbytes)
    monkeypatch.setattr(pp, "_pool_alloc", counted_alloc)
    monkeypatch.setattr(pp, "_pool_release", counted_release)
    for seed, hit in ((both, True), (neither, False)):
        random.seed(seed)
        h_img, h_lab = op(img, label)
        state = random.getstate()
        plain = P.crop(img, op.select(shape, label, _words(seed, 0.5))[:3], roi, np.float32(-3.5))
        assert np.array_equal(h_img, plain) != hit                                  # the coins did what the seed was chosen for
        random.seed(seed)
        d_img, d_lab = op(pp.upload_pooled(img), pp.upload_pooled(label))
        assert random.getstate() == state
        assert d_img.shape == roi and d_lab.shape == roi and d_img.dtype == np.float32 and d_lab.dtype == np.int32
        assert np.array_equal(d_img.numpy().view(np.uint32), np.asarray(h_img, np.float32).view(np.uint32)), (seed, hit)
        assert np.array_equal(d_lab.numpy(), h_lab), (seed, hit)
        d_img.free()
        d_lab.free()
        assert balance[0] == 0, (seed, hit)
        # without a label
        random.seed(seed)
        h_only, none = op(img, None)
        random.seed(seed)
        d_only, none_d = op(pp.upload_pooled(img), None)
        assert none is None and none_d is None and np.array_equal(d_only.numpy(), h_only)
        d_only.free()
        assert balance[0] == 0, (seed, hit)


def _words(seed, fg_prob):
    random.seed(seed)
    return P.draw_words(fg_prob)


def test_affine_patch_training_end_to_end(tmp_path, capsys):
    """configs/synthetic/vnet_synthetic_ct_patch_affine_96.yml shrunk to a 32^3 patch of 40 x 44 x 52 volumes and two
    iterations, with both coins certain so that the kernel is in the loop"""
    from medicalseg_amd.core import train
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd import transforms as T
    src = open(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_affine_96.yml")).read()
    for old, new in (("'../_base_/global_configs.yml'", "'%s'" % os.path.join(ROOT, "configs", "_base_", "global_configs.yml")),
                     ("iters: 100", "iters: 2"), ("num_samples: 16", "num_samples: 4"), ("size: [96, 96, 96]", "size: [32, 32, 32]"),
                     ("rotate_prob: 0.2", "rotate_prob: 1.0"), ("scale_prob: 0.2", "scale_prob: 1.0")):
        assert old in src, old
        src = src.replace(old, new)
    assert src.count("shape: [144, 128, 160]") == 2
    src = src.replace("shape: [144, 128, 160]", "shape: [40, 44, 52]")
    p = tmp_path / "affine_32.yml"
    p.write_text(src)
    cfg = Config(str(p))
    ds = cfg.train_dataset
    assert type(ds.transforms.transforms[0]) is T.RandomAffinePatchCrop3D and ds.transforms.device
    random.seed(0)
    train(cfg.model, ds, optimizer=cfg.optimizer, save_dir=str(tmp_path / "o"), iters=cfg.iters, batch_size=cfg.batch_size,
          save_interval=10, log_iters=1, losses=cfg.loss)
    logged = [float(v) for v in re.findall(r"\[TRAIN\].*? loss: ([^,]+),", capsys.readouterr().out)]
    assert len(logged) == 2 and np.isfinite(logged).all() and all(v > 0 for v in logged), logged


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import MskError
    d = dev()
    shape, roi = (5, 7, 9), (4, 4, 4)
    n, nv = 64, 5 * 7 * 9
    img, label = R.image_for(shape, 1), R.label_for(shape, 2)
    ip, lp, sel = _up(img)[0], _up(label)[0], _record((0, 1, 2))
    out_i, out_l = dmalloc(4 * n), dmalloc(4 * n)
    big = dmalloc(4 * n + 64)                                                        # holds a record behind an output
    eye = np.eye(3, dtype=np.float32)

    def with_entry(i, v):
        m = eye.copy().reshape(9)
        m[i] = v
        return m

    def a(img=ip, label=lp, d_=5, h=7, w=9, sel=sel, m=eye, out_i=out_i, out_l=out_l, rd=4, rh=4, rw=4):
        keep, mp = _mat(m) if m is not None else (None, None)
        return (keep, (V(img) if img else None, V(label) if label else None, d_, h, w, V(sel) if sel else None, mp,
                       V(out_i) if out_i else None, V(out_l) if out_l else None, rd, rh, rw, C.c_float(-3.5), 255))
    bad = [a(img=None), a(sel=None), a(m=None), a(out_i=None),                                            # null pointers
           a(label=None), a(out_l=None),                                                                  # only one of the pair
           a(img=ip + 2), a(label=lp + 1), a(sel=sel + 2), a(out_i=out_i + 2), a(out_l=out_l + 3),        # not 4-byte aligned
           a(d_=0), a(h=0), a(w=-1), a(rd=0), a(rh=-3), a(rw=0),                                          # extents < 1
           a(d_=8193), a(h=8193), a(w=8193), a(rd=8193), a(rh=8193), a(rw=8193),                          # extents > 8192
           a(d_=2048, h=1024, w=1024), a(rd=2048, rh=1024, rw=1024),                                      # 2^31 voxels
           a(m=with_entry(0, np.nan)), a(m=with_entry(5, np.inf)), a(m=with_entry(8, -np.inf)),           # the matrix
           a(m=with_entry(3, 4.5)), a(m=with_entry(7, -4.0001)),
           a(out_i=ip), a(out_i=ip + 16), a(out_i=lp), a(out_l=lp), a(out_l=lp + 4 * (nv - 1)), a(out_l=ip),  # outputs over inputs
           a(out_l=out_i), a(out_l=out_i + 4 * (n - 1)), a(out_i=out_l + 16),                             # ... over each other
           a(out_i=big, sel=big + 4 * n - 8), a(out_l=big, sel=big + 16)]                                 # ... over the record
    d.set_option("prof_only_halo", 0)
    d.prof_reset()
    d.prof_enable(True)
    try:
        for keep, args in bad:
            rc = d.lib.msk_affine_patch(d.ctx, *args)
            assert rc != 0, args
            assert _lib.last_error(d.ctx)
            with pytest.raises(MskError, match="msk_affine_patch"):
                d.call("msk_affine_patch", *args)
        d.sync()
        assert d.prof_report() == {}                                                 # the launch counter: nothing was enqueued
        for p, words in ((out_i, n), (out_l, n), (big, n + 16)):                     # ... and the outputs hold the sentinel
            assert (d.d2h(p, (words,), np.uint32) == SENTINEL_BITS).all()
        # ... and the same call with valid arguments runs, is counted once, and |m| = 4 is allowed
        d.call("msk_affine_patch", *a()[1])
        d.sync()
        report = d.prof_report()
        assert list(report) == ["affine_patch"] and report["affine_patch"][0] == 1, report
    finally:
        d.prof_enable(False)
        d.prof_reset()
    want_i, want_l = R.affine(img, label, roi, (0, 1, 2), eye, PAD, LABEL_PAD)
    assert np.array_equal(d.d2h(out_i, roi, np.float32), want_i) and np.array_equal(d.d2h(out_l, roi, np.int32), want_l)
    assert np.array_equal(d.d2h(ip, shape, np.float32), img) and np.array_equal(d.d2h(lp, shape, np.int32), label)
    assert (d.d2h(big, (n + 16,), np.uint32) == SENTINEL_BITS).all()
    m4 = with_entry(2, 4.0)
    keep, args = a(m=m4)
    d.call("msk_affine_patch", *args)
    assert np.array_equal(d.d2h(out_i, roi, np.float32), R.affine(img, None, roi, (0, 1, 2), m4.reshape(3, 3), PAD)[0])

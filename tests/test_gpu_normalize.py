"""Foreground statistics, clip + z-score and the non-zero bounding box on the device (msk_fg_stats / msk_clip_zscore /
msk_nonzero_bbox, medicalseg_amd/csrc/msk_normalize.hip) against the statement tests/normalize_reference.py, and the Python
surface built on them (preprocess.*_device, DevicePipeline chains, RandomResizedCrop3D's non-zero pre-crop).

Bounds.  Everything here is exact: every field of a record is compared with == and by its sign bit, every output volume bit for
bit.  The one exception is the image of RandomResizedCrop3D's order-1 resampling, held to the 2e-6 of tests/test_gpu_augment.py,
here relative to the largest value (the host path is scipy's float64 zoom, the device interpolates in float32: a few ulps of the
operands); its label, its crop box and its random stream are compared exactly."""
import ctypes as C
import random

import numpy as np
import pytest

import normalize_reference as N
from helpers import dev, dfree, dmalloc, redzone_check, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

PAIRS = [(0.5, 99.5), (0.0, 100.0), (50.0, 50.0), (33.3, 95.0)]


def _ws_bytes(n):
    b = C.c_size_t(0)
    assert dev().lib.msk_fg_stats_workspace(C.c_long(n), C.byref(b)) == 0
    return b.value


def _ivec(a):
    """int32 array -> guarded device pointer"""
    a = np.ascontiguousarray(a, np.int32).reshape(-1)
    return vec(a.view(np.float32))


def _same_record(got, want, tag):
    for name, a, b in zip(N.FIELDS, got, want):
        assert a == b and np.signbit(a) == np.signbit(b), (tag, name, a, b)


def _same_bits(got, want, tag):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, (tag, bad.size, int(bad[0]), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


# ---- 1. msk_fg_stats -----------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 257, 4095, 4097, 70001, 1052677]   # the last: more than 256 chunks, the finish pass takes a second row
KINDS = ["gauss", "ct", "three", "denormals"]


def _stats_data(kind, n):
    rng = np.random.default_rng(n + len(kind))
    if kind == "gauss":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "ct":
        return np.round(rng.standard_normal(n) * 300.0 - 200.0).astype(np.float32)       # integer-valued, many ties, some zeros
    if kind == "three":
        return rng.choice(np.array([-2.5, 0.0, 3.0], np.float32), n)
    x = (rng.integers(-40, 40, n).astype(np.float32) * np.float32(1e-45)).astype(np.float32)   # denormals, -0.0 and +0.0
    x[::7] = -0.0
    x[3::7] = 0.0
    return x


def _masks(n):
    rng = np.random.default_rng(n)
    one = np.zeros(n, np.int32)
    one[n // 2] = 5
    half = rng.integers(-1, 2, n).astype(np.int32)        # -1 and 0 are outside
    return {"none": np.zeros(n, np.int32), "one": one, "half": half, "all": np.full(n, 3, np.int32)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_fg_stats_matches_the_statement_exactly(n, kind):
    d = dev()
    x = _stats_data(kind, n)
    masks = _masks(n)
    cases = [(N.ALL, None), (N.NONZERO, None)] + [(N.MASK, k) for k in masks]
    want = {c: N.fg_stats_pairs(x, c[0], masks.get(c[1]), PAIRS) for c in cases}
    ws, rec = dmalloc(_ws_bytes(n)), dmalloc(128)
    for off in (0, 1):                                    # 16-byte aligned, then offset by one float: the 4-byte forms
        host = np.zeros(n + off, np.float32)
        host[off:] = x
        xp = vec(host)
        mp = {}
        for k, m in masks.items():
            hm = np.zeros(n + off, np.int32)
            hm[off:] = m
            mp[k] = _ivec(hm)
        for mode, k in cases:
            mptr = mp[k] + 4 * off if k is not None else None
            for (q_lo, q_hi), w in zip(PAIRS, want[(mode, k)]):
                d.call("msk_fg_stats", vp(xp + 4 * off), vp(mptr), C.c_long(n), mode, C.c_double(q_lo), C.c_double(q_hi), vp(ws),
                       vp(rec))
                _same_record(d.d2h(rec, (16,), np.float64), w, (kind, n, off, mode, k, q_lo, q_hi))
        assert np.array_equal(d.d2h(xp, (n + off,), np.uint32), host.view(np.uint32))       # x is not modified
        for k, m in masks.items():
            assert np.array_equal(d.d2h(mp[k] + 4 * off, (n,), np.int32), m)               # nor the mask
        for p in [xp] + list(mp.values()):
            dfree(p)
    for p in (ws, rec):
        dfree(p)


# ---- 2. msk_clip_zscore --------------------------------------------------------------------------------------------------------
FLAG_CASES = [(N.CLIP | N.ZSCORE, None), (N.CLIP, None), (N.ZSCORE, None), (N.CLIP | N.ZSCORE | N.MASK_OUT, -7.5),
              (N.ZSCORE | N.MASK_OUT, 2.0)]


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4099, 270001])   # n % 4 != 0 and == 0; one tile, several, a grid-stride tail
def test_clip_zscore_matches_the_statement_bit_for_bit(n):
    d = dev()
    x = _stats_data("ct", n) + np.float32(0.25) * (np.arange(n) % 3 == 0).astype(np.float32)
    x[::11] = 0.0
    x[5::11] = -0.0
    mask = _masks(n)["half"]
    ws, rec = dmalloc(_ws_bytes(n)), dmalloc(128)
    for off in (0, 1):                                    # the 16-byte path, then the 4-byte path
        host = np.zeros(n + off, np.float32)
        host[off:] = x
        hm = np.zeros(n + off, np.int32)
        hm[off:] = mask
        xp, mp, yp = vec(host), _ivec(hm), dmalloc(4 * (n + off))
        xo, mo, yo = xp + 4 * off, mp + 4 * off, yp + 4 * off
        for mode, m, mptr in ((N.ALL, None, None), (N.NONZERO, None, None), (N.MASK, mask, mo)):
            d.call("msk_fg_stats", vp(xo), vp(mptr), C.c_long(n), mode, C.c_double(0.5), C.c_double(99.5), vp(ws), vp(rec))
            want_rec = N.fg_stats(x, mode, m, 0.5, 99.5)
            params = N.params_of_record(want_rec)
            for flags, outside in FLAG_CASES:
                want = N.clip_zscore(x, params, flags, mode, m, 0.0 if outside is None else outside)
                tag = (n, off, mode, flags)
                # out of place, the values from the device record
                d.call("msk_clip_zscore", vp(xo), vp(mptr), C.c_long(n), mode, vp(rec), None, flags, C.c_float(outside or 0.0),
                       vp(yo))
                from_record = d.d2h(yo, (n,), np.float32)
                _same_bits(from_record, want, tag + ("record",))
                # out of place, the same values as four host doubles: equal bits
                d.call("msk_clip_zscore", vp(xo), vp(mptr), C.c_long(n), mode, None, params.ctypes.data_as(C.c_void_p), flags,
                       C.c_float(outside or 0.0), vp(yo))
                _same_bits(d.d2h(yo, (n,), np.float32), from_record, tag + ("host",))
            assert np.array_equal(d.d2h(xp, (n + off,), np.uint32), host.view(np.uint32))   # x is not modified
            # in place
            flags, outside = FLAG_CASES[3]
            zp = vec(host)
            d.call("msk_clip_zscore", vp(zp + 4 * off), vp(mptr), C.c_long(n), mode, vp(rec), None, flags, C.c_float(outside),
                   vp(zp + 4 * off))
            _same_bits(d.d2h(zp + 4 * off, (n,), np.float32), N.clip_zscore(x, params, flags, mode, m, outside), (n, off, mode, "in place"))
            dfree(zp)
        for p in (xp, mp, yp):
            dfree(p)
    for p in (ws, rec):
        dfree(p)


# ---- 3. msk_nonzero_bbox -------------------------------------------------------------------------------------------------------
def _bbox(vol):
    d = dev()
    a = np.ascontiguousarray(vol)
    src = vec(a.reshape(-1).view(np.float32))
    box = _ivec(np.full(8, 77, np.int32))
    d.call("msk_nonzero_bbox", vp(src), *a.shape, 0 if a.dtype == np.float32 else 1, vp(box))
    got = d.d2h(box, (8,), np.int32)
    assert np.array_equal(d.d2h(src, (a.size,), np.uint32), a.reshape(-1).view(np.uint32))
    dfree(src)
    dfree(box)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (17, 33, 65), (40, 64, 96)])
def test_nonzero_bbox_matches_the_statement(shape, dtype):
    rng = np.random.default_rng(sum(shape))
    vols = {"empty": np.zeros(shape, dtype), "full": np.full(shape, 3, dtype)}
    if dtype == np.float32:
        vols["minus zero"] = np.full(shape, -0.0, np.float32)          # empty for floats
        nan = np.zeros(shape, np.float32)
        nan[-1, 0, -1] = np.nan                                        # a NaN counts as non-zero
        vols["nan"] = nan
    else:
        neg = np.zeros(shape, np.int32)
        neg[0, -1, 0] = -(2 ** 31)                                     # the bit pattern of -0.0 is a non-zero integer
        vols["int min"] = neg
    for cd in (0, shape[0] - 1):
        for ch in (0, shape[1] - 1):
            for cw in (0, shape[2] - 1):
                v = np.zeros(shape, dtype)
                v[cd, ch, cw] = -2
                vols["corner %d %d %d" % (cd, ch, cw)] = v
    sparse = np.zeros(shape, dtype)
    sparse[rng.random(shape) < 0.01] = 1
    vols["one per cent"] = sparse
    for name, v in vols.items():
        got, want = _bbox(v), N.nonzero_bbox(v)
        assert got.tolist() == want.tolist(), (shape, dtype, name, got, want)


def test_nonzero_bbox_takes_a_volume_that_is_only_4_byte_aligned():
    d = dev()
    shape = (5, 9, 13)
    v = np.zeros(shape, np.float32)
    v[1:4, 2:7, 3:11] = 1.0
    host = np.full(v.size + 1, 9.0, np.float32)                        # a non-zero word in front that must not be read
    host[1:] = v.reshape(-1)
    src, box = vec(host), dmalloc(32)
    d.call("msk_nonzero_bbox", vp(src + 4), *shape, 0, vp(box))
    assert d.d2h(box, (8,), np.int32).tolist() == [1, 2, 3, 4, 7, 11, 3 * 5 * 8, 0]


# ---- 4. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    d = dev()
    from medicalseg_amd._lib import MskError
    n = 1000
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    xp, mp, ws = vec(x), _ivec(np.ones(n, np.int32)), dmalloc(_ws_bytes(n))
    rec, yp, box = vec(np.full(64, 7.0)), vec(np.full(n, 7.0)), _ivec(np.full(8, 7, np.int32))
    b = C.c_size_t(0)
    assert d.lib.msk_fg_stats_workspace(C.c_long(0), C.byref(b)) != 0 and d.lib.msk_fg_stats_workspace(C.c_long(1 << 31), C.byref(b)) != 0
    assert d.lib.msk_fg_stats_workspace(C.c_long(5), None) != 0

    def stats(x=xp, mask=None, n=n, mode=0, q=(0.5, 99.5), ws=ws, rec=rec):
        d.call("msk_fg_stats", vp(x), vp(mask), C.c_long(n), mode, C.c_double(q[0]), C.c_double(q[1]), vp(ws), vp(rec))

    for kw, text in ((dict(x=None), "null"), (dict(ws=None), "null"), (dict(rec=None), "null"), (dict(n=0), "n must be"),
                     (dict(n=1 << 31), "n must be"), (dict(mode=3), "mask_mode"), (dict(mode=-1), "mask_mode"),
                     (dict(mode=2), "needs a mask"), (dict(q=(-0.5, 50)), "percentiles"), (dict(q=(50, 100.5)), "percentiles"),
                     (dict(q=(60, 40)), "percentiles"), (dict(q=(float("nan"), 50)), "percentiles"), (dict(x=xp + 2, n=n - 1), "aligned"),
                     (dict(mask=mp + 2, mode=2, n=n - 1), "aligned"), (dict(ws=ws + 8), "aligned"), (dict(rec=rec + 4), "aligned"),
                     (dict(ws=xp), "overlaps"), (dict(ws=mp, mask=mp, mode=2), "overlaps"), (dict(rec=ws + 4096), "overlaps"),
                     (dict(rec=xp), "overlaps")):
        with pytest.raises(MskError, match=text):
            stats(**kw)
    assert np.all(vec_back(rec, 64) == 7.0)
    stats()
    assert np.all(vec_back(rec, 32) != 7.0) and np.all(vec_back(rec, 64)[32:] == 7.0)      # the record is 16 doubles

    params = np.array([-1.0, 1.0, 0.0, 1.0], np.float64)

    def apply(x=xp, mask=None, n=n, mode=0, rec=None, params=params, flags=3, y=yp):
        d.call("msk_clip_zscore", vp(x), vp(mask), C.c_long(n), mode, vp(rec), params.ctypes.data_as(C.c_void_p) if params is not None else None,
               flags, C.c_float(0.0), vp(y))

    for kw, text in ((dict(x=None), "null"), (dict(y=None), "null"), (dict(params=None), "record or four"), (dict(n=0), "n must be"),
                     (dict(n=1 << 31), "n must be"), (dict(mode=5), "mask_mode"), (dict(mode=2), "needs a mask"), (dict(flags=8), "flags"),
                     (dict(flags=-1), "flags"), (dict(x=xp + 2, n=n - 1), "aligned"), (dict(y=yp + 2, n=n - 1), "aligned"),
                     (dict(rec=rec + 4), "aligned"), (dict(y=xp + 16, n=n - 4), "overlap"), (dict(y=mp, mask=mp, mode=2), "overlap"),
                     (dict(y=rec, n=8, rec=rec), "overlap")):
        with pytest.raises(MskError, match=text):
            apply(**kw)
    assert np.all(vec_back(yp, n) == 7.0) and np.array_equal(vec_back(xp, n), x)
    apply()
    assert np.all(vec_back(yp, n) != 7.0)

    def bbox(src=xp, shape=(10, 10, 10), dtype=0, box=box):
        d.call("msk_nonzero_bbox", vp(src), *shape, dtype, vp(box))

    for kw, text in ((dict(src=None), "null"), (dict(box=None), "null"), (dict(shape=(0, 10, 10)), "extents"), (dict(shape=(10, -1, 10)), "extents"),
                     (dict(shape=(10, 10, 0)), "extents"), (dict(shape=(2048, 1024, 1024)), "2\\^31"), (dict(dtype=2), "dtype"),
                     (dict(src=xp + 2), "aligned"), (dict(box=box + 2), "aligned"), (dict(box=xp + 64), "overlaps")):
        with pytest.raises(MskError, match=text):
            bbox(**kw)
    assert np.all(vec_back(box, 8, np.int32) == 7) and np.array_equal(vec_back(xp, n), x)
    bbox()
    assert vec_back(box, 8, np.int32).tolist() == [0, 0, 0, 10, 10, 10, 1000, 0]


# ---- 5. the Python surface, end to end -----------------------------------------------------------------------------------------
def _bordered_volume():
    """24 x 40 x 56 with a zero border, CT-like values inside and a few interior zeros (holes the non-zero mask keeps)"""
    rng = np.random.default_rng(17)
    raw = np.zeros((24, 40, 56), np.float32)
    raw[3:20, 5:33, 7:50] = np.round(rng.standard_normal((17, 28, 43)) * 250.0 + 60.0).astype(np.float32) + np.float32(0.5)
    raw[8:10, 10:14, 20:30] = 0.0
    label = ((raw > 200) & (rng.random(raw.shape) < 0.7)).astype(np.int32)
    return raw, label


def test_chain_equals_the_host_array_forms_bit_for_bit():
    from medicalseg_amd import preprocess as P
    raw, label = _bordered_volume()
    chain = P.DevicePipeline().image(raw).crop_to_nonzero().zscore((0.5, 99.5), "nonzero")
    assert chain.box.tolist() == [3, 5, 7, 20, 33, 50, int((raw != 0).sum()), 0]
    got = chain.numpy()
    ci, cl, box = P.crop_to_nonzero(raw, label)
    assert box.tolist() == chain.box.tolist() and ci.shape == (17, 28, 43) and np.array_equal(cl, label[3:20, 5:33, 7:50])
    want = P.zscore_normalize(ci, (0.5, 99.5), "nonzero")
    _same_bits(got, want, "chain against the host-array forms")
    _same_bits(want, P.zscore_normalize(ci, (0.5, 99.5), "nonzero", on_device=False), "device against the numpy host path")
    rec = N.fg_stats(ci, N.NONZERO, None, 0.5, 99.5)
    _same_bits(want, N.clip_zscore(ci, N.params_of_record(rec), N.CLIP | N.ZSCORE | N.MASK_OUT, N.NONZERO, None, 0.0), "statement")
    # the whole chain of the issue: one enqueued sequence down to the model's input tensor
    t = P.DevicePipeline().image(raw).crop_to_nonzero().zscore((0.5, 99.5), "nonzero").resample([16, 16, 16], 1).tensor()
    res, _ = P.resample(want, new_shape=[16, 16, 16], order=1)
    _same_bits(t.numpy()[0, 0], res, "resampled")
    # CT plan values, and the device crop of image and label together
    _same_bits(P.DevicePipeline().image(raw).ct_normalize(-300.0, 500.0, 55.0, 240.0).numpy(),
               N.clip_zscore(raw, [-300.0, 500.0, 55.0, 240.0]), "ct_normalize chain")
    _same_bits(P.ct_normalize(raw, -300.0, 500.0, 55.0, 240.0), P.ct_normalize(raw, -300.0, 500.0, 55.0, 240.0, on_device=False), "ct")
    iv, lv = P.upload_pooled(raw), P.upload_pooled(label)
    oi, ol, box = P.crop_to_nonzero_device(iv, lv)
    _same_bits(oi.numpy(), ci, "device crop")
    assert np.array_equal(ol.numpy(), cl)
    zero = P.upload_pooled(np.zeros((3, 4, 5), np.float32))
    same, none, box0 = P.crop_to_nonzero_device(zero)
    assert same is zero and none is None and not box0.any()          # an empty volume is returned whole
    for v in (iv, lv, oi, ol, zero):
        v.free()


def test_foreground_fingerprint_pools_the_per_case_records():
    from medicalseg_amd import preprocess as P
    raw, label = _bordered_volume()
    cases = [(raw, label), (raw[::-1] * np.float32(0.5), label[::-1]), (raw, np.zeros_like(label))]
    fp = P.ForegroundFingerprint()
    vols = []
    for img, lab in cases:
        vols += [P.upload_pooled(np.ascontiguousarray(img)), P.upload_pooled(np.ascontiguousarray(lab))]
        fp.add(vols[-2], vols[-1])
    out = fp.result()
    recs = [N.fg_stats(np.ascontiguousarray(i), N.MASK, np.ascontiguousarray(m), 0.5, 99.5) for i, m in cases]
    for got, want in zip(out["records"], recs):
        _same_record(got, want, "fingerprint")
    n = s = ss = np.float64(0.0)
    for r in recs:
        n, s, ss = n + r[0], s + r[3], ss + r[4]
    mean = s / n
    assert out["n"] == int(n) and out["mean"] == mean and out["std"] == np.sqrt(max(ss / n - mean * mean, 0.0))
    assert out["min"] == min(r[1] for r in recs[:2]) and out["max"] == max(r[2] for r in recs[:2])
    assert np.array_equal(out["percentiles"], np.array([r[7:9] for r in recs]))
    fp.free()
    for v in vols:
        v.free()


def test_resized_crop_takes_its_nonzero_box_from_the_device():
    from medicalseg_amd import preprocess as P
    from medicalseg_amd import transforms as T
    raw, label = _bordered_volume()
    label[:, :6, :] = 0
    t = T.RandomResizedCrop3D(size=(12, 12, 10), scale=(0.8, 1.2), pre_crop=True, nonzero_mask=True)
    for seed in (4, 5):
        dl = P.upload_pooled(label)
        np.random.seed(seed)
        host_box = t._pre_crop_box(raw, label)
        host_next = np.random.random()
        np.random.seed(seed)
        assert t._pre_crop_box(raw, dl) == host_box                  # the same box ...
        assert np.random.random() == host_next                       # ... from the same random stream
        dl.free()
        random.seed(seed)
        np.random.seed(seed)
        h_img, h_lab = t(raw.copy(), label.copy())
        random.seed(seed)
        np.random.seed(seed)
        d_img, d_lab = t(P.upload_pooled(raw), P.upload_pooled(label))
        di, dlab = d_img.numpy(), d_lab.numpy()
        assert di.shape == h_img.shape and np.array_equal(dlab, h_lab), seed
        scale = max(float(np.abs(h_img).max()), 1.0)
        assert np.abs(di - h_img).max() <= 2e-6 * scale, (seed, np.abs(di - h_img).max())
        d_img.free()
        d_lab.free()
    with pytest.raises(ValueError):
        t._pre_crop_box(raw, P.upload_pooled(np.zeros_like(label)))  # an empty label fails as it does on the host

"""Intensity augmentation on the device (medicalseg_amd/csrc/msk_intensity.hip, preprocess.intensity_stats_device /
intensity_apply_device / gauss_blur_device, the five Random*3D intensity transforms) against the numpy statement of
tests/intensity_reference.py.

Statistics, SCALE, CONTRAST and the blur are compared with np.array_equal.  NOISE, GAMMA and RESTORE use the device's logf /
cosf / powf: they are compared with the float64 statement, within 4 x the largest deviation of the float32-numpy evaluation
of the same formula from the float64 one ON THAT INPUT (computed here, from the statement alone): device libm and numpy's
float32 libm may each be a few ulp off, in different directions; a wrong counter, seed or record is an error of order 1.
Every buffer is red-zoned (tests/helpers.py): a store outside it fails by name, a load outside it pulls in a NaN."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import intensity_reference as R
from helpers import SENTINEL_BITS, dev, dfree, dmalloc, redzone_check, vec  # noqa: F401  (redzone_check: autouse here)

pytestmark = pytest.mark.gpu

BIG = 37 * 190 * 187                       # 321 chunks: more than the finish pass has lanes; crosses 2^20 voxels
N_LIST = [1, 3, 255, 256, 257, 4095, 4096, 4097, 256 * 4096 + 1, BIG]
N_SHORT = [1, 257, 4097, BIG]
N_FINISH = 2052 * 4096 + 7                  # 2053 chunks: every lane of the finish pass takes one eight-deep round, lanes 0..4 one more term
V = C.c_void_p


@functools.lru_cache(maxsize=None)
def _data(kind, n):
    rng = np.random.default_rng(n + 17)
    if kind == "normal":
        a = rng.standard_normal(n)
    elif kind == "negative":
        a = -1.0 - rng.random(n) * 5.0       # a zero-initialised maximum would win
    elif kind == "constant":
        a = np.full(n, 0.3)
    elif kind == "positive":
        a = 1.0 + rng.random(n) * 5.0        # a zero-initialised minimum would win
    else:
        a = rng.standard_normal(n) - 1000.0  # "offset"
    a = a.astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _stats(kind, n):
    rec = R.stats(_data(kind, n))
    rec.setflags(write=False)
    return rec


def _up(a, offset=0):
    """float32 array -> (pointer to its first element, pointer to free); offset 4: one SENTINEL word in front, so the data
    are only 4-byte aligned"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if not offset:
        p = vec(a)
        return p, p
    assert offset == 4
    host = np.empty(a.size + 1, np.uint32)
    host[0] = SENTINEL_BITS
    host[1:] = a.view(np.uint32)
    p = vec(host.view(np.float32))
    return p + 4, p


def _empty(n, offset=0):
    p = dmalloc(4 * n + offset)
    return p + offset, p


def _record(rec):
    return vec(np.ascontiguousarray(rec, np.float64).view(np.float32))


def _workspace(n):
    b = C.c_size_t(0)
    assert dev().lib.msk_intensity_stats_workspace(C.c_long(n), C.byref(b)) == 0
    return dmalloc(b.value)


def _params(*v):
    p = np.zeros(4, np.float32)
    p[:len(v)] = v
    return p


def _apply(x, y, n, mode, params, rec_a=None, rec_b=None, seed=0):
    dev().call("msk_intensity_apply", V(x), V(y), C.c_long(n), mode, params.ctypes.data_as(V), V(rec_a) if rec_a else None,
               V(rec_b) if rec_b else None, C.c_uint64(seed))


# ---- msk_intensity_stats -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("kind", ["normal", "negative", "positive", "constant", "offset"])
def test_stats_equal_the_statement(kind, offset):
    d = dev()
    for n in N_LIST + ([N_FINISH] if kind == "normal" else []):
        x, x_base = _up(_data(kind, n), offset)
        ws, rec1, rec2 = _workspace(n), dmalloc(32), dmalloc(32)
        d.call("msk_intensity_stats", V(x), C.c_long(n), V(ws), V(rec1))
        d.call("msk_intensity_stats", V(x), C.c_long(n), V(ws), V(rec2))          # the same workspace again
        got1, got2 = d.d2h(rec1, (4,), np.float64), d.d2h(rec2, (4,), np.float64)
        want = _stats(kind, n)
        assert np.array_equal(got1, want), (n, got1.tolist(), want.tolist())
        assert np.array_equal(got2, want), (n, got2.tolist(), want.tolist())
        for p in (x_base, ws, rec1, rec2):
            dfree(p)


# ---- SCALE and CONTRAST: bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_scale_and_contrast_equal_the_statement(inplace, offset):
    d = dev()
    binds = 0
    for n in N_LIST:
        kind = "offset" if n == 4097 else "normal"
        data, rec = _data(kind, n), _stats(kind, n)
        rp = _record(rec)
        cases = [(R.SCALE, _params(f)) for f in (0.75, 1.25)]
        cases += [(R.CONTRAST, _params(f, keep)) for f in (0.75, 1.25) for keep in (0.0, 1.0)]
        for mode, params in cases:
            x, x_base = _up(data, offset)
            y, y_base = (x, None) if inplace else _empty(n, offset)
            _apply(x, y, n, mode, params, rp)
            got = d.d2h(y, (n,), np.float32)
            want = R.apply(data, mode, params, rec)
            assert np.array_equal(got, want), (n, mode, params.tolist(), float(np.abs(got - want).max()))
            if mode == R.CONTRAST and params[1]:
                binds += not np.array_equal(want, R.apply(data, mode, _params(params[0], 0.0), rec))
            if not inplace:
                assert np.array_equal(d.d2h(x, (n,), np.float32), data)
                dfree(y_base)
            dfree(x_base)
        dfree(rp)
    assert binds >= 5                                                             # the clamp did bind


def test_contrast_reads_the_record_the_device_computed():
    """stats and apply enqueued back to back: the record never visits the host"""
    d = dev()
    n = BIG
    data = _data("normal", n)
    x, _ = _up(data)
    ws, rec = _workspace(n), dmalloc(32)
    d.call("msk_intensity_stats", V(x), C.c_long(n), V(ws), V(rec))
    _apply(x, x, n, R.CONTRAST, _params(1.25, 1.0), rec)
    assert np.array_equal(d.d2h(x, (n,), np.float32), R.contrast(data, 1.25, True, _stats("normal", n)))


# ---- NOISE, GAMMA, RESTORE: the float64 statement, tolerance from the statement's own float32 evaluation ----------------------
def _close(got, want64, want32, what):
    tol = 4.0 * float(np.abs(want32.astype(np.float64) - want64).max())
    err = float(np.abs(got.astype(np.float64) - want64).max())
    print("%s: device error %.3e, float32-numpy deviation x 4 = %.3e" % (what, err, tol))
    assert np.isfinite(got).all() and err <= tol, (what, err, tol)


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("seed", [1, 0xF00DFACE12345678])
def test_noise_within_the_float32_deviation(seed, offset):
    d = dev()
    for n in N_SHORT:
        data = _data("normal", n)
        x, x_base = _up(data, offset)
        y, y_base = _empty(n, offset)
        p = _params(0.1)
        _apply(x, y, n, R.NOISE, p, seed=seed)
        got = d.d2h(y, (n,), np.float32)
        _close(got, R.noise(data, p[0], seed), R.noise(data, p[0], seed, np.float32), "noise n = %d" % n)
        if n == BIG:                                                              # another seed is an error of order 1
            assert float(np.abs(got - R.noise(data, p[0], seed + 1)).max()) > 0.1
            z = (got.astype(np.float64) - data) / float(p[0])
            assert abs(z.mean()) < 5 / np.sqrt(n) + 1e-4 and abs(z.std() - 1) < 5 / np.sqrt(2 * n) + 1e-4
        _apply(x, x, n, R.NOISE, p, seed=seed)                                    # in place: the same values
        assert np.array_equal(d.d2h(x, (n,), np.float32), got)
        dfree(x_base)
        dfree(y_base)


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("invert", [False, True], ids=["plain", "invert"])
def test_gamma_and_restore_within_the_float32_deviation(invert, offset):
    d = dev()
    for n in N_SHORT:
        for kind, g in (("normal", 0.7), ("offset", 1.5), ("constant", 0.7)):
            data, rec = _data(kind, n), _stats(kind, n)
            x, x_base = _up(data, offset)
            y, y_base = _empty(n, offset)
            ra = _record(rec)
            p = _params(g, float(invert))
            _apply(x, y, n, R.GAMMA, p, ra)
            got = d.d2h(y, (n,), np.float32)
            g32 = R.gamma(data, p[0], invert, rec, np.float32)
            _close(got, R.gamma(data, p[0], invert, rec), g32, "gamma %s %g n = %d" % (kind, g, n))
            if kind == "constant":
                assert np.array_equal(got, data)                                   # rg = 0 gives mn, not NaN
            elif n > 1:
                # retain_stats on the statement's own float32 gamma output, so that both sides start from the same volume
                rec_b = R.stats(g32)
                gx, gx_base = _up(g32, offset)
                rb = _record(rec_b)
                _apply(gx, gx, n, R.RESTORE, _params(), ra, rb)
                back = d.d2h(gx, (n,), np.float32)
                _close(back, R.restore(g32, rec, rec_b), R.restore(g32, rec, rec_b, np.float32), "restore %s n = %d" % (kind, n))
                if n == BIG:
                    assert abs(float(back.astype(np.float64).mean()) - rec[2] / n) < 1e-3 * max(1.0, abs(rec[2] / n))
                dfree(gx_base)
                dfree(rb)
            for ptr in (x_base, y_base, ra):
                dfree(ptr)


# ---- msk_gauss_blur3d ----------------------------------------------------------------------------------------------------------
BLUR_SHAPES = [(1, 1, 1), (2, 3, 5), (5, 6, 7), (16, 16, 16), (9, 70, 67), (20, 33, 130), (3, 5, 300), (150, 4, 6)]
BLUR_SIGMAS = [(0.5, 0.5, 0.5), (1, 1, 1), (2, 2, 2), (0, 1, 0), (2, 0, 0.5), (0, 0, 0)]


def _blur_input(shape):
    x = np.random.default_rng(int(np.prod(shape))).standard_normal(shape).astype(np.float32)
    x[0, 0, 0] += 1.0                                                             # unit impulses at two opposite corners:
    x[-1, -1, -1] += 1.0                                                          # the reflection is visible
    return x


def _blur(x, y, shape, sigmas, tmp):
    taps = [R.taps(s) for s in sigmas]
    args = []
    for t in taps:
        args += [t.ctypes.data_as(V) if len(t) else None, (len(t) - 1) // 2 if len(t) else 0]
    dev().call("msk_gauss_blur3d", V(x), V(y), *shape, *args, V(tmp))


@pytest.mark.parametrize("shape", BLUR_SHAPES)
def test_blur_equals_the_statement(shape):
    d = dev()
    n = int(np.prod(shape))
    data = _blur_input(shape)
    offsets = [0, 4] if shape == (9, 70, 67) else [0]
    for offset in offsets:
        x, _ = _up(data, offset)
        for sigmas in BLUR_SIGMAS if offset == 0 else BLUR_SIGMAS[:5:2]:
            y, y_base = _empty(n, offset)                                         # SENTINEL: an unwritten voxel is NaN
            tmp, tmp_base = _empty(n, offset)
            _blur(x, y, shape, sigmas, tmp)
            got = d.d2h(y, shape, np.float32)
            want = R.blur(data, sigmas)
            assert np.array_equal(got, want), (shape, sigmas, offset, float(np.abs(got - want).max()))
            dfree(y_base)
            dfree(tmp_base)
        assert np.array_equal(d.d2h(x, shape, np.float32), data)


def test_blur_argument_errors_launch_nothing():
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import MskError
    d = dev()
    shape = (5, 6, 7)
    n = 5 * 6 * 7
    data = _blur_input(shape)
    x, _ = _up(data)
    y, _ = _empty(n)
    tmp, _ = _empty(n)
    w9 = np.full(19, 1 / 19, np.float32)
    w1 = R.taps(0.5)
    p9, p1 = w9.ctypes.data_as(V), w1.ctypes.data_as(V)
    bad = [(V(x), V(y), 5, 6, 7, p9, 9, p1, 2, p1, 2, V(tmp)),                    # r = 9
           (V(x), V(y), 5, 6, 7, p1, 2, p1, 2, p9, 9, V(tmp)),
           (V(x), V(y), 5, 6, 7, p1, -1, p1, 2, p1, 2, V(tmp)),
           (V(x), V(x), 5, 6, 7, p1, 2, p1, 2, p1, 2, V(tmp)),                    # y == x
           (V(x), V(x + 16), 5, 6, 7, p1, 2, None, 0, None, 0, V(tmp)),           # y overlaps x
           (V(x), V(y), 5, 6, 7, p1, 2, p1, 2, p1, 2, V(y)),                      # tmp == y
           (V(x), V(y), 5, 6, 7, p1, 2, p1, 2, None, 0, None),                    # two axes, no tmp
           (V(x), V(y), 5, 6, 7, None, 2, p1, 2, p1, 2, V(tmp)),                  # no taps
           (V(x), V(y), 0, 6, 7, p1, 2, p1, 2, p1, 2, V(tmp)),
           (V(x), V(y), 2048, 1024, 1024, p1, 2, p1, 2, p1, 2, V(tmp)),           # 2^31 voxels
           (None, V(y), 5, 6, 7, p1, 2, p1, 2, p1, 2, V(tmp))]
    for args in bad:
        assert d.lib.msk_gauss_blur3d(d.ctx, *args) != 0, args
        assert _lib.last_error(d.ctx)
        with pytest.raises(MskError, match="msk_gauss_blur3d"):
            d.call("msk_gauss_blur3d", *args)
    rec, ws = dmalloc(32), _workspace(n)
    p = _params(1.0)
    bad_apply = [(V(x), V(y), C.c_long(n), 5, p.ctypes.data_as(V), None, None, C.c_uint64(0)),            # unknown mode
                 (V(x), V(y), C.c_long(n), R.CONTRAST, p.ctypes.data_as(V), None, None, C.c_uint64(0)),   # no record
                 (V(x), V(y), C.c_long(n), R.GAMMA, p.ctypes.data_as(V), None, None, C.c_uint64(0)),
                 (V(x), V(y), C.c_long(n), R.RESTORE, p.ctypes.data_as(V), V(rec), None, C.c_uint64(0)),
                 (V(x), V(x + 16), C.c_long(n), R.SCALE, p.ctypes.data_as(V), None, None, C.c_uint64(0)),  # partial overlap
                 (V(x), V(y), C.c_long(0), R.SCALE, p.ctypes.data_as(V), None, None, C.c_uint64(0)),
                 (V(x), V(y), C.c_long(n), R.SCALE, None, None, None, C.c_uint64(0))]
    for args in bad_apply:
        assert d.lib.msk_intensity_apply(d.ctx, *args) != 0, args
        assert _lib.last_error(d.ctx)
    for args in [(None, C.c_long(n), V(ws), V(rec)), (V(x), C.c_long(0), V(ws), V(rec)), (V(x), C.c_long(2 ** 31), V(ws), V(rec)),
                 (V(x), C.c_long(n), None, V(rec)), (V(x), C.c_long(n), V(ws), None), (V(x), C.c_long(n), V(ws), V(rec + 4))]:
        assert d.lib.msk_intensity_stats(d.ctx, *args) != 0, args
        assert _lib.last_error(d.ctx)
    # nothing was launched
    assert (d.d2h(y, (n,), np.uint32) == SENTINEL_BITS).all() and (d.d2h(tmp, (n,), np.uint32) == SENTINEL_BITS).all()
    assert (d.d2h(rec, (8,), np.uint32) == SENTINEL_BITS).all() and np.array_equal(d.d2h(x, shape, np.float32), data)
    # ... and the same call with valid arguments runs
    d.call("msk_gauss_blur3d", V(x), V(y), 5, 6, 7, p1, 2, p1, 2, p1, 2, V(tmp))
    assert np.array_equal(d.d2h(y, shape, np.float32), R.blur(data, (0.5, 0.5, 0.5)))


# ---- preprocess wrappers and the transforms --------------------------------------------------------------------------------------
def test_preprocess_wrappers_use_the_pool_and_download_nothing():
    import inspect
    import re

    from medicalseg_amd import preprocess as pp
    for fn in (pp.intensity_stats_device, pp.intensity_apply_device, pp.gauss_blur_device):
        assert not re.search(r"d2h|\.numpy\(|\.sync\(", inspect.getsource(fn)), fn.__name__
    shape = (9, 70, 67)
    data = _blur_input(shape)
    vol = pp.upload_pooled(data)
    rec = pp.intensity_stats_device(vol)
    assert rec.pooled and rec.shape == (4,) and rec.dtype == np.float64
    want_rec = R.stats(data)
    assert np.array_equal(rec.numpy(), want_rec)
    out = pp.intensity_apply_device(vol, pp.INTENSITY_CONTRAST, [0.75, 1], stats_a=rec, inplace=False)
    assert out is not vol and out.pooled and np.array_equal(out.numpy(), R.contrast(data, 0.75, True, want_rec))
    assert np.array_equal(vol.numpy(), data)
    same = pp.intensity_apply_device(vol, pp.INTENSITY_SCALE, [1.25])
    assert same is vol and np.array_equal(vol.numpy(), R.scale(data, 1.25))
    blurred = pp.gauss_blur_device(out, (2, 0, 0.5))
    assert blurred.pooled and np.array_equal(blurred.numpy(), R.blur(R.contrast(data, 0.75, True, want_rec), (2, 0, 0.5)))
    one = pp.gauss_blur_device(out, 1.0)
    assert np.array_equal(one.numpy(), R.blur(R.contrast(data, 0.75, True, want_rec), (1, 1, 1)))
    ptr = rec.ptr
    rec.free()
    again = pp.intensity_stats_device(vol)
    assert again.ptr == ptr                                                        # the record buffer comes back from the pool
    with pytest.raises(ValueError):
        pp.gauss_blur_device(out, 2.5)
    with pytest.raises(TypeError):
        pp.intensity_stats_device(pp.upload_pooled(np.zeros(shape, np.int32)))
    for v in (again, out, blurred, one, vol):
        v.free()


SHAPE = (20, 33, 40)


def _sample():
    img = (np.random.default_rng(5).standard_normal(SHAPE) * 0.5 + 1.0).astype(np.float32)
    label = (np.random.default_rng(6).integers(0, 3, SHAPE)).astype(np.int32)
    return img, label


def _ops(T, noise=0.0, exact=0.0, gamma=0.0, **gamma_kw):
    return [T.RandomGaussianNoise3D(noise, (0.05, 0.1)), T.RandomGaussianBlur3D(exact, (0.5, 1.5), per_axis=True),
            T.RandomBrightness3D(exact, (0.75, 1.25)), T.RandomContrast3D(exact, (0.75, 1.25)),
            T.RandomGamma3D(gamma, (0.7, 1.5), **gamma_kw)]


@pytest.mark.parametrize("seed", [0, 4])
def test_exact_transforms_device_path_equals_host_path(seed):
    """blur, brightness and contrast fired, noise and gamma did not: equal arrays op by op, and the max-normalisation's
    tolerance (test_gpu_patch.py) at the end of Compose"""
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    img, label = _sample()
    ops = _ops(T, exact=1.0)
    random.seed(seed)
    h_img, h_lab = img.copy(), label
    for op in ops:
        h_img, h_lab = op(h_img, h_lab)
    state = random.getstate()
    random.seed(seed)
    d_img, d_lab = pp.upload_pooled(img), pp.upload_pooled(label)
    lab_ptr = d_lab.ptr
    for op in ops:
        d_img, d_lab = op(d_img, d_lab)
    assert random.getstate() == state
    assert not np.array_equal(h_img, img) and np.array_equal(d_img.numpy(), h_img)
    assert h_lab is label and d_lab.ptr == lab_ptr and np.array_equal(d_lab.numpy(), label)
    d_img.free()
    d_lab.free()
    random.seed(seed)
    c_img, c_lab = T.Compose(ops)(img.copy(), label.copy())
    random.seed(seed)
    g_img, g_lab = T.Compose(ops, device=True)(img.copy(), label.copy())
    assert pp.DeviceVolume is type(g_lab) and np.array_equal(g_lab.numpy(), label) and np.array_equal(c_lab, label)
    gi = g_img.numpy()
    assert gi.shape == c_img.shape[1:] and np.abs(gi - c_img[0]).max() <= 2e-6, np.abs(gi - c_img[0]).max()
    g_img.free()
    g_lab.free()


CASES = [("noise", dict(noise=1.0)), ("gamma", dict(gamma=1.0)), ("gamma invert", dict(gamma=1.0, invert=True)),
         ("gamma alone", dict(gamma=1.0, retain_stats=False))]


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_noise_and_gamma_transforms_within_the_float32_deviation(name, kw):
    """one of noise / gamma fired, nothing else: Compose on the device against the float64 statement with the parameters the
    classes drew, within 4 x the deviation of the host path (the statement's float32 evaluation), both divided by the
    maximum as Compose does, plus the max-normalisation's 2e-6"""
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    img, label = _sample()
    ops = _ops(T, **kw)
    for seed in (0, 4):
        random.seed(seed)
        if "noise" in kw:
            _, u, bits = random.random(), random.random(), random.getrandbits(64)
            want64 = R.noise(img, np.float32(R.value((0.05, 0.1), u)), bits)
        else:
            random.random(), random.random(), random.getrandbits(64)                # the noise class's draws
            for _ in range(4 + 2 + 3):                                              # blur, brightness, contrast
                random.random()
            _, branch, u = random.random(), random.random(), random.random()
            g = np.float32(R.value(R.branch_range((0.7, 1.5), branch), u))
            rec = R.stats(img)
            invert = kw.get("invert", False)
            want64 = R.gamma(img, g, invert, rec)
            if kw.get("retain_stats", True):
                g32 = R.gamma(img, g, invert, rec, np.float32)
                want64 = R.restore(g32, rec, R.stats(g32))
        random.seed(seed)
        c_img, c_lab = T.Compose(ops)(img.copy(), label.copy())
        state = random.getstate()
        random.seed(seed)
        g_img, g_lab = T.Compose(ops, device=True)(img.copy(), label.copy())
        assert random.getstate() == state
        top = float(want64.max())
        assert top > 0
        want = want64 / top
        tol = 4.0 * float(np.abs(c_img[0].astype(np.float64) - want).max()) + 2e-6
        err = float(np.abs(g_img.numpy().astype(np.float64) - want).max())
        print("%s seed %d: device error %.3e, tolerance %.3e" % (name, seed, err, tol))
        assert err <= tol and tol < 1e-4
        assert type(g_lab) is pp.DeviceVolume and np.array_equal(g_lab.numpy(), label) and np.array_equal(c_lab, label)
        g_img.free()
        g_lab.free()

"""Order-3 resampling on the device (medicalseg_amd/csrc/msk_spline.hip, preprocess.resample_device / resized_crop_device
with order 3, transforms.Resize3D, transforms.RandomLowResolution3D) against the numpy statement of tests/spline_reference.py.
Results are compared with np.array_equal; the goldens captured from the reference keep their one-rounding tolerance.  Every
buffer, the float64 workspace included, is red-zoned (tests/helpers.py): a store outside it fails by name, a load outside it
pulls in a NaN, and a destination voxel that is never written reads back as NaN."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import spline_reference as R
from helpers import SENTINEL_BITS, dev, dfree, dmalloc, redzone_check, vec  # noqa: F401  (redzone_check: autouse here)

pytestmark = pytest.mark.gpu

V = C.c_void_p
# (volume, crop box or None, output): extents of 1 and n_out == 1; padded W = 65, one past a wavefront and one past an LDS
# chunk; a W line of 324 samples (six chunks, state carried both ways); D and H lines longer than the initialisation's
# horizon and than a chunk; (12,16,16): more than one workgroup in every pass and in the zoom; a crop box
CASES = [((9, 14, 11), None, (12, 7, 20)), ((1, 5, 3), None, (4, 5, 1)), ((2, 2, 2), None, (5, 1, 3)),
         ((3, 4, 41), None, (3, 9, 17)), ((3, 4, 300), None, (3, 4, 150)), ((40, 3, 5), None, (17, 3, 5)),
         ((3, 70, 5), None, (3, 33, 5)), ((12, 16, 16), None, (24, 32, 32)), ((10, 12, 16), (2, 3, 5, 6, 7, 9), (8, 8, 8))]


@functools.lru_cache(maxsize=None)
def _case(k):
    """input, box, output shape and the statement of one case, computed once and shared"""
    shape, box, out = CASES[k]
    img = (np.random.default_rng(300 + k).standard_normal(shape) * 400.0 - 300.0).astype(np.float32)
    if box is not None:
        i, j, kk, d, h, w = box
        inner = img[i:i + d, j:j + h, kk:kk + w].copy()
        img[...] = np.float32(1e6)                           # a clamp to the volume instead of the box shows
        img[i:i + d, j:j + h, kk:kk + w] = inner
    else:
        box = (0, 0, 0) + shape
    want = R.spline_crop_zoom(img, box, out)
    for a in (img, want):
        a.setflags(write=False)
    return img, box, out, want


def _workspace_bytes(box):
    b = C.c_size_t(0)
    assert dev().lib.msk_spline_workspace(*box[3:], C.byref(b)) == 0
    return b.value


def _run(sp, shape, box, dp, out, ws, ws_bytes):
    return dev().lib.msk_spline_resample3d(dev().ctx, V(sp), *shape, *box, V(dp), *out, V(ws), C.c_size_t(ws_bytes))


def _bits(ptr, shape):
    return dev().d2h(ptr, shape, np.uint32)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_kernel_equals_the_statement_and_only_reads_the_source(k):
    img, box, out, want = _case(k)
    d = dev()
    nbytes = _workspace_bytes(box)
    sp, dp, ws = vec(img), dmalloc(4 * want.size), dmalloc(nbytes)
    assert _run(sp, img.shape, box, dp, out, ws, nbytes) == 0, d.lib.msk_last_error(d.ctx)
    got = d.d2h(dp, out, np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        "%d of %d voxels differ, max |diff| %g" % ((got != want).sum(), want.size, np.abs(got - want).max())
    assert np.array_equal(_bits(sp, img.shape), img.view(np.uint32))
    for p in (sp, dp, ws):
        dfree(p)


@pytest.mark.parametrize("k", [0, 4, 8])
def test_result_does_not_depend_on_the_workspace(k):
    """a workspace full of NaN bits (dmalloc's sentinel) was the case above; here all-ones bits, and one larger than asked for"""
    img, box, out, want = _case(k)
    d = dev()
    nbytes = _workspace_bytes(box)
    big = nbytes + 4096 + 8
    sp, dp, ws = vec(img), dmalloc(4 * want.size), dmalloc(big)
    d.h2d(ws, np.full(big // 4, 0xFFFFFFFF, np.uint32))
    assert _run(sp, img.shape, box, dp, out, ws, big) == 0
    assert np.array_equal(_bits(dp, out), want.view(np.uint32))
    d.h2d(dp, np.full(want.size, SENTINEL_BITS, np.uint32))
    assert _run(sp, img.shape, box, dp, out, ws + 8, big - 8) == 0            # 8-byte aligned only, and dirty from the first run
    assert np.array_equal(_bits(dp, out), want.view(np.uint32))
    assert np.array_equal(_bits(ws + nbytes + 8, (1024,)), np.full(1024, 0xFFFFFFFF, np.uint32))   # nothing past what was asked for
    for p in (sp, dp, ws):
        dfree(p)


def test_argument_errors_leave_the_destination_alone():
    img, box, out, want = _case(8)
    shape = img.shape
    d = dev()
    nbytes = _workspace_bytes(box)
    sp, dp, ws = vec(img), dmalloc(4 * want.size), dmalloc(nbytes)
    need = (box[3] + 24) * (box[4] + 24) * (box[5] + 24) * 8
    bad = [
        (sp, shape, box, dp, out, ws, need - 8),                              # a workspace too small
        (sp, shape, box, dp, out, ws, 0),
        (sp, shape, box[:3] + (0, 7, 9), dp, out, ws, nbytes),                # empty extents
        (sp, shape, box, dp, (8, 0, 8), ws, nbytes),
        (sp, (0, 12, 16), box, dp, out, ws, nbytes),
        (sp, shape, (5, 3, 5, 6, 7, 9), dp, out, ws, nbytes),                 # boxes outside the volume: 5 + 6 > 10
        (sp, shape, (2, 3, 8, 6, 7, 9), dp, out, ws, nbytes),                 # 8 + 9 > 16
        (sp, shape, (-1, 3, 5, 6, 7, 9), dp, out, ws, nbytes),
        (None, shape, box, dp, out, ws, nbytes),                              # null pointers
        (sp, shape, box, None, out, ws, nbytes),
        (sp, shape, box, dp, out, None, nbytes),
        (sp, shape, box, dp, out, ws + 4, nbytes),                            # a misaligned workspace
    ]
    for args in bad:
        assert _run(*args) != 0, args
        assert d.lib.msk_last_error(d.ctx)
    d.sync()
    assert (_bits(dp, out) == SENTINEL_BITS).all()
    assert (_bits(ws, (nbytes // 4,)) == SENTINEL_BITS).all()
    assert _run(sp, shape, box, dp, out, ws, nbytes) == 0                     # and the context still works
    assert np.array_equal(_bits(dp, out), want.view(np.uint32))
    for p in (sp, dp, ws):
        dfree(p)


# ---- the preprocess wrappers and the transforms ------------------------------------------------------------------------------
def test_wrappers_equal_the_statement():
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    img, box, out, want = _case(0)
    vol = pp.upload(img)
    for pooled in (False, True):
        got = pp.resample_device(vol, out, order=3, pooled=pooled)
        assert got.pooled == pooled and got.dtype == np.float32 and got.shape == out
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
        got.free()
    vol.free()
    img, box, out, want = _case(8)
    vol = pp.upload_pooled(img)
    got = pp.resized_crop_device(vol, *box, out, 3)
    assert got.pooled and np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    got.free()
    vol.free()
    # Resize3D on a device volume: a tuple size and an int size (the shortest side, functional.py:41-46); the label takes order 0
    img = _case(0)[0]
    label = (np.arange(img.size) % 4).astype(np.int32).reshape(img.shape)
    for size, shape in (((12, 7, 20), (12, 7, 20)), (12, (12, 18, 14))):
        o_img, o_lab = T.Resize3D(size, order=3)(pp.upload_pooled(img), pp.upload_pooled(label))
        assert np.array_equal(o_img.numpy().view(np.uint32), R.spline_zoom(img, shape).view(np.uint32))
        h_img, h_lab = T.Resize3D(size, order=3)(img, label)
        assert np.array_equal(o_lab.numpy(), h_lab) and o_img.shape == h_img.shape
        o_img.free()
        o_lab.free()
    res, _ = pp.resample(img, new_shape=[12, 7, 20], order=3)
    assert res.dtype == np.float32 and np.array_equal(res, _case(0)[3])


def test_wrappers_stay_within_the_golden_tolerance():
    from medicalseg_amd import preprocess as pp
    unequal = total = 0
    for name, img, shape, want in R.golden_cases():
        vol = pp.upload_pooled(img)
        got = pp.resample_device(vol, shape, order=3, pooled=True)
        unequal += R.assert_within_golden_tolerance(got.numpy(), img, want, name)
        total += want.size
        got.free()
        vol.free()
    assert unequal <= 0.01 * total, (unequal, total)


def test_wrappers_refuse_and_keep_orders_0_and_1(monkeypatch):
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd._lib import MskError
    img = _case(0)[0]
    out = (12, 7, 20)
    label = (np.arange(img.size) % 4).astype(np.int32).reshape(img.shape)
    iv, lv = pp.upload(img), pp.upload(label)
    with pytest.raises(ValueError, match="float32"):
        pp.resample_device(lv, out, order=3)
    for order in (2, 4, 5):
        with pytest.raises(ValueError, match="0, 1 and 3"):
            pp.resample_device(iv, out, order=order)
        with pytest.raises(ValueError, match="0, 1 and 3"):
            pp.resized_crop_device(iv, 0, 0, 0, *img.shape, out, order)
    d = dev()
    with pytest.raises(MskError):                                              # the raw entry points still refuse order 3
        d.call("msk_resample3d", V(iv.ptr), *img.shape, V(iv.ptr), *img.shape, 3, 0)
    n = int(np.prod(out))
    for vol, dt in ((iv, 0), (lv, 1)):
        for order in ((0, 1) if dt == 0 else (0,)):
            dp = dmalloc(4 * n)
            d.call("msk_resample3d", V(vol.ptr), *img.shape, V(dp), *out, order, dt)
            got = pp.resample_device(vol, out, order=order)
            crop = pp.resized_crop_device(vol, 0, 0, 0, *img.shape, out, order)
            assert np.array_equal(got.numpy().view(np.uint32), _bits(dp, out))
            assert np.array_equal(crop.numpy().view(np.uint32), _bits(dp, out))
            got.free()
            crop.free()
            dfree(dp)
    # a refused call hands its output and its scratch back
    balance = [0]
    alloc, release = pp._pool_alloc, pp._pool_release
    monkeypatch.setattr(pp, "_pool_alloc", lambda dev_, nbytes: (balance.__setitem__(0, balance[0] + 1), alloc(dev_, nbytes))[1])
    monkeypatch.setattr(pp, "_pool_release", lambda dev_, ptr, nbytes: (balance.__setitem__(0, balance[0] - 1), release(dev_, ptr, nbytes))[1])
    with pytest.raises(MskError, match="msk_spline_resample3d"):
        pp.resized_crop_device(iv, 5, 0, 0, *img.shape, out, 3)               # a box outside the volume
    assert balance[0] == 0
    iv.free()
    lv.free()


@pytest.mark.parametrize("per_axis", [False, True])
def test_low_resolution_device_path_equals_host_path(per_axis, monkeypatch):
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    from medicalseg_amd.device import Device
    img = (np.random.default_rng(41).standard_normal((9, 20, 70)) * 0.5 + 0.25).astype(np.float32)
    label = (np.arange(img.size) % 3).astype(np.int32).reshape(img.shape)
    op = T.RandomLowResolution3D(prob=1.0, zoom=(0.4, 0.9), per_axis=per_axis)
    random.seed(17)
    h_img, h_lab = op(img, label)
    state = random.getstate()
    assert h_lab is label and not np.array_equal(h_img, img)
    iv, lv = pp.upload_pooled(img), pp.upload_pooled(label)
    random.seed(17)
    d_img, d_lab = op(iv, lv)
    assert random.getstate() == state
    assert d_lab is lv and d_img.pooled and d_img.shape == img.shape
    assert np.array_equal(d_img.numpy().view(np.uint32), h_img.view(np.uint32))
    # prob = 0: the same draws, the same volume, nothing launched
    calls = []
    real = Device.call

    def counting(self, name, *args):
        calls.append(name)
        return real(self, name, *args)
    monkeypatch.setattr(Device, "call", counting)
    random.seed(17)
    same, lab = T.RandomLowResolution3D(prob=0.0, zoom=(0.4, 0.9), per_axis=per_axis)(d_img, lv)
    monkeypatch.setattr(Device, "call", real)
    assert same is d_img and lab is lv and calls == [] and random.getstate() == state
    d_img.free()
    lv.free()

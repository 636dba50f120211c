"""msk_fill_holes3d (medicalseg_amd/csrc/msk_ccl.hip) against the statement tests/fillholes_reference.py, and the Python surface
built on it (preprocess.fill_holes_device / nonzero_mask_device, _Chain.zscore(fill_holes=True), transforms.FillHoles3D).

Everything is exact: every output voxel, every count and every status word is compared with ==.  The buffers of the C-ABI
cases sit between red zones (helpers.vec / dmalloc).  Shapes are chosen against the 4 x 8 x 32 tile of the union-find."""
import ctypes as C

import numpy as np
import pytest

import fillholes_reference as F
from helpers import dev, dmalloc, redzone_check, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

MASK, LABEL = 0, 1


def _ivec(a):
    a = np.ascontiguousarray(a, np.int32).reshape(-1)
    return vec(a.view(np.float32))


def _run(vols, mode, classes=None, dtype=np.int32, inplace=False, counts=True):
    """msk_fill_holes3d on a batch of equal-shape volumes -> (outputs [n, d, h, w], counts or None); asserts status == 0 and
    that an out-of-place call leaves the source as it was"""
    vols = np.stack([np.asarray(v) for v in vols]).astype(dtype)
    n, (d, h, w) = vols.shape[0], vols.shape[1:]
    src = vec(vols) if dtype == np.float32 else _ivec(vols)
    dst = src if inplace else dmalloc(vols.size * 4)
    st, cn = _ivec(np.full(n, -1)), (_ivec(np.full(n, -1)) if counts else 0)
    cls = np.ascontiguousarray(classes if classes is not None else [], np.int32)
    dev().call("msk_fill_holes3d", vp(src), vp(dst), n, d, h, w, 0 if dtype == np.float32 else 1, mode,
               cls.ctypes.data_as(C.c_void_p) if cls.size else None, int(cls.size), vp(st), vp(cn))
    out = vec_back(dst, vols.size, np.int32).reshape(vols.shape)
    assert (vec_back(st, n, np.int32) == 0).all(), "status"
    if not inplace:
        assert np.array_equal(vec_back(src, vols.size, np.uint32), vols.reshape(-1).view(np.uint32)), "the source was modified"
    return out, (vec_back(cn, n, np.int32) if counts else None)


def _same(got, want, tag):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d voxels differ, first %s: got %d want %d" % (
            tag, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _check_mask(x, tag, dtypes=(np.int32, np.float32)):
    want, filled = F.fill_mask(x)
    for dt in dtypes:
        out, cnt = _run([x], MASK, dtype=dt)
        _same(out[0], want, (tag, np.dtype(dt).name))
        assert cnt[0] == filled, (tag, cnt[0], filled)
    return filled


def _check_label(x, classes, tag, **kw):
    want, filled = F.fill_label(x, classes)
    out, cnt = _run([x], LABEL, classes, **kw)
    _same(out[0], want, tag)
    if cnt is not None:
        assert cnt[0] == filled, (tag, cnt[0], filled)
    return filled


# ---- 1. the mask form --------------------------------------------------------------------------------------------------------
def test_tiny_and_boundary_shapes():
    for value in (0, 1):
        assert _check_mask(np.full((1, 1, 1), value, np.int32), "1x1x1") == 0
    x = np.ones((3, 3, 3), np.int32)
    x[1, 1, 1] = 0
    assert _check_mask(x, "3x3x3 centre") == 1
    assert _check_label(7 * x, None, "3x3x3 centre label") == 1
    for shape in [(1, 7, 40), (12, 1, 70), (4, 8, 32), (5, 9, 33), (9, 17, 65)]:
        _check_mask(np.zeros(shape, np.int32), ("zeros", shape))
        _check_mask(np.ones(shape, np.int32), ("ones", shape))
        filled = _check_mask(F.binary_noise(shape, 0.62, 3), ("noise", shape))
        assert (filled == 0) == (1 in shape), (shape, filled)


@pytest.mark.parametrize("density", [0.5, 0.62, 0.75, 0.9])
@pytest.mark.parametrize("shape", [(4, 8, 32), (5, 9, 33), (9, 17, 65)])
def test_random_binary_volumes(shape, density):
    x = F.binary_noise(shape, density, int(density * 100) + shape[2])
    _check_mask(x, (shape, density), dtypes=(np.int32,))
    # float32: scaled values, a -0.0 inside a hole and a NaN in a wall
    want, filled = F.fill_mask(x)
    f = x.astype(np.float32) * np.float32(-2.5)
    holes = np.argwhere((want == 1) & (x == 0))
    walls = np.argwhere(x != 0)
    if len(holes):
        f[tuple(holes[0])] = -0.0
    f[tuple(walls[len(walls) // 2])] = np.nan
    assert np.array_equal(F.fill_mask(f)[0], want)
    out, cnt = _run([f], MASK, dtype=np.float32)
    _same(out[0], want, (shape, density, "float32"))
    assert cnt[0] == filled


def test_float_zero_rule():
    x = np.ones((5, 5, 5), np.float32)
    x[2, 2, 2] = -0.0
    x[2, 2, 3] = np.nan
    x[2, 2, 4] = 0.0
    out, cnt = _run([x], MASK, dtype=np.float32)
    _same(out[0], F.fill_mask(x)[0], "zero rule")
    assert cnt[0] == 1 and out[0, 2, 2, 2] == 1 and out[0, 2, 2, 3] == 1 and out[0, 2, 2, 4] == 0


def test_hand_built_volumes():
    assert _check_mask(F.hollow_box(), "hollow box") == 6 * 12 * 59
    assert _check_mask(F.box_with_corridor(), "corridor") == 0
    assert _check_mask(F.box_with_diagonal_leak(), "diagonal leak") == 6 * 12 * 54
    assert _check_mask(F.serpentine_corridor(reach_border=True), "serpentine to the border") == 0
    assert _check_mask(F.serpentine_corridor(reach_border=False), "serpentine, one voxel short") > 3000
    for build in (F.hollow_box, F.box_with_corridor, F.box_with_diagonal_leak):
        _check_label(build(value=255), None, build.__name__)
    _check_label(F.serpentine_corridor(reach_border=False, value=-9), None, "serpentine label")


def test_batch_volumes_are_independent():
    shape = (9, 17, 65)
    vols = [F.binary_noise(shape, 0.7, s) for s in (1, 2, 3)]
    vols[0][-1] = 0                # an all-zero last slice of volume 0 lies against ...
    vols[1][0] = 0                 # ... an all-zero first slice of volume 1 in memory
    vols[1][-1] = 1
    vols[2][0] = 1                 # and two solid slices: an enclosure that exists only across the volumes
    vols[1][-2, 5, 5] = 0
    want = [F.fill_mask(v) for v in vols]
    out, cnt = _run(vols, MASK)
    for i in range(3):
        _same(out[i], want[i][0], ("batch", i))
        assert cnt[i] == want[i][1], (i, cnt, [w[1] for w in want])
    assert len(set(int(c) for c in cnt)) == 3, "the three counts differ, so a swapped or summed count would show"
    lab = [F.label_noise(shape, 3, s) for s in (4, 5, 6)]
    out, cnt = _run(lab, LABEL, [1, 3])
    for i in range(3):
        w, f = F.fill_label(lab[i], [1, 3])
        _same(out[i], w, ("label batch", i))
        assert cnt[i] == f


def test_one_thousand_tiles():
    x = F.binary_noise((64, 128, 128), 0.62, 9)
    want, filled = F.fill_mask(x)
    out, cnt = _run([x], MASK)
    _same(out[0], want, "64x128x128")
    assert cnt[0] == filled and filled > 10000


# ---- 2. the label form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,classes", [(3, None), (3, [2]), (4, [1, 2]), (4, None), (20, None), (20, [3, 7, 8, 19]), (20, [11])])
def test_label_form(C_, classes):
    shape = (9, 17, 65)
    x = F.label_noise(shape, C_, 40 + C_)
    k = F.kinds(x, classes)
    assert k[F.BORDER] and k[F.MIXED]
    filled = _check_label(x, classes, ("label", C_, classes))
    assert (filled > 0) == (k[F.SINGLE] > 0)
    _check_label(x, classes, ("label in place", C_, classes), inplace=True)
    _check_label(x, classes, ("label without counts", C_, classes), counts=False)
    _check_label(x, classes, ("label in place without counts", C_, classes), inplace=True, counts=False)
    big = np.where(x == 1, np.int32(255), x)
    _check_label(big, None, ("label 255", C_))


def test_label_form_on_a_binary_mask_is_the_mask_form():
    x = F.binary_noise((9, 17, 65), 0.75, 77)
    out, cnt = _run([x], LABEL)
    want, filled = F.fill_mask(x)
    _same(out[0], want, "binary label")
    assert cnt[0] == filled and filled > 0


def test_argument_errors_are_reported_before_any_launch():
    from medicalseg_amd._lib import MskError
    x = F.binary_noise((4, 8, 32), 0.7, 1)
    src, fsrc, dst, st = _ivec(x), vec(x.astype(np.float32)), dmalloc(x.size * 4), _ivec([5])
    cls = np.arange(1, 66, dtype=np.int32)
    cp = cls.ctypes.data_as(C.c_void_p)

    def call(s, d, dims, dtype, mode, classes, ncls, status=st):
        dev().call("msk_fill_holes3d", vp(s), vp(d), 1, *dims, dtype, mode, classes, ncls, vp(status), None)

    for args in [(fsrc, dst, x.shape, 0, LABEL, None, 0), (src, dst, x.shape, 2, MASK, None, 0),
                 (src, dst, x.shape, 1, 3, None, 0), (src, dst, (0, 8, 32), 1, MASK, None, 0),
                 (src, dst, x.shape, 1, LABEL, cp, 65), (src, dst, x.shape, 1, MASK, cp, 2),
                 (src, dst, x.shape, 1, LABEL, None, 2), (src, 0, x.shape, 1, MASK, None, 0),
                 (src, dst, x.shape, 1, MASK, None, 0, 0), (src, src + 64, x.shape, 1, MASK, None, 0),
                 (fsrc, fsrc, x.shape, 0, MASK, None, 0), (src, dst, (1024, 1024, 1024), 1, MASK, None, 0)]:
        with pytest.raises(MskError):
            call(*args)
    assert vec_back(st, 1, np.int32)[0] == 5, "nothing was launched"
    assert np.array_equal(vec_back(src, x.size, np.int32).reshape(x.shape), x)


# ---- 3. the Python surface ---------------------------------------------------------------------------------------------------
SMALL = (5, 9, 33)


def test_fill_holes_device_on_volumes_and_tensors():
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.device import IntTensor, to_tensor
    x = F.label_noise(SMALL, 3, 8)
    for classes in (None, [1, 2]):
        v = pp.upload_pooled(x)
        out = pp.fill_holes_device(v, classes)
        assert isinstance(out, pp.DeviceVolume) and out.dtype == np.int32 and out.ptr != v.ptr
        _same(out.numpy(), F.fill_label(x, classes)[0], ("volume", classes))
        assert np.array_equal(v.numpy(), x), "the input volume was modified"
        out.free()
        v.free()
    b = F.binary_noise(SMALL, 0.7, 2)
    for arr in (b, b.astype(np.float32)):
        v = pp.upload_pooled(arr)
        out = pp.fill_holes_device(v, binary=True)
        _same(out.numpy(), F.fill_mask(b)[0], ("binary", arr.dtype))
        out.free()
        v.free()
        _same(pp.fill_holes(arr, binary=True), F.fill_mask(b)[0], "host array")
    v = pp.upload_pooled(b.astype(np.float32))
    with pytest.raises(ValueError, match="binary=True"):
        pp.fill_holes_device(v)
    v.free()
    batch = np.stack([F.label_noise(SMALL, 3, s) for s in (1, 2, 3)])[:, None]
    t = to_tensor(batch)
    out = pp.fill_holes_device(t, [1, 3])
    assert isinstance(out, IntTensor) and out.shape == t.shape and out.ptr != t.ptr
    _same(out.numpy(), pp.fill_holes_host(batch, [1, 3]), "IntTensor")
    assert np.array_equal(t.numpy(), batch), "the input tensor was modified"


def _pocket_volume():
    x = (np.random.default_rng(3).standard_normal((8, 12, 40)) * 40 + 200).astype(np.float32)
    x[:2] = 0
    x[:, :, :3] = 0
    x[4:6, 5:8, 20:30] = 0          # an enclosed pocket
    x[3, 3, 36:] = 0                # a channel to the face
    return x


def test_nonzero_mask_device():
    from medicalseg_amd import preprocess as pp
    x = _pocket_volume()
    v = pp.upload_pooled(x)
    for fill in (True, False):
        m = pp.nonzero_mask_device(v, fill_holes=fill)
        assert m.dtype == np.int32 and m.shape == v.shape
        _same(m.numpy(), pp.nonzero_mask_host(x, fill_holes=fill), ("nonzero mask", fill))
        m.free()
    assert F.fill_mask(x)[1] == 60
    v.free()


def test_chain_zscore_under_the_filled_mask_matches_the_host_bit_for_bit():
    from medicalseg_amd import preprocess as pp
    x = _pocket_volume()
    pipe = pp.DevicePipeline(pooled=True)
    for q in (None, (0.5, 99.5)):
        want = pp.zscore_normalize(x, q, "nonzero", fill_holes=True, on_device=False)
        chain = pipe.image(x).zscore(q, "nonzero", fill_holes=True)
        got = chain.numpy()
        chain.vol.free()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), q
        dev_arr = pp.zscore_normalize(x, q, "nonzero", fill_holes=True)
        assert np.array_equal(dev_arr.view(np.uint32), want.view(np.uint32)), q
        plain = pipe.image(x).zscore(q, "nonzero")
        assert not np.array_equal(plain.numpy(), got)
        plain.vol.free()


def test_fill_holes_transform_on_device_inputs():
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.device import IntTensor, to_tensor
    from medicalseg_amd.transforms import transform as T
    x, y = F.label_noise(SMALL, 3, 11), F.label_noise(SMALL, 4, 12)
    op = T.FillHoles3D([1, 2])
    hp, hl = op(x, y)
    dp, dl = op(pp.upload_pooled(x), pp.upload_pooled(y))
    assert isinstance(dp, pp.DeviceVolume) and isinstance(dl, pp.DeviceVolume)
    _same(dp.numpy(), hp, "pred")
    _same(dl.numpy(), hl, "label")
    dp.free()
    dl.free()
    # behind the largest-component transform, as a pred_transform chain on a prediction tensor
    m = F.hollow_box()
    m[0, 0, 0] = 1
    t = to_tensor(np.stack([m, F.binary_noise(m.shape, 0.8, 5)])[:, None])
    top, _ = T.TopkLargestConnectComponent(k=1)(t)
    out, _ = T.FillHoles3D()(top)
    assert isinstance(out, IntTensor)
    got = out.numpy()
    for i, vol in enumerate(t.numpy()[:, 0]):
        want, _ = T.FillHoles3D()(T.TopkLargestConnectComponent(k=1)(vol)[0])
        _same(got[i, 0], want.astype(np.int32), ("top-1 then fill", i))
    assert got[0, 0].sum() == 8 * 14 * 61

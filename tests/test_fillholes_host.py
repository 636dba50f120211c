"""Hole filling without a GPU: the statement tests/fillholes_reference.py against scipy.ndimage.binary_fill_holes and against its
own flood-fill form, the crop property that makes crop_to_nonzero + hole filling nnU-Net's "fill, then crop", the label form's
four kinds of zero component, the host paths of medicalseg_amd built on it, and the C ABI's declaration.  Everything is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.ndimage

import fillholes_reference as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, d) for s in F.SHAPES for d in F.DENSITIES]


def _body_with_pockets(shape, seed, margin=3):
    """a smooth body surrounded by a zero margin, with interior zero pockets and a few zero channels to the outside"""
    rng = np.random.default_rng(seed)
    f = scipy.ndimage.uniform_filter(rng.random(shape), size=5, mode="nearest")
    x = (rng.standard_normal(shape) * 50 + 300).astype(np.float32)
    x[f < np.quantile(f, 0.25)] = 0
    x[rng.random(shape) < 0.1] = 0
    out = np.zeros(shape, np.float32)
    inner = tuple(slice(margin, s - margin + (i % 2)) for i, s in enumerate(shape))
    out[inner] = x[inner]
    return out


# ---- 1. the statement --------------------------------------------------------------------------------------------------------
def test_mask_form_is_binary_fill_holes():
    total = 0
    for i, (shape, density) in enumerate(CASES):
        x = F.binary_noise(shape, density, i)
        got, filled = F.fill_mask(x)
        want = scipy.ndimage.binary_fill_holes(x != 0)
        assert got.dtype == np.int32 and np.array_equal(got, want.astype(np.int32)), (shape, density)
        assert filled == np.count_nonzero(want) - np.count_nonzero(x), (shape, density)
        if 1 in shape:
            assert filled == 0, "an axis of extent 1 admits no hole"
        loop, loop_filled = F.fill_loop(x, binary=True)
        assert np.array_equal(loop, got) and loop_filled == filled
        lab, lab_filled = F.fill_label(x)
        assert np.array_equal(lab, got) and lab_filled == filled, "on a binary mask the label form is the mask form"
        total += filled
    assert total > 0


def test_extent_two_admits_no_hole():
    for shape in ((2, 9, 9), (9, 2, 9), (9, 9, 2)):
        x = np.ones(shape, np.int32)
        x[tuple(s // 2 for s in shape)] = 0
        assert F.fill_mask(x)[1] == 0


def test_float_zero_rule():
    x = np.ones((5, 5, 5), np.float32)
    x[2, 2, 2] = -0.0                      # a zero: a hole
    x[2, 2, 3] = np.nan                    # non-zero: a wall
    x[2, 2, 4] = 0.0                       # on the face, cut off from the hole by the NaN
    got, filled = F.fill_mask(x)
    assert filled == 1 and got[2, 2, 2] == 1 and got[2, 2, 3] == 1 and got[2, 2, 4] == 0


@pytest.mark.parametrize("seed", range(4))
def test_crop_then_fill_is_fill_then_crop(seed):
    from medicalseg_amd import preprocess as pp
    x = _body_with_pockets([(14, 20, 40), (9, 17, 65), (16, 16, 16), (12, 30, 21)][seed], seed)
    box = pp.nonzero_bbox_host(x)
    sl = tuple(slice(int(a), int(b)) for a, b in zip(box[:3], box[3:6]))
    whole, filled = F.fill_mask(x)
    assert filled > 0 and any(s.start > 0 for s in sl)
    assert np.array_equal(whole[sl], F.fill_mask(x[sl])[0])
    cropped, _, _ = pp.crop_to_nonzero(x, on_device=False)
    assert np.array_equal(pp.nonzero_mask_host(cropped), whole[sl])


# ---- 2. the label form -------------------------------------------------------------------------------------------------------
def test_label_form_hand_made():
    x = np.zeros((7, 9, 9), np.int32)
    x[1:6, 1:8, 1:8] = 1
    x[2:5, 2:7, 2:7] = 2
    x[3, 3:6, 3:6] = 0                     # inside 2, itself inside 1: becomes 2
    got, filled = F.fill_label(x)
    assert filled == 9 and (got[3, 3:6, 3:6] == 2).all() and np.array_equal(got != x, (x == 0) & (got == 2))
    # a hole that touches two labels stays
    y = x.copy()
    y[2, 4, 4] = 0                         # opens the pocket towards label 1 at (1, 4, 4)
    got, filled = F.fill_label(y)
    assert filled == 0 and np.array_equal(got, y)
    assert F.kinds(y)[F.MIXED] == 1
    # classes excluding the encloser
    got, filled = F.fill_label(x, classes=[1])
    assert filled == 0 and np.array_equal(got, x) and F.kinds(x, [1])[F.EXCLUDED] == 1
    got, filled = F.fill_label(x, classes=[1, 2])
    assert filled == 9
    # any non-zero int32 value encloses: 255, a negative one
    for value in (255, -3, 2 ** 31 - 1, -2 ** 31):
        z = np.where(x == 2, np.int32(value), x).astype(np.int32)
        got, filled = F.fill_label(z)
        assert filled == 9 and (got[3, 3:6, 3:6] == value).all(), value
        assert np.array_equal(F.fill_loop(z)[0], got)


LABEL_CASES = [((9, 17, 65), 4, [1, 2]), ((9, 17, 65), 3, None), ((5, 9, 33), 4, [3]), ((9, 17, 65), 20, [7, 8, 9]),
               ((12, 1, 70), 3, None)]


def test_label_form_random_volumes_hold_all_four_kinds():
    seen = dict.fromkeys((F.BORDER, F.SINGLE, F.MIXED, F.EXCLUDED), 0)
    for i, (shape, C, classes) in enumerate(LABEL_CASES):
        x = F.label_noise(shape, C, 100 + i)
        got, filled = F.fill_label(x, classes)
        loop, loop_filled = F.fill_loop(x, classes)
        assert np.array_equal(got, loop) and filled == loop_filled, (shape, C, classes)
        assert filled == np.count_nonzero(got != x)
        for k, v in F.kinds(x, classes).items():
            seen[k] += v
    assert all(v > 0 for v in seen.values()), seen


# ---- 3. host paths -----------------------------------------------------------------------------------------------------------
def test_fill_holes_host_is_the_statement():
    from medicalseg_amd import preprocess as pp
    for i, (shape, density) in enumerate(CASES[::3]):
        x = F.binary_noise(shape, density, i)
        for arr in (x, x.astype(np.float32), x.astype(np.uint8)):
            got = pp.fill_holes_host(arr, binary=True)
            assert got.dtype == np.int32 and np.array_equal(got, F.fill_mask(x)[0])
        assert np.array_equal(pp.fill_holes(x, binary=True, on_device=False), F.fill_mask(x)[0])
        assert np.array_equal(pp.nonzero_mask_host(x.astype(np.float32)), F.fill_mask(x)[0])
        assert np.array_equal(pp.nonzero_mask_host(x, fill_holes=False), (x != 0).astype(np.int32))
    for i, (shape, C, classes) in enumerate(LABEL_CASES):
        x = F.label_noise(shape, C, 100 + i)
        assert np.array_equal(pp.fill_holes_host(x, classes), F.fill_label(x, classes)[0])
    batch = np.stack([F.label_noise((5, 9, 33), 3, s) for s in (1, 2)])[:, None]
    got = pp.fill_holes_host(batch, [1, 3])
    assert got.shape == batch.shape
    for i in range(2):
        assert np.array_equal(got[i, 0], F.fill_label(batch[i, 0], [1, 3])[0])


def test_zscore_under_the_filled_mask_host():
    from medicalseg_amd import preprocess as pp
    x = _body_with_pockets((14, 20, 40), 7)
    mask, filled = F.fill_mask(x)
    assert filled > 0
    for q in (None, (0.5, 99.5)):
        got = pp.zscore_normalize(x, q, "nonzero", fill_holes=True, on_device=False)
        want = pp.zscore_normalize(x, q, "mask", mask=mask, on_device=False)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        plain = pp.zscore_normalize(x, q, "nonzero", on_device=False)
        assert not np.array_equal(got, plain)
        hole = (mask == 1) & (x == 0)
        assert (plain[hole] == 0).all() and (got[hole] != 0).all(), "an enclosed zero is z-scored, not set to 0"
        assert np.array_equal(pp.zscore_normalize(x, q, "nonzero", fill_holes=False, on_device=False), plain)


def test_fill_holes_transform_on_numpy():
    from medicalseg_amd.cvlibs import manager
    from medicalseg_amd.transforms import transform as T
    assert manager.TRANSFORMS["FillHoles3D"] is T.FillHoles3D
    x = F.label_noise((9, 17, 65), 4, 5)
    for dtype in (np.uint8, np.int64, np.int32):
        for classes in (None, [1, 2], 2):
            pred, label = T.FillHoles3D(classes)(x.astype(dtype), x.astype(dtype))
            want = F.fill_label(x, None if classes is None else np.atleast_1d(classes))[0]
            assert pred.dtype == dtype and label.dtype == dtype
            assert np.array_equal(pred, want) and np.array_equal(label, want)
    pred, label = T.FillHoles3D()(x)
    assert label is None
    # composes behind the largest-component transform on a binary prediction
    m = F.hollow_box()
    m[0, 0, 0] = 1
    top, _ = T.TopkLargestConnectComponent(k=1)(m.copy())
    out, _ = T.FillHoles3D()(top)
    assert out.dtype == top.dtype and out[0, 0, 0] == 0 and out.sum() == 8 * 14 * 61


# ---- 4. ABI and argument errors ----------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_in_the_table():
    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    assert re.search(r"#define MSK_FILL_MASK 0\b", txt) and re.search(r"#define MSK_FILL_LABEL 1\b", txt)
    decl = re.search(r"int msk_fill_holes3d\(([^;]*)\);", txt)
    assert decl and re.sub(r"\s+", " ", decl.group(1)) == (
        "msk_ctx* ctx, const void* src, int32_t* dst, int n, int d, int h, int w, int dtype, int mode, "
        "const int32_t* classes, int nclasses, int32_t* status, int32_t* counts")
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "msk_fill_holes3d")
    res, args = _lib.SIGNATURES["msk_fill_holes3d"]
    assert res is ctypes.c_int and len(args) == 13
    from medicalseg_amd import preprocess as pp
    assert (pp.FILL_MASK, pp.FILL_LABEL) == (0, 1)


def test_wrappers_raise_the_stated_errors():
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.transforms import transform as T
    x = np.ones((4, 5, 6), np.float32)
    with pytest.raises(ValueError, match="binary=True"):
        pp.fill_holes_host(x)
    with pytest.raises(ValueError, match="binary=True"):
        pp.fill_holes(x)                                   # refused before anything is uploaded
    with pytest.raises(ValueError, match="at most 64 classes"):
        pp.fill_holes_host(x.astype(np.int32), classes=list(range(65)))
    with pytest.raises(ValueError, match="at most 64 classes"):
        T.FillHoles3D(classes=list(range(1, 66)))
    with pytest.raises(ValueError, match="takes no classes"):
        pp.fill_holes_host(x, classes=[1], binary=True)
    for bad in (np.ones((4, 5), np.int32), np.ones((2, 2, 4, 5, 6), np.int32), np.ones((1, 4, 5, 6), np.int32)):
        with pytest.raises(ValueError, match="expected a 3-D volume"):
            pp.fill_holes_host(bad)
    with pytest.raises(ValueError, match="expected a 3-D volume"):
        pp.fill_holes(np.ones((4, 5), np.int32))
    with pytest.raises(ValueError, match="expected a 3-D volume"):
        pp.nonzero_mask_host(np.ones(7, np.float32))
    with pytest.raises(TypeError, match="3-D DeviceVolume"):
        pp.nonzero_mask_device(x)
    with pytest.raises(TypeError, match="DeviceVolume or an IntTensor"):
        pp.fill_holes_device(x)
    for mode, mask in (("all", None), ("mask", np.ones(x.shape, np.int32))):
        for on_device in (False, True):                    # refused before anything is uploaded
            with pytest.raises(ValueError, match="needs mode 'nonzero'"):
                pp.zscore_normalize(x, mode=mode, mask=mask, fill_holes=True, on_device=on_device)
    with pytest.raises(ValueError, match="needs mode 'nonzero'"):
        pp._Chain(None, None).zscore(mode="all", fill_holes=True)
    assert sorted(pp.MASK_MODES) == ["all", "mask", "nonzero"]

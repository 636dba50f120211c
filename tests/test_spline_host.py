"""Order-3 resampling without a GPU: the statement of tests/spline_reference.py against scipy.ndimage.zoom, the host path
(transforms.transform._spline_zoom_host) against the statement (equal arrays), the statement against the goldens captured
from the reference's own resize_3d / resample, RandomLowResolution3D on host arrays, and the C ABI surface."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import scipy.ndimage

import spline_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = R.GOLDEN
PAIRS = [((9, 14, 11), (12, 7, 20)), ((1, 5, 3), (4, 5, 1)), ((2, 2, 2), (5, 1, 3)), ((3, 4, 41), (3, 9, 17)),
         ((12, 16, 16), (24, 32, 32)), ((20, 24, 28), (8, 8, 8)), ((6, 6, 6), (6, 6, 6))]
CROP = ((10, 12, 16), (2, 3, 5, 6, 7, 9), (8, 8, 8))


def _volume(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape) * 400.0 - 300.0


def _scipy(x, out_shape):
    return scipy.ndimage.zoom(x, np.array(out_shape) / np.array(x.shape), order=3, mode="nearest")


@pytest.mark.parametrize("sin,sout", PAIRS)
def test_statement_agrees_with_scipy_on_float64(sin, sout):
    x = _volume(sin, 11)
    want = _scipy(x, sout)
    got = R.spline_zoom_f64(x, sout)
    assert got.shape == want.shape == tuple(sout) and got.dtype == np.float64
    err = np.abs(got - want).max() / np.abs(x).max()
    print(sin, sout, "max err / max|x|", err)
    assert err <= 1e-12


def test_statement_agrees_with_scipy_on_a_crop_box():
    shape, box, sout = CROP
    x = _volume(shape, 12)
    i, j, k, d, h, w = box
    inner = x[i:i + d, j:j + h, k:k + w].copy()
    x[:i], x[i + d:], x[:, :j], x[:, j + h:], x[:, :, :k], x[:, :, k + w:] = (1e6,) * 6   # nothing outside the box is read
    want = _scipy(inner, sout)
    got = R.spline_zoom_f64(x[i:i + d, j:j + h, k:k + w], sout)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(inner).max()
    assert np.array_equal(R.spline_crop_zoom(x.astype(np.float32), box, sout), R.spline_zoom(inner.astype(np.float32), sout))


def test_statement_constants_are_what_the_docstring_says():
    assert R.PAD == 12 and R.HORIZON == 47
    assert R.Z == np.sqrt(3.0) - 2.0 and R.GAIN == (1 - R.Z) * (1 - 1 / R.Z) and R.LAST == R.Z / (R.Z * R.Z - 1)
    zn1, rden = R.axis_constants(25)
    assert abs(zn1 - R.Z ** 24) <= 1e-15 * abs(R.Z ** 24) * 24 and rden == 1.0 / (1.0 - zn1 * zn1)
    assert R.axis_constants(5000) == (0.0, 1.0)                      # the running product underflows, nothing divides by 0


@pytest.mark.parametrize("sin,sout", PAIRS + [((3, 4, 300), (3, 4, 150))])
def test_host_function_equals_the_statement(sin, sout):
    from medicalseg_amd.transforms.transform import _spline_zoom_host
    x = _volume(sin, 13).astype(np.float32)
    got = _spline_zoom_host(x, sout)
    assert got.dtype == np.float32 and np.array_equal(got, R.spline_zoom(x, sout))


def test_statement_against_the_reference_goldens():
    unequal = total = 0
    for name, img, shape, want in R.golden_cases():
        unequal += R.assert_within_golden_tolerance(R.spline_zoom(img, shape), img, want, name)
        total += want.size
    assert unequal <= 0.01 * total, (unequal, total)


def test_golden_file_is_the_references_order_3():
    """scipy itself reproduces the fixture, and order 1 does not: the file holds what its maker says"""
    for name, img, shape, want in R.golden_cases():
        assert np.array_equal(_scipy(img, shape), want), name
    name, img, shape, want = R.golden_cases()[0]
    assert not np.array_equal(scipy.ndimage.zoom(img, np.array(shape) / np.array(img.shape), order=1, mode="nearest"), want)
    g = np.load(GOLDEN)
    assert g["rz0_size"].tolist() == [9] and g["rz0_out"].shape == (10, 13, 9)      # int size: the shortest side, aspect kept
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_low_resolution_draws_a_fixed_stream_and_leaves_the_label():
    from medicalseg_amd import transforms as T
    from medicalseg_amd.transforms.transform import _nearest_zoom_host, _spline_zoom_host
    img = _volume((9, 12, 10), 14).astype(np.float32)
    label = (np.arange(img.size) % 3).astype(np.int32).reshape(img.shape)
    for per_axis, draws in ((False, 2), (True, 4)):
        states = []
        for prob in (0.0, 1.0):
            random.seed(5)
            out, lab = T.RandomLowResolution3D(prob=prob, zoom=(0.4, 0.8), per_axis=per_axis)(img.copy(), label)
            states.append(random.getstate())
            assert lab is label and out.shape == img.shape and out.dtype == np.float32
            assert np.array_equal(out, img) == (prob == 0.0)
        assert states[0] == states[1]                                 # the same draws whether or not the coin hits
        random.seed(5)
        u = [random.random() for _ in range(draws)]
        assert random.getstate() == states[0]
        zooms = [0.4 + (0.8 - 0.4) * v for v in (u[1:] if per_axis else u[1:] * 3)]
        small = tuple(max(1, int(round(n * z))) for n, z in zip(img.shape, zooms))
        want = _spline_zoom_host(_nearest_zoom_host(img, small), img.shape)
        assert np.array_equal(out, want)                              # `out` is the prob = 1 result
        assert np.array_equal(want, R.spline_zoom(scipy.ndimage.zoom(img, np.array(small) / np.array(img.shape), order=0,
                                                                     mode="nearest"), img.shape))
    random.seed(6)
    same = img.copy()
    out, _ = T.RandomLowResolution3D(prob=0.0)(same)
    assert out is same                                                # prob = 0 returns its input
    t = T.RandomLowResolution3D()
    assert (t.prob, t.zoom, t.per_axis) == (0.25, (0.5, 1.0), False)
    tiny, _ = T.RandomLowResolution3D(prob=1.0, zoom=(0.01, 0.01))(img.copy())   # every axis shrinks to one voxel
    assert tiny.shape == img.shape and np.allclose(tiny, img[0, 0, 0], rtol=1e-6, atol=0)


@pytest.mark.parametrize("kw", [{"prob": -0.1}, {"prob": 1.5}, {"zoom": (0.0, 0.5)}, {"zoom": (0.5, 1.5)}, {"zoom": (0.8, 0.4)},
                                {"zoom": (0.5,)}, {"zoom": "half"}])
def test_low_resolution_rejects_bad_arguments(kw):
    from medicalseg_amd import transforms as T
    with pytest.raises(ValueError):
        T.RandomLowResolution3D(**kw)


def test_header_ctypes_table_and_library_carry_the_entry_points():
    from medicalseg_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msegk.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in {"msk_spline_workspace": 4, "msk_spline_resample3d": 17}.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name + " is not declared in include/msegk.h"
        assert len(m.group(1).split(",")) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert hasattr(lib, name), "libmsegk.so does not export " + name
    assert _lib.SIGNATURES["msk_spline_resample3d"][1][-1] is ctypes.c_size_t


def test_workspace_answers_without_a_gpu():
    from medicalseg_amd import _lib
    lib = _lib.load()
    b = ctypes.c_size_t(0)
    for sd, sh, sw in ((1, 1, 1), (9, 14, 11), (48, 48, 48), (300, 512, 512), (1008, 1008, 12)):
        assert lib.msk_spline_workspace(sd, sh, sw, ctypes.byref(b)) == 0
        need = (sd + 24) * (sh + 24) * (sw + 24) * 8
        assert need <= b.value < need + 4096
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2 ** 31 - 1, 1, 1), (2000, 2000, 2000)):
        assert lib.msk_spline_workspace(*bad, ctypes.byref(b)) != 0
        assert lib.msk_last_error(None)
    assert lib.msk_spline_workspace(4, 4, 4, None) != 0


def test_the_shipped_configuration_builds_its_transforms():
    from medicalseg_amd import transforms as T
    from medicalseg_amd.cvlibs import Config, manager
    assert manager.TRANSFORMS["RandomLowResolution3D"] is T.RandomLowResolution3D
    ds = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_lowres_96.yml")).train_dataset
    ops = ds.transforms.transforms
    assert [type(o) for o in ops] == [T.RandomPatchCrop3D, T.RandomGaussianNoise3D, T.RandomGaussianBlur3D, T.RandomBrightness3D,
                                      T.RandomContrast3D, T.RandomGamma3D, T.RandomLowResolution3D]
    assert ds.transforms.device and (ops[6].prob, ops[6].zoom, ops[6].per_axis) == (0.25, (0.5, 1.0), False)


def test_device_wrappers_refuse_what_is_not_built():
    """the order and dtype checks come before anything touches the device"""
    from medicalseg_amd import preprocess as pp
    f32 = pp.DeviceVolume(None, 0, (4, 4, 4), np.float32)
    i32 = pp.DeviceVolume(None, 0, (4, 4, 4), np.int32)
    for order in (2, 4, 5):
        with pytest.raises(ValueError, match="0, 1 and 3"):
            pp.resample_device(f32, (5, 5, 5), order)
        with pytest.raises(ValueError, match="0, 1 and 3"):
            pp.resized_crop_device(f32, 0, 0, 0, 4, 4, 4, (5, 5, 5), order)
    with pytest.raises(ValueError, match="float32"):
        pp.resample_device(i32, (5, 5, 5), 3)
    with pytest.raises(ValueError, match="float32"):
        pp.resized_crop_device(i32, 0, 0, 0, 4, 4, 4, (5, 5, 5), 3)

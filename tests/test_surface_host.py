"""Surface-distance metrics without a GPU: the numpy specification of utils.metric (surface_mask, edt_squared,
surface_distances, surface_metrics) against the independent restatements of tests/surface_reference.py -- scipy's
erosion, a brute-force loop over the feature voxels, scipy's distance and feature transforms -- with == wherever both
sides are exact, the C ABI surface of msk_edt3d / msk_surface_count / msk_surface_gather, and the new keywords of
evaluate / val.py."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import surface_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks(shape, seed):
    rng = np.random.default_rng(seed)
    one = np.zeros(shape, bool)
    one[tuple(int(rng.integers(0, s)) for s in shape)] = True
    return {"random": rng.random(shape) < 0.5, "sparse": rng.random(shape) < 0.02, "blob": R.blob_mask(shape, seed),
            "full": np.ones(shape, bool), "empty": np.zeros(shape, bool), "single": one}


@pytest.mark.parametrize("shape", [(9, 10, 11), (1, 7, 9), (6, 1, 5), (5, 4, 1), (1, 1, 6), (1, 1, 1), (2, 2, 2)])
def test_surface_mask_is_mask_minus_its_erosion(shape):
    from medicalseg_amd.utils import metric
    for name, m in _masks(shape, 3).items():
        got = metric.surface_mask(m)
        assert got.dtype == bool and np.array_equal(got, R.surface(m)), (shape, name)
        assert np.array_equal(metric.surface_mask(m.astype(np.int32)), got)


@pytest.mark.parametrize("spacing", [None] + R.ANISO + [(0.5, 1.25, 3.0)])
@pytest.mark.parametrize("shape", [(7, 8, 9), (1, 6, 13), (5, 1, 4), (4, 9, 1), (1, 1, 1), (3, 17, 5)])
def test_edt_squared_equals_the_brute_force_minimum(shape, spacing):
    from medicalseg_amd.utils import metric
    for name, f in _masks(shape, 5).items():
        got = metric.edt_squared(f, spacing)
        want = R.edt2_brute(f, spacing)
        assert got.dtype == np.float64 and got.shape == tuple(shape)
        assert np.array_equal(got, want), (shape, spacing, name, float(np.nanmax(np.abs(got - want))))
        if name == "empty":
            assert np.all(np.isposinf(got))
        assert np.array_equal(metric.edt_squared(f, spacing, surface_only=True), R.edt2_brute(R.surface(f), spacing))


@pytest.mark.parametrize("shape", [(24, 31, 40), (3, 64, 80), (40, 40, 40)])
def test_edt_squared_against_scipy(shape):
    from medicalseg_amd.utils import metric
    for name, f in _masks(shape, 7).items():
        if name == "empty":
            continue
        got = metric.edt_squared(f)
        assert np.array_equal(got, np.rint(R.scipy_edt2(f))), (shape, name)      # unit spacing: exact integers
        assert np.array_equal(got, R.scipy_int_edt2(f).astype(np.float64)), (shape, name)
        for spacing in R.ANISO:
            got, want = metric.edt_squared(f, spacing), R.scipy_edt2(f, spacing)
            rel = np.abs(got - want) / np.maximum(want, np.finfo(np.float64).tiny)
            print("aniso", shape, name, spacing, "max rel", float(rel.max()))
            assert np.all(np.abs(got - want) <= R.SCIPY_RTOL * want), (shape, name, spacing, float(rel.max()))


def test_spacing_is_validated():
    from medicalseg_amd.utils import metric
    f = np.ones((2, 2, 2), bool)
    for bad in ((1, 1), (1, 0, 1), (1, -2, 1), (1, float("nan"), 1), (1, float("inf"), 1), (1e200, 1, 1)):
        with pytest.raises(ValueError):
            metric.edt_squared(f, bad)
    with pytest.raises(ValueError):
        metric.edt_squared(np.ones((2, 2), bool))
    with pytest.raises(ValueError):
        metric.surface_mask(np.ones((2, 2), bool))


def _cases():
    shape = (14, 20, 23)
    pred, label = R.blob_pair(shape, 4, 1)
    yield "blobs", pred, label, (1, 2, 3)
    cb = R.checkerboard(shape)
    yield "checkerboard vs blobs", cb, (label > 0).astype(np.int32), (1,)
    yield "checkerboard vs its complement", cb, 1 - cb, (0, 1)
    yield "noise", R.noise(shape, 2), R.noise(shape, 3), (0, 1)
    yield "identical", label, label.copy(), (0, 1, 2, 3)
    a, b = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    a[2:5, 3:8, 2:6] = 1
    b[9:13, 12:19, 15:22] = 1
    yield "disjoint", a, b, (0, 1)
    yield "thin", a[3:4], b[3:4] + a[3:4][:, ::-1, ::-1], (0, 1)


def test_metrics_equal_the_scipy_restatement():
    from medicalseg_amd.utils import metric
    for name, pred, label, classes in _cases():
        for c in classes:
            sd = metric.surface_distances(pred, label, c)
            assert np.all(np.diff(sd.d2_pl) >= 0) and np.all(np.diff(sd.d2_lp) >= 0)
            got = (sd.hd(), sd.hd95(), sd.assd())
            want = R.metrics_scipy(pred, label, c)
            print(name, c, got)
            assert got == want or (np.isnan(got).all() and np.isnan(want).all()), (name, c, got, want)
            assert sd.percentile(95) == sd.hd95() or sd.empty
            if not sd.empty:
                assert sd.percentile(100) == sd.hd()
        res = metric.surface_metrics(pred[None, None], label[None], int(max(classes)) + 1, classes=classes)
        for i, c in enumerate(classes):
            want = R.metrics_scipy(pred, label, c)
            for k, v in zip(("hd", "hd95", "assd"), want):
                assert res[k][i] == v or (np.isnan(res[k][i]) and np.isnan(v)), (name, c, k)
        assert res["classes"].tolist() == list(classes)


def test_hand_made_cases():
    from medicalseg_amd.utils import metric
    a, b = np.zeros((5, 9, 9), np.int32), np.zeros((5, 9, 9), np.int32)
    a[2, 4, 1] = 1
    b[2, 4, 5] = 1
    sd = metric.surface_distances(a, b, 1)
    assert sd.d2_pl.tolist() == [16.0] and sd.d2_lp.tolist() == [16.0]
    assert (sd.hd(), sd.hd95(), sd.assd()) == (4.0, 4.0, 4.0)
    sd = metric.surface_distances(a, b, 1, spacing=(3.0, 2.0, 0.5))        # the offset is along x
    assert (sd.hd(), sd.assd()) == (2.0, 2.0)
    b[2, 4, 5], b[4, 4, 1] = 0, 1                                            # ... now along z
    assert metric.surface_distances(a, b, 1, spacing=(3.0, 2.0, 0.5)).hd() == 6.0
    # identical masks: every distance is zero; the foreground default of surface_metrics is 1 .. C - 1
    res = metric.surface_metrics(b, b, 3)
    assert res["classes"].tolist() == [1, 2]
    assert res["hd"][0] == 0.0 and res["hd95"][0] == 0.0 and res["assd"][0] == 0.0
    assert np.isnan(res["hd"][1]) and np.isnan(res["hd95"][1]) and np.isnan(res["assd"][1])


def test_absent_class_is_nan_and_left_out_of_the_means():
    from medicalseg_amd.utils import metric
    pred, label = R.blob_pair((10, 12, 14), 3, 4)
    only_label = np.where(pred == 2, 0, pred)                     # class 2 absent from the prediction
    for p, l in ((only_label, label), (label, only_label)):
        sd = metric.surface_distances(p, l, 2)
        assert sd.empty and np.isnan(sd.hd()) and np.isnan(sd.hd95()) and np.isnan(sd.assd()) and np.isnan(sd.percentile(50))
    cases = [metric.surface_metrics(only_label, label, 3), metric.surface_metrics(pred, label, 3),
             metric.surface_metrics(np.zeros_like(pred), label, 3)]
    s = metric.surface_summary(cases)
    assert s["surface_nan"] == 3
    h = np.stack([c["hd95"] for c in cases])
    assert s["class_hd95"].tolist() == [float(np.mean(h[:2, 0])), float(h[1, 1])]
    assert s["hd95"] == float(np.mean([h[0, 0], np.mean(h[1])]))          # the all-nan case leaves the mean
    allnan = metric.surface_summary(cases[2:])
    assert np.isnan(allnan["hd95"]) and np.isnan(allnan["assd"]) and allnan["surface_nan"] == 2


def test_host_and_device_inputs_do_not_mix():
    from medicalseg_amd.preprocess import DeviceVolume
    from medicalseg_amd.utils import metric
    fake = DeviceVolume(None, 0, (2, 2, 2), np.int32)
    with pytest.raises(TypeError, match="both be device arrays or both be host arrays"):
        metric.surface_distances(fake, np.zeros((2, 2, 2), np.int32), 1)
    with pytest.raises(ValueError):
        metric.surface_distances(np.zeros((2, 1, 2, 2, 2), np.int32), np.zeros((2, 1, 2, 2, 2), np.int32), 1)
    with pytest.raises(ValueError, match="Shape of `pred` and `label should be equal"):
        metric.surface_distances(np.zeros((2, 2, 2), np.int32), np.zeros((2, 2, 3), np.int32), 1)


def test_header_ctypes_table_and_library_carry_the_entry_points():
    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    C = ctypes
    vp, i = C.c_void_p, C.c_int
    want = {"msk_edt3d": [vp, vp, i, i, i, i, i, vp, vp],
            "msk_surface_count": [vp, vp, i, i, i, i, vp],
            "msk_surface_gather": [vp, vp, i, i, i, i, vp, vp, C.c_long, vp]}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in want.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, "msegk.h does not declare " + name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args)
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and got == args
        assert hasattr(lib, name), "libmsegk.so does not export " + name
    m = re.search(r"#define\s+MSK_EDT_MAX_EXTENT\s+(\d+)", txt)
    from medicalseg_amd.utils import metric
    assert m and int(m.group(1)) == metric.EDT_MAX_EXTENT >= 1024


def test_evaluate_and_val_carry_the_new_keywords():
    from medicalseg_amd.core import evaluate
    sig = inspect.signature(evaluate)
    assert sig.parameters["surface_metrics"].default is False
    assert sig.parameters["surface_spacing"].default is None
    out = subprocess.run([sys.executable, os.path.join(ROOT, "val.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "--surface_metrics" in out.stdout

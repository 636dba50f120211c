"""Hard-label metrics without a GPU: the C ABI surface of msk_confusion3d, the host path of utils.metric
(confusion_counts / calculate_area / mean_iou / dice / accuracy / kappa / per_case) against the per-class-mask
restatement tests/metrics_reference.py, hand-made cases with known answers, and the new keywords of evaluate / val.py."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12   # same integers, same float64 operations up to their order: a handful of roundings at 2.2e-16


def test_header_ctypes_table_and_library_carry_the_entry_point():
    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    m = re.search(r"int\s+msk_confusion3d\s*\(([^)]*)\)", txt)
    assert m, "msegk.h does not declare msk_confusion3d"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 9
    res, args = _lib.SIGNATURES["msk_confusion3d"]
    C = ctypes
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "msk_confusion3d"), "libmsegk.so does not export msk_confusion3d"


CASES = [(1, 255), (2, 255), (3, 255), (20, 255), (64, 255), (2, 1), (3, 0), (20, 7), (64, 63)]


@pytest.mark.parametrize("C,ignore", CASES)
def test_host_counts_and_areas_equal_the_restatement(C, ignore):
    from medicalseg_amd.utils import metric
    for seed, shape, n in ((0, (5, 6, 7), 3), (1, (1, 1, 1), 2), (2, (3, 9, 11), 1)):
        pred, label = R.random_case(shape, C, 100 * C + seed, n=n, ignore_index=ignore)
        got = metric.confusion_counts(pred, label, C, ignore)
        want = R.confusion(pred, label, C, ignore)
        assert got.dtype == np.uint64 and got.shape == (n, (C + 1) ** 2 + 1)
        assert np.array_equal(got, want)
        assert int(got.sum()) == n * int(np.prod(shape))
        assert np.array_equal(metric.confusion_counts(pred[:, 0], label[:, 0], C, ignore), want)   # [N, D, H, W]
        a, b = metric.calculate_area(pred, label, C, ignore), R.areas(pred, label, C, ignore)
        for x, y in zip(a, b):
            assert x.dtype == np.int64 and x.shape == (C,) and np.array_equal(x, y)
        for i in range(n):     # per volume
            pv = metric.areas_from_counts(got, C, ignore, per_volume=True)
            for x, y in zip(pv, R.areas(pred[i:i + 1], label[i:i + 1], C, ignore)):
                assert np.array_equal(x[i], y)


def test_host_accumulation_and_shape_errors():
    from medicalseg_amd.utils import metric
    p1, l1 = R.random_case((4, 5, 6), 3, 1)
    p2, l2 = R.random_case((4, 5, 6), 3, 2)
    acc = metric.confusion_counts(p1, l1, 3)
    ret = metric.confusion_counts(p2, l2, 3, out=acc)
    assert ret is acc and np.array_equal(acc, R.confusion(p1, l1, 3) + R.confusion(p2, l2, 3))
    with pytest.raises(ValueError, match=r"Shape of `pred` and `label should be equal, but there are"):
        metric.calculate_area(p1, l1[:, :, :3], 3)
    with pytest.raises(ValueError):
        metric.confusion_counts(p1, l1, 65)
    with pytest.raises(ValueError):
        metric.confusion_counts(p1, l1, 0)


class _Lazy:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


@pytest.mark.parametrize("C,ignore", CASES)
def test_metric_functions_equal_the_restatement(C, ignore):
    from medicalseg_amd.utils import metric
    pred, label = R.random_case((6, 7, 8), C, 7 * C + 3, n=2, ignore_index=ignore)
    i, p, l = metric.calculate_area(pred, label, C, ignore)
    for args in ((i, p, l), (_Lazy(i), _Lazy(p), _Lazy(l))):       # arrays, or anything with .numpy()
        for name in ("mean_iou", "dice"):
            cls, mean = getattr(metric, name)(*args)
            rcls, rmean = getattr(R, name)(i, p, l)
            assert cls.dtype == np.float64
            np.testing.assert_allclose(cls, rcls, rtol=RTOL, atol=0)
            np.testing.assert_allclose(mean, rmean, rtol=RTOL, atol=0)
        cls, macc = metric.accuracy(args[0], args[1])
        rcls, rmacc = R.accuracy(i, p)
        np.testing.assert_allclose(cls, rcls, rtol=RTOL, atol=0)
        np.testing.assert_allclose(macc, rmacc, rtol=RTOL, atol=0)
        np.testing.assert_allclose(metric.kappa(*args), R.kappa(i, p, l), rtol=RTOL, atol=0)
    # per case: the same functions on each volume alone
    pc = metric.per_case(metric.confusion_counts(pred, label, C, ignore), C, ignore)
    for v in range(2):
        a = R.areas(pred[v:v + 1], label[v:v + 1], C, ignore)
        np.testing.assert_allclose(pc["class_dice"][v], R.dice(*a)[0], rtol=RTOL, atol=0)
        np.testing.assert_allclose(pc["mdice"][v], R.dice(*a)[1], rtol=RTOL, atol=0)
        np.testing.assert_allclose(pc["miou"][v], R.mean_iou(*a)[1], rtol=RTOL, atol=0)
        np.testing.assert_allclose(pc["acc"][v], R.accuracy(a[0], a[1])[1], rtol=RTOL, atol=0)
        np.testing.assert_allclose(pc["kappa"][v], R.kappa(*a), rtol=RTOL, atol=0)


def test_hand_made_cases():
    from medicalseg_amd.utils import metric
    rng = np.random.default_rng(5)
    label = rng.integers(0, 3, (2, 1, 4, 4, 4)).astype(np.int32)
    # perfect prediction -> every metric 1
    a = metric.calculate_area(label.copy(), label, 3)
    assert np.array_equal(metric.mean_iou(*a)[0], np.ones(3)) and metric.mean_iou(*a)[1] == 1.0
    assert np.array_equal(metric.dice(*a)[0], np.ones(3)) and metric.dice(*a)[1] == 1.0
    assert metric.accuracy(a[0], a[1])[1] == 1.0
    np.testing.assert_allclose(metric.kappa(*a), 1.0, rtol=RTOL)
    # disjoint: every voxel predicted as another class -> 0
    a = metric.calculate_area((label + 1) % 3, label, 3)
    assert metric.mean_iou(*a)[1] == 0.0 and metric.dice(*a)[1] == 0.0 and metric.accuracy(a[0], a[1])[1] == 0.0
    assert not metric.dice(*a)[0].any()
    # class 3 absent from both: scores 0 and still enters the mean
    a = metric.calculate_area(label.copy(), label, 4)
    assert np.array_equal(metric.dice(*a)[0], [1, 1, 1, 0]) and metric.dice(*a)[1] == 0.75
    assert np.array_equal(metric.mean_iou(*a)[0], [1, 1, 1, 0]) and metric.mean_iou(*a)[1] == 0.75
    assert np.array_equal(metric.accuracy(a[0], a[1])[0], [1, 1, 1, 0])
    # a known 2-class case: label 1 on 4 voxels, prediction 1 on 6 voxels, 2 of them shared
    l = np.zeros((1, 1, 1, 1, 16), np.int32)
    p = np.zeros_like(l)
    l[..., :4] = 1
    p[..., 2:8] = 1
    i_, p_, l_ = metric.calculate_area(p, l, 2)
    assert i_.tolist() == [8, 2] and p_.tolist() == [10, 6] and l_.tolist() == [12, 4]
    np.testing.assert_allclose(metric.dice(i_, p_, l_)[0], [16 / 22, 4 / 10], rtol=RTOL)
    np.testing.assert_allclose(metric.mean_iou(i_, p_, l_)[0], [8 / 14, 2 / 8], rtol=RTOL)
    np.testing.assert_allclose(metric.accuracy(i_, p_)[1], 10 / 16, rtol=RTOL)
    po, pe = 10 / 16, (10 * 12 + 6 * 4) / 256
    np.testing.assert_allclose(metric.kappa(i_, p_, l_), (po - pe) / (1 - pe), rtol=RTOL)
    # ignored voxels leave intersect / pred_area and stay in label_area when ignore_index is a class
    l[..., 0] = 255
    assert [x.tolist() for x in metric.calculate_area(p, l, 2)] == [[8, 2], [9, 6], [12, 3]]
    i2 = metric.calculate_area(p, l, 2, ignore_index=1)     # every label-1 voxel is ignored, yet label_area[1] counts them
    assert [x.tolist() for x in i2] == [[8, 0], [9, 4], [12, 3]]


def test_evaluate_and_val_carry_the_new_keywords():
    from medicalseg_amd.core import evaluate
    sig = inspect.signature(evaluate)
    assert sig.parameters["hard_metrics"].default is False
    assert sig.parameters["pred_transform"].default is None
    out = subprocess.run([sys.executable, os.path.join(ROOT, "val.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "--hard_metrics" in out.stdout

"""AUC from exact pair counts without a GPU: the C ABI surface of msk_auc_pack / msk_auc_workspace / msk_auc_counts, the
host specification utils.metric.auc_counts against a brute-force pair counter, auc_from_counts(auc_counts(...)) against
the existing rank-statistic path utils.metric.auc_roc (equal floats, no tolerance) and sklearn, the error conventions,
and the new keyword of evaluate / val.py."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import auc_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"msk_auc_pack": 7, "msk_auc_workspace": 3, "msk_auc_counts": 8}


def test_header_ctypes_table_and_library_carry_the_entry_points():
    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, "msegk.h does not declare " + name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert hasattr(lib, name), "libmsegk.so does not export " + name
    # the header cites the reference call sites
    for name in ("msk_auc_pack", "msk_auc_counts"):
        comment = txt[:txt.index("int " + name)].rsplit("/*", 1)[1]
        assert "core/val.py:121-131,174" in comment and "utils/metric.py:64-107" in comment


def test_workspace_answers_without_a_gpu_and_grows():
    from medicalseg_amd import _lib
    lib = _lib.load()

    def ws(count, classes):
        b = ctypes.c_size_t(0)
        assert lib.msk_auc_workspace(ctypes.c_long(count), classes, ctypes.byref(b)) == 0
        return b.value

    assert ws(1, 1) >= 4
    prev = 0
    for count in (1, 4096, 4097, 128 ** 3, 20 * 128 ** 3):
        b = ws(count, 3)
        assert b > prev and b >= 4 * 3 * count           # a second key buffer at least
        assert ws(count, 20) > b
        prev = b
    assert ws(20 * 128 ** 3, 3) < 1.2 * 4 * 3 * 20 * 128 ** 3      # ... and little else
    b = ctypes.c_size_t(0)
    for count, classes in ((0, 2), (2 ** 31, 2), (10, 0), (10, 65)):
        assert lib.msk_auc_workspace(ctypes.c_long(count), classes, ctypes.byref(b)) != 0
    assert lib.msk_auc_workspace(ctypes.c_long(10), 2, None) != 0


def test_loader_binds_missing_auc_symbols_to_raising_stubs(tmp_path):
    from medicalseg_amd import _lib
    so = str(tmp_path / "libfake_msegk.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-w", "-o", so, os.path.join(ROOT, "tests", "fake_msegk.c")])
    real_path, real_lib = _lib.LIB_PATH, _lib._lib
    try:
        _lib.LIB_PATH, _lib._lib = so, None
        lib = _lib.load()
        for name in ENTRY_POINTS:
            with pytest.raises(_lib.MskError, match=name):
                getattr(lib, name)(None)
    finally:
        _lib.LIB_PATH, _lib._lib = real_path, real_lib


@pytest.mark.parametrize("name", A.GENERATORS)
@pytest.mark.parametrize("C", [2, 3, 5])
def test_auc_counts_equal_the_brute_force_pair_count(name, C):
    from medicalseg_amd.utils import metric
    for seed, shape in ((1, (1, 1, 1)), (2, (1, 1, 7)), (3, (3, 5, 7)), (4, (10, 15, 20))):     # n <= 3000
        kind, values, label = A.case(name, shape, C, 100 * C + seed, all_present=seed != 3)
        s = A.scores_of(kind, values)
        got = metric.auc_counts(s, label, C)
        assert got.dtype == np.uint64 and got.shape == (C, 3)
        assert np.array_equal(got, A.brute_counts(s, label)), (name, C, shape)
        assert np.array_equal(metric.auc_counts(s, label[:, 0], C), got)            # (N, *spatial) labels
        assert np.array_equal(got[:, 1] + got[:, 2], np.full(C, label.size, np.uint64))


def test_hand_made_counts():
    from medicalseg_amd.utils import metric
    # class 1: positives 0.8, 0.5 ; negatives 0.5, 0.2 -> pairs: 0.8 beats both (4), 0.5 ties one (1) and beats one (2)
    s1 = np.array([0.8, 0.5, 0.5, 0.2], np.float32)
    s = np.stack([1 - s1, s1], axis=0).reshape(1, 2, 1, 1, 4)
    lab = np.array([1, 1, 0, 0], np.int32).reshape(1, 1, 1, 1, 4)
    c = metric.auc_counts(s, lab, 2)
    assert c[1].tolist() == [7, 2, 2]
    assert metric.auc_from_counts(c, 2) == 7 / 8
    # -0.0 is +0.0: one tie, not a smaller score
    s = np.array([[-0.0, 0.0], [0.0, -0.0]], np.float32).reshape(1, 2, 1, 1, 2)
    assert metric.auc_counts(s, np.array([0, 1], np.int32).reshape(1, 1, 1, 1, 2), 2)[:, 0].tolist() == [1, 1]


def _sklearn_auc(scores, label, C):
    import sklearn.metrics as skm
    s = np.moveaxis(scores, 1, -1).reshape(-1, C).astype(np.float64)
    lab = label.reshape(-1)
    if C == 2:
        return skm.roc_auc_score(lab == 1, s[:, 1])
    return float(np.mean([skm.roc_auc_score(lab == c, s[:, c]) for c in range(C)]))


@pytest.mark.parametrize("name", [g for g in A.GENERATORS if g != "constant"] + ["constant"])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_auc_from_counts_equals_the_rank_statistic_path_bit_for_bit(name, C):
    from medicalseg_amd.utils import metric
    for seed, shape in ((1, (3, 5, 7)), (2, (33, 37, 70)), (3, (128, 128, 128 // C))):      # up to 2 M scores
        kind, values, label = A.case(name, shape, C, 10 * C + seed)
        s = A.scores_of(kind, values)
        want = metric.auc_roc(s, label, num_classes=C)                # the existing host path (average ranks, float64)
        got = metric.auc_from_counts(metric.auc_counts(s, label, C), C)
        assert got == want, (name, C, shape, got, want)
        if seed < 3:
            # 4-D layout (N, C, H, W): the same voxels as two "slices"
            s4, l4 = s.reshape((1, C, shape[0], -1)), label.reshape((1, 1, shape[0], -1))
            assert metric.auc_from_counts(metric.auc_counts(s4, l4, C), C) == want
            assert abs(got - _sklearn_auc(s, label, C)) <= 1e-12, (name, C, shape)
    if name == "separated_up":
        assert got == 1.0
    if name == "separated_down":
        assert got == 0.0
    if name == "constant":
        assert got == 0.5


def test_batches_pool_like_one_array():
    from medicalseg_amd.utils import metric
    parts = [A.case("quantised", (4, 5, 6), 3, seed) for seed in (1, 2, 3)]
    s = np.concatenate([p[1] for p in parts])
    lab = np.concatenate([p[2] for p in parts])
    assert s.shape == (3, 3, 4, 5, 6)
    assert np.array_equal(metric.auc_counts(s, lab, 3), A.brute_counts(s, lab))
    assert metric.auc_from_counts(metric.auc_counts(s, lab, 3), 3) == metric.auc_roc(s, lab, num_classes=3)


def test_error_conventions():
    from medicalseg_amd.utils import metric
    _, s, lab = A.case("uniform", (3, 4, 5), 3, 1)
    good = metric.auc_counts(s, lab, 3)
    # a class without positives: counted, and refused where the macro average is formed
    lab0 = np.where(lab == 2, 0, lab)
    c = metric.auc_counts(s, lab0, 3)
    assert c[2].tolist()[1:] == [0, lab.size] and c[2, 0] == 0
    with pytest.raises(ValueError, match="Number of classes in y_true not equal to the number of columns in 'y_score'"):
        metric.auc_from_counts(c, 3)
    with pytest.raises(ValueError, match="Number of classes in y_true"):
        metric.auc_roc(s, lab0, num_classes=3)                      # the host path says the same
    # binary, one class present
    _, s2, lab2 = A.case("uniform", (3, 4, 5), 2, 2)
    for fill in (0, 1):
        c2 = metric.auc_counts(s2, np.full_like(lab2, fill), 2)
        with pytest.raises(ValueError, match="Only one class present in y_true"):
            metric.auc_from_counts(c2, 2)
    # n_neg == 0 in a multi-class row cannot happen with every class present; n_pos == 0 was shown above
    # labels outside [0, C): the host function's condition and message
    for bad in (255, -1):
        lb = lab.copy()
        lb.flat[7] = bad
        with pytest.raises(RuntimeError, match="labels with ignore_index is not supported yet."):
            metric.auc_counts(s, lb, 3)
    # scores that no softmax produces are reported, not sorted
    for bad in (np.nan, np.inf, -0.5):
        sb = s.copy()
        sb.flat[11] = bad
        with pytest.raises(ValueError, match="negative or not finite"):
            metric.auc_counts(sb, lab, 3)
    with pytest.raises(ValueError):
        metric.auc_counts(s, lab, 4)                                # channel count != num_classes
    with pytest.raises(ValueError, match="length of `logit` and `label` should be equal"):
        metric.auc_counts(s, lab[..., :3], 3)
    with pytest.raises(ValueError):
        metric.auc_from_counts(good, 2)
    assert 0.0 <= metric.auc_from_counts(good, 3) <= 1.0


def test_evaluate_and_val_carry_the_new_keyword():
    from medicalseg_amd.core import evaluate
    assert inspect.signature(evaluate).parameters["auc_device"].default is False
    out = subprocess.run([sys.executable, os.path.join(ROOT, "val.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--auc_device" in out.stdout

"""Exact AUC counts on the device (medicalseg_amd/csrc/msk_auc.hip: msk_auc_pack / msk_auc_counts through
utils.metric.AucScores) against the host specification utils.metric.auc_counts of the DOWNLOADED scores, word for word:
integers, no tolerance.  Then the conventions of auc_from_counts on device counts, accumulation over several add() calls,
growth, the reports for labels outside [0, C) and non-finite scores, and evaluate(auc_roc=True, auc_device=True) against the
host path of the same evaluation with ==."""
import ctypes as C

import numpy as np
import pytest

import auc_reference as A

pytestmark = pytest.mark.gpu

CHUNK = 4096          # keys per workgroup of the radix passes (msk_auc.hip: kChunk)
SHAPES = [(1, 1, 1), (1, 1, 63), (1, 1, 4097), (1, 1, CHUNK - 1), (1, 1, CHUNK), (1, 1, CHUNK + 1), (33, 37, 70),
          (128, 128, 128)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _probs_on_device(kind, values, label):
    """-> (probs Tensor (owned, not in the arena), label IntTensor, the scores as downloaded, the label as downloaded)"""
    from medicalseg_amd.device import Tensor, to_tensor
    t, lt = to_tensor(values), to_tensor(label)
    probs = Tensor.empty(t.dev, t.n, t.d, t.h, t.w, t.c, arena=False)
    if kind == "logits":
        t.dev.call("msk_softmax_c", t.msk(), probs.msk())
    else:
        t.dev.d2d(probs.ptr, t.ptr, 4 * t.voxels * t.c)
    return probs, lt, probs.numpy(), lt.numpy()


def _assert_same(got, want, what):
    if not np.array_equal(got, want):
        c = int(np.argwhere((got != want).any(axis=1))[0, 0])
        raise AssertionError("%s: class %d differs: device {U2, n_pos, n_neg} = %s, host = %s" % (
            what, c, got[c].tolist(), want[c].tolist()))


def _check(name, shape, ncls, seed, capacity=None):
    from medicalseg_amd.utils import metric
    kind, values, label = A.case(name, shape, ncls, seed)
    probs, lt, host_probs, host_label = _probs_on_device(kind, values, label)
    assert np.array_equal(host_label, label)
    if kind == "scores":
        assert np.array_equal(_bits(host_probs), _bits(values)), "the upload changed the scores"
    acc = metric.AucScores(probs.dev, ncls, capacity or probs.voxels)
    try:
        acc.add(probs, lt)
        got = acc.counts()
        assert got.dtype == np.uint64 and got.shape == (ncls, 3)
        want = metric.auc_counts(host_probs, label, ncls)
        _assert_same(got, want, "%s %s C=%d" % (name, shape, ncls))
        assert np.array_equal(_bits(probs.numpy()), _bits(host_probs)) and np.array_equal(lt.numpy(), label), \
            "an input was modified"
    finally:
        acc.free()
        probs.dev.free(probs.ptr)
    return got, want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ncls", [2, 3, 20])
def test_device_counts_equal_host_counts_of_the_downloaded_scores(shape, ncls):
    for i, name in enumerate(A.GENERATORS):
        _check(name, shape, ncls, 1000 * ncls + 10 * shape[2] + i)


def test_auc_roc_accepts_device_inputs_and_returns_the_host_float():
    from medicalseg_amd.utils import metric
    for ncls, name in ((2, "saturated"), (3, "saturated"), (5, "quantised"), (3, "separated_up"), (3, "separated_down")):
        kind, values, label = A.case(name, (33, 37, 70), ncls, 7 * ncls)
        probs, lt, host_probs, _ = _probs_on_device(kind, values, label)
        try:
            got = metric.auc_roc(probs, lt, num_classes=ncls)
            want = metric.auc_roc(host_probs, label, num_classes=ncls)       # numpy inputs: the existing path
            assert isinstance(got, float) and got == want, (name, ncls, got, want)
            if name.startswith("separated"):
                assert got == (1.0 if name.endswith("up") else 0.0)
            with pytest.raises(TypeError):
                metric.auc_roc(probs, label, num_classes=ncls)               # device scores, host label
        finally:
            probs.dev.free(probs.ptr)


def test_a_class_without_positives():
    from medicalseg_amd.utils import metric
    for ncls in (2, 3):
        kind, values, label = A.case("saturated", (1, 1, 4097), ncls, 5)
        label = np.where(label == ncls - 1, 0, label).astype(np.int32)
        probs, lt, host_probs, _ = _probs_on_device(kind, values, label)
        acc = metric.AucScores(probs.dev, ncls, probs.voxels)
        try:
            acc.add(probs, lt)
            got = acc.counts()
            _assert_same(got, metric.auc_counts(host_probs, label, ncls), "absent class, C=%d" % ncls)
            assert got[ncls - 1].tolist() == [0, 0, 4097]
            with pytest.raises(ValueError, match="Only one class present" if ncls == 2 else "Number of classes in y_true"):
                metric.auc_from_counts(got, ncls)
        finally:
            acc.free()
            probs.dev.free(probs.ptr)


def _parts(ncls):
    """three batches of different shapes (distinct upload buffers) and their concatenation as one (1, C, 1, 1, V) batch"""
    parts = [A.case("quantised", (4, 5, 6), ncls, 1), A.case("uniform", (1, 1, CHUNK + 5), ncls, 2),
             A.case("special", (3, 5, 7), ncls, 3)]
    flat = np.concatenate([np.moveaxis(p[1], 1, -1).reshape(-1, ncls) for p in parts])
    lab = np.concatenate([p[2].reshape(-1) for p in parts])
    V = lab.size
    return parts, np.ascontiguousarray(flat.T).reshape(1, ncls, 1, 1, V), lab.reshape(1, 1, 1, 1, V)


@pytest.mark.parametrize("capacity", [None, 5])
def test_accumulation_growth_and_counts_between_adds(capacity):
    from medicalseg_amd.utils import metric
    ncls = 3
    parts, allv, alll = _parts(ncls)
    want = metric.auc_counts(allv, alll, ncls)
    dev_parts = [_probs_on_device(*p) for p in parts]
    one = _probs_on_device("scores", allv, alll)
    dev = one[0].dev
    accs = []
    try:
        # three add calls == one add of the concatenation == the host counts
        a = metric.AucScores(dev, ncls, capacity or alll.size)
        accs.append(a)
        for probs, lt, _, _ in dev_parts:
            a.add(probs, lt)
        got3 = a.counts()
        if capacity:
            assert a.capacity >= alll.size > capacity          # it grew, keeping what it held
        b = metric.AucScores(dev, ncls, capacity or alll.size)
        accs.append(b)
        b.add(one[0], one[1])
        _assert_same(got3, b.counts(), "three adds against one")
        _assert_same(got3, want, "three adds against the host")
        # add -> counts -> add -> counts: the sorted buffer is still a bag of keys
        c = metric.AucScores(dev, ncls, capacity or alll.size)
        accs.append(c)
        c.add(dev_parts[0][0], dev_parts[0][1])
        first = c.counts()
        _assert_same(first, metric.auc_counts(parts[0][1], parts[0][2], ncls), "first batch alone")
        c.add(dev_parts[1][0], dev_parts[1][1])
        c.add(dev_parts[2][0], dev_parts[2][1])
        _assert_same(c.counts(), want, "counts of the union after an earlier counts()")
        _assert_same(c.counts(), want, "counts() twice")
        for (probs, lt, hp, hl), p in zip(dev_parts, parts):
            assert np.array_equal(_bits(probs.numpy()), _bits(hp)) and np.array_equal(lt.numpy(), p[2]), "an input was modified"
    finally:
        for x in accs:
            x.free()
        for probs in [p[0] for p in dev_parts] + [one[0]]:
            dev.free(probs.ptr)


def test_bad_labels_and_scores_are_reported():
    from medicalseg_amd.utils import metric
    kind, values, label = A.case("uniform", (1, 1, 4097), 3, 9)
    for bad in (255, -1):
        lb = label.copy()
        lb.flat[4000] = bad
        probs, lt, _, _ = _probs_on_device(kind, values, lb)
        acc = metric.AucScores(probs.dev, 3, probs.voxels)
        try:
            acc.add(probs, lt)
            with pytest.raises(RuntimeError, match="labels with ignore_index is not supported yet."):
                acc.counts()
            with pytest.raises(RuntimeError, match="labels with ignore_index is not supported yet."):
                metric.auc_roc(probs, lt, num_classes=3)
        finally:
            acc.free()
            probs.dev.free(probs.ptr)
    for bad in (np.nan, np.inf, -0.25):
        sb = values.copy()
        sb[0, 1, 0, 0, 123] = bad
        probs, lt, _, _ = _probs_on_device(kind, sb, label)
        acc = metric.AucScores(probs.dev, 3, probs.voxels)
        try:
            acc.add(probs, lt)
            with pytest.raises(ValueError, match="negative or not finite"):
                acc.counts()
        finally:
            acc.free()
            probs.dev.free(probs.ptr)


def test_entry_points_refuse_bad_arguments():
    from medicalseg_amd._lib import MskError
    from medicalseg_amd.device import get_device
    from medicalseg_amd.utils import metric
    dev = get_device()
    kind, values, label = A.case("uniform", (1, 1, 63), 2, 1)
    probs, lt, _, _ = _probs_on_device(kind, values, label)
    acc = metric.AucScores(dev, 2, 64)
    vp = C.c_void_p
    try:
        with pytest.raises(MskError):      # offset + voxels > capacity
            dev.call("msk_auc_pack", probs.msk(), vp(lt.ptr), vp(acc.keys), C.c_long(64), C.c_long(2), vp(acc.res + 48))
        with pytest.raises(MskError):      # null label
            dev.call("msk_auc_pack", probs.msk(), None, vp(acc.keys), C.c_long(64), C.c_long(0), vp(acc.res + 48))
        with pytest.raises(MskError):      # workspace too small
            dev.call("msk_auc_counts", vp(acc.keys), C.c_long(64), C.c_long(63), 2, vp(acc.keys), C.c_size_t(16), vp(acc.res))
        with pytest.raises(MskError):      # count > capacity
            dev.call("msk_auc_counts", vp(acc.keys), C.c_long(64), C.c_long(65), 2, vp(acc.keys), C.c_size_t(1 << 20), vp(acc.res))
        with pytest.raises(ValueError):
            acc.counts()                   # nothing added
        with pytest.raises(TypeError):
            acc.add(values, label)         # host arrays
    finally:
        acc.free()
        dev.free(probs.ptr)


def test_evaluate_auc_device_equals_the_host_path():
    """Same eval-mode forward, same msk_softmax_c bits, exact integers: the two floats are equal, and nothing else moves."""
    from medicalseg_amd.core import evaluate
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from oracle import vnet_numpy as O
    shape, ncls, K, S = (16, 16, 16), 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4
    model = VNet(elu=False, in_channels=1, num_classes=ncls, kernel_size=K, stride_size=S)
    missing, unexpected = model.set_state_dict(O.init_params(2, 1, ncls, K, S))
    assert not missing and not unexpected
    ds = SyntheticCT(num_samples=3, shape=shape, num_classes=ncls, mode="val")
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    host = evaluate(model, ds, losses, print_detail=False, auc_roc=True)
    devr = evaluate(model, ds, losses, print_detail=False, auc_roc=True, auc_device=True)
    print("auc_roc host %.17g device %.17g, mdice %.6f / %.6f" % (host["auc_roc"], devr["auc_roc"], host["mdice"], devr["mdice"]))
    assert devr["auc_roc"] == host["auc_roc"]
    assert devr["mdice"] == host["mdice"]
    assert 0.0 <= devr["auc_roc"] <= 1.0

"""msk_confusion3d (medicalseg_amd/csrc/msk_metrics.hip) through utils.metric: the device counts equal the host path
(np.bincount, itself held to the per-class-mask restatement in tests/test_metrics_host.py) word for word -- integers,
no tolerance -- and evaluate(hard_metrics=True) reports what the host computes from the downloaded predictions."""
import numpy as np
import pytest

import metrics_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 4097), (33, 37, 70), (128, 128, 128)]


def _device_counts(pred, label, C, ignore=255, out=None):
    """pred / label: int32 [N, 1, D, H, W] host arrays -> [N, K*K + 1] uint64 from the device; checks the inputs survive"""
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import metric
    p, l = to_tensor(pred), to_tensor(label)
    res = metric.confusion_counts(p, l, C, ignore, out=out)
    assert isinstance(res, metric.ConfusionCounts) and res.shape == (pred.shape[0], (C + 1) ** 2 + 1)
    got = res.numpy()
    assert got.dtype == np.uint64
    assert np.array_equal(p.numpy(), pred) and np.array_equal(l.numpy(), label), "an input was modified"
    if out is None:
        res.free()
    return got


def _check(pred, label, C, ignore=255):
    from medicalseg_amd.utils import metric
    want = metric.confusion_counts(pred, label, C, ignore)
    got = _device_counts(pred, label, C, ignore)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("C=%d ignore=%d shape %s: %d words differ, first %s: got %d want %d" % (
            C, ignore, pred.shape, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [1, 2, 3, 20, 64])
def test_random_volumes_match_host(shape, C):
    n = 1 if shape == (128, 128, 128) else 2
    _check(*R.random_case(shape, C, 11 * C + shape[2], n=n), C)                       # ignore 255, out-of-range values
    _check(*R.random_case(shape, C, 13 * C + shape[2], n=n, ignore_index=C - 1), C, ignore=C - 1)   # ignore inside [0, C)
    _check(*R.random_case(shape, C, 17 * C + shape[2], n=n, out_of_range=False, ignore_frac=0.0), C)   # plain classes


@pytest.mark.parametrize("shape", SHAPES)
def test_one_bin_and_blobs(shape):
    full = (1, 1) + shape
    for C in (1, 2, 20):
        z = np.zeros(full, np.int32)
        _check(z, z.copy(), C)                                           # everything in bin (0, 0)
        _check(z + (C - 1), z + (C - 1), C)                              # ... in bin (C-1, C-1)
        _check(z - 5, z + 1000, C)                                       # ... in bin (other, other)
        _check(z, z + 255, C)                                            # ... ignored
        _check(*R.blobs(shape, C, 3), C)


def test_each_volume_of_a_batch_has_its_own_row():
    from medicalseg_amd.utils import metric
    for shape in ((1, 1, 4097), (33, 37, 70), (3, 5, 7)):                # odd voxel counts: volumes 1, 2 start unaligned
        pred, label = R.random_case(shape, 3, 21, n=3)
        label[1] = 0
        pred[1] = 1                                                      # volume 1: one bin, distinct from its neighbours
        got = _device_counts(pred, label, 3)
        for i in range(3):
            assert np.array_equal(got[i:i + 1], metric.confusion_counts(pred[i:i + 1], label[i:i + 1], 3)), (shape, i)
        # [N, D, H, W] tensors
        from medicalseg_amd.device import to_tensor
        c = metric.confusion_counts(to_tensor(pred[:, 0]), to_tensor(label[:, 0]), 3)
        assert np.array_equal(c.numpy(), got)
        c.free()


def test_device_volumes_and_calculate_area():
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.utils import metric
    pred, label = R.random_case((33, 37, 70), 3, 31, n=1)
    pv, lv = pp.upload(pred[0, 0]), pp.upload(label[0, 0])
    c = metric.confusion_counts(pv, lv, 3)
    assert np.array_equal(c.numpy(), metric.confusion_counts(pred, label, 3))
    c.free()
    for a, b in zip(metric.calculate_area(pv, lv, 3), R.areas(pred, label, 3)):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    fv = pp.upload(pred[0, 0].astype(np.float32))
    with pytest.raises(TypeError):
        metric.confusion_counts(fv, lv, 3)
    with pytest.raises(ValueError, match="Shape of `pred` and `label should be equal"):
        metric.confusion_counts(pv, pp.upload(label[0, 0, :5]), 3)
    for v in (pv, lv, fv):
        v.free()


@pytest.mark.parametrize("off_pred,off_label", [(1, 1), (3, 3), (1, 2), (0, 3)])
def test_four_byte_aligned_offsets(off_pred, off_label):
    """views that start 4, 8 or 12 bytes into a buffer: equal offsets take the vector path behind a scalar head,
    different offsets the element path"""
    from medicalseg_amd.device import IntTensor, get_device
    from medicalseg_amd.utils import metric
    dev = get_device()
    shape = (9, 31, 33)
    pred, label = R.random_case(shape, 3, 41, n=2)
    nbytes = pred.nbytes
    bufs = []
    for a, off in ((pred, off_pred), (label, off_label)):
        ptr = dev.malloc(nbytes + 64)
        dev.memset(ptr, 0x7F, nbytes + 64)
        t = IntTensor(dev, ptr + 4 * off, a.shape)
        dev.h2d(t.ptr, a)
        bufs.append((ptr, t))
    c = metric.confusion_counts(bufs[0][1], bufs[1][1], 3)
    assert np.array_equal(c.numpy(), metric.confusion_counts(pred, label, 3))
    c.free()
    for ptr, _ in bufs:
        dev.free(ptr)


def test_accumulate_and_overwrite():
    import ctypes as C
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import metric
    shape, ncls = (33, 37, 70), 20
    p1, l1 = R.random_case(shape, ncls, 51, n=2)
    p2, l2 = R.blobs(shape, ncls, 52, n=2)
    a, b = _device_counts(p1, l1, ncls), _device_counts(p2, l2, ncls)
    tp1, tl1 = to_tensor(p1), to_tensor(l1)
    acc = metric.confusion_counts(tp1, tl1, ncls)
    ret = metric.confusion_counts(to_tensor(p2), to_tensor(l2), ncls, out=acc)
    assert ret is acc and np.array_equal(acc.numpy(), a + b)
    # rows(): one row of a zeroed set buffer per call
    whole = metric.ConfusionCounts(acc.dev, 4, ncls, 255, zero=True)
    metric.confusion_counts(to_tensor(p2), to_tensor(l2), ncls, out=whole.rows(2, 2))
    metric.confusion_counts(to_tensor(p1), to_tensor(l1), ncls, out=whole.rows(0, 2))
    assert np.array_equal(whole.numpy(), np.concatenate([a, b]))
    whole.free()
    # accumulate = 0 over garbage == a fresh call
    acc.dev.memset(acc.ptr, 0xA5, acc.shape[0] * acc.shape[1] * 8)
    tp1, tl1 = to_tensor(p1), to_tensor(l1)
    acc.dev.call("msk_confusion3d", C.c_void_p(tp1.ptr), C.c_void_p(tl1.ptr), 2, C.c_long(int(np.prod(shape))), ncls, 255,
                 C.c_void_p(acc.ptr), 0)
    assert np.array_equal(acc.numpy(), a)
    with pytest.raises(ValueError):
        metric.confusion_counts(tp1, tl1, 3, out=acc)         # another num_classes
    acc.free()


def test_invalid_arguments_are_errors():
    import ctypes as C
    from medicalseg_amd._lib import MskError
    from medicalseg_amd.device import get_device, to_tensor
    dev = get_device()
    t = to_tensor(np.zeros((1, 1, 2, 2, 2), np.int32))
    out = dev.malloc(8 * (65 * 65 + 1))
    for n, vox, ncls in ((1, 8, 0), (1, 8, 65), (0, 8, 2), (1, 0, 2)):
        with pytest.raises(MskError):
            dev.call("msk_confusion3d", C.c_void_p(t.ptr), C.c_void_p(t.ptr), n, C.c_long(vox), ncls, 255, C.c_void_p(out), 0)
    with pytest.raises(MskError):
        dev.call("msk_confusion3d", C.c_void_p(t.ptr), None, 1, C.c_long(8), 2, 255, C.c_void_p(out), 0)
    dev.free(out)


def test_repeat_runs_are_bitwise_identical():
    pred, label = R.random_case((128, 128, 128), 20, 61, n=1)
    a, b = _device_counts(pred, label, 20), _device_counts(pred, label, 20)
    assert a.tobytes() == b.tobytes()


def _eval_setup(ncls, shape=(32, 32, 32), samples=3):
    from medicalseg_amd import models
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    model = models.VNet(num_classes=ncls)
    ds = SyntheticCT(num_samples=samples, shape=shape, num_classes=ncls, mode="val")
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    return model, ds, losses


def _host_predictions(model, ds, transform=None):
    """the predictions evaluate() scores, downloaded: inference per volume (+ the host form of the transform)"""
    from medicalseg_amd import nn
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    model.eval()
    preds, labels = [], []
    with nn.fused_inference():
        for i in range(len(ds)):
            im, lab, _ = ds[i]
            pred, _ = infer.inference(model, to_tensor(im[None]), ori_shape=lab.shape[-3:], transforms=ds.transforms.transforms)
            p = pred.numpy()
            if transform is not None:
                p = np.asarray(transform(p[0, 0])[0]).astype(np.int32)[None, None]
            preds.append(p)
            labels.append(np.asarray(lab).astype(np.int32).reshape(p.shape))
    return np.concatenate(preds), np.concatenate(labels)


def _check_eval_result(res, preds, labels, ncls):
    from medicalseg_amd.utils import metric
    c = metric.confusion_counts(preds, labels, ncls)
    areas = metric.areas_from_counts(c, ncls)
    for a, b in zip(areas, R.areas(preds, labels, ncls)):
        assert np.array_equal(a, b)
    assert np.array_equal(res["class_iou"], metric.mean_iou(*areas)[0])
    assert np.array_equal(res["class_dice"], metric.dice(*areas)[0])
    assert res["miou"] == float(metric.mean_iou(*areas)[1])
    assert res["dice"] == float(metric.dice(*areas)[1])
    assert res["acc"] == float(metric.accuracy(areas[0], areas[1])[1])
    assert res["kappa"] == float(metric.kappa(*areas))
    per = [R.dice(*R.areas(preds[i:i + 1], labels[i:i + 1], ncls))[1] for i in range(len(preds))]
    np.testing.assert_allclose(res["dice_per_case"], np.mean(per), rtol=1e-12, atol=0)


def test_evaluate_hard_metrics_match_host():
    from medicalseg_amd.core import evaluate
    ncls = 3
    model, ds, losses = _eval_setup(ncls)
    plain = evaluate(model, ds, losses, print_detail=False)
    assert sorted(plain) == ["mdice"]
    res = evaluate(model, ds, losses, print_detail=False, hard_metrics=True)
    assert sorted(res) == sorted(["mdice", "miou", "dice", "dice_per_case", "acc", "kappa", "class_iou", "class_dice"])
    assert res["mdice"] == plain["mdice"]
    preds, labels = _host_predictions(model, ds)
    print("hard metrics:", {k: v for k, v in res.items() if np.ndim(v) == 0}, "pred classes", np.unique(preds).tolist())
    _check_eval_result(res, preds, labels, ncls)


def test_inference_top1_component_dice_and_evaluate_pred_transform():
    from medicalseg_amd import nn
    from medicalseg_amd.core import evaluate, infer
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.transforms import transform as T
    from medicalseg_amd.utils import metric
    ncls = 2
    model, ds, losses = _eval_setup(ncls)
    op = T.TopkLargestConnectComponent(k=1)
    preds, labels = _host_predictions(model, ds, transform=op)
    # inference -> top-1 component -> dice, all on the device, against the host computation on the downloaded arrays
    im, lab, _ = ds[0]
    with nn.fused_inference():
        pred, _ = infer.inference(model, to_tensor(im[None]))
        top, _ = op(pred)
        got = metric.dice(*metric.calculate_area(top, to_tensor(labels[:1]), ncls))
    want = R.dice(*R.areas(preds[:1], labels[:1], ncls))
    np.testing.assert_allclose(got[0], want[0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-12, atol=0)
    res = evaluate(model, ds, losses, print_detail=False, hard_metrics=True, pred_transform=op)
    _check_eval_result(res, preds, labels, ncls)
    res2 = evaluate(model, ds, losses, print_detail=False, hard_metrics=True, pred_transform=lambda p: op(p)[0])
    assert res2["dice"] == res["dice"] and res2["dice_per_case"] == res["dice_per_case"]

"""Test-time augmentation on the device (medicalseg_amd/csrc/msk_tta.hip, core/infer.py aug_inference, evaluate(aug_eval=True))
against the numpy statement of tests/tta_reference.py.  msk_softmax_c's device output is the primitive; the flips, the ordered
float32 sums and the one multiply are done in numpy and compared with np.array_equal: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import tta_reference as R

pytestmark = pytest.mark.gpu

ALL_SHAPES = R.SHAPES + R.MORE_SHAPES


class Owned:
    """device tensors outside the arena and the input pool, freed on exit"""

    def __enter__(self):
        from medicalseg_amd.device import get_device
        self.dev, self.ptrs = get_device(), []
        return self

    def __exit__(self, *exc):
        self.dev.sync()
        for p in self.ptrs:
            self.dev.free(p)
        return False

    def empty(self, n, d, h, w, c):
        from medicalseg_amd.device import Tensor
        t = Tensor.empty(self.dev, n, d, h, w, c, arena=False)
        self.ptrs.append(t.ptr)
        return t

    def upload(self, ncdhw):
        a = np.ascontiguousarray(np.moveaxis(np.asarray(ncdhw, np.float32), 1, -1))
        t = self.empty(*a.shape)
        self.dev.h2d(t.ptr, a)
        return t

    def ints(self, count, fill):
        p = self.dev.malloc(4 * count)
        self.ptrs.append(p)
        self.dev.h2d(p, np.full(count, fill, np.int32))
        return p

    def softmax(self, t):
        """msk_softmax_c(t), downloaded as NCDHW"""
        out = self.empty(t.n, t.d, t.h, t.w, t.c)
        self.dev.call("msk_softmax_c", t.msk(), out.msk())
        return out.numpy()


def _rand(shape, seed):
    n, d, h, w, c = shape
    return np.random.default_rng(seed).standard_normal((n, c, d, h, w)).astype(np.float32)


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_flip_axes_equals_np_flip(shape):
    x = _rand(shape, 3)
    with Owned() as o:
        src = o.upload(x)
        for mask in range(8):
            dst = o.upload(np.full_like(x, np.nan))
            o.dev.call("msk_flip_axes", src.msk(), dst.msk(), mask)
            got = dst.numpy()
            assert np.array_equal(got.view(np.uint32), R.flip(x, mask).view(np.uint32)), (shape, mask)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_flip_axes_on_channel_slice_views(shape):
    n, d, h, w, c = shape
    wide = _rand((n, d, h, w, c + 3), 4)
    with Owned() as o:
        src = o.upload(wide)
        for mask in range(8):
            fill = np.full_like(wide, 7.0)
            dst = o.upload(fill)
            o.dev.call("msk_flip_axes", src.channel_slice(2, 2 + c).msk(), dst.channel_slice(1, 1 + c).msk(), mask)
            want = fill.copy()
            want[:, 1:1 + c] = R.flip(wide[:, 2:2 + c], mask)
            assert np.array_equal(dst.numpy(), want), (shape, mask)            # the channels around the view are untouched


def _mask_lists():
    out = [[m] for m in range(8)]                        # K = 1
    out += [[m, m ^ 5] for m in range(8)]                # K = 2
    out += [list(range(8)), [7, 2, 5, 0, 3, 6, 1, 4]]    # K = 8
    return out


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_accumulate_and_finish_equal_the_statement(shape):
    n, d, h, w, c = shape
    logits = [R.logits_case(shape, 10 + k) for k in range(8)]
    with Owned() as o:
        dev = o.dev
        lt = [o.upload(x) for x in logits]
        sm = [o.softmax(t) for t in lt]                  # the primitive, computed once
        if c == 1:
            assert all((s == 1.0).all() for s in sm)
        acc, probs = o.upload(np.full_like(logits[0], np.nan)), o.empty(n, d, h, w, c)
        pred = o.ints(n * d * h * w, -1)
        for masks in _mask_lists():
            for k, m in enumerate(masks):
                dev.call("msk_tta_accumulate", lt[k].msk(), m, acc.msk(), 1 if k == 0 else 0)
            dev.call("msk_tta_finish", acc.msk(), len(masks), probs.msk(), C.c_void_p(pred))
            want_acc, want_probs, want_pred = R.tta_reference(sm[:len(masks)], masks)
            assert np.array_equal(acc.numpy(), want_acc), (shape, masks)
            assert np.array_equal(probs.numpy(), want_probs), (shape, masks)
            assert np.array_equal(dev.d2h(pred, (n, d, h, w), np.int32), want_pred), (shape, masks)
            if c == 1:
                assert (want_probs == 1.0).all() and (want_pred == 0).all()
        # the saturated and the tied blocks did what they are there for (last mask list: all 8 flips of different logits;
        # first list entries: single passes)
        one = R.tta_reference(sm[:1], [0])
        if c > 1:
            assert (one[1][:, c // 2, -1, -1, w // 2:] == 1.0).all() and (one[1][:, 0, -1, -1, w // 2:] == 0.0).all()
            assert (one[2][:, 0, :, : max(1, w // 3)] == 0).all()


def test_accumulate_and_finish_on_channel_slice_views():
    shape = (2, 3, 5, 7, 3)
    n, d, h, w, c = shape
    wide = [np.concatenate([_rand((n, d, h, w, 2), 20 + k), R.logits_case(shape, 30 + k)], axis=1) for k in range(2)]
    with Owned() as o:
        lt = [o.upload(x) for x in wide]
        views = [t.channel_slice(2, 2 + c) for t in lt]
        sm = [o.softmax(v) for v in views]
        fill = np.full((n, c + 1, d, h, w), 7.0, np.float32)
        acc, probs = o.upload(fill), o.upload(fill)
        pred = o.ints(n * d * h * w, -1)
        av, pv = acc.channel_slice(1, 1 + c), probs.channel_slice(0, c)
        for k, m in enumerate([6, 3]):
            o.dev.call("msk_tta_accumulate", views[k].msk(), m, av.msk(), 1 if k == 0 else 0)
        o.dev.call("msk_tta_finish", av.msk(), 2, pv.msk(), C.c_void_p(pred))
        want_acc, want_probs, want_pred = R.tta_reference(sm, [6, 3])
        assert np.array_equal(acc.numpy()[:, 1:], want_acc) and (acc.numpy()[:, 0] == 7.0).all()
        assert np.array_equal(probs.numpy()[:, :c], want_probs) and (probs.numpy()[:, c] == 7.0).all()
        assert np.array_equal(o.dev.d2h(pred, (n, d, h, w), np.int32), want_pred)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 3), (1, 4, 6, 130, 20)])
def test_finish_honours_null_outputs(shape):
    from medicalseg_amd._lib import NULL_TENSOR
    n, d, h, w, c = shape
    x = R.logits_case(shape, 5)
    with Owned() as o:
        dev = o.dev
        t = o.upload(x)
        sm = o.softmax(t)
        acc = o.empty(n, d, h, w, c)
        dev.call("msk_tta_accumulate", t.msk(), 5, acc.msk(), 1)
        want_acc, want_probs, want_pred = R.tta_reference([sm], [5])
        probs, pred = o.upload(np.full_like(x, 7.0)), o.ints(n * d * h * w, -1)
        dev.call("msk_tta_finish", acc.msk(), 1, NULL_TENSOR, C.c_void_p(pred))
        assert (probs.numpy() == 7.0).all()
        assert np.array_equal(dev.d2h(pred, (n, d, h, w), np.int32), want_pred)
        pred2 = o.ints(n * d * h * w, -1)
        dev.call("msk_tta_finish", acc.msk(), 1, probs.msk(), None)
        assert np.array_equal(probs.numpy(), want_probs)
        assert (dev.d2h(pred2, (n, d, h, w), np.int32) == -1).all()
        dev.call("msk_tta_finish", acc.msk(), 1, NULL_TENSOR, None)                 # nothing to do: fine
        assert np.array_equal(acc.numpy(), want_acc)


def test_argument_errors_launch_nothing():
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import NULL_TENSOR, MskError
    shape = (2, 3, 5, 7, 3)
    n, d, h, w, c = shape
    x = _rand(shape, 6)
    with Owned() as o:
        dev = o.dev
        a, other = o.upload(x), o.upload(_rand((2, 3, 5, 8, 3), 7))
        b = o.upload(np.full_like(x, 7.0))
        pred = o.ints(n * d * h * w, -1)
        bad = [("msk_flip_axes", (a.msk(), other.msk(), 1)), ("msk_flip_axes", (a.msk(), b.msk(), 8)),
               ("msk_flip_axes", (a.msk(), b.msk(), -1)), ("msk_flip_axes", (a.msk(), a.msk(), 1)),
               ("msk_flip_axes", (a.msk(), NULL_TENSOR, 0)),
               ("msk_tta_accumulate", (other.msk(), 0, b.msk(), 1)), ("msk_tta_accumulate", (a.msk(), 8, b.msk(), 1)),
               ("msk_tta_accumulate", (a.msk(), -1, b.msk(), 0)), ("msk_tta_accumulate", (a.msk(), 0, a.channel_slice(0, 2).msk(), 1)),
               ("msk_tta_finish", (a.msk(), 0, b.msk(), C.c_void_p(pred))), ("msk_tta_finish", (a.msk(), -3, b.msk(), None)),
               ("msk_tta_finish", (a.msk(), 1, other.msk(), C.c_void_p(pred)))]
        for name, args in bad:
            rc = getattr(dev.lib, name)(dev.ctx, *args)
            assert rc != 0, (name, args[1:])
            assert _lib.last_error(dev.ctx), name
            with pytest.raises(MskError, match=name):
                dev.call(name, *args)
        assert (b.numpy() == 7.0).all() and (dev.d2h(pred, (n * d * h * w,), np.int32) == -1).all()
        assert np.array_equal(a.numpy(), x)


# ---- aug_inference ---------------------------------------------------------------------------------------------------------
def _stub(f, calls=None):
    from medicalseg_amd.device import to_tensor

    def model(x):
        a = x.numpy()
        if calls is not None:
            calls.append(a)
        return [to_tensor(f(a))]
    return model


def _statement(o, logits_per_pass, masks):
    return R.tta_reference([o.softmax(o.upload(lg)) for lg in logits_per_pass], masks)


@pytest.mark.parametrize("axes", [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2), (2, 0)])
def test_aug_inference_plumbing_with_a_host_stub(axes):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    x = _rand((1, 6, 10, 14, 1), 40)
    masks = [m for _, m in infer.tta_passes(1.0, axes)]
    calls = []
    pred, probs, plain = infer.aug_inference(_stub(R.ramp_model, calls), to_tensor(x), flip_axes=axes, with_plain=True)
    assert len(calls) == len(masks) == 2 ** len(axes)
    for got, m in zip(calls, masks):
        assert np.array_equal(got, R.flip(x, m))                                   # what the model was shown
    with Owned() as o:
        _, want_probs, want_pred = _statement(o, [R.ramp_model(R.flip(x, m)) for m in masks], masks)
    assert pred.shape == (1, 1, 6, 10, 14) and probs.shape == (1, 3, 6, 10, 14)
    assert np.array_equal(probs.numpy(), want_probs)
    assert np.array_equal(pred.numpy()[:, 0], want_pred)
    assert np.array_equal(plain.numpy(), R.ramp_model(x))
    two = infer.aug_inference(_stub(R.ramp_model), to_tensor(x), flip_axes=axes)
    assert len(two) == 2 and np.array_equal(two[1].numpy(), want_probs)


def test_aug_inference_of_a_flip_equivariant_model_is_the_plain_softmax():
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    x = _rand((1, 6, 10, 14, 1), 41)
    with Owned() as o:
        p = o.softmax(o.upload(R.pointwise_model(x)))
    for axis in range(3):
        pred, probs = infer.aug_inference(_stub(R.pointwise_model), to_tensor(x), flip_axes=(axis,))
        assert np.array_equal(probs.numpy(), p)                                    # (P + P) * 0.5 == P
        assert np.array_equal(pred.numpy()[:, 0], np.argmax(p, axis=1))


def _vnet(seed=5):
    from medicalseg_amd.models import VNet
    rng = np.random.default_rng(seed)
    model = VNet(num_classes=3)
    state = model.state_dict()
    for k_, v in state.items():                      # non-trivial running statistics and slopes
        if k_.endswith("._mean"):
            state[k_] = rng.standard_normal(v.shape).astype(np.float32) * 0.1
        elif k_.endswith("._variance"):
            state[k_] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif "relu" in k_ and k_.endswith("_weight"):
            state[k_] = rng.uniform(0.1, 0.4, v.shape).astype(np.float32)
    model.set_state_dict(state)
    model.eval()
    return model


@pytest.fixture(scope="module")
def vnet():
    return _vnet()


def _device_softmax_of(logit):
    from medicalseg_amd.device import Tensor
    p = Tensor.empty(logit.dev, logit.n, logit.d, logit.h, logit.w, logit.c)
    logit.dev.call("msk_softmax_c", logit.msk(), p.msk())
    return p.numpy()


def _resized(o, ncdhw, size):
    """msk_interp_trilinear_fwd of a host array -> host array"""
    src = o.upload(ncdhw)
    dst = o.empty(src.n, size[0], size[1], size[2], src.c)
    o.dev.call("msk_interp_trilinear_fwd", src.msk(), dst.msk())
    return dst.numpy()


def _mem_free(dev):
    free, total = C.c_size_t(), C.c_size_t()
    dev.sync()
    dev.call("msk_mem_info", C.byref(free), C.byref(total))
    return free.value


def test_aug_inference_of_a_real_net_equals_the_hand_composition(vnet):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    x = _rand((1, 16, 16, 16, 1), 42)
    sm, plain_logits = [], None
    for m in range(8):
        _, logit = infer.inference(vnet, to_tensor(R.flip(x, m)))
        if m == 0:
            plain_logits = logit.numpy()
        sm.append(_device_softmax_of(logit))
    _, want_probs, want_pred = R.tta_reference(sm, list(range(8)))
    pred, probs, plain = infer.aug_inference(vnet, to_tensor(x), flip_axes=(0, 1, 2), with_plain=True)
    assert np.array_equal(probs.numpy(), want_probs)
    assert np.array_equal(pred.numpy()[:, 0], want_pred)
    assert np.array_equal(plain.numpy(), plain_logits)
    # a second call at the same shape allocates no device memory
    dev = probs.dev
    before = _mem_free(dev)
    pred2, probs2, _ = infer.aug_inference(vnet, to_tensor(x), flip_axes=(0, 1, 2), with_plain=True)
    assert np.array_equal(probs2.numpy(), want_probs) and np.array_equal(pred2.numpy()[:, 0], want_pred)
    assert _mem_free(dev) == before
    # the tensors of the first call belong to an earlier forward
    from medicalseg_amd._lib import MskError
    with pytest.raises(MskError, match="stale"):
        probs.numpy()


def test_aug_inference_resizes_the_mean_probabilities_to_ori_shape(vnet):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor

    class Resize3D:
        size = (16, 16, 16)
    x = _rand((1, 16, 16, 16, 1), 43)
    _, mean = infer.aug_inference(vnet, to_tensor(x), flip_axes=(0, 1, 2))
    mean = mean.numpy()
    with Owned() as o:
        want = _resized(o, mean, (24, 20, 31))
    pred, probs = infer.aug_inference(vnet, to_tensor(x), ori_shape=(24, 20, 31), transforms=[Resize3D()], flip_axes=(0, 1, 2))
    assert probs.shape == (1, 3, 24, 20, 31) and pred.shape == (1, 1, 24, 20, 31)
    assert np.array_equal(probs.numpy(), want)
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))            # the argmax comes after the resize


def test_aug_inference_with_scales_equals_the_hand_composition(vnet):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import Tensor, to_tensor
    x = _rand((1, 32, 32, 32, 1), 44)
    scales, sm, masks = [0.5, 1.0, 1.5], [], []
    with Owned() as o:
        for s in scales:
            xs = x if s == 1.0 else _resized(o, x, infer.tta_size((32, 32, 32), s))
            for m in (0, 4):
                _, logit = infer.inference(vnet, to_tensor(R.flip(xs, m)))
                assert logit.shape[2:] == infer.tta_size((32, 32, 32), s)
                if s != 1.0:
                    back = Tensor.empty(logit.dev, 1, 32, 32, 32, logit.c)
                    logit.dev.call("msk_interp_trilinear_fwd", logit.msk(), back.msk())
                    logit = back
                sm.append(_device_softmax_of(logit))
                masks.append(m)
    _, want_probs, want_pred = R.tta_reference(sm, masks)
    pred, probs = infer.aug_inference(vnet, to_tensor(x), scales=scales, flip_axes=(2,))
    assert np.array_equal(probs.numpy(), want_probs)
    assert np.array_equal(pred.numpy()[:, 0], want_pred)


# ---- evaluate --------------------------------------------------------------------------------------------------------------
def _eval_setup():
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    ds = SyntheticCT(num_samples=3, shape=(16, 16, 16), num_classes=3, mode="val")
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    return ds, losses


def test_evaluate_without_aug_eval_is_the_plain_loop(vnet):
    """the loop evaluate ran before aug_eval existed, by hand: inference, the loss's dice, the host AUC of msk_softmax_c"""
    from medicalseg_amd import nn
    from medicalseg_amd.core import evaluate, infer
    from medicalseg_amd.datasets import DataLoader
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import loss_computation, metric
    ds, losses = _eval_setup()
    mdice, scores, labels = 0.0, [], []
    with nn.fused_inference():
        for im, label, idx in DataLoader(ds, batch_size=1, shuffle=False, drop_last=False, num_workers=0):
            pred, logits = infer.inference(vnet, to_tensor(im), ori_shape=label.shape[-3:], transforms=ds.transforms.transforms)
            _, pcd = loss_computation(logits, to_tensor(label.astype('int32')), losses)
            scores.append(_device_softmax_of(logits))
            labels.append(np.asarray(label))
            mdice += np.mean(np.asarray(pcd))
    want = {"mdice": float(mdice / 3), "auc_roc": metric.auc_roc(np.concatenate(scores), np.concatenate(labels), num_classes=3)}
    got = evaluate(vnet, ds, losses, print_detail=False, auc_roc=True)
    assert got == want
    assert evaluate(vnet, ds, losses, print_detail=False, auc_roc=True, aug_eval=False, scales=[0.5], flip_axes=(0, 1)) == want


def test_evaluate_with_aug_eval(vnet):
    from medicalseg_amd.core import evaluate, infer
    from medicalseg_amd.datasets import DataLoader
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import metric
    ds, losses = _eval_setup()
    plain = evaluate(vnet, ds, losses, print_detail=False, hard_metrics=True, auc_roc=True)
    got = evaluate(vnet, ds, losses, print_detail=False, hard_metrics=True, auc_roc=True, aug_eval=True, flip_axes=(0, 1, 2))
    dev_auc = evaluate(vnet, ds, losses, print_detail=False, auc_roc=True, auc_device=True, aug_eval=True, flip_axes=(0, 1, 2))
    assert got["mdice"] == plain["mdice"] == dev_auc["mdice"]                      # the plain pass's, as before
    counts = None
    scores, labels = [], []
    for it, (im, label, idx) in enumerate(DataLoader(ds, batch_size=1, shuffle=False, drop_last=False, num_workers=0)):
        pred, probs = infer.aug_inference(vnet, to_tensor(im), flip_axes=(0, 1, 2))
        if counts is None:
            counts = metric.ConfusionCounts(pred.dev, 3, 3, 255, zero=True)
        metric.confusion_counts(pred, to_tensor(label.astype('int32')), 3, 255, out=counts.rows(it, len(label)))
        scores.append(probs.numpy())
        labels.append(np.asarray(label))
    c = counts.numpy()
    counts.free()
    areas = metric.areas_from_counts(c, 3, 255)
    class_iou, miou = metric.mean_iou(*areas)
    class_dice, hdice = metric.dice(*areas)
    assert got["miou"] == float(miou) and got["dice"] == float(hdice)
    assert np.array_equal(got["class_iou"], class_iou) and np.array_equal(got["class_dice"], class_dice)
    assert got["acc"] == float(metric.accuracy(areas[0], areas[1])[1]) and got["kappa"] == float(metric.kappa(*areas))
    want_auc = metric.auc_roc(np.concatenate(scores), np.concatenate(labels), num_classes=3)
    assert got["auc_roc"] == want_auc == dev_auc["auc_roc"]
    print("aug_eval: auc %.6f (plain %.6f), miou %.6f (plain %.6f)" % (got["auc_roc"], plain["auc_roc"], got["miou"], plain["miou"]))
    with pytest.raises(ValueError):
        evaluate(vnet, ds, losses, print_detail=False, aug_eval=True, scales=[0.5, 1.5])

"""BCELoss on the device (msk_bce_fwd / msk_bce_bwd, medicalseg_amd/csrc/msk_loss_bce.hip) against the float64
restatement tests/bce_reference.py, and BCELoss inside the training stack (MixedLoss with DiceLoss on the same logits,
a one-channel head, VNetDeepSup's four outputs, train() + evaluate() from the shipped YAML).

Bounds: the loss is a sum of fp32 per-workgroup partials combined in fp64 (relative error <= 1e-5); the gradient is
per element in fp32 from stable sigmoids (relative L2 <= 1e-6, max-abs <= 1e-5 max|g|)."""
import ctypes as C
import os

import numpy as np
import pytest

import bce_reference as R
from helpers import dev, dmalloc, redzone_check, t_from_ncdhw, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {None: 0, 'dynamic': 1}


def _pw_args(pos_weight):
    if pos_weight is None:
        return 0, 0.0
    if pos_weight == 'dynamic':
        return 2, 0.0
    return 1, float(pos_weight)


def _labels(rng, N, D, H, W, Cn, ignore_frac=0.1):
    y = rng.integers(0, max(Cn, 2), (N, D, H, W)).astype(np.int32)
    y[rng.random(y.shape) < ignore_frac] = 255
    if Cn > 1:
        y.flat[1] = Cn + 2          # outside [0, C), not ignored: an all-zero target row
    return y


def _device_labels(y):
    d = dev()
    p = dmalloc(y.nbytes)
    d.h2d(p, y)
    return p


def _fwd(zt, yp, weight, pos_weight):
    d = dev()
    out, stats = vec(np.zeros(4)), dmalloc(8 * 8)
    pwm, pwv = _pw_args(pos_weight)
    d.call("msk_bce_fwd", zt.msk(), vp(yp), 255, MODES[weight], pwm, C.c_float(pwv), vp(out), vp(stats))
    return float(vec_back(out, 1)[0]), stats


def _grad_ok(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    if scale == 0:
        return not got.any()
    l2 = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    return l2 <= 1e-6 and np.abs(got - ref).max() <= 1e-5 * scale


def _close_with_dice(got, ref):
    """BCE + Dice gradient against float64: the dice term's statistics are fp32 sums over the volume, so the bound of the
    existing CE / Dice kernel tests (tests/test_gpu_ops.py test_loss_fwd_bwd: 2e-5 of max|g|) applies to the sum"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()


def _loss_ok(got, ref):
    return abs(got - ref) <= 1e-5 * abs(ref) if ref != 0 else got == 0


@pytest.mark.parametrize("layout", ["dense", "dense_acc", "slice", "slice_acc"])
@pytest.mark.parametrize("pos_weight", [None, 2.5, 'dynamic'])
@pytest.mark.parametrize("weight", [None, 'dynamic'])
@pytest.mark.parametrize("shape", [(2, 16, 16, 16), (1, 5, 7, 9)])
@pytest.mark.parametrize("Cn", [1, 2, 3, 20])
def test_bce_kernels_match_restatement(Cn, shape, weight, pos_weight, layout):
    d = dev()
    N, D, H, W = shape
    rng = np.random.default_rng(Cn * 1000 + D)
    z = (rng.standard_normal((N, Cn, D, H, W)) * 2).astype(np.float32)
    y = _labels(rng, N, D, H, W, Cn)
    yp = _device_labels(y)
    sliced, acc = layout.startswith("slice"), layout.endswith("acc")
    c0, wide = (1, Cn + 3) if sliced else (0, Cn)
    zw = np.zeros((N, wide, D, H, W), np.float32)
    zw[:, c0:c0 + Cn] = z
    zt = t_from_ncdhw(zw).channel_slice(c0, c0 + Cn) if sliced else t_from_ncdhw(z)
    loss, stats = _fwd(zt, yp, weight, pos_weight)
    ref_loss, ref_g = R.bce(z, y, 255, weight, pos_weight)
    assert _loss_ok(loss, ref_loss), (loss, ref_loss)
    # dlogits: a channel slice of a wider buffer too; with accumulate the old values stay underneath
    coef = 0.75
    base = (rng.standard_normal((N, wide, D, H, W)) * np.abs(ref_g).max()).astype(np.float32)
    dw = t_from_ncdhw(base)
    dt = dw.channel_slice(c0, c0 + Cn) if sliced else dw
    d.call("msk_bce_bwd", zt.msk(), vp(yp), 255, vp(stats), C.c_float(coef), int(acc), dt.msk())
    got = dw.numpy()
    want = coef * ref_g + (base[:, c0:c0 + Cn].astype(np.float64) if acc else 0.0)
    assert _grad_ok(got[:, c0:c0 + Cn], want)
    if sliced:   # the other channels of the wide buffer are untouched
        assert np.array_equal(got[:, :c0], base[:, :c0]) and np.array_equal(got[:, c0 + Cn:], base[:, c0 + Cn:])


@pytest.mark.parametrize("Cn", [1, 3])
def test_bce_all_voxels_ignored(Cn):
    d = dev()
    rng = np.random.default_rng(5)
    z = rng.standard_normal((1, Cn, 5, 7, 9)).astype(np.float32)
    y = np.full((1, 5, 7, 9), 255, np.int32)
    yp = _device_labels(y)
    zt = t_from_ncdhw(z)
    for weight in (None, 'dynamic'):
        for pos_weight in (None, 2.5, 'dynamic'):
            loss, stats = _fwd(zt, yp, weight, pos_weight)
            assert loss == 0.0
            dz = t_from_ncdhw(np.full_like(z, 7.0))
            d.call("msk_bce_bwd", zt.msk(), vp(yp), 255, vp(stats), C.c_float(1.0), 0, dz.msk())
            assert not dz.numpy().any()


def test_bce_bench_shape_matches_and_is_bitwise_repeatable():
    """2 x 128^3, 3 classes (the bench shape): the same comparison, and two evaluations give identical bits."""
    d = dev()
    rng = np.random.default_rng(128)
    N, Cn, S = 2, 3, 128
    z = (rng.standard_normal((N, Cn, S, S, S)) * 2).astype(np.float32)
    y = _labels(rng, N, S, S, S, Cn)
    yp = _device_labels(y)
    zt = t_from_ncdhw(z)
    ref_loss, ref_g = R.bce(z, y, 255, 'dynamic', 'dynamic')
    runs = []
    for _ in range(2):
        loss, stats = _fwd(zt, yp, 'dynamic', 'dynamic')
        dz = t_from_ncdhw(np.zeros_like(z))
        d.call("msk_bce_bwd", zt.msk(), vp(yp), 255, vp(stats), C.c_float(1.0), 0, dz.msk())
        runs.append((loss, d.d2h(stats, (8,), np.float64), dz.numpy()))
    assert _loss_ok(runs[0][0], ref_loss)
    assert _grad_ok(runs[0][2], ref_g)
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    # the counts are exact: mask, pos, neg
    st = runs[0][1]
    onehot = R.targets(y, Cn)
    assert st[5] == np.count_nonzero(y != 255)
    assert st[6] == np.count_nonzero(onehot == 1) and st[7] == np.count_nonzero(onehot == 0)


class _Capture:
    """Stands in as the producer of a logits tensor: records the gradient Scalar.backward hands over (and passes it on)."""
    num_outputs = 1

    def __init__(self, inner=None):
        self.inner, self.grads = inner, []

    def backward(self, g):
        self.grads.append(g.numpy())
        if self.inner is not None:
            self.inner.backward(g)


def _dice_grad(z, y, ignore_index=255):
    """d DiceLoss(sigmoid_norm=True) / d logits, float64 (as tests/test_gpu_ops.py states it)."""
    z = z.astype(np.float64)
    Cn = z.shape[1]
    s = 1 / (1 + np.exp(-z))
    ysafe = np.where((y >= 0) & (y < Cn), y, 0)
    t = np.moveaxis(np.eye(Cn)[ysafe], -1, 1) * ((y != ignore_index) & (y >= 0) & (y < Cn))[:, None]
    inter, den = (s * t).sum((0, 2, 3, 4)), (s * s).sum((0, 2, 3, 4)) + (t * t).sum((0, 2, 3, 4))
    den = np.maximum(den, 1e-6).reshape(1, -1, 1, 1, 1)
    return -(1.0 / Cn) * (2 * t / den - (2 * inter.reshape(1, -1, 1, 1, 1) / den ** 2) * 2 * s) * s * (1 - s)


def test_mixed_bce_dice_gradient_is_the_sum_of_both():
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import BCELoss, DiceLoss, MixedLoss, VNet
    rng = np.random.default_rng(32)
    model = VNet(num_classes=3)
    model.train()
    x = rng.standard_normal((1, 1, 32, 32, 32)).astype(np.float32)
    y = _labels(rng, 1, 32, 32, 32, 3)
    yt = to_tensor(y)
    logits = model(x)[0]
    z = logits.numpy()

    def grad_of(make_loss):
        cap = _Capture()
        logits.producer = cap
        make_loss().backward()
        return cap.grads[0]

    mixed = MixedLoss([BCELoss(), DiceLoss()], [1, 1])
    g_mixed = grad_of(lambda: sum(mixed(logits, yt)[0]))
    g_bce = grad_of(lambda: BCELoss()(logits, yt))
    g_dice = grad_of(lambda: DiceLoss()(logits, yt)[0])
    both = g_bce.astype(np.float64) + g_dice
    assert np.abs(g_mixed - both).max() <= 1e-6 * np.abs(both).max()
    _, ref = R.bce(z, y)
    assert _grad_ok(g_bce, ref)
    assert _close_with_dice(g_mixed, ref + _dice_grad(z, y))
    # the values: BCE term + dice term, each where the restatement puts it
    loss_list, dice = mixed(logits, yt)
    assert _loss_ok(float(loss_list[0]), R.bce(z, y)[0])


def test_one_channel_vnet_bce_dice_trains():
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import BCELoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(1)
    model = VNet(num_classes=1)
    model.train()
    opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    losses = {"types": [MixedLoss([BCELoss(), DiceLoss()], [1, 1])], "coef": [1]}
    x = rng.standard_normal((1, 1, 32, 32, 32)).astype(np.float32)
    y = rng.integers(0, 2, (1, 32, 32, 32)).astype(np.int32)
    y[rng.random(y.shape) < 0.1] = 255
    values = []
    for step in range(5):
        logits_list = model(x)
        cap = _Capture(model)
        logits_list[0].producer = cap
        z = logits_list[0].numpy() if step == 0 else None
        loss_list, _ = loss_computation(logits_list, to_tensor(y), losses)
        loss = sum(loss_list)
        loss.backward()
        opt.step()
        values.append(float(loss))
        if step == 0:
            ref = R.bce(z, y)[1] + _dice_grad(z, y)
            assert _close_with_dice(cap.grads[0], ref)
    assert np.all(np.isfinite(values))
    assert all(np.isfinite(p.numpy()).all() for p in model.parameters())


def test_vnet_deepsup_bce_on_every_output():
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import BCELoss, VNetDeepSup
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(4)
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3)
    model.train()
    opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    losses = {"types": [BCELoss() for _ in range(4)], "coef": [0.25] * 4}
    x = rng.standard_normal((1, 1, 32, 32, 32)).astype(np.float32)
    y = _labels(rng, 1, 32, 32, 32, 3)
    outs = model(x)
    assert len(outs) == 4
    loss_list, _ = loss_computation(outs, to_tensor(y), losses)
    assert len(loss_list) == 4
    for o, term in zip(outs, loss_list):
        assert _loss_ok(float(term), 0.25 * R.bce(o.numpy(), y)[0])
    loss = sum(loss_list)
    loss.backward()
    opt.step()
    assert np.isfinite(float(loss))
    assert all(np.isfinite(p.numpy()).all() for p in model.parameters())


def test_train_and_evaluate_from_bce_yaml(tmp_path):
    import warnings

    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.core import evaluate, train
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import VNet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # data_root warning
        cfg = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_bce_128.yml"))
    for key in ("train_dataset", "val_dataset"):
        cfg.dic[key]["shape"] = [32, 32, 32]
    ds, val = cfg.train_dataset, cfg.val_dataset
    assert ds.shape == (32, 32, 32)
    losses = cfg.loss
    model = cfg.model                 # the YAML's model: block (VNet, 3 classes) and optimizer (sgd -> Momentum)
    assert isinstance(model, VNet) and model.num_classes == 3
    opt = cfg.optimizer
    assert isinstance(opt, optim.Momentum)
    train(model, ds, val_dataset=val, optimizer=opt, save_dir=str(tmp_path / "out"), iters=3, batch_size=2,
          save_interval=3, log_iters=1, losses=losses, keep_checkpoint_max=1)
    assert os.path.exists(tmp_path / "out" / "iter_3" / "model.pdparams")
    res = evaluate(model, val, losses, print_detail=True)
    assert np.isfinite(res["mdice"])

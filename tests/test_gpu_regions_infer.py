"""Region-based training on the device beyond the loss kernels: msk_regions_to_label against the statement
(tests/mlabel_reference.py), inference / sliding_window_inference with `regions`, DiceBCERegionLoss inside the training stack
(VNet and the native deep-supervision heads) and evaluate's region Dice."""
import ctypes as C

import numpy as np
import pytest

import mlabel_cases as K
import mlabel_reference as M
from helpers import dev, dmalloc, redzone_check, t_from_ncdhw, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

REGIONS, ORDER = [[1, 2, 3], [2, 3], [3]], [1, 2, 3]


def _special(z):
    """0, -0.0, NaN, a denormal and a tiny positive logit, +-inf: only what is above 0 fires"""
    R = z.shape[1]
    vals = np.array([0.0, -0.0, np.nan, 1e-45, 1e-30, -1e-45, np.inf, -np.inf], np.float32)
    for k in range(12):
        z[0, :, 0, 0, k % z.shape[4]] = np.roll(vals, k)[np.arange(R) % vals.size]
    return z


@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 9, 16, 17)])
@pytest.mark.parametrize("R", [1, 3, 4, 8, 20])
def test_regions_to_label_equals_statement(R, shape, layout):
    d = dev()
    N, D, H, W = shape
    rng = np.random.default_rng(R * 100 + D)
    z = _special(rng.standard_normal((N, R, D, H, W)).astype(np.float32))
    order = [int(v) for v in rng.permutation(np.arange(1, 40))[:R]]
    c0, wide = (1, R + 3) if layout == "slice" else (0, R)
    zw = np.zeros((N, wide, D, H, W), np.float32)
    zw[:, c0:c0 + R] = z
    zt = t_from_ncdhw(zw).channel_slice(c0, c0 + R) if layout == "slice" else t_from_ncdhw(z)
    out = dmalloc(N * D * H * W * 4)
    d.call("msk_regions_to_label", zt.msk(), (C.c_int32 * R)(*order), vp(out))
    got = d.d2h(out, (N, D, H, W), np.int32)
    assert np.array_equal(got, M.regions_to_label(z, order))
    assert len(np.unique(got)) > 1


def test_regions_to_label_argument_errors():
    d = dev()
    from medicalseg_amd._lib import MskError, MskTensor
    t33 = t_from_ncdhw(np.zeros((1, 33, 2, 2, 2), np.float32))
    t3 = t_from_ncdhw(np.zeros((1, 3, 2, 2, 2), np.float32))
    out = dmalloc(8 * 4)
    order = (C.c_int32 * 33)(*range(33))
    with pytest.raises(MskError, match=r"\[1,32\]"):
        d.call("msk_regions_to_label", t33.msk(), order, vp(out))
    with pytest.raises(MskError, match="null"):
        d.call("msk_regions_to_label", t3.msk(), None, vp(out))
    with pytest.raises(MskError, match="null"):
        d.call("msk_regions_to_label", t3.msk(), order, None)
    with pytest.raises(MskError, match="aligned"):
        d.call("msk_regions_to_label", t3.msk(), order, C.c_void_p(out + 2))
    with pytest.raises(MskError, match="voxel count"):
        d.call("msk_regions_to_label", MskTensor(t3.ptr, 2, 1024, 1024, 1024, 3, 3), order, vp(out))
    assert np.all(d.d2h(out, (8,), np.uint32) == 0x7FC0BEEF)


def _vnet(train=False):
    from medicalseg_amd.models import VNet
    model = VNet(num_classes=3)
    model.train() if train else model.eval()
    return model


def test_inference_and_sliding_window_rebuild_the_label_map_from_their_logits():
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import RegionSpec
    model = _vnet()
    spec = RegionSpec(REGIONS, ORDER)
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 1, 16, 16, 16)).astype(np.float32)
    pred, logits = infer.inference(model, to_tensor(x), regions=spec)
    z, got = logits.numpy(), pred.numpy()
    assert got.shape == (1, 1, 16, 16, 16) and np.array_equal(got[:, 0], M.regions_to_label(z, ORDER))
    assert len(np.unique(got)) > 1                                    # an untrained net still fires somewhere and not everywhere
    x = rng.standard_normal((1, 1, 24, 16, 16)).astype(np.float32)
    pred, logits = infer.sliding_window_inference(model, to_tensor(x), (16, 16, 16), overlap=0.5, mirror_axes=(0,), regions=spec)
    z, got = logits.numpy(), pred.numpy()
    assert got.shape == (1, 1, 24, 16, 16) and np.array_equal(got[:, 0], M.regions_to_label(z, ORDER))
    # without regions the same call still ends in the arg-max
    pred, logits = infer.sliding_window_inference(model, to_tensor(x), (16, 16, 16), overlap=0.5, mirror_axes=(0,))
    assert np.array_equal(pred.numpy()[:, 0], logits.numpy().argmax(1))
    infer.sliding_release(dev())


class _Capture:
    """Stands in as the producer of a logits tensor: records the gradient Scalar.backward hands over (and passes it on)."""
    num_outputs = 1

    def __init__(self, inner=None):
        self.inner, self.grads = inner, []

    def backward(self, g):
        self.grads.append(g.numpy())
        if self.inner is not None:
            self.inner.backward(g)


def _labels(rng, shape):
    y = rng.integers(0, 4, shape).astype(np.int32)
    y[rng.random(shape) < 0.1] = 255
    return y


def test_one_training_step_of_vnet_hands_the_kernels_gradient_to_the_model():
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import DiceBCERegionLoss
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(32)
    model = _vnet(train=True)
    x = rng.standard_normal((2, 1, 16, 16, 16)).astype(np.float32)
    y = _labels(rng, (2, 16, 16, 16))
    logits = model(x)[0]
    z = logits.numpy()
    cap = _Capture(logits.producer)
    logits.producer = cap
    loss_fn = DiceBCERegionLoss(REGIONS, ORDER, lambda_dice=1.5, lambda_bce=0.5)
    loss_list, dice = loss_computation([logits], to_tensor(y), {"types": [loss_fn], "coef": [2.0]})
    loss = sum(loss_list)
    loss.backward()
    ref = M.mlabel_loss(z, y, M.build_table(REGIONS), False, True, K.SMOOTH, coef_bce=1.0, coef_dice=3.0)
    assert np.isfinite(float(loss)) and K.rel_ok(float(loss), ref["loss"])
    assert K.rel_ok(np.asarray(dice), ref["dice"])
    assert len(cap.grads) == 1 and K.grad_ok(cap.grads[0], ref["grad"])
    # ... and it is the kernel's own: the same call on the same logits gives the same bits
    d = dev()
    node = loss.terms[0][1]
    dz = t_from_ncdhw(np.zeros_like(z))
    zt = t_from_ncdhw(z)
    ptr, length = loss_fn.region_spec.device_table(d)
    d.call("msk_mlabel_loss_bwd", zt.msk(), vp(node.labels.ptr), 255, vp(ptr), length, 0, 1, C.c_float(K.SMOOTH), vp(node.stats_ptr),
           C.c_float(1.0), C.c_float(3.0), 0, dz.msk())
    assert np.array_equal(dz.numpy(), cap.grads[0])
    assert all(np.isfinite(p.grad_numpy()).all() for p in model.parameters() if p.arena is not None and p.arena.grad_ptr is not None)


def test_training_steps_on_native_deep_supervision_heads():
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import DiceBCERegionLoss, VNetDeepSup
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(4)
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    model.train()
    opt = optim.Momentum(1e-2, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    losses = {"types": [DiceBCERegionLoss(REGIONS, ORDER) for _ in range(4)], "coef": [0.25] * 4}
    x = rng.standard_normal((1, 1, 16, 16, 16)).astype(np.float32)
    y = _labels(rng, (1, 16, 16, 16))
    table = M.build_table(REGIONS)
    values = []
    for step in range(2):
        outs = model(x)
        assert [(o.d, o.h, o.w) for o in outs] == [(16, 16, 16), (2, 2, 2), (4, 4, 4), (8, 8, 8)]
        loss_list, dice = loss_computation(outs, to_tensor(y), losses)
        assert len(loss_list) == 4 and np.asarray(dice).shape == (3,)
        if step == 0:      # every head against ITS level of the label pyramid
            for o, term in zip(outs, loss_list):
                node = term.terms[0][1]
                yl = node.labels.numpy().reshape(1, o.d, o.h, o.w)
                ref = M.mlabel_loss(o.numpy(), yl, table, False, True, K.SMOOTH)
                assert K.rel_ok(float(term), 0.25 * ref["loss"])
        loss = sum(loss_list)
        loss.backward()
        grads_finite = all(np.isfinite(p.grad_numpy()).all() for p in model.parameters()
                           if p.arena is not None and p.arena.grad_ptr is not None)
        opt.step()
        values.append(float(loss))
        assert grads_finite
    assert np.all(np.isfinite(values)) and values[1] < values[0], values


def test_evaluate_region_dice_equals_numpy_on_the_downloaded_prediction():
    from medicalseg_amd.core import evaluate, infer
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import DiceBCERegionLoss
    model = _vnet()
    ds = SyntheticCT(num_samples=2, shape=(16, 16, 16), num_classes=4, mode="val")
    loss_fn = DiceBCERegionLoss(REGIONS, ORDER)
    res = evaluate(model, ds, {"types": [loss_fn], "coef": [1]}, print_detail=False, hard_metrics=True)
    inter, pa, la, per_case = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(3, np.int64), []
    from medicalseg_amd.datasets import DataLoader
    for im, label, _ in DataLoader(ds, batch_size=1, shuffle=False, drop_last=False):      # the volumes as evaluate sees them
        pred, _ = infer.inference(model, to_tensor(im), regions=loss_fn.region_spec)
        p, l = pred.numpy().reshape(16, 16, 16), np.asarray(label).reshape(16, 16, 16)
        valid = l != 255
        rows = [(int((np.isin(l, r) & np.isin(p, r) & valid).sum()), int((np.isin(p, r) & valid).sum()),
                 int((np.isin(l, r) & valid).sum())) for r in REGIONS]
        a, b, c = (np.array(v, np.int64) for v in zip(*rows))
        inter, pa, la = inter + a, pa + b, la + c
        per_case.append(np.mean([2 * a[r] / (b[r] + c[r]) if b[r] + c[r] else 0.0 for r in range(3)]))
    want = np.array([2 * inter[r] / (pa[r] + la[r]) if pa[r] + la[r] else 0.0 for r in range(3)])
    assert np.array_equal(res["class_region_dice"], want) and res["region_dice"] == float(np.mean(want))
    assert res["region_dice_per_case"] == float(np.mean(per_case))
    assert np.isfinite(res["mdice"]) and want.max() > 0


def test_train_and_evaluate_from_the_regions_yaml(tmp_path):
    import os
    import warnings

    from medicalseg_amd.core import evaluate, train
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceBCERegionLoss, VNet
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # data_root warning
        cfg = Config(os.path.join(root, "configs", "synthetic", "vnet_synthetic_ct_patch_regions_96.yml"))
    cfg.dic["train_dataset"]["shape"] = [20, 16, 24]
    cfg.dic["val_dataset"]["shape"] = [16, 16, 16]
    cfg.dic["train_dataset"]["transforms"][0]["size"] = [16, 16, 16]
    ds, val = cfg.train_dataset, cfg.val_dataset
    losses = cfg.loss
    assert isinstance(losses["types"][0], DiceBCERegionLoss) and losses["types"][0].ignore_index == 255
    model, opt = cfg.model, cfg.optimizer
    assert isinstance(model, VNet) and model.num_classes == 3
    train(model, ds, val_dataset=val, optimizer=opt, save_dir=str(tmp_path / "out"), iters=2, batch_size=2,
          save_interval=2, log_iters=1, losses=losses, keep_checkpoint_max=1)      # validates with the loss's region_spec
    assert os.path.exists(tmp_path / "out" / "iter_2" / "model.pdparams")
    res = evaluate(model, val, losses, print_detail=False, hard_metrics=True)
    assert np.isfinite(res["mdice"]) and np.asarray(res["class_region_dice"]).shape == (3,)

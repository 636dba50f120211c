"""BoundaryLoss / DiceBoundaryLoss WITHOUT a GPU: the statement tests/boundary_reference.py against Kervadec's one_hot2dist restated
with scipy, against torch autograd and on its edge cases, and the control flow of the loss objects, MixedLoss, loss_computation
and Scalar.backward through the real host stack over a stand-in library (tests/fake_msegk.c + fake_msegk_region.c + fake_msegk_pyramid.c +
fake_msegk_clip.c + fake_msegk_boundary.c; its numbers are garbage by construction)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import boundary_reference as B
import fake_lib
from fake_lib import calls, fake as _fake  # noqa: F401  (calls is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
YML = os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_diceboundary_96.yml")

fake_pkg = fake_lib.fake_pkg_fixture("fake_msegk.c", "fake_msegk_region.c", "fake_msegk_pyramid.c", "fake_msegk_clip.c",
                                    "fake_msegk_boundary.c")

VOLUMES = [(5, 6, 7), (12, 33, 65), (9, 17, 130)]
SPACINGS = [None, (2.5, 1.0, 0.7)]


# ---- the statement --------------------------------------------------------------------------------------------------------------
def _one_hot2dist(lab, c, spacing):
    """Kervadec's one_hot2dist for one class of one volume, restated with scipy, rounded to float32 as the statement is"""
    from scipy.ndimage import distance_transform_edt
    pos = lab == c
    if not pos.any():                                # his guard: an absent class keeps its zeros
        return np.zeros(lab.shape, np.float32)
    neg = ~pos
    return (distance_transform_edt(neg, sampling=spacing) * neg - (distance_transform_edt(pos, sampling=spacing) - 1) * pos).astype(np.float32)


@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "spaced"])
@pytest.mark.parametrize("shape", VOLUMES, ids=["5x6x7", "12x33x65", "9x17x130"])
def test_statement_is_one_hot2dist_bit_for_bit(shape, spacing):
    pytest.importorskip("scipy")
    lab = B.example_volume(shape, seed=shape[2])
    assert (lab == 1).any() and (lab == 2).any() and not (lab == 3).any() and (lab == 255).any()
    for c in (0, 1, 2, 255):                        # present and not filling the volume
        phi = B.signed_distance(lab, c, spacing)
        assert phi.dtype == np.float32 and np.array_equal(phi.view(np.uint32), _one_hot2dist(lab, c, spacing).view(np.uint32)), c
        inside_max = np.float32(1.0 - (1.0 if spacing is None else min(spacing)))      # 1 - the smallest step out of the class
        assert (phi[lab == c] <= inside_max).all() and (phi[lab != c] > 0).all()
    absent = B.signed_distance(lab, 3, spacing)     # an absent class: zeros, here and in the scipy formula
    assert not absent.any() and not np.signbit(absent).any() and not _one_hot2dist(lab, 3, spacing).any()
    full = B.signed_distance(np.full(shape, 4, np.int32), 4, spacing)   # a class that fills the volume
    assert not full.any() and not np.signbit(full).any()


@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "spaced"])
def test_a_one_voxel_class_gets_plus_zero(spacing):
    lab = np.zeros((5, 6, 7), np.int32)
    lab[2, 3, 4] = 1
    phi = B.signed_distance(lab, 1, spacing)
    if spacing is None:                              # d_in = 1: 1 - 1 = +0.0, not -(1 - 1) = -0.0
        assert phi[2, 3, 4] == 0.0 and not np.signbit(phi[2, 3, 4])
        assert phi[2, 3, 5] == 1.0 and phi[0, 3, 4] == 2.0 and phi[2, 0, 0] == 5.0
    else:                                            # d_in = 0.7, the smallest spacing: Kervadec's constant stays 1
        assert phi[2, 3, 4] == np.float32(1.0 - 0.7)
        assert phi[2, 3, 5] == np.float32(0.7) and phi[0, 3, 4] == np.float32(5.0)
    assert not np.signbit(phi[phi == 0]).any()
    lab2 = np.zeros((3, 3, 3), np.int32)
    lab2[1, 1, :] = 1                                # a line through the volume: every voxel of it has d_in = 1
    phi2 = B.signed_distance(lab2, 1)
    assert np.array_equal(phi2[1, 1, :].view(np.uint32), np.zeros(3, np.uint32))


def _torch_loss(torch, z, y, phi, S, ignore_index):
    Cn = z.shape[1]
    zt = torch.from_numpy(z).requires_grad_(True)
    p = torch.softmax(zt, dim=1)
    valid = torch.from_numpy(((y >= 0) & (y < Cn) & (y != ignore_index)))[:, None]
    t = p[:, S] * torch.from_numpy(phi.astype(np.float64)) * valid
    n_valid = int(valid.sum())
    loss = t.sum() / (max(n_valid, 1) * len(S))
    loss.backward()
    return float(loss), zt.grad.numpy()


@pytest.mark.parametrize("case", [((1, 5, 6, 7), 3, None), ((2, 12, 33, 65), 3, None), ((1, 9, 17, 130), 5, [1, 3]),
                                  ((1, 4, 16, 16), 20, None)], ids=["5x6x7", "2x12x33x65", "9x17x130-subset", "c20"])
def test_loss_and_gradient_are_autograd_s(case):
    torch = pytest.importorskip("torch")
    (N, D, H, W), Cn, classes = case
    rng = np.random.default_rng(D)
    y = np.stack([B.example_volume((D, H, W), seed=s) for s in range(N)])
    if Cn == 20:
        y = rng.integers(0, Cn, y.shape).astype(np.int32)
        y[:, :, 0, :] = 255
    y.flat[5] = Cn + 2                               # out of range, not ignored: takes no part
    z = rng.standard_normal((N, Cn, D, H, W)) * 2
    ref = B.boundary_loss(z, y, classes)
    want, grad = _torch_loss(torch, z, y, ref["phi"], ref["S"], 255)
    assert ref["n_valid"] == int(((y >= 0) & (y < Cn) & (y != 255)).sum()) < y.size
    assert abs(ref["loss"] - want) <= 1e-12 and np.abs(ref["grad"] - grad).max() <= 1e-12
    assert abs(ref["stats"][1] - ref["stats"][3:].sum()) <= 1e-9 and ref["abs"] >= abs(ref["loss"])
    outside = [c for c in range(Cn) if c not in ref["S"]]
    assert not ref["per_class"][outside].any() and np.abs(ref["grad"][:, outside]).max() > 0   # no term, but a gradient
    flat = np.moveaxis(ref["grad"], 1, -1).reshape(-1, Cn)
    assert not flat[(y.reshape(-1) == 255) | (y.reshape(-1) >= Cn)].any()
    # nothing ignored: Kervadec's (probs[:, idc] * dist_maps[:, idc]).mean()
    y2 = np.where((y == 255) | (y >= Cn), 0, y)
    ref2 = B.boundary_loss(z, y2, classes)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    assert abs(ref2["loss"] - (p[:, ref2["S"]] * ref2["phi"]).mean()) <= 1e-12
    # float32 evaluation stays far inside the device bounds
    r32 = B.boundary_loss(z.astype(np.float32), y, classes, dtype=np.float32)
    r64 = B.boundary_loss(z.astype(np.float32), y, classes)
    assert abs(r32["loss"] - r64["loss"]) <= 1e-6 * r64["abs"]
    assert np.abs(r32["grad"] - r64["grad"]).max() <= 2e-6 * np.abs(r64["grad"]).max()


def test_no_valid_voxel_gives_zero():
    z = np.random.default_rng(2).standard_normal((1, 3, 2, 3, 4))
    y = np.full((1, 2, 3, 4), 255, np.int32)
    y.flat[3] = 3
    for dtype in (np.float32, np.float64):
        ref = B.boundary_loss(z, y, dtype=dtype)
        assert ref["n_valid"] == 0 and ref["loss"] == 0.0 and ref["abs"] == 0.0 and not ref["grad"].any() and not ref["stats"].any()
    # another ignore_index: 255 is then out of range and takes no part either
    y = np.zeros((1, 2, 3, 4), np.int32)
    y[0, 0, 0, :2] = 1
    y[0, 1, 2, :] = 255
    assert B.boundary_loss(z, y, ignore_index=1)["n_valid"] == 24 - 2 - 4
    assert B.class_mask(3) == 0b110 and B.class_mask(5, [3, 1]) == 0b1010 and B.class_list(4, [2, 2, 0]) == [0, 2]


def test_metric_signed_distance_on_numpy_is_the_statement():
    from medicalseg_amd.utils import metric
    lab = B.example_volume((7, 9, 11), seed=3)
    for c in (1, 2, 3):
        for sp in SPACINGS:
            got = metric.signed_distance(lab, cls=c, spacing=sp)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), B.signed_distance(lab, c, sp).view(np.uint32))
    with pytest.raises(ValueError):
        metric.signed_distance(lab[0])
    with pytest.raises(ValueError):
        metric.signed_distance(lab, spacing=(1.0, -1.0, 1.0))


# ---- the loss objects over the stand-in library ------------------------------------------------------------------------------------
def _bcalls():
    return [_fake("fake_boundary_calls", C.c_long, i) for i in range(4)]


def _logits(model=None, n=1, classes=3):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import VNet
    model = model or VNet(num_classes=classes)
    model.train()
    rng = np.random.default_rng(0)
    outs = model(rng.standard_normal((n, 1, 16, 16, 16)).astype(np.float32))
    y = to_tensor(rng.integers(0, 3, (n, 16, 16, 16)).astype(np.int32))
    return model, outs, y


def test_the_yaml_builds_its_loss_model_and_optimizer(fake_pkg):
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceBoundaryLoss, VNet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = Config(YML)
        base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicetopk_96.yml"))
    assert cfg.dic["loss"] == {"types": [{"type": "DiceBoundaryLoss", "lambda_boundary": 0.01}], "coef": [1]}
    shipped = cfg.loss["types"][0]
    assert type(shipped) is DiceBoundaryLoss and shipped.ignore_index == 255 and shipped.classes is None and shipped.spacing is None
    assert shipped.batch_dice and not shipped.do_bg and (shipped.lambda_dice, shipped.lambda_boundary, shipped.smooth) == (1.0, 0.01, 1e-5)
    # everything but the loss is the dicetopk_96 recipe
    assert {k: v for k, v in cfg.dic.items() if k != "loss"} == {k: v for k, v in base.dic.items() if k != "loss"}
    assert type(cfg.model) is VNet and cfg.optimizer is not None


def test_both_are_registered_and_exported(fake_pkg):
    import medicalseg_amd.models as models
    from medicalseg_amd.cvlibs import manager
    from medicalseg_amd.models.losses import BoundaryLoss, DiceBoundaryLoss
    assert models.BoundaryLoss is BoundaryLoss and models.DiceBoundaryLoss is DiceBoundaryLoss
    assert manager.LOSSES["BoundaryLoss"] is BoundaryLoss and manager.LOSSES["DiceBoundaryLoss"] is DiceBoundaryLoss


def test_constructors_and_calls_refuse_the_argument_errors(fake_pkg):
    from medicalseg_amd.models import BoundaryLoss, DiceBoundaryLoss, VNet
    for make in (lambda: BoundaryLoss(classes=[]), lambda: BoundaryLoss(classes=[-1]), lambda: BoundaryLoss(classes=[64]),
                 lambda: DiceBoundaryLoss(classes=[1, 99]), lambda: BoundaryLoss(spacing=(1.0, 0.0, 1.0)),
                 lambda: DiceBoundaryLoss(spacing=(1.0, 2.0)), lambda: DiceBoundaryLoss(activation="sigmoid")):
        with pytest.raises(ValueError):
            make()
    BoundaryLoss(classes=[0, 63]), DiceBoundaryLoss(classes=(2, 1), spacing=[2.5, 1, 0.7])
    _, outs, y = _logits()
    for loss in (BoundaryLoss(classes=[1, 3]), DiceBoundaryLoss(classes=[3])):
        with pytest.raises(ValueError, match="3-class logits"):
            loss(outs[0], y)
    _, outs, y = _logits(VNet(num_classes=1))
    for loss in (BoundaryLoss(), DiceBoundaryLoss()):
        with pytest.raises(ValueError, match="2 .. 64"):
            loss(outs[0], y)
    wide = outs[0].empty_like()
    wide.c = 65
    with pytest.raises(ValueError, match="2 .. 64"):
        BoundaryLoss()(wide, y)


def test_boundary_is_sdf_then_forward_then_backward(fake_pkg, calls):
    from medicalseg_amd.models import BoundaryLoss
    from medicalseg_amd.models.losses.fused import BoundaryNode, Scalar
    _, outs, y = _logits()
    before = _bcalls()
    del calls[:]
    fn = BoundaryLoss(classes=[2, 1], spacing=(2.5, 1.0, 0.7), ignore_index=7)
    loss = fn(outs[0], y)
    assert isinstance(loss, Scalar) and len(loss.terms) == 1 and type(loss.terms[0][1]) is BoundaryNode and loss.terms[0][2] == "boundary"
    node = loss.terms[0][1]
    assert (BoundaryNode.SLOTS, BoundaryNode.writes) == ({"boundary": 0}, False) and node.stats_doubles() == 3 + 3
    assert not [c for c in calls if "boundary" in c or "sdf" in c]            # nothing runs before the value is asked for
    float(loss)
    (2.0 * loss).backward()
    assert [c for c in calls if "loss" in c or "sdf" in c] == ["msk_label_sdf", "msk_boundary_loss_fwd", "msk_boundary_loss_bwd"]
    assert [a - b for a, b in zip(_bcalls(), before)] == [1, 1, 1, 1]
    serial = [_fake("fake_boundary_serial", C.c_long, i) for i in range(3)]
    assert serial[0] < serial[1] < serial[2]
    assert [_fake("fake_boundary_last_int", C.c_int, i) for i in range(7)] == [0, 7, 1, 1, 16, 16, 16]
    assert [_fake("fake_boundary_last_mask", C.c_uint64, i) for i in range(3)] == [0b110] * 3
    assert [_fake("fake_boundary_last_spacing", C.c_double, i) for i in range(3)] == [2.5, 1.0, 0.7]
    assert _fake("fake_boundary_last_coef", C.c_float) == 2.0
    # forward and backward read the maps the sdf call wrote, and the backward the forward's record; labels are the loss's
    ptr = lambda i: _fake("fake_boundary_last_ptr", C.c_void_p, i)
    assert ptr(0) == ptr(1) == ptr(2) == node.phi_ptr and ptr(3) == ptr(4) == y.ptr and ptr(5) == node.ws_ptr
    assert ptr(6) == ptr(7) == node.stats_ptr
    assert _fake("fake_boundary_last_ws_bytes", C.c_size_t) == node.ws_bytes == 16 ** 3 * 16 + 512
    # a second evaluation of the same node launches nothing, and an equal loss shares the node
    del calls[:]
    assert BoundaryLoss(classes=[1, 2], spacing=(2.5, 1.0, 0.7), ignore_index=7)(outs[0], y).terms[0][1] is node
    assert BoundaryLoss(classes=[1])(outs[0], y).terms[0][1] is not node
    float(loss), float(fn(outs[0], y)), node.evaluate()
    assert not [c for c in calls if "boundary" in c or "sdf" in c]
    # no spacing: a null pointer; the default set is every class but 0
    float(BoundaryLoss()(outs[0], y))
    assert _fake("fake_boundary_last_int", C.c_int, 2) == 0 and _fake("fake_boundary_last_mask", C.c_uint64, 0) == 0b110


def test_diceboundary_dice_writes_and_boundary_adds(fake_pkg, calls):
    from medicalseg_amd.device import Device
    from medicalseg_amd.models import DiceBoundaryLoss
    from medicalseg_amd.models.losses.fused import BoundaryNode, RegionNode
    _, outs, y = _logits()
    del calls[:]
    before = _bcalls()
    fn = DiceBoundaryLoss(lambda_dice=2.0, lambda_boundary=0.5)
    loss, dice = fn(outs[0], y)
    assert [type(t[1]) for t in loss.terms] == [RegionNode, BoundaryNode] and np.asarray(dice).shape == (3,)
    assert _fake("fake_region_last_int", C.c_int, 1) == 0            # focal_on = 0: the region node carries the Dice term only
    float(loss)
    seen = []
    real = Device.call

    def spy(self, name, *args):
        if name in ("msk_region_loss_bwd", "msk_boundary_loss_bwd"):
            seen.append((name, args[-2]))
        return real(self, name, *args)
    Device.call, keep = spy, Device.call
    try:
        (3.0 * loss).backward()
    finally:
        Device.call = keep
    mine = [c for c in calls if "loss" in c or "sdf" in c]
    assert mine == ["msk_region_loss_fwd", "msk_label_sdf", "msk_boundary_loss_fwd", "msk_region_loss_bwd", "msk_boundary_loss_bwd"]
    assert seen == [("msk_region_loss_bwd", 0), ("msk_boundary_loss_bwd", 1)]
    assert (_fake("fake_region_last_coef", C.c_float, 0), _fake("fake_region_last_coef", C.c_float, 1)) == (0.0, 6.0)
    assert _fake("fake_boundary_last_coef", C.c_float) == 1.5
    assert [a - b for a, b in zip(_bcalls(), before)] == [1, 1, 1, 1]    # exactly one sdf call per node and forward
    # lambda_boundary is read at every forward: raised between iterations, the same node, a new coefficient, no new map
    fn.lambda_boundary = 0.25
    del calls[:]
    loss2, _ = fn(outs[0], y)
    assert loss2.terms[1][0] == 0.25 and loss2.terms[1][1] is loss.terms[1][1]
    float(loss2)
    assert not [c for c in calls if "boundary" in c or "sdf" in c]


def test_mixed_ce_boundary_adds_into_the_ce_gradient(fake_pkg, calls):
    from medicalseg_amd.models import BoundaryLoss, CrossEntropyLoss, MixedLoss
    _, outs, y = _logits()
    terms, dice = MixedLoss([CrossEntropyLoss(), BoundaryLoss()], [1, 0.25])(outs[0], y)
    assert dice is None and len(terms) == 2
    del calls[:]
    sum(terms).backward()
    mine = [c for c in calls if "loss" in c or "sdf" in c]
    assert mine.index("msk_label_sdf") < mine.index("msk_boundary_loss_fwd") < mine.index("msk_boundary_loss_bwd")
    assert mine.index("msk_loss_bwd_ex") < mine.index("msk_boundary_loss_bwd")
    assert [mine.count(c) for c in ("msk_loss_bwd_ex", "msk_label_sdf", "msk_boundary_loss_fwd", "msk_boundary_loss_bwd")] == [1, 1, 1, 1]
    assert _fake("fake_boundary_last_int", C.c_int, 0) == 1 and _fake("fake_boundary_last_coef", C.c_float) == 0.25


def test_loss_computation_passes_the_dice_through_and_deep_supervision_gets_a_node_per_head(fake_pkg, calls, monkeypatch):
    from medicalseg_amd.models import BoundaryLoss, DiceBoundaryLoss, MixedLoss, VNetDeepSup
    from medicalseg_amd.models.losses.fused import BoundaryNode
    from medicalseg_amd.utils import loss_computation
    _, outs, y = _logits()
    loss_list, dice = loss_computation(outs, y, {"types": [DiceBoundaryLoss()], "coef": [0.5]})
    assert len(loss_list) == 1 and len(loss_list[0].terms) == 2 and np.asarray(dice).shape == (3,)
    loss_list, dice = loss_computation(outs, y, {"types": [BoundaryLoss()], "coef": [1]})
    assert len(loss_list) == 1 and dice is None
    terms, dice = MixedLoss([BoundaryLoss(), DiceBoundaryLoss()], [1, 2])(outs[0], y)
    assert len(terms) == 2 and np.asarray(dice).shape == (3,)
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    _, outs, y = _logits(model)
    heads = [(o.d, o.h, o.w) for o in outs]
    assert len(set(heads)) > 1
    before = _bcalls()
    loss_list, dice = loss_computation(outs, y, {"types": [DiceBoundaryLoss() for _ in range(4)], "coef": [0.25] * 4})
    nodes = [t[1] for l in loss_list for t in l.terms if type(t[1]) is BoundaryNode]
    assert len(loss_list) == 4 and len({id(n) for n in nodes}) == 4
    for node, o in zip(nodes, outs):                 # the map is built from the head's own label level
        assert tuple(node.labels.shape) == (1, o.d, o.h, o.w)
    backwards = []
    real = type(model).backward
    monkeypatch.setattr(type(model), "backward", lambda self, grads: (backwards.append(grads), real(self, grads))[1])
    sum(loss_list).backward()
    assert [a - b for a, b in zip(_bcalls(), before)] == [4, 4, 4, 4]
    assert [_fake("fake_boundary_last_int", C.c_int, i) for i in range(3, 7)] == [1] + list(heads[-1])
    assert len(backwards) == 1 and len(backwards[0]) == 4 and all(g is not None for g in backwards[0])

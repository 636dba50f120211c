"""TopKLoss / DiceTopKLoss WITHOUT a GPU: the statement tests/topk_reference.py against torch and on its edge cases, and the
control flow of the loss objects, MixedLoss, loss_computation and Scalar.backward through the real host stack over a stand-in
library (tests/fake_msegk.c + fake_msegk_region.c + fake_msegk_topk.c; its numbers are garbage by construction)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import fake_lib
import topk_reference as T
from fake_lib import calls, fake as _fake  # noqa: F401  (calls is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DICETOPK_YML = os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicetopk_96.yml")

fake_pkg = fake_lib.fake_pkg_fixture("fake_msegk.c", "fake_msegk_region.c", "fake_msegk_topk.c")


# ---- the statement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 50, 100])
@pytest.mark.parametrize("weighted", [False, True])
def test_statement_is_torch_topk_of_cross_entropy(k, weighted):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(k)
    N, Cn, D, H, W = 2, 4, 5, 6, 7
    z = rng.standard_normal((N, Cn, D, H, W)) * 2
    y = rng.integers(0, Cn, (N, D, H, W)).astype(np.int32)
    w = rng.uniform(0.5, 2, Cn).astype(np.float32) if weighted else None
    ref = T.topk_ce(z, y, k, weight=w, dtype=np.float64)
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(z), torch.from_numpy(y.astype(np.int64)), reduction="none",
                                           weight=None if w is None else torch.from_numpy(w.astype(np.float64)))
    V = N * D * H * W
    want = torch.topk(ce.view(-1), int(V * k / 100), sorted=False)[0].mean().item()
    assert ref["K"] == int(V * k / 100) and ref["n_valid"] == V
    assert abs(ref["loss"] - want) <= 1e-12 * abs(want)
    # the gradient of the statement is autograd's where no two voxels tie
    zt = torch.from_numpy(z).requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(zt, torch.from_numpy(y.astype(np.int64)), reduction="none",
                                           weight=None if w is None else torch.from_numpy(w.astype(np.float64)))
    torch.topk(ce.view(-1), int(V * k / 100), sorted=False)[0].mean().backward()
    assert ref["record"][3] == 1
    assert np.abs(ref["grad"] - zt.grad.numpy()).max() <= 1e-12


def test_ordered_sum_is_the_library_s():
    from medicalseg_amd.transforms.transform import _ordered_sum
    rng = np.random.default_rng(1)
    for n in (1, 255, 4096, 4097, 70001):
        v = rng.standard_normal(n)
        assert T.ordered_sum(v) == _ordered_sum(v)


def test_sort_key_orders_the_zeros_and_round_trips():
    x = np.array([-np.inf, -2.0, -1e-45, -0.0, 0.0, 1e-45, 3.0, np.inf, np.nan], np.float32)
    k = T.sort_key(x)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(T.unsort_key(k).view(np.uint32), x.view(np.uint32))


def test_select_edge_cases():
    # all values equal: everything ties
    rec = T.select(np.full(10, 2.5, np.float32), 3)
    assert rec.tolist() == [2.5, 3, 0, 10, 0.0, 3, 0.3, 7.5]
    # K = 1 and K = n
    x = np.array([3.0, -1.0, 7.0, 7.0, 0.5], np.float32)
    assert T.select(x, 1).tolist() == [7.0, 1, 0, 2, 0.0, 1, 0.5, 7.0]
    assert T.select(x, 5).tolist() == [-1.0, 5, 4, 1, 17.5, 1, 1.0, 16.5]
    assert T.select(x, 3).tolist() == [3.0, 3, 2, 1, 14.0, 1, 1.0, 17.0]
    assert not T.select(x, 0).any()
    # negative values only
    assert T.select(np.array([-3.0, -1.0, -2.0], np.float32), 2).tolist() == [-2.0, 2, 1, 1, -1.0, 1, 1.0, -3.0]
    # -0.0 sorts below +0.0
    z = np.array([0.0, -0.0, -0.0, 0.0, -1.0], np.float32)
    r2, r3 = T.select(z, 2), T.select(z, 3)
    assert (r2[0], np.signbit(r2[0]), r2[2], r2[3]) == (0.0, False, 0, 2)
    assert (r3[0], bool(np.signbit(r3[0])), r3[2], r3[3], r3[5], r3[6]) == (0.0, True, 2, 2, 1, 0.5)
    # the sum above T takes the fixed order: 5000 values span two chunks
    rng = np.random.default_rng(0)
    v = rng.standard_normal(5000).astype(np.float32)
    rec = T.select(v, 500)
    top = np.sort(v)[::-1][:500]
    assert rec[0] == top[-1] and rec[2] + rec[5] == 500
    assert abs(rec[7] - top.astype(np.float64).sum()) <= 1e-12 * abs(rec[7])
    assert rec[4] == T.ordered_sum(np.where(T.sort_key(v) > T.sort_key(np.float32(rec[0]))[0], v.astype(np.float64), 0.0))


def test_no_valid_voxel_and_the_k_rule():
    z = np.random.default_rng(2).standard_normal((1, 3, 2, 3, 4))
    y = np.full((1, 2, 3, 4), 255, np.int32)
    for dtype in (np.float32, np.float64):
        ref = T.topk_ce(z, y, 10, dtype=dtype)
        assert ref["K"] == 0 and ref["loss"] == 0.0 and not ref["record"].any() and not ref["grad"].any()
        assert np.all(ref["l"] == -1.0)
    assert [T.k_of(n, 10) for n in (0, 1, 9, 10, 19, 20, 1000)] == [0, 1, 1, 1, 1, 2, 100]
    assert T.k_of(7, 100) == 7 and T.k_of(1000, 0.05) == 1 and T.k_of(3000, 0.1) == 3
    # a label outside [0, C) takes no part either, and ignored voxels are not counted in K
    y = np.zeros((1, 2, 3, 4), np.int32)
    y.flat[:4] = 255
    y.flat[4] = 7
    ref = T.topk_ce(z, y, 50, dtype=np.float64)
    assert ref["n_valid"] == 19 and ref["K"] == 9
    assert np.all(ref["l"][:5] == -1.0) and np.all(ref["l"][5:] >= 0) and not np.moveaxis(ref["grad"], 1, -1).reshape(-1, 3)[:5].any()


# ---- the loss objects over the stand-in library ------------------------------------------------------------------------------------
def _topk_calls():
    return [_fake("fake_topk_calls", C.c_long, i) for i in range(4)]


def _logits(model=None, n=1, classes=3):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import VNet
    model = model or VNet(num_classes=classes)
    model.train()
    rng = np.random.default_rng(0)
    outs = model(rng.standard_normal((n, 1, 16, 16, 16)).astype(np.float32))
    y = to_tensor(rng.integers(0, 3, (n, 16, 16, 16)).astype(np.int32))
    return model, outs, y


def test_the_yaml_builds_through_config(fake_pkg):
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceTopKLoss
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = Config(DICETOPK_YML)
        base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicece_96.yml"))
    assert cfg.dic["loss"] == {"types": [{"type": "DiceTopKLoss", "k": 10}], "coef": [1]}
    shipped = cfg.loss["types"][0]
    assert type(shipped) is DiceTopKLoss and shipped.k == 10.0 and shipped.ignore_index == 255
    assert shipped.batch_dice and not shipped.do_bg and (shipped.lambda_dice, shipped.lambda_topk, shipped.smooth) == (1.0, 1.0, 1e-5)
    # everything but the loss is the dicece_96 recipe
    assert {k: v for k, v in cfg.dic.items() if k != "loss"} == {k: v for k, v in base.dic.items() if k != "loss"}


def test_both_are_registered_and_exported(fake_pkg):
    import medicalseg_amd.models as models
    from medicalseg_amd.cvlibs import manager
    from medicalseg_amd.models.losses import DiceTopKLoss, TopKLoss
    assert models.TopKLoss is TopKLoss and models.DiceTopKLoss is DiceTopKLoss
    assert manager.LOSSES["TopKLoss"] is TopKLoss and manager.LOSSES["DiceTopKLoss"] is DiceTopKLoss


def test_constructors_and_calls_refuse_the_argument_errors(fake_pkg):
    from medicalseg_amd.models import DiceTopKLoss, TopKLoss, VNet
    for make in (lambda: TopKLoss(k=0), lambda: TopKLoss(k=100.5), lambda: TopKLoss(k=-1), lambda: DiceTopKLoss(k=0),
                 lambda: DiceTopKLoss(k=101), lambda: TopKLoss(weight=[1.0, -0.5, 1.0]), lambda: DiceTopKLoss(weight=[-1.0, 1.0, 1.0]),
                 lambda: TopKLoss(k=float("nan"))):
        with pytest.raises(ValueError):
            make()
    TopKLoss(k=100), TopKLoss(k=0.5), DiceTopKLoss(k=100, weight=[0.0, 1.0, 2.0])
    _, outs, y = _logits()
    for loss in (TopKLoss(weight=[1, 2]), DiceTopKLoss(weight=[1, 2, 3, 4])):
        with pytest.raises(ValueError, match="entries for 3 classes"):
            loss(outs[0], y)
    _, outs, y = _logits(VNet(num_classes=1))
    for loss in (TopKLoss(), DiceTopKLoss(), DiceTopKLoss(activation="sigmoid")):
        with pytest.raises(ValueError, match="2 .. 64"):
            loss(outs[0], y)
    wide = outs[0].empty_like()
    wide.c = 65
    with pytest.raises(ValueError, match="2 .. 64"):
        TopKLoss()(wide, y)


def test_topk_is_one_forward_and_one_backward_call(fake_pkg, calls):
    from medicalseg_amd.models import TopKLoss
    from medicalseg_amd.models.losses.fused import Scalar, TopKNode
    _, outs, y = _logits()
    before = _topk_calls()
    del calls[:]
    fn = TopKLoss(k=25, weight=[1.0, 2.0, 0.5], ignore_index=7)
    loss = fn(outs[0], y)
    assert isinstance(loss, Scalar) and len(loss.terms) == 1 and type(loss.terms[0][1]) is TopKNode and loss.terms[0][2] == "topk"
    node = loss.terms[0][1]
    assert (TopKNode.SLOTS, TopKNode.writes) == ({"topk": 0}, False)
    float(loss)
    (2.0 * loss).backward()
    assert [c for c in calls if "loss" in c or "topk" in c] == ["msk_topk_ce_fwd", "msk_topk_ce_bwd"]
    assert [a - b for a, b in zip(_topk_calls(), before)] == [1, 0, 1, 1]
    assert _fake("fake_topk_ws_n", C.c_long) == 16 * 16 * 16
    assert _fake("fake_topk_last_int", C.c_int, 0) == 0 and _fake("fake_topk_last_int", C.c_int, 1) == 7
    assert (_fake("fake_topk_last_float", C.c_float, 0), _fake("fake_topk_last_float", C.c_float, 1)) == (25.0, 2.0)
    # the backward call reads the workspace and the record the forward call wrote; labels and weights are the loss's
    ptr = lambda i: _fake("fake_topk_last_ptr", C.c_void_p, i)
    assert ptr(0) == ptr(1) == node.ws_ptr and ptr(2) == ptr(3) == node.stats_ptr
    assert ptr(4) == fn._topk_weight_dev[1] and ptr(5) == y.ptr
    # a second evaluation of the same node launches nothing, and an equal loss shares the node
    del calls[:]
    again = TopKLoss(k=25, weight=[1.0, 2.0, 0.5], ignore_index=7)
    again._topk_weight_dev = fn._topk_weight_dev
    assert again(outs[0], y).terms[0][1] is node and TopKLoss(k=50)(outs[0], y).terms[0][1] is not node
    float(loss), float(fn(outs[0], y)), node.evaluate()
    assert not [c for c in calls if "topk" in c]


def test_dicetopk_is_two_forward_and_two_backward_calls(fake_pkg, calls):
    from medicalseg_amd.models import DiceTopKLoss
    from medicalseg_amd.models.losses.fused import RegionNode, TopKNode
    _, outs, y = _logits()
    del calls[:]
    loss, dice = DiceTopKLoss(lambda_dice=2.0, lambda_topk=0.5)(outs[0], y)
    assert [type(t[1]) for t in loss.terms] == [RegionNode, TopKNode] and np.asarray(dice).shape == (3,)
    assert _fake("fake_region_last_int", C.c_int, 1) == 0            # focal_on = 0: the region node carries the Dice term only
    float(loss)
    seen = []
    from medicalseg_amd.device import Device
    real = Device.call

    def spy(self, name, *args):
        if name == "msk_region_loss_bwd":
            seen.append((name, args[-2]))
        if name == "msk_topk_ce_bwd":
            seen.append((name, args[-2]))
        return real(self, name, *args)
    Device.call, keep = spy, Device.call
    try:
        (3.0 * loss).backward()
    finally:
        Device.call = keep
    mine = [c for c in calls if "loss" in c or "topk" in c]
    assert mine == ["msk_region_loss_fwd", "msk_topk_ce_fwd", "msk_region_loss_bwd", "msk_topk_ce_bwd"]
    assert seen == [("msk_region_loss_bwd", 0), ("msk_topk_ce_bwd", 1)]
    assert (_fake("fake_region_last_coef", C.c_float, 0), _fake("fake_region_last_coef", C.c_float, 1)) == (0.0, 6.0)
    assert _fake("fake_topk_last_float", C.c_float, 1) == 1.5


def test_mixed_ce_topk_adds_into_the_ce_gradient(fake_pkg, calls):
    from medicalseg_amd.models import CrossEntropyLoss, MixedLoss, TopKLoss
    _, outs, y = _logits()
    terms, dice = MixedLoss([CrossEntropyLoss(), TopKLoss()], [1, 0.25])(outs[0], y)
    assert dice is None and len(terms) == 2
    del calls[:]
    sum(terms).backward()
    mine = [c for c in calls if "loss" in c or "topk" in c]
    assert mine.index("msk_loss_bwd_ex") < mine.index("msk_topk_ce_bwd")
    assert mine.count("msk_loss_bwd_ex") == 1 and mine.count("msk_topk_ce_bwd") == 1
    assert _fake("fake_topk_last_int", C.c_int, 0) == 1 and _fake("fake_topk_last_float", C.c_float, 1) == 0.25


def test_loss_computation_passes_the_dice_through_and_deep_supervision_gets_a_node_per_head(fake_pkg, calls, monkeypatch):
    from medicalseg_amd.models import DiceTopKLoss, MixedLoss, TopKLoss, VNetDeepSup
    from medicalseg_amd.utils import loss_computation
    _, outs, y = _logits()
    loss_list, dice = loss_computation(outs, y, {"types": [DiceTopKLoss()], "coef": [0.5]})
    assert len(loss_list) == 1 and len(loss_list[0].terms) == 2 and np.asarray(dice).shape == (3,)
    loss_list, dice = loss_computation(outs, y, {"types": [TopKLoss()], "coef": [1]})
    assert len(loss_list) == 1 and dice is None
    terms, dice = MixedLoss([TopKLoss(), DiceTopKLoss()], [1, 2])(outs[0], y)
    assert len(terms) == 2 and np.asarray(dice).shape == (3,)
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3)
    _, outs, y = _logits(model)
    before = _topk_calls()
    loss_list, dice = loss_computation(outs, y, {"types": [DiceTopKLoss() for _ in range(4)], "coef": [0.25] * 4})
    nodes = {id(t[1]) for l in loss_list for t in l.terms}
    assert len(loss_list) == 4 and len(nodes) == 8
    backwards = []
    real = type(model).backward
    monkeypatch.setattr(type(model), "backward", lambda self, grads: (backwards.append(grads), real(self, grads))[1])
    sum(loss_list).backward()
    assert [a - b for a, b in zip(_topk_calls(), before)] == [4, 0, 4, 4]
    assert len(backwards) == 1 and len(backwards[0]) == 4 and all(g is not None for g in backwards[0])

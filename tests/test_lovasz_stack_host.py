"""LovaszSoftmaxLoss / DiceLovaszLoss WITHOUT a GPU: the control flow of the loss objects, MixedLoss, loss_computation and
Scalar.backward through the real host stack over a stand-in library (tests/fake_msegk.c + fake_msegk_region.c +
fake_msegk_pyramid.c + fake_msegk_lovasz.c; its numbers are garbage by construction).  The statement has its own file,
tests/test_lovasz_host.py."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import fake_lib
from fake_lib import calls, fake as _fake  # noqa: F401  (calls is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DICELOVASZ_YML = os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicelovasz_96.yml")

fake_pkg = fake_lib.fake_pkg_fixture("fake_msegk.c", "fake_msegk_region.c", "fake_msegk_pyramid.c", "fake_msegk_lovasz.c")


def _lovasz_calls():
    return [_fake("fake_lovasz_calls", C.c_long, i) for i in range(3)]


def _mine(calls):
    return [c for c in calls if "loss" in c or "lovasz" in c or "pyramid" in c]


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
    from medicalseg_amd.models import DiceLovaszLoss
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = Config(DICELOVASZ_YML)
        base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicece_96.yml"))
    assert cfg.dic["loss"] == {"types": [{"type": "DiceLovaszLoss"}], "coef": [1]}
    shipped = cfg.loss["types"][0]
    assert type(shipped) is DiceLovaszLoss and shipped.classes == "present" and not shipped.per_image and shipped.ignore_index == 255
    assert shipped.batch_dice and not shipped.do_bg and (shipped.lambda_dice, shipped.lambda_lovasz, shipped.smooth) == (1.0, 1.0, 1e-5)
    # everything but the loss is the dicece_96 recipe
    assert {k: v for k, v in cfg.dic.items() if k != "loss"} == {k: v for k, v in base.dic.items() if k != "loss"}


def test_both_are_registered_and_exported(fake_pkg):
    import medicalseg_amd.models as models
    from medicalseg_amd.cvlibs import manager
    from medicalseg_amd.models.losses import DiceLovaszLoss, LovaszSoftmaxLoss
    assert models.LovaszSoftmaxLoss is LovaszSoftmaxLoss and models.DiceLovaszLoss is DiceLovaszLoss
    assert manager.LOSSES["LovaszSoftmaxLoss"] is LovaszSoftmaxLoss and manager.LOSSES["DiceLovaszLoss"] is DiceLovaszLoss


def test_constructors_and_calls_refuse_the_argument_errors(fake_pkg):
    from medicalseg_amd.models import DiceLovaszLoss, LovaszSoftmaxLoss, VNet
    for make in (lambda: LovaszSoftmaxLoss(classes="some"), lambda: LovaszSoftmaxLoss(classes=[]), lambda: LovaszSoftmaxLoss(classes=[1, 1]),
                 lambda: LovaszSoftmaxLoss(classes=[-1]), lambda: LovaszSoftmaxLoss(classes=[64]), lambda: LovaszSoftmaxLoss(classes=[0.5]),
                 lambda: DiceLovaszLoss(classes="none"), lambda: DiceLovaszLoss(classes=[2, 2]), lambda: DiceLovaszLoss(smooth=-1)):
        with pytest.raises(ValueError):
            make()
    LovaszSoftmaxLoss(classes="all"), LovaszSoftmaxLoss(classes=[0, 63]), DiceLovaszLoss(classes=(1, 2), per_image=True)
    _, outs, y = _logits()
    for loss in (LovaszSoftmaxLoss(classes=[1, 3]), DiceLovaszLoss(classes=[3])):
        with pytest.raises(ValueError, match="outside the 3"):
            loss(outs[0], y)
    _, outs, y = _logits(VNet(num_classes=1))
    for loss in (LovaszSoftmaxLoss(), DiceLovaszLoss(), DiceLovaszLoss(activation="sigmoid")):
        with pytest.raises(ValueError, match="2 .. 64"):
            loss(outs[0], y)
    wide = outs[0].empty_like()
    wide.c = 65
    with pytest.raises(ValueError, match="2 .. 64"):
        LovaszSoftmaxLoss()(wide, y)


def test_lovasz_is_one_forward_and_one_backward_call(fake_pkg, calls):
    from medicalseg_amd.models import LovaszSoftmaxLoss
    from medicalseg_amd.models.losses.fused import LOVASZ_ALL, LOVASZ_LIST, LOVASZ_PRESENT, LovaszNode, Scalar
    _, outs, y = _logits(n=2)
    before = _lovasz_calls()
    del calls[:]
    fn = LovaszSoftmaxLoss(classes=[0, 2], per_image=True, ignore_index=7)
    loss = fn(outs[0], y)
    assert isinstance(loss, Scalar) and len(loss.terms) == 1 and type(loss.terms[0][1]) is LovaszNode and loss.terms[0][2] == "lovasz"
    node = loss.terms[0][1]
    assert (LovaszNode.SLOTS, LovaszNode.writes) == ({"lovasz": 0}, False)
    assert (LOVASZ_PRESENT, LOVASZ_ALL, LOVASZ_LIST) == (0, 1, 2)
    float(loss)
    (2.0 * loss).backward()
    assert _mine(calls) == ["msk_lovasz_fwd", "msk_lovasz_bwd"]
    assert [a - b for a, b in zip(_lovasz_calls(), before)] == [1, 1, 1]
    # per_image: two groups of one sample's voxels each; the record has 4 doubles per plane and two more
    assert [_fake("fake_lovasz_ws_arg", C.c_long, i) for i in range(3)] == [16 * 16 * 16, 3, 2]
    assert node.groups == 2 and node.stats_doubles() == 4 * 2 * 3 + 2
    ints = [_fake("fake_lovasz_last_int", C.c_int, i) for i in range(5)]
    assert ints == [0, 7, LOVASZ_LIST, 1, 1]
    assert _fake("fake_lovasz_last_mask", C.c_uint64) == 0b101 and _fake("fake_lovasz_last_coef", C.c_float) == 2.0
    # the backward call reads the workspace and the record the forward call wrote, and both hear the size the query returned
    ptr = lambda i: _fake("fake_lovasz_last_ptr", C.c_void_p, i)
    assert ptr(0) == ptr(1) == node.ws_ptr and ptr(2) == ptr(3) == node.stats_ptr and ptr(4) == y.ptr and ptr(5) == node.out_ptr
    size = 16 * 16 * 16 * 3 * 2 * 16 + 8192
    assert _fake("fake_lovasz_last_bytes", C.c_size_t, 0) == _fake("fake_lovasz_last_bytes", C.c_size_t, 1) == node.ws_bytes == size
    # a second evaluation of the same node launches nothing, and an equal loss shares the node
    del calls[:]
    assert LovaszSoftmaxLoss(classes=[0, 2], per_image=True, ignore_index=7)(outs[0], y).terms[0][1] is node
    others = (LovaszSoftmaxLoss(), LovaszSoftmaxLoss(classes="all"), LovaszSoftmaxLoss(classes=[0, 2], ignore_index=7))
    assert all(o(outs[0], y).terms[0][1] is not node for o in others)
    float(loss), float(fn(outs[0], y)), node.evaluate()
    assert not [c for c in calls if "lovasz" in c]
    # the default: the batch is one group, the classes present count
    float(others[0](outs[0], y))
    assert [_fake("fake_lovasz_ws_arg", C.c_long, i) for i in range(3)] == [2 * 16 * 16 * 16, 3, 1]
    assert [_fake("fake_lovasz_last_int", C.c_int, i) for i in (1, 2, 3)] == [255, LOVASZ_PRESENT, 0]
    float(others[1](outs[0], y))
    assert _fake("fake_lovasz_last_int", C.c_int, 2) == LOVASZ_ALL and _fake("fake_lovasz_last_mask", C.c_uint64) == 0


def test_dicelovasz_is_two_forward_and_two_backward_calls(fake_pkg, calls):
    from medicalseg_amd.device import Device
    from medicalseg_amd.models import DiceLovaszLoss
    from medicalseg_amd.models.losses.fused import LovaszNode, RegionNode
    _, outs, y = _logits()
    del calls[:]
    loss, dice = DiceLovaszLoss(lambda_dice=2.0, lambda_lovasz=0.5)(outs[0], y)
    assert [type(t[1]) for t in loss.terms] == [RegionNode, LovaszNode] and np.asarray(dice).shape == (3,)
    assert _fake("fake_region_last_int", C.c_int, 1) == 0            # focal_on = 0: the region node carries the Dice term only
    float(loss)
    seen = []
    real = Device.call

    def spy(self, name, *args):
        if name in ("msk_region_loss_bwd", "msk_lovasz_bwd"):
            seen.append((name, args[-2]))
        return real(self, name, *args)
    Device.call, keep = spy, Device.call
    try:
        (3.0 * loss).backward()
    finally:
        Device.call = keep
    assert _mine(calls) == ["msk_region_loss_fwd", "msk_lovasz_fwd", "msk_region_loss_bwd", "msk_lovasz_bwd"]
    assert seen == [("msk_region_loss_bwd", 0), ("msk_lovasz_bwd", 1)]           # the first writes, the second adds
    assert (_fake("fake_region_last_coef", C.c_float, 0), _fake("fake_region_last_coef", C.c_float, 1)) == (0.0, 6.0)
    assert _fake("fake_lovasz_last_coef", C.c_float) == 1.5 and _fake("fake_lovasz_last_int", C.c_int, 0) == 1


def test_mixed_ce_lovasz_adds_into_the_ce_gradient(fake_pkg, calls):
    from medicalseg_amd.models import CrossEntropyLoss, MixedLoss, LovaszSoftmaxLoss
    _, outs, y = _logits()
    terms, dice = MixedLoss([LovaszSoftmaxLoss(), CrossEntropyLoss()], [0.25, 1])(outs[0], y)
    assert dice is None and len(terms) == 2
    del calls[:]
    sum(terms).backward()
    mine = _mine(calls)
    # the writing node runs first on its logits, whatever the order of the members
    assert mine.index("msk_loss_bwd_ex") < mine.index("msk_lovasz_bwd")
    assert mine.count("msk_loss_bwd_ex") == 1 and mine.count("msk_lovasz_bwd") == 1
    assert _fake("fake_lovasz_last_int", C.c_int, 0) == 1 and _fake("fake_lovasz_last_coef", C.c_float) == 0.25


def test_loss_computation_passes_the_dice_through(fake_pkg, calls):
    from medicalseg_amd.models import DiceLovaszLoss, LovaszSoftmaxLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    _, outs, y = _logits()
    loss_list, dice = loss_computation(outs, y, {"types": [DiceLovaszLoss()], "coef": [0.5]})
    assert len(loss_list) == 1 and len(loss_list[0].terms) == 2 and np.asarray(dice).shape == (3,)
    loss_list, dice = loss_computation(outs, y, {"types": [LovaszSoftmaxLoss()], "coef": [1]})
    assert len(loss_list) == 1 and dice is None
    terms, dice = MixedLoss([LovaszSoftmaxLoss(), DiceLovaszLoss()], [1, 2])(outs[0], y)
    assert len(terms) == 2 and np.asarray(dice).shape == (3,)


def test_native_heads_get_their_level_of_the_label_pyramid(fake_pkg, calls, monkeypatch):
    """node_for hands every native deep-supervision head its own pyramid level: LovaszNode needs no code for it"""
    from medicalseg_amd.models import DiceLovaszLoss, VNetDeepSup
    from medicalseg_amd.models.losses.fused import LovaszNode
    from medicalseg_amd.utils import loss_computation
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    _, outs, y = _logits(model)
    assert len(outs) == 4 and len({(o.d, o.h, o.w) for o in outs}) > 1
    backwards = []
    real = type(model).backward
    monkeypatch.setattr(type(model), "backward", lambda self, grads: (backwards.append(grads), real(self, grads))[1])
    before = _lovasz_calls()
    del calls[:]
    loss_list, dice = loss_computation(outs, y, {"types": [DiceLovaszLoss() for _ in range(4)], "coef": [0.25] * 4})
    nodes = {id(t[1]): t[1] for l in loss_list for t in l.terms}
    assert len(loss_list) == 4 and len(nodes) == 8 and np.asarray(dice).shape == (3,)
    lovasz = {id(n.logits): n for n in nodes.values() if type(n) is LovaszNode}
    assert lovasz[id(outs[0])].labels is y
    sizes = []
    for o in outs:
        node = lovasz[id(o)]
        assert tuple(node.labels.shape) == (1, o.d, o.h, o.w)
        float(loss_list[outs.index(o)])
        sizes.append(_fake("fake_lovasz_ws_arg", C.c_long, 0))
    assert sizes == [o.d * o.h * o.w for o in outs]                    # each workspace is sized for its own head
    sum(loss_list).backward()
    mine = _mine(calls)
    assert mine.count("msk_label_pyramid") == 1 and mine.count("msk_lovasz_fwd") == 4 and mine.count("msk_lovasz_bwd") == 4
    assert [a - b for a, b in zip(_lovasz_calls(), before)] == [4, 4, 4]
    assert len(backwards) == 1 and len(backwards[0]) == 4 and all(g is not None for g in backwards[0])

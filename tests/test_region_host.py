"""SoftDiceLoss / TverskyLoss / FocalLoss / DiceCELoss WITHOUT a GPU: the control flow of the loss objects, MixedLoss,
loss_computation and Scalar.backward through the real host stack over a stand-in library (tests/fake_msegk.c +
tests/fake_msegk_region.c; numbers are garbage by construction, nothing numeric is asserted)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import fake_lib
from fake_lib import calls, fake as _fake  # noqa: F401  (calls is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DICECE_YML = os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicece_96.yml")


fake_pkg = fake_lib.fake_pkg_fixture("fake_msegk.c", "fake_msegk_region.c")


def _region_calls():
    return [_fake("fake_region_calls", C.c_long, i) for i in range(2)]


def _logits(model=None, n=1):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import VNet
    model = model or VNet(num_classes=3)
    model.train()
    rng = np.random.default_rng(0)
    outs = model(rng.standard_normal((n, 1, 16, 16, 16)).astype(np.float32))
    y = to_tensor(rng.integers(0, 3, (n, 16, 16, 16)).astype(np.int32))
    return model, outs, y


def test_the_four_classes_build_from_yaml(fake_pkg):
    import yaml
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceCELoss, FocalLoss, SoftDiceLoss, TverskyLoss
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = Config(DICECE_YML)
    assert cfg.dic["loss"] == {"types": [{"type": "DiceCELoss"}], "coef": [1]}
    assert cfg.dic["train_dataset"]["transforms"][0]["label_pad"] == 255
    shipped = cfg.loss["types"][0]
    assert type(shipped) is DiceCELoss and shipped.ignore_index == 255 and shipped.batch_dice and not shipped.do_bg
    assert (shipped.lambda_dice, shipped.lambda_ce, shipped.gamma, shipped.smooth) == (1.0, 1.0, 0.0, 1e-5)
    # everything but the loss and the crop's label_pad is the nnU-Net recipe
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_nnunet_96.yml"))
    mine = {k: v for k, v in cfg.dic.items() if k != "loss"}
    del mine["train_dataset"]["transforms"][0]["label_pad"]
    assert mine == {k: v for k, v in base.dic.items() if k != "loss"}

    cfg._losses = None
    cfg.dic["loss"] = yaml.safe_load("""
        types:
          - type: SoftDiceLoss
            batch_dice: False
            do_bg: True
            squared_pred: True
          - type: TverskyLoss
            alpha: 0.4
            beta: 0.6
            activation: sigmoid
          - type: FocalLoss
            gamma: 1.5
            weight: [1.0, 2.0, 3.0]
          - type: MixedLoss
            losses:
              - type: CrossEntropyLoss
                weight: Null
              - type: DiceCELoss
                lambda_ce: 0.5
                gamma: 2
            coef: [1, 1]
        coef: [1, 1, 1, 1]
    """)
    sd, tv, fl, mixed = cfg.loss["types"]
    assert type(sd) is SoftDiceLoss and (sd.batch_dice, sd.do_bg, sd.squared_pred, sd.ignore_index) == (False, True, True, 255)
    assert type(tv) is TverskyLoss and (tv.alpha, tv.beta, tv.activation) == (0.4, 0.6, "sigmoid")
    assert type(fl) is FocalLoss and fl.gamma == 1.5 and fl.weight.tolist() == [1.0, 2.0, 3.0] and fl.edge_label is False
    assert type(mixed.losses[1]) is DiceCELoss and (mixed.losses[1].lambda_ce, mixed.losses[1].gamma) == (0.5, 2.0)


def test_constructors_refuse_the_argument_errors(fake_pkg):
    from medicalseg_amd.models import DiceCELoss, FocalLoss, SoftDiceLoss, TverskyLoss
    for make in (lambda: FocalLoss(gamma=0.5), lambda: FocalLoss(gamma=-1), lambda: DiceCELoss(gamma=0.99),
                 lambda: SoftDiceLoss(smooth=-1e-5), lambda: TverskyLoss(squared_pred=True), lambda: TverskyLoss(alpha=-0.1),
                 lambda: DiceCELoss(activation='sigmoid'), lambda: SoftDiceLoss(activation='tanh')):
        with pytest.raises(ValueError):
            make()
    FocalLoss(gamma=0), FocalLoss(gamma=1), TverskyLoss(activation='sigmoid'), SoftDiceLoss(smooth=0)
    # what only the logits show: softmax over one class, a weight list of the wrong length
    from medicalseg_amd.models import VNet
    _, outs, y = _logits(VNet(num_classes=1))
    with pytest.raises(ValueError, match="at least 2 classes"):
        SoftDiceLoss()(outs[0], y)
    SoftDiceLoss(activation='sigmoid')(outs[0], y)
    _, outs, y = _logits()
    with pytest.raises(ValueError, match="2 entries for 3 classes"):
        FocalLoss(weight=[1, 2])(outs[0], y)


def test_per_class_dice_comes_back_for_the_new_names(fake_pkg):
    from medicalseg_amd.models import DiceCELoss, FocalLoss, MixedLoss, SoftDiceLoss, TverskyLoss
    from medicalseg_amd.utils import loss_computation
    _, outs, y = _logits()
    for loss in (SoftDiceLoss(), TverskyLoss(), DiceCELoss()):
        loss_list, dice = loss_computation(outs, y, {"types": [loss], "coef": [0.5]})
        assert len(loss_list) == 1 and np.asarray(dice).shape == (3,)
        terms, dice = MixedLoss([FocalLoss(), loss], [1, 2])(outs[0], y)
        assert len(terms) == 2 and np.asarray(dice).shape == (3,)
        loss_list, dice = loss_computation(outs, y, {"types": [MixedLoss([FocalLoss(), loss], [1, 2])], "coef": [1]})
        assert len(loss_list) == 2 and np.asarray(dice).shape == (3,)
    loss_list, dice = loss_computation(outs, y, {"types": [FocalLoss()], "coef": [1]})
    assert len(loss_list) == 1 and dice is None
    with pytest.raises(ValueError, match="edge maps"):
        loss_computation(outs, y, {"types": [FocalLoss(edge_label=True)], "coef": [1]})


def test_dicece_is_one_forward_and_one_backward_call(fake_pkg, calls):
    from medicalseg_amd.models import DiceCELoss, FocalLoss, SoftDiceLoss
    model, outs, y = _logits()
    before = _region_calls()
    del calls[:]
    loss, _ = DiceCELoss(lambda_dice=2.0, lambda_ce=0.5)(outs[0], y)
    assert len(loss.terms) == 2 and loss.terms[0][1] is loss.terms[1][1]            # both terms on ONE node
    float(loss)
    (3.0 * loss).backward()
    mine = [c for c in calls if "loss" in c]
    assert mine == ["msk_region_loss_fwd", "msk_region_loss_bwd"]
    assert [a - b for a, b in zip(_region_calls(), before)] == [1, 1]
    assert _fake("fake_region_last_int", C.c_int, 0) == 0 and _fake("fake_region_last_int", C.c_int, 1) == 1
    assert (_fake("fake_region_last_coef", C.c_float, 0), _fake("fake_region_last_coef", C.c_float, 1)) == (1.5, 6.0)
    # equal settings share the node, different settings do not
    _, outs, y = _logits(model)
    del calls[:]
    a, b, c = SoftDiceLoss()(outs[0], y)[0], SoftDiceLoss()(outs[0], y)[0], SoftDiceLoss(do_bg=True)(outs[0], y)[0]
    f = FocalLoss(gamma=0)(outs[0], y)
    assert a.terms[0][1] is b.terms[0][1] and a.terms[0][1] is not c.terms[0][1] and f.terms[0][1] is not a.terms[0][1]
    (a + b + c + f).backward()
    mine = [x for x in calls if "loss" in x]
    assert mine.count("msk_region_loss_fwd") == 3 and mine.count("msk_region_loss_bwd") == 3 and len(mine) == 6
    assert _fake("fake_region_last_int", C.c_int, 0) == 1                             # the later nodes add into the first's


def test_mixed_ce_softdice_accumulates_into_the_ce_gradient(fake_pkg, calls):
    from medicalseg_amd.models import CrossEntropyLoss, MixedLoss, SoftDiceLoss
    _, outs, y = _logits()
    terms, dice = MixedLoss([CrossEntropyLoss(), SoftDiceLoss()], [1, 1])(outs[0], y)
    del calls[:]
    sum(terms).backward()
    mine = [c for c in calls if "loss" in c]
    assert mine.index("msk_loss_bwd_ex") < mine.index("msk_region_loss_bwd")
    assert mine.count("msk_loss_bwd_ex") == 1 and mine.count("msk_region_loss_bwd") == 1
    assert _fake("fake_region_last_int", C.c_int, 0) == 1
    assert (_fake("fake_region_last_coef", C.c_float, 0), _fake("fake_region_last_coef", C.c_float, 1)) == (0.0, 1.0)


def test_deep_supervision_gets_four_nodes_and_one_model_backward(fake_pkg, calls, monkeypatch):
    from medicalseg_amd.models import DiceCELoss, VNetDeepSup
    from medicalseg_amd.utils import loss_computation
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3)
    _, outs, y = _logits(model)
    assert len(outs) == 4
    before = _region_calls()
    loss_list, dice = loss_computation(outs, y, {"types": [DiceCELoss() for _ in range(4)], "coef": [0.25] * 4})
    nodes = {id(t[1]) for l in loss_list for t in l.terms}
    assert len(loss_list) == 4 and len(nodes) == 4 and np.asarray(dice).shape == (3,)
    backwards = []
    real = type(model).backward
    monkeypatch.setattr(type(model), "backward", lambda self, grads: (backwards.append(grads), real(self, grads))[1])
    sum(loss_list).backward()
    assert [a - b for a, b in zip(_region_calls(), before)] == [4, 4]
    assert len(backwards) == 1 and len(backwards[0]) == 4 and all(g is not None for g in backwards[0])

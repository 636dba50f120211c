"""Region-based training WITHOUT a GPU: the control flow of RegionSpec, DiceBCERegionLoss, loss_computation, Scalar.backward,
inference / sliding_window_inference / evaluate with and without `regions`, through the real host stack over a stand-in library
(tests/fake_msegk.c + fake_msegk_region.c + fake_msegk_pyramid.c + fake_msegk_mlabel.c; numbers are garbage by construction,
nothing numeric is asserted)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import fake_lib
import mlabel_reference as M
from fake_lib import calls, fake as _fake  # noqa: F401  (calls is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REGIONS_YML = os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_regions_96.yml")
REGIONS, ORDER = [[1, 2, 3], [2, 3], [3]], [1, 2, 3]

fake_pkg = fake_lib.fake_pkg_fixture("fake_msegk.c", "fake_msegk_region.c", "fake_msegk_pyramid.c", "fake_msegk_mlabel.c")

# the calls behind the model's own: what the loss objects and the three prediction paths add
TAIL = ("msk_argmax_c", "msk_regions_to_label", "msk_sw_gather", "msk_sw_accumulate", "msk_softmax_c", "msk_interp_trilinear_fwd",
        "msk_loss_fwd_ex", "msk_loss_bwd_ex", "msk_region_loss_fwd", "msk_region_loss_bwd", "msk_mlabel_loss_fwd",
        "msk_mlabel_loss_bwd", "msk_label_pyramid", "msk_confusion3d", "msk_tta_accumulate", "msk_tta_finish")


def _tail(calls):
    return [c for c in calls if c in TAIL]


def _compute(calls):
    """the calls without the memory traffic of uploads and first-use allocations"""
    return [c for c in calls if c not in ("msk_malloc", "msk_free", "msk_h2d", "msk_h2d_async", "msk_d2h", "msk_memset")]


def _mlabel_calls():
    return [_fake("fake_mlabel_calls", C.c_long, i) for i in range(3)]


def _batch(n=1, seed=0):
    from medicalseg_amd.device import to_tensor
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 1, 16, 16, 16)).astype(np.float32)
    return x, to_tensor(rng.integers(0, 4, (n, 16, 16, 16)).astype(np.int32))


def _loss(**kw):
    from medicalseg_amd.models import DiceBCERegionLoss
    return DiceBCERegionLoss(REGIONS, ORDER, **kw)


def test_region_spec_checks_and_table(fake_pkg):
    from medicalseg_amd.models import DiceBCERegionLoss, RegionSpec
    spec = RegionSpec([[1, 2, 3], [2, 3], 3], [1, 2, 3])
    assert spec.regions == ((1, 2, 3), (2, 3), (3,)) and spec.class_order == (1, 2, 3) and spec.num_regions == 3
    assert np.array_equal(spec.table(), M.build_table(REGIONS)) and spec.table().dtype == np.uint32
    for bad in ([], [[1], []], [[256]], [[-1]], [[1.5]], [[1]] * 33, 3):
        with pytest.raises(ValueError):
            RegionSpec(bad)
    with pytest.raises(ValueError, match="class_order"):
        RegionSpec(REGIONS, [1, 2])
    RegionSpec([[v] for v in range(32)])
    with pytest.raises(ValueError, match="smooth"):
        DiceBCERegionLoss(REGIONS, smooth=-1.0)
    loss = _loss()
    assert loss.region_spec.class_order == (1, 2, 3) and (loss.lambda_dice, loss.lambda_bce, loss.batch_dice) == (1.0, 1.0, True)
    assert (loss.smooth, loss.squared_pred, loss.ignore_index) == (1e-5, False, 255)
    # the device copy of the table is made once per device
    from medicalseg_amd.device import get_device
    dev = get_device()
    a, b = spec.device_table(dev), spec.device_table(dev)
    assert a == b and a[1] == 256


def test_loss_is_one_forward_and_one_backward_call(fake_pkg, calls):
    from medicalseg_amd.models import DiceBCERegionLoss, VNet
    from medicalseg_amd.utils import loss_computation
    model = VNet(num_classes=3)
    model.train()
    x, y = _batch(2)
    outs = model(x)
    before = _mlabel_calls()
    del calls[:]
    loss_fn = _loss(lambda_dice=2.0, lambda_bce=0.5, batch_dice=False, squared_pred=True, smooth=1e-3)
    loss_list, dice = loss_computation(outs, y, {"types": [loss_fn], "coef": [3.0]})
    assert len(loss_list) == 1 and np.asarray(dice).shape == (3,)
    loss = loss_list[0]
    assert len(loss.terms) == 2 and loss.terms[0][1] is loss.terms[1][1]            # both terms on ONE node
    assert [t[2] for t in loss.terms] == ["bce", "dice"]
    float(loss)
    loss.backward()
    assert _tail(calls) == ["msk_mlabel_loss_fwd", "msk_mlabel_loss_bwd"]
    assert [a - b for a, b in zip(_mlabel_calls(), before)] == [1, 1, 0]
    ints = [_fake("fake_mlabel_last_int", C.c_int, i) for i in range(6)]
    assert ints == [0, 256, 1, 0, 255, 3]                    # accumulate, table_len, squared, batch_dice, ignore_index, R
    assert (_fake("fake_mlabel_last_float", C.c_float, 0), _fake("fake_mlabel_last_float", C.c_float, 1)) == (1.5, 6.0)
    assert _fake("fake_mlabel_last_float", C.c_float, 2) == np.float32(1e-3)
    assert [_fake("fake_mlabel_table", C.c_uint32, v) for v in range(5)] == [0, 1, 3, 7, 0]
    # equal settings share the node, other settings do not; a second node adds into the first's gradient
    outs = model(x)
    del calls[:]
    a, b, c = _loss()(outs[0], y)[0], _loss()(outs[0], y)[0], _loss(squared_pred=True)(outs[0], y)[0]
    assert a.terms[0][1] is not c.terms[0][1]
    (a + c).backward()
    assert _tail(calls).count("msk_mlabel_loss_bwd") == 2 and _fake("fake_mlabel_last_int", C.c_int, 0) == 1
    # as a member of a MixedLoss it hands its per-region Dice through
    from medicalseg_amd.models import MixedLoss
    terms, dice = MixedLoss([_loss(), _loss(squared_pred=True)], [1, 2])(outs[0], y)
    assert len(terms) == 2 and np.asarray(dice).shape == (3,)
    # the logits' channel count must equal R
    with pytest.raises(ValueError, match="3 channels for 2 regions"):
        DiceBCERegionLoss([[1, 2], [2]])(outs[0], y)


def test_native_heads_get_their_level_of_the_label_pyramid(fake_pkg, calls, monkeypatch):
    from medicalseg_amd.models import VNetDeepSup
    from medicalseg_amd.utils import loss_computation
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    model.train()
    x, y = _batch()
    backwards = []
    real = type(model).backward
    monkeypatch.setattr(type(model), "backward", lambda self, grads: (backwards.append(grads), real(self, grads))[1])
    outs = model(x)
    assert len(outs) == 4
    before = _mlabel_calls()
    del calls[:]
    losses = {"types": [_loss() for _ in range(4)], "coef": [8 / 15, 1 / 15, 2 / 15, 4 / 15]}
    loss_list, dice = loss_computation(outs, y, losses)
    nodes = {id(t[1]): t[1] for l in loss_list for t in l.terms}
    assert len(loss_list) == 4 and len(nodes) == 4 and np.asarray(dice).shape == (3,)
    by_logits = {id(n.logits): n for n in nodes.values()}
    assert by_logits[id(outs[0])].labels is y
    for o in outs[1:]:
        assert tuple(by_logits[id(o)].labels.shape) == (1, o.d, o.h, o.w)
    sum(loss_list).backward()
    tail = _tail(calls)
    # the full-resolution output is scored against the label itself; the first head asks for the pyramid, one launch for all
    assert tail == ["msk_mlabel_loss_fwd", "msk_label_pyramid"] + ["msk_mlabel_loss_fwd"] * 3 + ["msk_mlabel_loss_bwd"] * 4
    assert [a - b for a, b in zip(_mlabel_calls(), before)] == [4, 4, 0]
    assert len(backwards) == 1 and len(backwards[0]) == 4 and all(g is not None for g in backwards[0])


def _eval_model():
    from medicalseg_amd.models import VNet
    model = VNet(num_classes=3)
    model.eval()
    return model


def test_inference_paths_without_regions_make_the_calls_they_made(fake_pkg, calls):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import RegionSpec
    model = _eval_model()
    x = np.random.default_rng(0).standard_normal((1, 1, 16, 16, 16)).astype(np.float32)
    spec = RegionSpec(REGIONS, ORDER)
    before = _mlabel_calls()
    infer.inference(model, to_tensor(x))            # the first forward folds the BatchNorms and allocates: not part of the comparison
    del calls[:]
    pred, logits = infer.inference(model, to_tensor(x))
    plain = list(calls)
    assert _tail(plain) == ["msk_argmax_c"] and plain[-1] == "msk_argmax_c"
    del calls[:]
    pred_r, logits_r = infer.inference(model, to_tensor(x), regions=spec)
    # one alternative to the arg-max, nothing else
    assert _compute(calls)[:-1] == _compute(plain)[:-1] and calls[-1] == "msk_regions_to_label"
    assert tuple(pred_r.shape) == tuple(pred.shape) == (1, 1, 16, 16, 16)
    assert [_fake("fake_mlabel_order", C.c_int32, r) for r in range(4)] == [1, 2, 3, -1]
    assert [_fake("fake_mlabel_label_shape", C.c_int, i) for i in range(4)] == [1, 16, 16, 16]
    # after the resize back, where there is one
    from medicalseg_amd.transforms import Resize3D
    tf = [Resize3D(size=[16, 16, 16])]
    del calls[:]
    infer.inference(model, to_tensor(x), ori_shape=(20, 18, 16), transforms=tf)
    assert _tail(calls) == ["msk_interp_trilinear_fwd", "msk_argmax_c"]
    del calls[:]
    infer.inference(model, to_tensor(x), ori_shape=(20, 18, 16), transforms=tf, regions=spec)
    assert _tail(calls) == ["msk_interp_trilinear_fwd", "msk_regions_to_label"]
    assert [_fake("fake_mlabel_label_shape", C.c_int, i) for i in range(4)] == [1, 20, 18, 16]
    # sliding window: 2 x 1 x 1 windows of 16^3 at overlap 0
    x2 = to_tensor(np.concatenate([x, x], axis=2))
    infer.sliding_window_inference(model, x2, (16, 16, 16), overlap=0.0)      # allocates the kept buffers and the plan tables
    del calls[:]
    infer.sliding_window_inference(model, x2, (16, 16, 16), overlap=0.0)
    sw_plain = list(calls)
    assert _tail(sw_plain) == ["msk_sw_gather", "msk_sw_accumulate"] * 2 + ["msk_argmax_c"]
    del calls[:]
    infer.sliding_window_inference(model, x2, (16, 16, 16), overlap=0.0, regions=spec)
    assert _compute(calls)[:-1] == _compute(sw_plain)[:-1] and calls[-1] == "msk_regions_to_label"
    infer.sliding_release(x2.dev)
    assert [a - b for a, b in zip(_mlabel_calls(), before)] == [0, 0, 3]
    # aug_inference averages softmax probabilities
    with pytest.raises(ValueError, match="regions"):
        infer.aug_inference(model, x2, flip_axes=(0,), regions=spec)
    with pytest.raises(ValueError, match="class_order"):
        infer.inference(model, x2, regions=RegionSpec(REGIONS))


def test_evaluate_takes_the_region_spec_of_the_loss(fake_pkg, calls):
    from medicalseg_amd.core import evaluate
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import DiceCELoss, DiceBCERegionLoss, RegionSpec
    model = _eval_model()
    val = SyntheticCT(num_samples=2, shape=(16, 16, 16), num_classes=4, mode="val")
    # without regions: the calls of today
    del calls[:]
    res = evaluate(model, val, {"types": [DiceCELoss()], "coef": [1]}, print_detail=False)
    assert _tail(calls) == ["msk_argmax_c", "msk_region_loss_fwd"] * 2 and set(res) == {"mdice"}
    del calls[:]
    res = evaluate(model, val, {"types": [DiceCELoss()], "coef": [1]}, print_detail=False, hard_metrics=True)
    assert _tail(calls) == ["msk_argmax_c", "msk_region_loss_fwd", "msk_confusion3d"] * 2
    assert "region_dice" not in res and "dice" in res
    # the loss's own spec is the default
    losses = {"types": [_loss()], "coef": [1]}
    del calls[:]
    res = evaluate(model, val, losses, print_detail=False)
    assert _tail(calls) == ["msk_regions_to_label", "msk_mlabel_loss_fwd"] * 2 and set(res) == {"mdice"}
    del calls[:]
    res = evaluate(model, val, losses, print_detail=False, hard_metrics=True, sliding_window=(16, 16, 16), sw_overlap=0.0)
    assert _tail(calls) == (["msk_sw_gather", "msk_sw_accumulate"] + ["msk_regions_to_label", "msk_mlabel_loss_fwd",
                                                                          "msk_confusion3d"]) * 2
    assert np.asarray(res["class_region_dice"]).shape == (3,) and {"region_dice", "region_dice_per_case"} <= set(res)
    # an explicit spec wins over the loss's
    del calls[:]
    evaluate(model, val, losses, print_detail=False, regions=RegionSpec(REGIONS, [3, 2, 1]))
    assert [_fake("fake_mlabel_order", C.c_int32, r) for r in range(3)] == [3, 2, 1]
    for kw in (dict(auc_roc=True), dict(aug_eval=True)):
        with pytest.raises(ValueError, match="regions"):
            evaluate(model, val, losses, print_detail=False, **kw)
    with pytest.raises(ValueError, match="class_order"):
        evaluate(model, val, {"types": [DiceBCERegionLoss(REGIONS)], "coef": [1]}, print_detail=False)
    from medicalseg_amd.core import infer
    infer.sliding_release(model.dev)


def test_yaml_recipe_builds(fake_pkg):
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceBCERegionLoss, VNet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = Config(REGIONS_YML)
        base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicece_96.yml"))
    loss = cfg.loss["types"][0]
    assert type(loss) is DiceBCERegionLoss and loss.ignore_index == 255
    assert loss.region_spec.regions == ((1, 2, 3), (2, 3), (3,)) and loss.region_spec.class_order == (1, 2, 3)
    assert cfg.dic["train_dataset"]["num_classes"] == 4 and cfg.dic["val_dataset"]["num_classes"] == 4
    assert cfg.dic["model"]["num_classes"] == 3 and isinstance(cfg.model, VNet)
    # everything but the loss and the label values is the dicece recipe
    mine = {k: v for k, v in cfg.dic.items() if k != "loss"}
    theirs = {k: v for k, v in base.dic.items() if k != "loss"}
    for d in (mine, theirs):
        for ds in ("train_dataset", "val_dataset"):
            d[ds] = {k: v for k, v in d[ds].items() if k != "num_classes"}
        d["train_dataset"]["transforms"] = [dict(d["train_dataset"]["transforms"][0], num_classes=None)] + \
            d["train_dataset"]["transforms"][1:]
    assert mine == theirs

"""The label pyramid of nnU-Net's deep supervision WITHOUT a GPU: the integer statement (tests/pyramid_reference.py) against
torch's 'nearest-exact' resize, the C ABI entry, and the control flow of VNetDeepSup(native_heads=True), the label selection of
the loss nodes and Scalar.backward through the real host stack over a stand-in library (tests/fake_msegk.c +
tests/fake_msegk_region.c + tests/fake_msegk_pyramid.c; numbers are garbage by construction, nothing numeric is asserted
there)."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import fake_lib
import pyramid_reference as R
from fake_lib import calls, fake as _fake  # noqa: F401  (calls is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NNUNET_YML = os.path.join(ROOT, "configs", "synthetic", "vnetdeepsup_synthetic_ct_patch_nnunet_96.yml")
MRI_YML = os.path.join(ROOT, "configs", "synthetic", "vnetdeepsup_native_synthetic_mri_512_512_12.yml")

# in -> out pairs on which the statement was cross-checked against torch and scipy
PAIRS = [(16, 8), (16, 4), (12, 12), (12, 9), (9, 8), (8, 4), (7, 3), (5, 2), (9, 1), (32, 16)]


# ---- the statement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
def test_statement_matches_torch_nearest_exact(pair):
    import torch
    n_in, n_out = pair
    src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in)
    want = torch.nn.functional.interpolate(src, size=n_out, mode="nearest-exact").reshape(-1).numpy().astype(np.int64)
    assert np.array_equal(R.src_index(n_in, n_out), want)


def test_indices_stay_inside_the_source():
    for n_in in range(1, 41):
        for n_out in range(1, n_in + 1):
            i = R.src_index(n_in, n_out)
            assert i.shape == (n_out,) and i.min() >= 0 and i.max() < n_in and np.all(np.diff(i) >= 0)
    i = R.src_index(32768, 32768)          # the longest axis the kernel takes: the products stay below 2^31
    assert (2 * 32767 + 1) * 32768 < 2 ** 31 and np.array_equal(i, np.arange(32768))


def test_identity_and_values_pass_through():
    rng = np.random.default_rng(0)
    lab = rng.integers(-5, 300, (2, 7, 5, 9)).astype(np.int32)
    lab[0, 0, 0, 0], lab[1, 6, 4, 8] = 255, 2 ** 31 - 1
    assert np.array_equal(R.pyramid_level(lab, (7, 5, 9)), lab)
    lv = R.label_pyramid(lab, [(3, 2, 4), (1, 1, 1)])
    assert [l.shape for l in lv] == [(2, 3, 2, 4), (2, 1, 1, 1)] and lv[0].dtype == np.int32
    assert lv[1][1, 0, 0, 0] == lab[1, 3, 2, 4]                      # the centre voxel
    assert lv[0][0, 2, 1, 3] == lab[0, (5 * 7) // 6, (3 * 5) // 4, (7 * 9) // 8]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_cabi_declares_the_entry():
    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"int\s+msk_label_pyramid\s*\(([^)]*)\)", txt)
    assert m, "include/msegk.h does not declare msk_label_pyramid"
    assert len(m.group(1).split(",")) == 9
    res, args = _lib.SIGNATURES["msk_label_pyramid"]
    vp, i = C.c_void_p, C.c_int
    assert res is i and args == [vp, vp, i, i, i, i, i, vp, vp]
    assert os.path.exists(_lib.LIB_PATH), "run ./build.sh (or __graft_entry__.build()) first"
    assert hasattr(C.CDLL(_lib.LIB_PATH), "msk_label_pyramid")


# ---- the host stack over the stand-in library ---------------------------------------------------------------------------------
fake_pkg = fake_lib.fake_pkg_fixture("fake_msegk.c", "fake_msegk_region.c", "fake_msegk_pyramid.c")


def _pyramid_calls():
    return _fake("fake_pyramid_calls", C.c_long)


def _last_extents():
    n = _fake("fake_pyramid_levels", C.c_int)
    flat = [_fake("fake_pyramid_extent", C.c_int, i) for i in range(3 * n)]
    return [tuple(flat[3 * i:3 * i + 3]) for i in range(n)]


def _dicece(n=4):
    from medicalseg_amd.models import DiceCELoss
    return {"types": [DiceCELoss() for _ in range(n)], "coef": [8 / 15, 1 / 15, 2 / 15, 4 / 15][:n]}


def _mixed(n=4):
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    return {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1]) for _ in range(n)], "coef": [0.25] * n}


def _batch(n=1, seed=0):
    from medicalseg_amd.device import to_tensor
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 1, 16, 16, 16)).astype(np.float32)
    return x, to_tensor(rng.integers(0, 3, (n, 16, 16, 16)).astype(np.int32))


HEAD_EXTENTS = [(2, 2, 2), (4, 4, 4), (8, 8, 8)]        # h1 (coarsest), h2, h3 of a 16^3 input with 2x2x2 strides


@pytest.mark.parametrize("make_losses,terms_per_head", [(_dicece, 1), (_mixed, 2)], ids=["DiceCELoss", "MixedLoss"])
def test_native_step_is_one_pyramid_launch_four_nodes_one_backward(fake_pkg, calls, monkeypatch, make_losses, terms_per_head):
    from medicalseg_amd.models import VNetDeepSup
    from medicalseg_amd.utils import loss_computation
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    model.train()
    losses = make_losses()
    x, y = _batch()
    backwards = []
    real = type(model).backward
    monkeypatch.setattr(type(model), "backward", lambda self, grads: (backwards.append(grads), real(self, grads))[1])
    levels_seen = []
    for step in range(2):
        before = _pyramid_calls()
        del calls[:], backwards[:]
        outs = model(x)
        assert [(o.d, o.h, o.w) for o in outs] == [(16, 16, 16)] + HEAD_EXTENTS
        assert outs[0].native_head is None and [o.native_head[1] for o in outs[1:]] == [0, 1, 2]
        loss_list, dice = loss_computation(outs, y, losses)
        nodes = {id(t[1]): t[1] for l in loss_list for t in l.terms}
        assert len(loss_list) == 4 * terms_per_head and len(nodes) == 4 and np.asarray(dice).shape == (3,)
        # every head's node holds the level of its own extent; the full-resolution output holds the label itself
        by_logits = {id(n.logits): n for n in nodes.values()}
        assert by_logits[id(outs[0])].labels is y
        for o in outs[1:]:
            assert tuple(by_logits[id(o)].labels.shape) == (1, o.d, o.h, o.w)
        levels_seen.append([by_logits[id(o)].labels for o in outs[1:]])
        loss_computation(outs, y, losses)                         # a second request in the same step: the cached levels
        sum(loss_list).backward()
        assert _pyramid_calls() - before == 1 and calls.count("msk_label_pyramid") == 1
        assert _last_extents() == HEAD_EXTENTS
        assert [_fake("fake_pyramid_shape", C.c_int, i) for i in range(4)] == [1, 16, 16, 16]
        assert _fake("fake_pyramid_label", C.c_void_p) == y.ptr
        assert not [c for c in calls if c.startswith("msk_interp_")]
        assert len(backwards) == 1 and len(backwards[0]) == 4 and all(g is not None for g in backwards[0])
        assert [(g.d, g.h, g.w) for g in backwards[0]] == [(16, 16, 16)] + HEAD_EXTENTS
    # the second forward reset the arena: the levels were built again, as new objects of the new generation
    first, second = levels_seen
    assert all(a is not b for a, b in zip(first, second))
    assert all(b.gen == model.dev.arena.gen and a.gen == b.gen - 1 for a, b in zip(first, second))


def test_native_heads_off_makes_the_calls_of_the_code_without_the_helper(fake_pkg, calls, monkeypatch):
    from medicalseg_amd import nn
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import VNetDeepSup
    from medicalseg_amd.models.losses import fused
    from medicalseg_amd.utils import loss_computation

    def run(model, losses):
        nn.Dropout3D.step = 0
        model.train()
        x, y = _batch()
        del calls[:]
        outs = model(x)
        assert len(outs) == 4 and all((o.d, o.h, o.w) == (16, 16, 16) and o.native_head is None for o in outs)
        ll, _ = loss_computation(outs, y, losses)
        sum(ll).backward()
        return list(calls)

    for make_losses in (_dicece, _mixed):
        before = _pyramid_calls()
        mine = run(VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=False), make_losses())
        default = run(VNetDeepSup(elu=False, in_channels=1, num_classes=3), make_losses())
        # the same run with the label selection taken out again: the nodes get the label as the caller gave it
        with monkeypatch.context() as m:
            m.setattr(fused, "label_for", lambda logits, labels: to_tensor(labels, logits.dev))
            m.setattr(fused, "label_pyramid", None)
            without = run(VNetDeepSup(elu=False, in_channels=1, num_classes=3), make_losses())
        assert mine == default == without
        assert _pyramid_calls() == before and "msk_label_pyramid" not in mine
        assert mine.count("msk_interp_trilinear_fwd") == 3 and mine.count("msk_interp_trilinear_bwd") == 3


def test_eval_mode_returns_the_full_resolution_output_only(fake_pkg, calls, monkeypatch):
    from medicalseg_amd import nn
    from medicalseg_amd.models import VNetDeepSup
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    heads = {id(model.out_tr64), id(model.out_tr128), id(model.out_tr256)}
    ran = []
    real = nn.Conv3D.run_forward
    monkeypatch.setattr(nn.Conv3D, "run_forward", lambda self, *a, **k: (ran.append(id(self)), real(self, *a, **k))[1])
    x, _ = _batch()
    model.eval()
    outs = model(x)
    assert isinstance(outs, list) and len(outs) == 1 and (outs[0].d, outs[0].h, outs[0].w) == (16, 16, 16)
    assert not heads & set(ran) and not [c for c in calls if c.startswith("msk_interp_")]
    del ran[:]
    model.train()
    assert len(model(x)) == 4 and heads <= set(ran)
    # the up-sampling form keeps its four outputs in eval mode, as before
    plain = VNetDeepSup(elu=False, in_channels=1, num_classes=3)
    plain.eval()
    assert len(plain(x)) == 4
    # one set of parameters under either setting
    assert list(plain.state_dict().keys()) == list(model.state_dict().keys())
    assert [tuple(v.shape) for v in plain.state_dict().values()] == [tuple(v.shape) for v in model.state_dict().values()]
    assert ({n for n, p in plain.named_parameters() if getattr(p, "frozen", False)}
            == {n for n, p in model.named_parameters() if getattr(p, "frozen", False)})


def test_a_mismatched_label_without_the_mark_still_raises(fake_pkg):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import BCELoss, CrossEntropyLoss, DiceCELoss, DiceLoss, VNet, VNetDeepSup
    model = VNet(num_classes=3)
    model.train()
    x, _ = _batch()
    small = to_tensor(np.zeros((1, 8, 8, 8), dtype=np.int32))
    before = _pyramid_calls()
    out = model(x)[0]
    for loss in (CrossEntropyLoss(), DiceLoss(), DiceCELoss(), BCELoss()):
        with pytest.raises(ValueError, match=r"label shape \(1, 8, 8, 8\) does not match logits \(1, 3, 16, 16, 16\)"):
            loss(out, small)
    # a marked head takes its level, but not from a label of another batch size
    ds = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    ds.train()
    outs = ds(x)
    with pytest.raises(ValueError, match="does not match logits"):
        DiceCELoss()(outs[1], to_tensor(np.zeros((2, 16, 16, 16), dtype=np.int32)))
    assert _pyramid_calls() == before


def test_label_pyramid_allocates_the_levels_from_the_arena(fake_pkg, calls):
    from medicalseg_amd.device import IntTensor, get_device
    from medicalseg_amd.models.losses.fused import label_pyramid
    _, y = _batch(n=2)
    dev = get_device()
    levels = label_pyramid(y, [(8, 8, 8), (3, 2, 5)])
    assert [type(l) for l in levels] == [IntTensor, IntTensor]
    assert [l.shape for l in levels] == [(2, 8, 8, 8), (2, 3, 2, 5)] and all(l.gen == dev.arena.gen for l in levels)
    assert _last_extents() == [(8, 8, 8), (3, 2, 5)]
    assert [_fake("fake_pyramid_dst", C.c_void_p, i) for i in range(2)] == [l.ptr for l in levels]
    assert calls[-1] == "msk_label_pyramid"


def test_both_yaml_files_build(fake_pkg):
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceCELoss, MixedLoss, VNetDeepSup
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = Config(NNUNET_YML)
        base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicece_96.yml"))
    model = cfg.model
    assert type(model) is VNetDeepSup and model.native_heads and model.num_classes == 3
    losses = cfg.loss
    assert [type(t) for t in losses["types"]] == [DiceCELoss] * 4 and len({id(t) for t in losses["types"]}) == 4
    assert np.allclose(losses["coef"], np.array([8, 1, 2, 4]) / 15, rtol=0, atol=1e-15) and abs(sum(losses["coef"]) - 1) < 1e-15
    assert all(t.ignore_index == 255 for t in losses["types"])
    # everything but the model and the loss is the DiceCE recipe
    assert ({k: v for k, v in cfg.dic.items() if k not in ("loss", "model")}
            == {k: v for k, v in base.dic.items() if k not in ("loss", "model")})

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = Config(MRI_YML)
        base = Config(os.path.join(ROOT, "configs", "synthetic", "vnetdeepsup_synthetic_mri_512_512_12.yml"))
    assert cfg.dic["model"] == dict(base.dic["model"], native_heads=True)
    assert {k: v for k, v in cfg.dic.items() if k != "model"} == {k: v for k, v in base.dic.items() if k != "model"}
    model = cfg.model
    assert type(model) is VNetDeepSup and model.native_heads
    assert [type(t) for t in cfg.loss["types"]] == [MixedLoss] * 4 and cfg.loss["coef"] == [0.25] * 4
    # the MRI geometry: the slice axis goes 12 -> 9 -> 8 -> 4
    model.train()
    outs = model(np.zeros((1, 1, 32, 32, 12), dtype=np.float32))
    assert [(o.d, o.h, o.w) for o in outs] == [(32, 32, 12), (4, 4, 4), (8, 8, 8), (16, 16, 9)]

"""BCELoss without a GPU: registration, constructor validation (reference losses/binary_cross_entropy_loss.py:84-120), the
shipped YAML, the edge_label guard, and the float64 restatement (tests/bce_reference.py) against torch's
binary_cross_entropy_with_logits."""
import os

import numpy as np
import pytest

import bce_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bce_loss_is_registered():
    from medicalseg_amd.cvlibs import manager
    from medicalseg_amd.models import BCELoss
    assert "BCELoss" in manager.LOSSES
    assert manager.LOSSES["BCELoss"] is BCELoss


def test_constructor_validation_matches_reference():
    from medicalseg_amd.models import BCELoss
    loss = BCELoss()
    assert loss.weight is None and loss.pos_weight is None and loss.ignore_index == 255 and loss.edge_label is False
    assert loss.EPS == 1e-10
    BCELoss(weight='dynamic', pos_weight='dynamic')
    BCELoss(pos_weight=2.5, ignore_index=0, edge_label=True)
    with pytest.raises(ValueError, match="if type of `weight` is str, it should equal to 'dynamic', but it is static"):
        BCELoss(weight='static')
    with pytest.raises(ValueError, match="if type of `pos_weight` is str, it should equal to 'dynamic', but it is auto"):
        BCELoss(pos_weight='auto')
    with pytest.raises(TypeError, match="The type of `pos_weight` is wrong, it should be float or str"):
        BCELoss(pos_weight=2)                      # an int raises in the reference too
    with pytest.raises(TypeError, match="The type of `pos_weight` is wrong"):
        BCELoss(pos_weight=[1.0])
    with pytest.raises(TypeError, match="The type of `weight` is wrong"):
        BCELoss(weight=np.ones(3, np.float32))     # per-element weight tensors: not supported


def test_bce_yaml_resolves_to_mixed_loss_with_bce_member():
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import BCELoss, DiceLoss, MixedLoss
    with pytest.warns(UserWarning):   # data_root == 'data/' warning, like the reference
        cfg = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_bce_128.yml"))
    losses = cfg.loss
    assert losses["coef"] == [1] and len(losses["types"]) == 1
    mixed = losses["types"][0]
    assert isinstance(mixed, MixedLoss) and mixed.coef == [1, 1]
    assert [type(m) for m in mixed.losses] == [BCELoss, DiceLoss]
    assert mixed.losses[0].weight is None and mixed.losses[0].pos_weight is None and mixed.losses[0].ignore_index == 255


def test_edge_label_without_edges_raises():
    from medicalseg_amd.models import BCELoss
    from medicalseg_amd.utils import loss_computation

    class _Logits:   # never reached: the guard fires before the loss touches its inputs
        pass

    losses = {"types": [BCELoss(edge_label=True)], "coef": [1]}
    with pytest.raises(ValueError, match="edge_label"):
        loss_computation([_Logits()], None, losses)


@pytest.mark.parametrize("C", [1, 2, 3, 5])
@pytest.mark.parametrize("weight", [None, 'dynamic'])
@pytest.mark.parametrize("pos_weight", [None, 2.5, 'dynamic'])
def test_restatement_matches_torch_float64(C, weight, pos_weight):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    rng = np.random.default_rng(C * 7 + (weight is None) + 3 * (pos_weight is None))
    N, D, H, W = 2, 3, 4, 5
    x = rng.standard_normal((N, C, D, H, W)) * 3
    label = rng.integers(0, max(C, 2), (N, D, H, W))
    label[rng.random((N, D, H, W)) < 0.1] = 255                      # ignored voxels
    label[0, 0, 0, 0] = C + 1 if C > 1 else 0                        # outside [0, C) but not ignored: all-zero row
    loss, grad = R.bce(x, label, 255, weight, pos_weight)

    # torch side: mask and one-hot built explicitly here (Paddle's GPU one_hot: zero row outside [0, C))
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lab = torch.tensor(label)
    mask = (lab != 255).double().unsqueeze(1)
    if C == 1:
        y = lab.double().unsqueeze(1)
    else:
        inside = (lab >= 0) & (lab < C)
        y = F.one_hot(torch.where(inside, lab, torch.zeros_like(lab)), C).permute(0, 4, 1, 2, 3).double()
        y = y * inside.double().unsqueeze(1)
    pos, neg = float((y == 1).sum()), float((y == 0).sum())
    w = None
    if weight == 'dynamic':
        w = 2 * neg / (pos + neg + 1e-10) * y + 2 * pos / (pos + neg + 1e-10) * (1 - y)
    pw = None
    if pos_weight == 'dynamic':
        pw = torch.tensor(2 * neg / (pos + neg + 1e-10), dtype=torch.float64)
    elif pos_weight is not None:
        pw = torch.tensor(pos_weight, dtype=torch.float64)
    elem = F.binary_cross_entropy_with_logits(xt, y, weight=w, pos_weight=pw, reduction='none')
    ref = (elem * mask).mean() / (mask.mean() + 1e-10)
    ref.backward()
    ref = float(ref.detach())
    assert abs(loss - ref) <= 1e-12 * abs(ref)
    g = xt.grad.numpy()
    assert np.abs(grad - g).max() <= 1e-12 * np.abs(g).max()


def test_restatement_all_ignored_is_zero():
    x = np.random.default_rng(0).standard_normal((1, 3, 2, 2, 2))
    loss, grad = R.bce(x, np.full((1, 2, 2, 2), 255), 255, 'dynamic', 'dynamic')
    assert loss == 0.0 and not grad.any()


def test_loader_binds_a_missing_symbol_to_a_raising_stub(tmp_path):
    """A library without the BCE entry points (the no-compute stand-in tests/fake_msegk.c) still loads; calling one
    raises MskError naming it."""
    import subprocess
    from medicalseg_amd import _lib
    so = str(tmp_path / "libfake_msegk.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-w", "-o", so,
                           os.path.join(ROOT, "tests", "fake_msegk.c")])
    real_path, real_lib = _lib.LIB_PATH, _lib._lib
    try:
        _lib.LIB_PATH, _lib._lib = so, None
        lib = _lib.load()
        assert lib.msk_version() == -1                # the stand-in, loaded
        with pytest.raises(_lib.MskError, match="msk_bce_fwd"):
            lib.msk_bce_fwd(None)
    finally:
        _lib.LIB_PATH, _lib._lib = real_path, real_lib

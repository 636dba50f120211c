"""The statement of the region losses (tests/region_reference.py) WITHOUT a GPU: against torch autograd in float64, against
torch's cross_entropy at gamma = 0, Dice against the Tversky form at alpha = beta = 0.5, and the all-ignored edge."""
import itertools

import numpy as np
import pytest

import region_reference as R

torch = pytest.importorskip("torch")


def _data(rng, shape, C, ignore_frac=0.1):
    N, D, H, W = shape
    z = rng.standard_normal((N, C, D, H, W)) * 2
    y = rng.integers(0, max(C, 2), (N, D, H, W)).astype(np.int32)
    y[rng.random(y.shape) < ignore_frac] = 255
    if C > 1:
        y.flat[1] = C + 2          # outside [0, C), not ignored: an all-zero target row, no focal term
    return z, y


def _torch_loss(z, y, activation, squared_pred, batch_dice, do_bg, smooth, tversky, lambda_r, lambda_f, gamma, weight):
    """The same loss written with torch operations only; the gradient is autograd's."""
    C = z.shape[1]
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y.astype(np.int64))
    m = (yt != 255).double()[:, None]
    t = (yt[:, None] == (1 if C == 1 else torch.arange(C).view(1, C, 1, 1, 1))).double()
    p = torch.softmax(zt, 1) if activation == 'softmax' else torch.sigmoid(zt)
    ax = (2, 3, 4)
    TP, SP, ST = (m * p * t).sum(ax), (m * p ** (2 if squared_pred else 1)).sum(ax), (m * t).sum(ax)
    if batch_dice:
        TP, SP, ST = TP.sum(0, keepdim=True), SP.sum(0, keepdim=True), ST.sum(0, keepdim=True)
    if tversky is None:
        sc = (2 * TP + smooth) / torch.clamp(SP + ST + smooth, min=1e-8)
    else:
        a, b = tversky
        sc = (TP + smooth) / (TP + a * (SP - TP) + b * (ST - TP) + smooth)
    if not do_bg and C > 1:
        sc = sc[:, 1:]
    L = lambda_r * (1 - sc.mean())
    if lambda_f:
        valid = (yt >= 0) & (yt < C) & (yt != 255)
        yy = torch.where(valid, yt, torch.zeros_like(yt))
        lp = torch.log_softmax(zt, 1).gather(1, yy[:, None])[:, 0]
        wy = torch.tensor(weight, dtype=torch.float64)[yy] * valid
        L = L + lambda_f * (wy * (-(1 - lp.exp()) ** gamma * lp)).sum() / wy.sum()
    L.backward()
    return float(L.detach()), zt.grad.numpy()


@pytest.mark.parametrize("shape", [(2, 16, 16, 16), (3, 5, 7, 9)])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 20])
def test_statement_matches_torch_autograd(C, shape):
    rng = np.random.default_rng(100 * C + shape[1])
    z, y = _data(rng, shape, C)
    w = rng.uniform(0.5, 2, C)
    worst = 0.0
    for activation, squared, batch, do_bg, tversky, gamma in itertools.product(
            ('softmax', 'sigmoid'), (False, True), (True, False), (True, False), (None, (0.3, 0.7)), (0.0, 2.0)):
        if (C == 1 and activation == 'softmax') or (tversky and squared):
            continue
        if activation == 'sigmoid' and gamma:     # no focal term with the sigmoid: one pass over gamma is enough
            continue
        lam_f = 1.0 if activation == 'softmax' else 0.0
        got = R.region_loss(z, y, activation, squared, batch, do_bg, 1e-5, tversky, 1.0, lam_f, gamma, w)
        ref_l, ref_g = _torch_loss(z, y, activation, squared, batch, do_bg, 1e-5, tversky, 1.0, lam_f, gamma, w)
        e_l = abs(got["loss"] - ref_l) / abs(ref_l)
        e_g = np.abs(got["grad"] - ref_g).max() / np.abs(ref_g).max()
        worst = max(worst, e_l, e_g)
        assert e_l <= 1e-12 and e_g <= 1e-12, (activation, squared, batch, do_bg, tversky, gamma, e_l, e_g)
    print("worst relative deviation from torch autograd: %.2e" % worst)


@pytest.mark.parametrize("weighted", [False, True])
def test_gamma_zero_is_torch_cross_entropy(weighted):
    rng = np.random.default_rng(7)
    z, y = _data(rng, (2, 6, 7, 8), 4)
    y.flat[1] = 2                                                  # cross_entropy rejects labels outside [0, C)
    w = rng.uniform(0.5, 2, 4) if weighted else None
    got = R.region_loss(z, y, lambda_r=0.0, lambda_f=1.0, gamma=0.0, weight=w)
    zt = torch.tensor(z, requires_grad=True)
    ce = torch.nn.functional.cross_entropy(zt, torch.tensor(y.astype(np.int64)), ignore_index=255,
                                           weight=None if w is None else torch.tensor(w))
    ce.backward()
    assert abs(got["L_f"] - float(ce)) <= 1e-12 * abs(float(ce))
    assert np.abs(got["grad"] - zt.grad.numpy()).max() <= 1e-12 * np.abs(zt.grad.numpy()).max()


def test_dice_is_tversky_at_one_half():
    """(2 TP + s) / (SP + ST + s) = (TP + s/2) / (TP + (SP - TP)/2 + (ST - TP)/2 + s/2): smooth halves."""
    rng = np.random.default_rng(8)
    z, y = _data(rng, (2, 5, 7, 9), 3)
    for batch, do_bg in itertools.product((True, False), (True, False)):
        dice = R.region_loss(z, y, batch_dice=batch, do_bg=do_bg, smooth=1e-3)
        tv = R.region_loss(z, y, batch_dice=batch, do_bg=do_bg, smooth=0.5e-3, tversky=(0.5, 0.5))
        assert abs(dice["L_r"] - tv["L_r"]) <= 1e-13
        assert np.abs(dice["grad"] - tv["grad"]).max() <= 1e-12 * np.abs(dice["grad"]).max()
        assert np.allclose(dice["dice"], tv["dice"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("activation", ["softmax", "sigmoid"])
def test_all_ignored_labels(activation):
    rng = np.random.default_rng(9)
    z = rng.standard_normal((2, 3, 4, 5, 6))
    y = np.full((2, 4, 5, 6), 255, np.int32)
    for tversky in (None, (0.3, 0.7)):
        r = R.region_loss(z, y, activation, tversky=tversky, lambda_f=1.0 if activation == 'softmax' else 0.0, gamma=2.0)
        assert r["L_f"] == 0.0 and np.isfinite(r["L_r"]) and not r["grad"].any()
        assert r["L_r"] == 0.0                 # every score is smooth / smooth
    y[0, 0, 0, 0] = 1                          # one live voxel: the gradient is still 0 wherever m = 0
    r = R.region_loss(z, y, activation, lambda_f=1.0 if activation == 'softmax' else 0.0)
    g = np.moveaxis(r["grad"], 1, -1)
    assert not g[y == 255].any() and g[y != 255].any()


def test_argument_errors():
    z, y = np.zeros((1, 3, 2, 2, 2)), np.zeros((1, 2, 2, 2), np.int32)
    for kw in (dict(gamma=0.5, lambda_f=1.0), dict(gamma=-1.0), dict(smooth=-1.0), dict(tversky=(0.3, 0.7), squared_pred=True),
               dict(activation='sigmoid', lambda_f=1.0)):
        with pytest.raises(ValueError):
            R.region_loss(z, y, **kw)
    with pytest.raises(ValueError):
        R.region_loss(z[:, :1], y, activation='softmax')

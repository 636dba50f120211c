"""Float64 numpy statement of the region losses (SoftDiceLoss, TverskyLoss, FocalLoss, DiceCELoss): loss value, the side
outputs and d loss / d logits.  Checked against torch autograd in tests/test_region_loss.py; the device kernels
(medicalseg_amd/csrc/msk_loss_region.hip) are checked against it in tests/test_gpu_region_loss.py.

Per voxel: m = (y != ignore_index); t_c = (y == c) for C > 1 (a label outside [0, C) that is not ignored gives an all-zero
row, as in bce_reference.targets), t = (y == 1) for C == 1; p = softmax over the classes or sigmoid.
Per (group g, class c), a group being the batch (batch_dice) or a sample: TP = sum m p t, SP = sum m p^q, ST = sum m t.
  Dice     score = (2 TP + smooth) / max(SP + ST + smooth, 1e-8)
  Tversky  score = (TP + smooth) / (TP + alpha (SP - TP) + beta (ST - TP) + smooth)          (q = 1)
  L_r = 1 - mean of score over the groups and the scored classes K
  L_f = sum valid w_y (1 - u)^gamma (-log u) / sum valid w_y,  valid = m and 0 <= y < C,  u = p_y  (softmax only)
  L = lambda_r L_r + lambda_f L_f"""
import numpy as np

CLAMP = 1e-8


def mask(y, ignore_index=255):
    return (np.asarray(y) != ignore_index)[:, None].astype(np.float64)


def targets(y, C):
    y = np.asarray(y)
    if C == 1:
        return (y[:, None] == 1).astype(np.float64)
    return (y[:, None] == np.arange(C).reshape(1, C, 1, 1, 1)).astype(np.float64)


def probabilities(z, activation):
    """-> (p, log_softmax or None)"""
    z = np.asarray(z, dtype=np.float64)
    if activation == 'sigmoid':
        return np.exp(-np.logaddexp(0, -z)), None
    if activation != 'softmax' or z.shape[1] < 2:
        raise ValueError("activation is 'softmax' (C >= 2) or 'sigmoid'")
    zs = z - z.max(1, keepdims=True)
    e = np.exp(zs)
    se = e.sum(1, keepdims=True)
    return e / se, zs - np.log(se)


def sums(p, t, m, squared_pred=False, batch_dice=True):
    """-> TP, SP, ST, each [G, C]"""
    ax = (2, 3, 4)
    TP, SP, ST = (m * p * t).sum(ax), (m * (p * p if squared_pred else p)).sum(ax), (m * t).sum(ax)
    if batch_dice:
        TP, SP, ST = TP.sum(0, keepdims=True), SP.sum(0, keepdims=True), ST.sum(0, keepdims=True)
    return TP, SP, ST


def scored_classes(C, do_bg):
    K = np.ones(C, bool)
    if not do_bg and C > 1:
        K[0] = False
    return K


def scores(TP, SP, ST, smooth, tversky=None):
    """-> score, dscore/dTP, dscore/dSP, each [G, C]; tversky = None (Dice) or (alpha, beta)"""
    if tversky is None:
        num, raw = 2 * TP + smooth, SP + ST + smooth
        den = np.maximum(raw, CLAMP)
        return num / den, 2 / den, np.where(raw >= CLAMP, -num / den ** 2, 0.0)
    alpha, beta = tversky
    k = 1 - alpha - beta
    num, den = TP + smooth, k * TP + alpha * SP + beta * ST + smooth
    return num / den, 1 / den - num * k / den ** 2, -num * alpha / den ** 2


def region_loss(z, y, activation='softmax', squared_pred=False, batch_dice=True, do_bg=False, smooth=1e-5, tversky=None,
                lambda_r=1.0, lambda_f=0.0, gamma=0.0, weight=None, ignore_index=255):
    """logits z [N, C, D, H, W], labels y [N, D, H, W] int -> dict of float64 results:
    loss, L_r, L_f, grad (d loss / d z), grad_r, grad_f (the unscaled parts), dice ([C]: mean over the groups of the score),
    TP, SP, ST, A, B ([G, C]), f_num, f_den."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y)
    N, C = z.shape[:2]
    if tversky is not None and squared_pred:
        raise ValueError("Tversky takes squared_pred=False")
    if not (gamma == 0 or gamma >= 1):
        raise ValueError("gamma must be 0 or >= 1")
    if smooth < 0:
        raise ValueError("smooth must be >= 0")
    if lambda_f and activation != 'softmax':
        raise ValueError("the focal / CE term needs the softmax")
    m, t = mask(y, ignore_index), targets(y, C)
    p, logp = probabilities(z, activation)
    q = 2 if squared_pred else 1
    TP, SP, ST = sums(p, t, m, squared_pred, batch_dice)
    G = TP.shape[0]
    K = scored_classes(C, do_bg)
    sc, dTP, dSP = scores(TP, SP, ST, smooth, tversky)
    nk = G * K.sum()
    L_r = 1 - (sc * K).sum() / nk
    A, B = -dTP * K / nk, -dSP * K / nk
    Ab = np.broadcast_to(A, (N, C))[:, :, None, None, None]
    Bb = np.broadcast_to(B, (N, C))[:, :, None, None, None]
    g = m * (Ab * t + Bb * (2 * p if q == 2 else 1.0))
    grad_r = p * (g - (p * g).sum(1, keepdims=True)) if activation == 'softmax' else p * (1 - p) * g

    L_f, grad_f, f_num, f_den = 0.0, np.zeros_like(z), 0.0, 0.0
    if activation == 'softmax':
        w = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64).reshape(C)
        valid = (y != ignore_index) & (y >= 0) & (y < C)
        yy = np.where(valid, y, 0)
        wy = np.where(valid, w[yy], 0.0)
        u = np.take_along_axis(p, yy[:, None], 1)[:, 0]
        logu = np.take_along_axis(logp, yy[:, None], 1)[:, 0]            # z_y - max - log sum exp, never log(p_y)
        omu = (p * (1 - targets(yy, C))).sum(1)                          # 1 - u as the sum of the other classes
        if gamma == 0:
            f, uf = -logu, -np.ones_like(u)                               # u f'(u)
        else:
            f = -omu ** gamma * logu
            uf = gamma * omu ** (gamma - 1) * u * logu - omu ** gamma
        f_num, f_den = float((wy * f).sum()), float(wy.sum())
        if f_den != 0:
            L_f = f_num / f_den
            grad_f = (wy * uf / f_den)[:, None] * (t - p) * valid[:, None]
    return {"loss": lambda_r * L_r + lambda_f * L_f, "L_r": float(L_r), "L_f": float(L_f),
            "grad": lambda_r * grad_r + lambda_f * grad_f, "grad_r": grad_r, "grad_f": grad_f,
            "dice": sc.mean(0), "TP": TP, "SP": SP, "ST": ST, "A": A, "B": B, "f_num": f_num, "f_den": f_den}

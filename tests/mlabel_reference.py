"""Float64 numpy statement of region-based training (DiceBCERegionLoss, msk_mlabel_loss_fwd / msk_mlabel_loss_bwd,
msk_regions_to_label, utils.metric.region_areas_from_counts).  Checked against torch autograd in tests/test_mlabel_host.py; the
device kernels (medicalseg_amd/csrc/msk_loss_mlabel.hip) are checked against it in tests/test_gpu_mlabel_loss.py and
tests/test_gpu_regions_infer.py.

Settings: R channels (1 <= R <= 32); table[v], a uint32 bit mask for the label values v in [0, V), 1 <= V <= 256; ignore_index;
q = 2 with squared_pred, otherwise 1; a group is the whole batch (batch_dice) or one sample, G groups; smooth.

Per voxel: m = (y != ignore_index); t_r = bit r of table[y] when 0 <= y < V, otherwise 0 (a negative or too large label that is
not ignored gives an all-zero target row); p_r = sigmoid(z_r) in the overflow-free form (exp(-|z|)).

  Dice   per (group, region): TP = sum m p t, SP = sum m p^q, ST = sum m t;
         score = (2 TP + smooth) / max(SP + ST + smooth, 1e-8);  L_dice = 1 - mean over groups and regions of score.  Every
         region counts: there is no do_bg.
  BCE    l = max(z, 0) - z t + log1p(exp(-|z|));  L_bce = sum m sum_r l / (R sum m), and 0 when no voxel is valid.
  grad   coef_bce m (p - t) / (R sum m) + coef_dice m (A t + B q p^(q-1)) p (1 - p),
         A = -2 / (G R den),  B = (2 TP + smooth) / (G R den^2) where den > 1e-8, otherwise 0.

Two conventions differ from nnU-Net's DC_and_BCE_loss: the Dice term is 1 - dice, as SoftDiceLoss writes it, where nnU-Net
writes -dice; and with an ignore label nnU-Net divides the BCE sum by the valid voxels only, not by R times that:
lambda_bce = R reproduces it."""
import numpy as np

CLAMP = 1e-8


def build_table(regions, length=256):
    """uint32 [length]: bit r of table[v] set when v is in regions[r] (an entry is a label value or a list of them)"""
    t = np.zeros(length, dtype=np.uint32)
    for r, values in enumerate(regions):
        for v in ([values] if isinstance(values, (int, np.integer)) else values):
            t[int(v)] |= np.uint32(1 << r)
    return t


def targets(y, table, R):
    """-> t [N, R, D, H, W] float64"""
    y = np.asarray(y).astype(np.int64)
    table = np.asarray(table, dtype=np.uint32)
    inside = (y >= 0) & (y < table.size)
    bits = np.where(inside, table[np.where(inside, y, 0)], 0).astype(np.uint32)
    return np.stack([((bits >> np.uint32(r)) & np.uint32(1)).astype(np.float64) for r in range(R)], axis=1)


def sigmoid(z):
    """overflow-free: 1 / (1 + e) or e / (1 + e), e = exp(-|z|); -> (p, 1 - p, e)"""
    e = np.exp(-np.abs(z))
    inv = 1.0 / (1.0 + e)
    return np.where(z >= 0, inv, e * inv), np.where(z >= 0, e * inv, inv), e


def mlabel_loss(z, y, table, squared_pred=False, batch_dice=True, smooth=1e-5, coef_bce=1.0, coef_dice=1.0, ignore_index=255,
                dtype=np.float64):
    """logits z [N, R, D, H, W], labels y [N, D, H, W] int, table uint32 [V] -> dict: loss, L_bce, L_dice, grad, dice ([R]: mean
    over the groups of the score), TP, SP, ST, A, B ([G, R]), bce_sum, valid.  dtype = np.float32 evaluates every step in
    float32 (the float32 evaluation tests/test_mlabel_host.py holds against the GPU tests' bounds)."""
    z = np.asarray(z, dtype=dtype)
    y = np.asarray(y)
    N, R = z.shape[:2]
    m = (y != ignore_index)[:, None].astype(dtype)
    t = targets(y, table, R).astype(dtype)
    p, omp, e = sigmoid(z)
    q = 2 if squared_pred else 1
    ax = (2, 3, 4)
    TP, SP, ST = (m * p * t).sum(ax, dtype=dtype), (m * (p * p if q == 2 else p)).sum(ax, dtype=dtype), (m * t).sum(ax, dtype=dtype)
    if batch_dice:
        TP, SP, ST = TP.sum(0, keepdims=True), SP.sum(0, keepdims=True), ST.sum(0, keepdims=True)
    G = TP.shape[0]
    smooth = dtype(smooth)
    num, raw = 2 * TP + smooth, SP + ST + smooth
    den = np.maximum(raw, dtype(CLAMP))
    score = num / den
    L_dice = 1 - score.sum(dtype=dtype) / (G * R)
    A = -2 / (G * R * den)
    B = np.where(raw > CLAMP, num / (G * R * den * den), 0).astype(dtype)
    l = np.maximum(z, 0) - z * t + np.log1p(e)
    bce_sum, valid = (m * l).sum(dtype=dtype), m.sum(dtype=dtype)
    L_bce = bce_sum / (R * valid) if valid != 0 else dtype(0)
    Ab = np.broadcast_to(A, (N, R))[:, :, None, None, None]
    Bb = np.broadcast_to(B, (N, R))[:, :, None, None, None]
    kb = dtype(coef_bce) / (R * valid) if valid != 0 else dtype(0)
    grad = kb * m * np.where(t != 0, -omp, p) + dtype(coef_dice) * m * (Ab * t + Bb * (2 * p if q == 2 else 1)) * p * omp
    return {"loss": float(coef_bce * L_bce + coef_dice * L_dice), "L_bce": float(L_bce), "L_dice": float(L_dice), "grad": grad,
            "dice": score.mean(0), "TP": TP, "SP": SP, "ST": ST, "A": A, "B": B, "bce_sum": float(bce_sum), "valid": float(valid)}


def regions_to_label(z, class_order):
    """z [N, R, D, H, W] -> int32 [N, D, H, W]: out = 0, then for r = 0 .. R-1 in order out[z_r > 0] = class_order[r].  The
    last region that fires wins (nnU-Net's loop).  The comparison is on the LOGIT: a NaN does not fire, and neither does 0 or
    -0.0.  (In float32, 1 / (1 + expf(-z)) > 0.5 is false for a tiny positive z, so the probability form is not the
    specification.)"""
    z = np.asarray(z)
    out = np.zeros((z.shape[0],) + z.shape[2:], dtype=np.int32)
    with np.errstate(invalid='ignore'):
        for r, cls in enumerate(class_order):
            out[z[:, r] > 0] = cls
    return out


def region_areas(confusion, table, R):
    """confusion: [K, K] counts, rows the label's class and columns the prediction's, the last row and column the "other" class
    (a value outside the classes), which belongs to no region; class c < K - 1 belongs to region r when bit r of table[c] is
    set.  -> (intersect, pred_area, label_area), int64 [R]: the voxels whose label and prediction / prediction / label lie in
    the region."""
    confusion = np.asarray(confusion).astype(np.int64)
    K = confusion.shape[0]
    inter, pa, la = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    for r in range(R):
        members = [c for c in range(K - 1) if c < len(table) and (int(table[c]) >> r) & 1]
        for l in range(K):
            for p in range(K):
                n = int(confusion[l, p])
                inter[r] += n if (l in members and p in members) else 0
                pa[r] += n if p in members else 0
                la[r] += n if l in members else 0
    return inter, pa, la

"""Float64 numpy restatement of BCELoss (reference medicalseg/models/losses/binary_cross_entropy_loss.py:84-172) as
medicalseg_amd implements it: loss value and d loss / d logits.  Checked against torch's binary_cross_entropy_with_logits
in tests/test_bce_loss.py; the device kernels are checked against it in tests/test_gpu_bce.py."""
import numpy as np

EPS = 1e-10


def targets(label, C):
    """y [N, C, D, H, W]: the label value (C == 1) or one_hot(label, C) with an all-zero row outside [0, C)."""
    label = np.asarray(label)
    if C == 1:
        return label[:, None].astype(np.float64)
    return (label[:, None] == np.arange(C).reshape(1, C, 1, 1, 1)).astype(np.float64)


def weights(y, weight=None, pos_weight=None):
    """-> (w, pw): the element weight (scalar 1 or an array like y) and the positive-class weight."""
    pos = float(np.count_nonzero(y == 1))
    neg = float(np.count_nonzero(y == 0))
    sum_num = pos + neg + EPS
    w = 1.0
    if weight == 'dynamic':
        w = 2 * neg / sum_num * y + 2 * pos / sum_num * (1 - y)
    if pos_weight == 'dynamic':
        pw = 2 * neg / sum_num
    elif pos_weight is None:
        pw = 1.0
    else:
        pw = float(pos_weight)
    return w, pw


def bce(logits, label, ignore_index=255, weight=None, pos_weight=None):
    """logits [N, C, D, H, W], label [N, D, H, W] int -> (loss, dloss/dlogits), float64."""
    x = np.asarray(logits, dtype=np.float64)
    label = np.asarray(label)
    C = x.shape[1]
    y = targets(label, C)
    mask = (label != ignore_index).astype(np.float64)[:, None]
    w, pw = weights(y, weight, pos_weight)
    sp = np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0)          # log(1 + e^-x)
    elem = w * ((1 - y) * x + (1 + (pw - 1) * y) * sp)
    den = mask.sum() / label.size + EPS                              # mean(mask), mask [N, 1, D, H, W]
    loss = (elem * mask).sum() / x.size / den
    sig_neg = np.exp(-np.logaddexp(0, x))                            # sigmoid(-x)
    grad = mask * w * ((1 - y) - (1 + (pw - 1) * y) * sig_neg) / x.size / den
    return float(loss), grad

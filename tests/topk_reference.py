"""The statement of the top-k select and of the top-k cross entropy (msk_topk_select / msk_topk_ce_fwd / msk_topk_ce_bwd,
medicalseg_amd/csrc/msk_loss_topk.hip; TopKLoss and DiceTopKLoss) in numpy.

Select.  x is n float32 values and 0 <= K <= n.  Values are ordered by the sortable key of their 32-bit pattern: sign bit set ->
all bits flipped, else the sign bit set.  So -0.0 < +0.0, a NaN with a clear sign bit lies above +inf, and nothing is left to a
float comparison.  The record is 8 doubles {T, K, n_gt, n_eq, S_gt, r, tie_w, S}: T the value whose key is the K-th largest key,
n_gt / n_eq the keys above / equal to it, S_gt the float64 sum of the values above T in the fixed order of msk_intensity_stats
(ordered_sum below; an element that is not above T contributes +0.0), r = K - n_gt, tie_w = r / n_eq, S = S_gt + r * T.
K == 0: all zeros.

Top-k cross entropy.  Logits z [N, C, D, H, W] (numpy's layout; the device holds [N, D, H, W, C]), labels int32 [N, D, H, W].  A
voxel is valid when its label is in [0, C) and is not ignore_index.  l_i = w[y_i] * (log(sum_c exp(z_c - m)) - (z_y - m)), m the
row maximum, the sum over c ascending; invalid voxels get the sentinel -1.  K = floor(double(n_valid) * double(float32(k)) /
100), at least 1 when n_valid > 0.  loss = S / K of the select over l (0 when n_valid == 0).  Gradient: dL/dz_i = coef * u_i *
w[y_i] * (softmax(z_i) - onehot(y_i)) / K with u_i = 1 for l_i above T, tie_w at T, 0 below and at invalid voxels."""
import numpy as np

SENTINEL = np.float32(-1.0)


def sort_key(x):
    b = np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unsort_key(k):
    k = np.asarray(k, np.uint32).reshape(-1)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return b.view(np.float32)


def _lanes_then_tree(terms):
    """float64 [groups, k, 256] -> [groups]: lane l adds its k terms in order, then the tree v[l] += v[l+s], s = 128 .. 1"""
    acc = np.zeros((terms.shape[0], 256), np.float64)
    for j in range(terms.shape[1]):
        acc = acc + terms[:, j, :]
    s = 128
    while s >= 1:
        acc = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    return acc[:, 0]


def ordered_sum(v):
    """msk_intensity_stats' float64 sum: chunks of 4096 (256 lanes x 16 strided terms, then the tree), then the chunk values by
    the same scheme; missing elements count as +0.0 (transforms.transform._ordered_sum, which a test holds this one to)"""
    v = np.asarray(v, np.float64).reshape(-1)
    nc = -(-v.size // 4096)
    pad = np.zeros(nc * 4096, np.float64)
    pad[:v.size] = v
    p = _lanes_then_tree(pad.reshape(nc, 16, 256))
    rows = -(-nc // 256)
    pad = np.zeros(rows * 256, np.float64)
    pad[:nc] = p
    return float(_lanes_then_tree(pad.reshape(1, rows, 256))[0])


def select(x, K):
    """the record {T, K, n_gt, n_eq, S_gt, r, tie_w, S} as 8 float64"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n, K = x.size, int(K)
    assert 0 <= K <= n
    if K == 0:
        return np.zeros(8, np.float64)
    keys = sort_key(x)
    kth = np.partition(keys, n - K)[n - K]
    T = np.float64(unsort_key(kth)[0])
    above = keys > kth
    n_gt, n_eq = int(above.sum()), int((keys == kth).sum())
    S_gt = np.float64(ordered_sum(np.where(above, x.astype(np.float64), 0.0)))
    r = np.float64(K - n_gt)
    tie_w = r / np.float64(n_eq)
    S = S_gt + r * T
    return np.array([T, K, n_gt, n_eq, S_gt, r, tie_w, S], np.float64)


def k_of(n_valid, k):
    """K of the top k per cent of n_valid voxels, with the device's conversions"""
    K = int(np.floor(np.float64(n_valid) * np.float64(np.float32(k)) / np.float64(100.0)))
    return max(K, 1) if n_valid > 0 else 0


def _rows(z, y, ignore_index):
    C = z.shape[1]
    zz = np.moveaxis(np.asarray(z), 1, -1).reshape(-1, C)
    yy = np.asarray(y).reshape(-1)
    valid = (yy >= 0) & (yy < C) & (yy != ignore_index)
    return zz, yy, valid


def voxel_loss(z, y, ignore_index=255, weight=None, dtype=np.float64):
    """l [V] in `dtype` (sentinel -1 at invalid voxels) and the validity mask"""
    zz, yy, valid = _rows(z, y, ignore_index)
    zz = zz.astype(dtype)
    C = zz.shape[1]
    w = np.ones(C, dtype) if weight is None else np.asarray(weight, np.float32).astype(dtype)
    yc = np.where(valid, yy, 0)
    m = zz.max(axis=1)
    se = np.zeros(zz.shape[0], dtype)
    for c in range(C):
        se = se + np.exp(zz[:, c] - m)
    zym = zz[np.arange(zz.shape[0]), yc] - m
    l = w[yc] * (np.log(se) - zym)
    return np.where(valid, l, dtype(-1.0)).astype(dtype), valid


def membership(l, T, tie_w, valid):
    """u: 1 above T, tie_w at T, 0 below and at invalid voxels; float32 l compares by the sortable key"""
    if l.dtype == np.float32:
        a, t = sort_key(l), sort_key(np.float32(T))[0]
    else:
        a, t = l, T
    u = np.where(a > t, 1.0, np.where(a == t, np.float64(tie_w), 0.0))
    return np.where(valid, u, 0.0)


def grad_from(z, y, u, K, coef=1.0, ignore_index=255, weight=None):
    """float64 [N, C, D, H, W]: coef * u * w[y] * (softmax(z) - onehot(y)) / K"""
    zz, yy, valid = _rows(z, y, ignore_index)
    zz = zz.astype(np.float64)
    V, C = zz.shape
    w = np.ones(C) if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    yc = np.where(valid, yy, 0)
    e = np.exp(zz - zz.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    p[np.arange(V), yc] -= 1.0
    g = p * (np.float64(coef) * u * w[yc] / max(float(K), 1.0))[:, None]
    g[u == 0] = 0.0
    N = z.shape[0]
    return np.moveaxis(g.reshape((N,) + tuple(z.shape[2:]) + (C,)), -1, 1)


def topk_ce(z, y, k, ignore_index=255, weight=None, coef=1.0, dtype=np.float64):
    """The whole statement in `dtype`: float32 is what the device evaluates (the select's record on the float32 l), float64 the
    value the bounds are held to (T, tie_w and S from a float64 sort of l)."""
    l, valid = voxel_loss(z, y, ignore_index, weight, dtype)
    n_valid = int(valid.sum())
    K = k_of(n_valid, k)
    if dtype == np.float32:
        rec = select(l, K)
    elif K == 0:
        rec = np.zeros(8, np.float64)
    else:
        T = np.sort(l)[l.size - K]
        n_gt, n_eq = int((l > T).sum()), int((l == T).sum())
        S_gt = float(l[l > T].sum())
        r = float(K - n_gt)
        rec = np.array([T, K, n_gt, n_eq, S_gt, r, r / n_eq, S_gt + r * T], np.float64)
    loss = rec[7] / K if K else 0.0
    u = membership(l, rec[0], rec[6], valid) if K else np.zeros(l.size)
    return {"l": l, "valid": valid, "n_valid": n_valid, "K": K, "record": rec, "loss": float(loss), "u": u,
            "grad": grad_from(z, y, u, K, coef, ignore_index, weight)}

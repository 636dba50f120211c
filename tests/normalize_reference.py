"""The statement of foreground statistics, percentile clipping, z-scoring and the non-zero bounding box (msk_fg_stats /
msk_clip_zscore / msk_nonzero_bbox, medicalseg_amd/csrc/msk_normalize.hip; preprocess.fg_stats_device, clip_zscore_device,
nonzero_bbox_device and their host paths) in numpy.  Written apart from the product code; nothing here imports it.

Valid voxels.  x is a flat buffer of n finite float32, n in [1, 2^31).  mask_mode 0: every voxel; 1: x != 0 (so -0.0 is outside:
nnU-Net's non-zero mask WITHOUT its hole filling); 2: mask > 0, mask an int32 buffer of n words.

Order.  Values are ordered by the sortable key of their bit pattern (topk_reference.sort_key: -0.0 < +0.0); s is the valid
values in ascending key order, widened to float64.  min = s[0] and max = s[-1], so their sign bits are defined too.

Moments.  n_valid, min, max exact.  sum and sumsq are float64 sums in the FIXED order of msk_intensity_stats over the full
raster, an invalid voxel adding +0.0 (intensity_reference.ordered_sum; sumsq adds the exact (double)x * (double)x).
mean = sum / n_valid, var = max(sumsq / n_valid - mean * mean, 0), std = sqrt(var), each a separately rounded float64 operation.

Percentiles.  q_lo <= q_hi in [0, 100]; numpy's default ("linear") method, restated:
    h = (n_valid - 1) * (q / 100.0);  i = floor(h);  g = h - i;  a = s[i];  b = s[min(i + 1, n_valid - 1)];  d = b - a
    p = b - d * (1 - g) if g >= 0.5 else a + d * g
every operation rounded on its own (no fused multiply-add).

Record.  16 float64 {n_valid, min, max, sum, sumsq, mean, std, p_lo, p_hi, a_lo, b_lo, g_lo, a_hi, b_hi, g_hi, 0}; all zeros
when n_valid == 0.

Apply.  The four values lo = float32(p_lo), hi = float32(p_hi), m = float32(mean), inv = float32(1.0 / max(std, 1e-8)) (the
reciprocal in float64) come from a record or from four host doubles {lo, hi, mean, std}.  In float32, each operation rounded on
its own:  c = lo if x < lo else x;  c = hi if c > hi else c  (min(max(x, lo), hi) with the sign of a zero that ties with a bound
settled: x is kept);  y = (c - m) * inv.  The flags switch the clip and the z-score on and off independently (clip only: y = c).
With mask_out an invalid voxel becomes the float `outside`; otherwise it is transformed like every other voxel.

Bounding box.  A [D, H, W] volume, float32 (x != 0; a NaN counts as non-zero) or int32 (v != 0): 8 int32
{d0, h0, w0, d1, h1, w1, count, 0}, the upper corner exclusive, all zeros for an empty volume."""
import numpy as np

import intensity_reference as I
import topk_reference as T

ALL, NONZERO, MASK = 0, 1, 2
CLIP, ZSCORE, MASK_OUT = 1, 2, 4
FIELDS = ("n_valid", "min", "max", "sum", "sumsq", "mean", "std", "p_lo", "p_hi", "a_lo", "b_lo", "g_lo", "a_hi", "b_hi", "g_hi",
          "zero")


def valid(x, mask_mode, mask=None):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if mask_mode == ALL:
        return np.ones(x.size, bool)
    if mask_mode == NONZERO:
        return x != 0
    assert mask_mode == MASK and mask is not None
    return np.ascontiguousarray(mask, np.int32).reshape(-1) > 0


def percentile(s, q):
    """(p, a, b, g) of the ascending float64 array s (at least one element)"""
    nv = s.size
    h = np.float64(nv - 1) * (np.float64(q) / np.float64(100.0))
    i = np.floor(h)
    g = h - i
    i = int(i)
    a = np.float64(s[i])
    b = np.float64(s[min(i + 1, nv - 1)])
    d = b - a
    if g >= 0.5:
        t = d * (np.float64(1.0) - g)
        p = b - t
    else:
        t = d * g
        p = a + t
    return p, a, b, g


def fg_stats(x, mask_mode=ALL, mask=None, q_lo=0.5, q_hi=99.5):
    """the record as 16 float64"""
    return fg_stats_pairs(x, mask_mode, mask, [(q_lo, q_hi)])[0]


def fg_stats_pairs(x, mask_mode, mask, pairs):
    """the records of several percentile pairs over the same voxels (one sort, one pair of sums)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    v = valid(x, mask_mode, mask)
    nv = int(v.sum())
    if nv == 0:
        return [np.zeros(16, np.float64) for _ in pairs]
    s = T.unsort_key(np.sort(T.sort_key(x[v]))).astype(np.float64)
    base = _moments(x, v, nv, s)
    out = []
    for q_lo, q_hi in pairs:
        assert 0.0 <= q_lo <= q_hi <= 100.0
        rec = base.copy()
        p_lo, a_lo, b_lo, g_lo = percentile(s, q_lo)
        p_hi, a_hi, b_hi, g_hi = percentile(s, q_hi)
        rec[7:15] = [p_lo, p_hi, a_lo, b_lo, g_lo, a_hi, b_hi, g_hi]
        out.append(rec)
    return out


def _moments(x, v, nv, s):
    rec = np.zeros(16, np.float64)
    d = np.where(v, x.astype(np.float64), 0.0)
    n64 = np.float64(nv)
    ssum = np.float64(I.ordered_sum(d))
    ssq = np.float64(I.ordered_sum(d * d))
    mean = ssum / n64
    e2 = ssq / n64
    mm = mean * mean
    var = e2 - mm
    var = var if var > 0.0 else np.float64(0.0)
    rec[:7] = [n64, s[0], s[-1], ssum, ssq, mean, np.sqrt(var)]
    return rec


def params_of_record(rec):
    """{lo, hi, mean, std} of a record, the four doubles the apply pass takes"""
    return np.array([rec[7], rec[8], rec[5], rec[6]], np.float64)


def apply_values(params):
    """(lo, hi, m, inv) as float32 from the four doubles"""
    p = np.asarray(params, np.float64)
    inv = np.float64(1.0) / max(p[3], np.float64(1e-8))
    return np.float32(p[0]), np.float32(p[1]), np.float32(p[2]), np.float32(inv)


def clip_zscore(x, params, flags=CLIP | ZSCORE, mask_mode=ALL, mask=None, outside=0.0):
    x = np.ascontiguousarray(x, np.float32)
    lo, hi, m, inv = apply_values(params)
    y = x.copy()
    if flags & CLIP:
        y = np.where(y < lo, lo, y)
        y = np.where(y > hi, hi, y)
    if flags & ZSCORE:
        y = ((y - m).astype(np.float32) * inv).astype(np.float32)
    if flags & MASK_OUT:
        v = valid(x, mask_mode, mask).reshape(x.shape)
        y = np.where(v, y, np.float32(outside))
    return y.astype(np.float32)


def nonzero_bbox(vol):
    vol = np.asarray(vol)
    assert vol.ndim == 3
    nz = np.nonzero(vol != 0)
    box = np.zeros(8, np.int32)
    if nz[0].size:
        box[:3] = [int(c.min()) for c in nz]
        box[3:6] = [int(c.max()) + 1 for c in nz]
        box[6] = nz[0].size
    return box

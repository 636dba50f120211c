"""The numpy statement of sliding-window inference (core/infer.py SlidingPlan / sliding_window_inference, csrc/msk_sliding.hip)
and the inputs of its tests.  The plan is restated here from the rules, independently of SlidingPlan.

Per axis (size = volume extent, r = window extent):
    P        = max(size, r); before = (r - size) // 2 voxels of implicit padding in front when size < r
    starts   = [0] if P == r, else interval = max(1, int(r * (1 - overlap))), num = ceil((P - r) / interval) + 1,
               start_i = min(i * interval, P - r)                                   (padded coordinates)
    g[k]     = 1 ('constant') or exp(-0.5 * ((k - (r - 1) / 2) / (sigma_scale * r)) ** 2) ('gaussian'), float64
    S[p]     = sum of g[p - start_i] over the windows that contain p, float64, in window order
    T[i][k]  = float32(g[k] / S[start_i + k])
Windows: batch item slowest, then the d, h, w starts, w fastest; origin in volume coordinates = start - before.
Blend, float32, one rounding per operation, windows in order, padding skipped:
    w   = (Td[id][z] * Th[ih][y]) * Tw[iw][x]
    acc = acc + (w * logit)
All arrays are NCDHW."""
import math

import numpy as np

import tta_reference as T

LITERAL_STARTS = [  # (size, r, overlap) -> starts, the checked values of the specification
    ((5, 4, .5), [0, 1]), ((7, 4, .5), [0, 2, 3]), ((9, 4, .5), [0, 2, 4, 5]), ((300, 260, .25), [0, 40]), ((8, 4, 0), [0, 4]),
    ((2, 4, .5), [0])]


def axis_plan(size, r, overlap=0.5, mode='gaussian', sigma_scale=0.125):
    """-> (P, before, starts, table): table is float32 [len(starts), r]"""
    P = max(size, r)
    before = (r - size) // 2 if size < r else 0
    if P == r:
        starts = [0]
    else:
        interval = max(1, int(r * (1 - overlap)))
        num = int(math.ceil((P - r) / interval)) + 1
        starts = [min(i * interval, P - r) for i in range(num)]
    if mode == 'constant':
        g = [1.0] * r
    else:
        g = [math.exp(-0.5 * ((k - (r - 1) / 2) / (sigma_scale * r)) ** 2) for k in range(r)]
    S = [0.0] * P
    for s in starts:
        for k in range(r):
            S[s + k] += g[k]
    table = np.array([[np.float32(g[k] / S[s + k]) for k in range(r)] for s in starts], np.float32)
    return P, before, starts, table


class Plan:
    def __init__(self, shape, roi, overlap=0.5, mode='gaussian', sigma_scale=0.125):
        self.shape, self.roi = tuple(shape), tuple(roi)
        axes = [axis_plan(s, r, overlap, mode, sigma_scale) for s, r in zip(shape, roi)]
        self.padded = tuple(a[0] for a in axes)
        self.before = tuple(a[1] for a in axes)
        self.starts = [a[2] for a in axes]
        self.tables = [a[3] for a in axes]

    def windows(self, n=1):
        out = []
        for b in range(n):
            for i in range(len(self.starts[0])):
                for j in range(len(self.starts[1])):
                    for k in range(len(self.starts[2])):
                        out.append((b, i, j, k))
        return out

    def origin(self, window):
        b, i, j, k = window
        return (b, self.starts[0][i] - self.before[0], self.starts[1][j] - self.before[1], self.starts[2][k] - self.before[2])


def _overlap(o, r, size):
    """the window-local range [lo, hi) of an axis that lies inside the volume"""
    return max(0, -o), min(r, size - o)


def crop(vol, plan, window, cval=0.0):
    """crop-with-padding of one window of an NCDHW volume -> [C, rd, rh, rw]"""
    vol = np.asarray(vol, np.float32)
    b, d0, h0, w0 = plan.origin(window)
    out = np.full((vol.shape[1],) + plan.roi, np.float32(cval), np.float32)
    (z0, z1), (y0, y1), (x0, x1) = (_overlap(o, r, s) for o, r, s in zip((d0, h0, w0), plan.roi, plan.shape))
    out[:, z0:z1, y0:y1, x0:x1] = vol[b, :, d0 + z0:d0 + z1, h0 + y0:h0 + y1, w0 + x0:w0 + x1]
    return out


def crops(vol, plan, cval=0.0):
    """every window of the volume batch, in window order"""
    return [crop(vol, plan, wd, cval) for wd in plan.windows(np.asarray(vol).shape[0])]


def blend(window_logits, plan, n=1, acc=None):
    """window_logits[i]: [C, rd, rh, rw] logits of window i (window order) -> acc [n, C, D, H, W], the float32 blend.
    `acc`: start from this array instead of zeros (it is not modified)."""
    windows = plan.windows(n)
    assert len(window_logits) == len(windows)
    c = np.asarray(window_logits[0]).shape[0]
    acc = np.zeros((n, c) + plan.shape, np.float32) if acc is None else np.array(acc, np.float32)
    td, th, tw = plan.tables
    for lg, wd in zip(window_logits, windows):
        lg = np.asarray(lg, np.float32)
        b, d0, h0, w0 = plan.origin(wd)
        wzy = (td[wd[1]][:, None] * th[wd[2]][None, :]).astype(np.float32)
        w = (wzy[:, :, None] * tw[wd[3]][None, None, :]).astype(np.float32)
        (z0, z1), (y0, y1), (x0, x1) = (_overlap(o, r, s) for o, r, s in zip((d0, h0, w0), plan.roi, plan.shape))
        part = (w[None, z0:z1, y0:y1, x0:x1] * lg[:, z0:z1, y0:y1, x0:x1]).astype(np.float32)
        view = acc[b, :, d0 + z0:d0 + z1, h0 + y0:h0 + y1, w0 + x0:w0 + x1]
        view[...] = (view + part).astype(np.float32)
    return acc


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def volume(n, shape, c, seed):
    return np.random.default_rng(seed).standard_normal((n, c) + tuple(shape)).astype(np.float32)


def integer_volume(n, shape, seed):
    """one channel of integers in [-8, 8]"""
    return np.random.default_rng(seed).integers(-8, 9, (n, 1) + tuple(shape)).astype(np.float32)


def window_logits(plan, n, c, seed):
    """random logits per window in the style of tta_reference.logits_case (a tied block, a +-80 block)"""
    rd, rh, rw = plan.roi
    return [T.logits_case((1, rd, rh, rw, c), seed + i)[0] for i in range(len(plan.windows(n)))]


ramp_model = T.ramp_model
pointwise_model = T.pointwise_model


def model_on_windows(f, vol, plan, cval=0.0):
    """f applied to every window on its own -> list of [C, rd, rh, rw]"""
    return [f(p[None])[0] for p in crops(vol, plan, cval)]

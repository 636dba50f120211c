"""The specification of gradient clipping and Nesterov momentum, in plain numpy: what medicalseg_amd/csrc/msk_clip.hip
(msk_grad_clip_coef, msk_sgd_momentum_clip, msk_adam_clip) must equal.  Written apart from the product code; nothing here
imports it.

g is the flat float32 gradient arena of n elements.

  sumsq(g)  S = ordered_sum(float64(g) ** 2), the summation scheme of tests/intensity_reference.py: chunks of 4096 elements,
            lane l of 256 adds its 16 terms in ascending order, then the tree v[l] += v[l+s], s = 128 .. 1; the chunk values
            are reduced by the same scheme; elements past n add +0.0.  float64(g) ** 2 is exact.
  record    gs = float64(float32(grad_scale)), c = float64(float32(clip_norm)), c > 0 (NaN or <= 0: an argument error);
            norm = gs * sqrt(S);  coef = float32(c / (norm if norm > c else c)), and c = +inf gives coef = 1 (measure only);
            the record is the 4 doubles {S, norm, float64(coef), 0.0}
  update    Paddle's order: clip, then L2 decay, then momentum.
            gs_eff = float32(float32(gs) * coef)  (a float32 product);  g' = g * gs_eff;
            with a value clip g' = min(max(g', lo), hi);
            t = g' + wd * p;  v = mu * v + t;
            p -= lr * v,  or with Nesterov  p -= lr * (t + mu * v)   (param - (grad + velocity_out * mu) * lr)
  adam      the same g', then g'' = g' + wd * p;  m = b1 m + (1 - b1) g'';  v = b2 v + (1 - b2) g''^2;
            p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps sqrt(1 - b2^t))

The sum, the norm and the coefficient are exact statements (the device equals S bit for bit; sqrt, the product and the
division are single IEEE operations).  The updates are stated in float64 on the float32 constants the kernels hold.
"""
import numpy as np

from intensity_reference import CHUNK, chunk_sums, ordered_sum, reduce_chunks  # noqa: F401  (the summation scheme is that file's)

BLOCK = 64 * CHUNK      # sumsq works through the arena in runs of whole chunks, so that its temporaries stay in the cache


def sumsq(g):
    """ordered_sum(float64(g) ** 2): a chunk value depends on its own 4096 elements only, so the chunk values of consecutive
    blocks of whole chunks, concatenated, are the chunk values of the whole array"""
    g = np.asarray(g, np.float32).reshape(-1)
    parts = [chunk_sums(g[i:i + BLOCK].astype(np.float64) ** 2) for i in range(0, g.size, BLOCK)]
    return reduce_chunks(np.concatenate(parts))


def coef_of(norm, clip_norm):
    """float32 coefficient of a float64 norm"""
    c = np.float64(np.float32(clip_norm))
    if not c > 0:
        raise ValueError("clip_norm must be > 0")
    if not norm > c:                # c = +inf: c / c would be NaN; a finite c gives c / c == 1 exactly
        return np.float32(1.0)
    return np.float32(c / norm)


def record(g, grad_scale, clip_norm):
    """{S, norm, coef, 0} as a float64 array of 4"""
    S = sumsq(g)
    norm = np.float64(np.float32(grad_scale)) * np.sqrt(np.float64(S))
    return np.array([S, norm, np.float64(coef_of(norm, clip_norm)), 0.0], np.float64)


def clipped(g, grad_scale, coef=1.0, lo=None, hi=None):
    """g' in float64"""
    gs_eff = np.float32(np.float32(grad_scale) * np.float32(coef))
    out = np.asarray(g, np.float32).astype(np.float64) * np.float64(gs_eff)
    if lo is not None or hi is not None:
        lo = -np.inf if lo is None else np.float64(np.float32(lo))
        hi = np.inf if hi is None else np.float64(np.float32(hi))
        out = np.minimum(np.maximum(out, lo), hi)
    return out


def sgd_step(p, g, v, lr, mu, wd, grad_scale=1.0, nesterov=False, coef=1.0, lo=None, hi=None):
    """(p, v) after one step, float64; lr, mu, wd enter as the float32 values the kernel holds"""
    lr, mu, wd = (np.float64(np.float32(s)) for s in (lr, mu, wd))
    p, v = np.asarray(p, np.float64), np.asarray(v, np.float64)
    t = clipped(g, grad_scale, coef, lo, hi) + wd * p
    v = mu * v + t
    p = p - lr * (t + mu * v) if nesterov else p - lr * v
    return p, v


def adam_step(p, g, m1, m2, t, lr, b1, b2, eps, wd, grad_scale=1.0, coef=1.0, lo=None, hi=None):
    """(p, m1, m2) after step t (1-based), float64"""
    lr, b1, b2, eps, wd = (np.float64(np.float32(s)) for s in (lr, b1, b2, eps, wd))
    p, m1, m2 = (np.asarray(a, np.float64) for a in (p, m1, m2))
    gg = clipped(g, grad_scale, coef, lo, hi) + wd * p
    m1 = b1 * m1 + (1 - b1) * gg
    m2 = b2 * m2 + (1 - b2) * gg * gg
    c2 = np.sqrt(1 - b2 ** t)
    p = p - lr * c2 / (1 - b1 ** t) * m1 / (np.sqrt(m2) + eps * c2)
    return p, m1, m2

"""Float64 statement of the per-voxel operations of msk_elementwise.hip (numpy only, nothing imported from the product).

Tensors are channels-last matrices [voxels, C]; per-channel vectors broadcast along the last axis.  Every function upcasts
its inputs to float64 and returns float64 (argmax: int64); nothing here knows about launch geometry, vector widths or
kernel forms -- that is the point: every form of an operation has to agree with the one statement below.

    u      = scale * x + shift                       (scale None: u = x)
    a      = prelu(u, alpha_in)                      (alpha_in None: a = u;  the unit's own PReLU of the join forms)
    s      = a + tile(res)                           (res None: s = a;  res with fewer channels is tiled: channel c reads c % cres)
    out    = prelu(s, alpha)                         (alpha None: out = s)
    prelu(t, al) = t if t > 0 else al * t            (the kernels test !(t > 0): zero takes the negative branch)
"""
import numpy as np


def f8(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def tile_res(res, C):
    """[V, cres] -> [V, C] with channel c reading c % cres (None -> 0.0)"""
    if res is None:
        return 0.0
    res = f8(res)
    return res[:, np.arange(C) % res.shape[1]]


def prelu(t, alpha):
    return t if alpha is None else np.where(t > 0, t, f8(alpha) * t)


def bn_stats(x):
    """(mean[C], M2[C]): what msk_bn_stats leaves in stats[2C] (M2 = sum of squared deviations, not the variance)"""
    x = f8(x)
    mean = x.mean(axis=0)
    return mean, ((x - mean) ** 2).sum(axis=0)


def pre_activation(x, scale, shift, res=None, alpha_in=None):
    """s of the module docstring"""
    x = f8(x)
    u = x if scale is None else x * f8(scale) + f8(shift)
    return prelu(u, alpha_in) + tile_res(res, x.shape[1])


def affine_act_fwd(x, scale, shift, res, alpha, alpha_in=None):
    return prelu(pre_activation(x, scale, shift, res, alpha_in), alpha)


def affine_act_bwd(x, scale, shift, res, alpha, mean, invstd, dout, bn_mode, M=None, sums=None):
    """Backward of out = prelu(scale * x + shift + tile(res), alpha).  Returns a dict:
         du     dout * prelu'(s)                 (= dres, the gradient of the residual at full channel count)
         xhat   (x - mean) * invstd              (mean None: zeros)
         sums   [3, C]: sum du, sum du * xhat, sum dout * s over s <= 0 (the PReLU slope's gradient; zero without alpha)
         dx     bn_mode 1: scale * (du - S0 / M - xhat * S1 / M) with (S0, S1) = `sums` given, else the exact sums above
                bn_mode 2: scale * du;  bn_mode 0: du"""
    x, dout = f8(x), f8(dout)
    s = pre_activation(x, scale, shift, res)
    neg = ~(s > 0)
    du = dout if alpha is None else np.where(neg, f8(alpha) * dout, dout)
    xhat = np.zeros_like(x) if mean is None else (x - f8(mean)) * f8(invstd)
    S = np.stack([du.sum(axis=0), (du * xhat).sum(axis=0),
                  (dout * s * neg).sum(axis=0) if alpha is not None else np.zeros(x.shape[1])])
    if bn_mode == 1:
        S0, S1 = (S[0], S[1]) if sums is None else (f8(sums)[0], f8(sums)[1])
        M = x.shape[0] if M is None else M
        dx = f8(scale) * (du - S0 / M - xhat * S1 / M)
    elif bn_mode == 2:
        dx = f8(scale) * du
    else:
        dx = du
    return {"du": du, "xhat": xhat, "sums": S, "dx": dx}


def add_act_join_bwd(y, scale, shift, alpha_in, res, alpha, dout, mean=None, invstd=None):
    """Backward of out = prelu(a + res, alpha), a = prelu(scale * y + shift, alpha_in) (scale / alpha_in None: a = y).
       da = dres = dout * prelu'(a + res);  dalpha = sum dout * (a + res) over (a + res) <= 0;
       unit (mean given): du = da * prelu'(u), xhat = (y - mean) * invstd,
                          unit_sums [3, C] = sum du, sum du * xhat, sum da * u over u <= 0"""
    y, dout = f8(y), f8(dout)
    u = y if scale is None else y * f8(scale) + f8(shift)
    a = prelu(u, alpha_in)
    s = a + f8(res)
    neg = ~(s > 0)
    da = np.where(neg, f8(alpha) * dout, dout)
    r = {"da": da, "dalpha": (dout * s * neg).sum(axis=0)}
    if mean is not None:
        uneg = ~(u > 0)
        du = np.where(uneg, f8(alpha_in) * da, da)
        xhat = (y - f8(mean)) * f8(invstd)
        r.update(du=du, xhat=xhat, unit_sums=np.stack([du.sum(axis=0), (du * xhat).sum(axis=0), (da * u * uneg).sum(axis=0)]))
    return r


def copy_scale(src, mask, dst_old, vox_per_n, accumulate):
    """dst = src * mask[n, c] (+ dst_old); mask [N, C] or None, sample n = voxel // vox_per_n"""
    s = f8(src)
    if mask is not None:
        s = s * f8(mask)[np.arange(s.shape[0]) // vox_per_n]
    return s + f8(dst_old) if accumulate else s


def channel_sum(x):
    return f8(x).sum(axis=0)


def elu_fwd(x, alpha):
    x = f8(x)
    return np.where(x > 0, x, alpha * np.expm1(np.minimum(x, 0.0)))


def elu_bwd(out, dout, alpha):
    out = f8(out)
    return f8(dout) * np.where(out > 0, 1.0, out + alpha)


def softmax_c(x):
    x = f8(x)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def argmax_c(x):
    return np.asarray(x).argmax(axis=1)      # the first maximum wins, in numpy as in the kernel


def bn_bwd_dy(du, xhat, scale, sums, M):
    """dy of the fused BatchNorm backward (msk_wbf.h WbfBnBwd) and the bound the kernels scale it by:
         dy    = scale * (du - S0 / M - xhat * S1 / M)
         bound = max|scale| * (max|du| + max|S0 / M| + max|xhat| * max|S1 / M|)  >= max|dy|"""
    du, xhat, scale, sums = f8(du), f8(xhat), f8(scale), f8(sums)
    dy = scale * (du - sums[0] / M - xhat * sums[1] / M)
    bound = np.abs(scale).max() * (np.abs(du).max() + np.abs(sums[0] / M).max() + np.abs(xhat).max() * np.abs(sums[1] / M).max())
    return dy, bound

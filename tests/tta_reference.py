"""The numpy statement of test-time augmentation (core/infer.py aug_inference, csrc/msk_tta.hip) and the inputs of its tests.

For passes k = 0 .. K-1 with logits L_k (already resized back where the scale is not 1) and masks m_k:
    P_k   = unflip_{m_k}(softmax_c(L_k))          softmax_c: msk_softmax_c's output, the primitive
    acc   = (((P_0 + P_1) + P_2) + ...)           float32, in pass order
    probs = acc * float32(1 / K)                  np.float32(1) / np.float32(K): the correctly rounded reciprocal
    pred  = argmax_c(acc)                         first maximum wins
All arrays are NCDHW; bit a of a mask mirrors axis a of (D, H, W)."""
import numpy as np

SHAPES = [(2, 3, 5, 7, 3), (1, 1, 1, 9, 1), (1, 4, 6, 130, 20)]     # (n, d, h, w, c) of the issue: odd extents, extent 1, long W
# ... and the shapes at which the tile kernels take another path: several whole rows per workgroup with a partial last
# group, a row cut into chunks (W > 256 voxels), a C that is no multiple of 4 on quad-aligned rows
MORE_SHAPES = [(4, 5, 7, 8, 3), (2, 5, 9, 12, 20), (1, 2, 3, 260, 3), (1, 2, 2, 300, 20), (1, 3, 2, 6, 2)]


def flip(a, mask):
    """mirror an NCDHW array along the axes of mask (bit 0 = D, bit 1 = H, bit 2 = W); an involution"""
    axes = tuple(2 + b for b in range(3) if mask >> b & 1)
    return np.ascontiguousarray(np.flip(a, axes)) if axes else np.ascontiguousarray(a)


def softmax_host(x):
    """a float32 softmax over axis 1 for the host tests (the GPU tests take msk_softmax_c's output instead)"""
    x = np.asarray(x, np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True), dtype=np.float32)
    return (e * (np.float32(1) / e.sum(axis=1, keepdims=True, dtype=np.float32))).astype(np.float32)


def tta_reference(softmaxes, masks):
    """-> (acc, probs, pred) of the statement above; softmaxes[k] = softmax_c(L_k) in the frame of pass k"""
    assert len(softmaxes) == len(masks) >= 1
    acc = None
    for p, m in zip(softmaxes, masks):
        p = flip(np.asarray(p, np.float32), m)
        acc = p.copy() if acc is None else (acc + p).astype(np.float32)
    probs = (acc * (np.float32(1) / np.float32(len(masks)))).astype(np.float32)
    return acc, probs, np.argmax(acc, axis=1).astype(np.int32)


def logits_case(shape, seed):
    """NCDHW logits ~ N(0, 4^2) for an (n, d, h, w, c) shape, with a block of equal logits (ties: the first class must win)
    and a block of +-80 (softmax saturates to exact 1 and 0)"""
    n, d, h, w, c = shape
    rng = np.random.default_rng(seed)
    x = (4.0 * rng.standard_normal((n, c, d, h, w))).astype(np.float32)
    x[:, :, 0, :, : max(1, w // 3)] = np.float32(1.5)
    x[:, :, -1, -1, w // 2:] = np.float32(-80.0)
    x[:, c // 2, -1, -1, w // 2:] = np.float32(80.0)
    return x


def ramp_model(x):
    """host stand-in for a network: 3 channels of x times a fixed position-dependent ramp -- not flip-equivariant, exact"""
    x = np.asarray(x, np.float32)
    d, h, w = x.shape[2:]
    ramp = (np.arange(d, dtype=np.float32)[:, None, None] * np.float32(0.25) + np.arange(h, dtype=np.float32)[None, :, None] *
            np.float32(0.125) + np.arange(w, dtype=np.float32)[None, None, :] * np.float32(0.5) - np.float32(2.0))
    return np.concatenate([x * ramp, x * (np.float32(1.0) - ramp), x * np.float32(0.5) + ramp], axis=1).astype(np.float32)


def pointwise_model(x):
    """flip-equivariant stand-in: a pointwise map to 3 channels"""
    x = np.asarray(x, np.float32)
    return np.concatenate([x, x * np.float32(-0.5), x * x], axis=1).astype(np.float32)

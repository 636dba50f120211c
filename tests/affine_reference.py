"""The specification of the rotated and scaled patch crop, in plain numpy: what medicalseg_amd/csrc/msk_affine.hip
(msk_affine_patch) and the host path of transforms.RandomAffinePatchCrop3D must equal bit for bit.  Written apart from the
product code; nothing here imports it.

image x [D,H,W] float32 (finite), optional label [D,H,W] int32, patch extent roi = (rd, rh, rw), patch origin (d0, h0, w0) (the
first three words of a patch record of tests/patch_reference.py; negative on an axis shorter than the patch), a 3x3 float32
matrix M, pad (float32) and label_pad (int32).

For the output voxel (z, y, x), with the integer offsets o = (z - rd//2, y - rh//2, x - rw//2) and per SOURCE axis a (0 = D,
1 = H, 2 = W):

    p_a = ((M[a,0]*o_z + M[a,1]*o_y) + M[a,2]*o_x) + float32(origin_a + roi_a//2)

every multiply and every add rounded to float32 on its own (no FMA).

  image   f_a = floor(p_a), t_a = p_a - f_a (exact).  The eight corners are f + {0,1}^3; a corner outside the volume has the
          value pad (scipy's mode='grid-constant').  lerp(a, b, t) = a + t*(b - a): a float32 subtract, multiply and add, each
          rounded.  Along W first, then H, then D:
              c_ij = lerp(corner(i,j,0), corner(i,j,1), t_w)
              out  = lerp(lerp(c_00, c_01, t_h), lerp(c_10, c_11, t_h), t_d)
  label   the index floor(p_a + 0.5f) per axis (a float32 add); the label there, or label_pad outside the volume.

The matrix is M = Rd(a_d) . Rh(a_h) . Rw(a_w) . diag(s_d, s_h, s_w), computed in float64 and rounded to float32 once, with the
right-handed rotations about the D, H and W axes (c = cos a, s = sin a; a in degrees through math.radians):

         | 1  0  0 |          |  c  0  s |          | c -s  0 |
    Rd = | 0  c -s |     Rh = |  0  1  0 |     Rw = | s  c  0 |
         | 0  s  c |          | -s  0  c |          | 0  0  1 |

M maps an offset inside the patch (columns: patch D, H, W) to an offset inside the volume (rows: source D, H, W).  At 90 degrees
Rd takes the unit offset e_h to e_w and e_w to -e_h; Rh takes e_w to e_d and e_d to -e_w; Rw takes e_d to e_h and e_h to -e_d.
A scale above 1 reads a larger region of the volume, so the content shrinks (nnU-Net's convention).

`dtype=np.float64` evaluates the same formulas, from the same float32 matrix, in float64: the yardstick for scipy and for the
float32 rounding.
"""
import math

import numpy as np


def matrix(angles_deg, scales):
    """M = Rd . Rh . Rw . diag(scales) in float64, rounded to float32; scales: one number or three"""
    if np.isscalar(scales):
        scales = (scales, scales, scales)
    a = [math.radians(float(v)) for v in angles_deg]
    c = [math.cos(v) for v in a]
    s = [math.sin(v) for v in a]
    rd = np.array([[1.0, 0.0, 0.0], [0.0, c[0], -s[0]], [0.0, s[0], c[0]]], np.float64)
    rh = np.array([[c[1], 0.0, s[1]], [0.0, 1.0, 0.0], [-s[1], 0.0, c[1]]], np.float64)
    rw = np.array([[c[2], -s[2], 0.0], [s[2], c[2], 0.0], [0.0, 0.0, 1.0]], np.float64)
    m = rd @ rh @ rw @ np.diag(np.array([float(v) for v in scales], np.float64))
    return m.astype(np.float32)


def coords(roi, origin, m, dtype=np.float32):
    """p [3, rd, rh, rw] in `dtype`: the source coordinates of every patch voxel"""
    m = np.asarray(m, np.float32).astype(dtype)
    o = [(np.arange(r) - r // 2).astype(dtype) for r in roi]
    oz, oy, ox = o[0][:, None, None], o[1][None, :, None], o[2][None, None, :]
    out = np.empty((3,) + tuple(roi), dtype)
    for a in range(3):
        centre = dtype(int(origin[a]) + int(roi[a]) // 2)
        out[a] = ((m[a, 0] * oz + m[a, 1] * oy) + m[a, 2] * ox) + centre
    return out


def _gather(vol, idx, outside):
    """vol at the integer index arrays idx (z, y, x), `outside` where an index leaves the volume"""
    ok = np.ones(idx[0].shape, bool)
    clipped = []
    for i, n in zip(idx, vol.shape):
        ok &= (i >= 0) & (i < n)
        clipped.append(np.clip(i, 0, n - 1))
    return np.where(ok, vol[tuple(clipped)], outside)


def sample_image(x, p, pad, dtype=np.float32):
    x = np.asarray(x, np.float32).astype(dtype)
    pad = dtype(np.float32(pad))
    f = np.floor(p)
    t = p - f
    i0 = f.astype(np.int64)

    def corner(dz, dy, dx):
        return _gather(x, (i0[0] + dz, i0[1] + dy, i0[2] + dx), pad).astype(dtype)

    def lerp(a, b, w):
        return a + w * (b - a)

    c = [[lerp(corner(i, j, 0), corner(i, j, 1), t[2]) for j in (0, 1)] for i in (0, 1)]
    out = lerp(lerp(c[0][0], c[0][1], t[1]), lerp(c[1][0], c[1][1], t[1]), t[0])
    assert out.dtype == dtype
    return out


def sample_label(label, p, label_pad):
    label = np.asarray(label, np.int32)
    i = np.floor(p + p.dtype.type(0.5)).astype(np.int64)
    return _gather(label, (i[0], i[1], i[2]), np.int32(label_pad)).astype(np.int32)


def affine(x, label, roi, origin, m, pad=0.0, label_pad=0, dtype=np.float32):
    """(image patch in `dtype`, label patch int32 or None)"""
    p = coords(roi, origin, m, dtype)
    return sample_image(x, p, pad, dtype), None if label is None else sample_label(label, p, label_pad)


def near_tie(p, eps=1e-3):
    """voxels whose coordinate lies within eps of a rounding tie (a fraction of 0.5) on some axis"""
    return (np.abs((p - np.floor(p)) - 0.5) < eps).any(axis=0)


# ---- test data ---------------------------------------------------------------------------------------------------------------
# (volume, roi, origin, angles in degrees, scale): a padded axis; a long row; one that reads far outside the volume
CASES = [((9, 70, 67), (12, 16, 20), (-1, 20, 11), (17, -23, 29), 1.1),
         ((20, 33, 130), (8, 8, 64), (5, 10, 40), (-30, 30, 11.5), 0.7),
         ((24, 24, 24), (16, 16, 16), (4, 4, 4), (30, 30, 30), 1.4)]
# a tiny volume; a row wider than one workgroup, in-plane rotation only; an odd rw (and rh) that ends inside a box of the tile map
GPU_CASES = CASES + [((5, 6, 7), (4, 4, 4), (0, 1, 1), (10, 20, 30), 1.0),
                     ((3, 40, 260), (2, 8, 256), (0, 16, 2), (0, 0, 25), 1.25),
                     ((6, 10, 21), (4, 5, 7), (1, 3, 8), (20, -10, 15), 0.9)]


def image_for(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def label_for(shape, seed, num_classes=3):
    return np.random.default_rng(seed).integers(0, num_classes, shape).astype(np.int32)

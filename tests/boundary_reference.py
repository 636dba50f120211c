"""The statement of the signed distance map and of the boundary loss (msk_label_sdf / msk_boundary_loss_fwd / msk_boundary_loss_bwd,
medicalseg_amd/csrc/msk_loss_boundary.hip; BoundaryLoss and DiceBoundaryLoss) in numpy: Kervadec et al., "Boundary loss for highly
unbalanced segmentation", MIDL 2019.

Signed distance map of class c in one label volume lab [D, H, W], spacing None or (sz, sy, sx).  pos = (lab == c); everything else
is outside, 255 and labels beyond the class range included.  d_out = sqrt(edt_squared(pos)) is the distance to the nearest voxel of
the class, d_in = sqrt(edt_squared(~pos)) the distance to the nearest voxel not of it (utils.metric.edt_squared is the numpy
specification of the exact transform; the square root is float64 and correctly rounded).  phi = d_out outside the class and
1 - d_in inside it -- written this way, not -(d_in - 1), so that a voxel with d_in = 1 gets +0.0 -- and 0 where the squared distance
is +inf (the class is absent or fills the volume).  The result is rounded once to float32: that float32 value IS phi, on host and
device alike.  The constant 1 is Kervadec's, whatever the spacing.  Wherever the class is present and does not fill the volume this
is his one_hot2dist (tests/test_boundary_host.py restates it with scipy and compares the bits).

Loss.  Logits z [N, C, D, H, W] (numpy's layout; the device holds [N, D, H, W, C]), labels int32 [N, D, H, W], a class set S (default
1 .. C-1).  A voxel is valid when its label is in [0, C) and is not ignore_index.  p = softmax(z); t_c(v) = p_c(v) phi_c(v) for c
in S at valid v, else 0.  L = sum t / (n_valid |S|); A = sum |t| / (n_valid |S|); L_c = sum_v t_c(v) / n_valid;
dL/dz_k(v) = p_k(v) ([k in S] phi_k(v) - sum_{c in S} t_c(v)) / (n_valid |S|) at valid voxels and exactly 0 elsewhere (classes
outside S do get a gradient).  n_valid = 0: L = 0 and a zero gradient.  With nothing ignored L is Kervadec's
(probs[:, idc] * dist_maps[:, idc]).mean()."""
import numpy as np

from medicalseg_amd.utils.metric import edt_squared


def class_list(C, classes=None):
    """S as a sorted list: 1 .. C-1 unless given"""
    S = list(range(1, C)) if classes is None else sorted({int(c) for c in classes})
    assert S and 0 <= S[0] and S[-1] < C
    return S


def class_mask(C, classes=None):
    return sum(1 << c for c in class_list(C, classes))


def signed_distance(lab, c, spacing=None):
    """phi of class c, float32 [D, H, W]"""
    lab = np.asarray(lab)
    pos = lab == c
    with np.errstate(invalid="ignore"):
        d_out = np.sqrt(edt_squared(pos, spacing))
        d_in = np.sqrt(edt_squared(~pos, spacing))
        phi = np.where(pos, 1.0 - d_in, d_out)
    phi = np.where(np.isfinite(phi), phi, 0.0)
    return phi.astype(np.float32)


def distance_maps(labels, S, spacing=None):
    """float32 [N, |S|, D, H, W]: the class-planar layout of msk_label_sdf"""
    labels = np.asarray(labels)
    return np.stack([np.stack([signed_distance(vol, c, spacing) for c in S]) for vol in labels])


def boundary_loss(z, labels, classes=None, ignore_index=255, spacing=None, coef=1.0, dtype=np.float64, phi=None):
    """The whole statement evaluated in `dtype` (float64: the value the bounds are held to; float32: what one rounding per
    operation costs).  phi: the maps, when the caller has them already."""
    z = np.asarray(z)
    labels = np.asarray(labels)
    N, C = z.shape[:2]
    S = class_list(C, classes)
    if phi is None:
        phi = distance_maps(labels, S, spacing)
    zz = np.moveaxis(z, 1, -1).reshape(-1, C).astype(dtype)
    yy = labels.reshape(-1)
    valid = (yy >= 0) & (yy < C) & (yy != ignore_index)
    n_valid = int(valid.sum())
    ph = np.zeros(zz.shape, dtype)
    ph[:, S] = np.moveaxis(np.asarray(phi), 1, -1).reshape(-1, len(S)).astype(dtype)
    e = np.exp(zz - zz.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    t = p * ph * valid[:, None]
    den = dtype(max(n_valid, 1) * len(S))
    per_class_sum = t.sum(axis=0, dtype=np.float64)
    total, total_abs = float(per_class_sum.sum()), float(np.abs(t).sum(dtype=np.float64))
    g = p * (ph - t.sum(axis=1, keepdims=True)) * (dtype(coef) / den)
    g[~valid] = 0.0
    if n_valid == 0:
        g[:] = 0.0
    return {"n_valid": n_valid, "S": S, "phi": phi,
            "loss": total / float(den) if n_valid else 0.0,
            "abs": total_abs / float(den) if n_valid else 0.0,
            "per_class": per_class_sum / max(n_valid, 1),
            "stats": np.concatenate([[n_valid, total, total_abs], per_class_sum]),
            "grad": np.moveaxis(g.reshape((N,) + tuple(z.shape[2:]) + (C,)), -1, 1)}


def example_volume(shape, seed=0):
    """A label volume [D, H, W] for the tests: background 0, a large blob of class 1 around the centre, 2 per cent scattered voxels
    of class 2, NO voxel of class 3 (an absent class) and a strip of 255 along one edge."""
    D, H, W = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    r = ((z - D / 2) / (0.35 * D)) ** 2 + ((y - H / 2) / (0.3 * H)) ** 2 + ((x - W * 0.45) / (0.3 * W)) ** 2
    lab = np.zeros(shape, np.int32)
    lab[r < 1.0] = 1
    lab[rng.random(shape) < 0.02] = 2
    lab[:, 0, :] = 255
    return lab

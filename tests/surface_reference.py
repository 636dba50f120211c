"""Restatements of the surface-distance definitions of medicalseg_amd/utils/metric.py (surface_mask, edt_squared,
surface_distances), written independently of it: scipy's binary erosion, a brute-force loop over the feature voxels,
scipy's distance / feature transform.  tests/test_surface_host.py holds the package's numpy specification to them;
tests/test_gpu_surface.py holds the device to that specification (and to scipy at the sizes it is used at)."""
import numpy as np
from scipy import ndimage

ANISO = [(3.3, 0.6875, 0.6875), (1.0, 1.0, 2.0)]
SCIPY_RTOL = 8 * 2.0 ** -52      # the handful of float64 roundings on scipy's side (sqrt, its own sums, the squaring here)


def surface(mask):
    m = np.asarray(mask, dtype=bool)
    return m & ~ndimage.binary_erosion(m)


def edt2_brute(features, spacing=None):
    """min over the feature voxels u of fl(fl(fl(wx dx^2) + fl(wy dy^2)) + fl(wz dz^2)), one numpy operation per fl"""
    f = np.asarray(features, dtype=bool)
    sz, sy, sx = (np.float64(v) for v in ((1.0, 1.0, 1.0) if spacing is None else spacing))
    wz, wy, wx = sz * sz, sy * sy, sx * sx
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in f.shape), indexing="ij")
    out = np.full(f.shape, np.inf, dtype=np.float64)
    for uz, uy, ux in np.argwhere(f):
        tx = wx * ((x - ux) ** 2).astype(np.float64)
        ty = wy * ((y - uy) ** 2).astype(np.float64)
        tz = wz * ((z - uz) ** 2).astype(np.float64)
        out = np.minimum(out, (tx + ty) + tz)
    return out


def scipy_edt2(features, spacing=None):
    """scipy's Euclidean distance to the nearest feature, squared (the features must not be empty)"""
    f = np.asarray(features, dtype=bool)
    assert f.any()
    return ndimage.distance_transform_edt(~f, sampling=spacing) ** 2


def scipy_int_edt2(features):
    """unit spacing: the exact integer squared distances, from the indices of scipy's feature transform"""
    f = np.asarray(features, dtype=bool)
    assert f.any()
    idx = ndimage.distance_transform_edt(~f, return_distances=False, return_indices=True)
    grid = np.indices(f.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(axis=0)


def metrics_scipy(pred, label, cls):
    """(hd, hd95, assd) in voxel units by the definitions, from scipy's erosion and feature transform"""
    P, L = surface(np.asarray(pred) == cls), surface(np.asarray(label) == cls)
    if not P.any() or not L.any():
        return float("nan"), float("nan"), float("nan")
    d_pl = np.sqrt(np.sort(scipy_int_edt2(L)[P].astype(np.float64)))
    d_lp = np.sqrt(np.sort(scipy_int_edt2(P)[L].astype(np.float64)))
    hd = float(max(d_pl.max(), d_lp.max()))
    hd95 = float(np.percentile(np.concatenate([d_pl, d_lp]), 95))
    assd = float((np.mean(d_pl) + np.mean(d_lp)) / 2)
    return hd, hd95, assd


def blob_mask(shape, seed, count=4, fill=0.08):
    """boolean [D, H, W]: a few ellipsoids, about `fill` of the volume"""
    rng = np.random.default_rng(seed)
    grid = np.indices(shape).astype(np.float64)
    m = np.zeros(shape, dtype=bool)
    for _ in range(count):
        c = [rng.uniform(0, s - 1) for s in shape]
        r = [max(0.6, s * (fill / count) ** (1 / 3.0) * rng.uniform(0.5, 1.1)) for s in shape]
        m |= sum(((grid[a] - c[a]) / r[a]) ** 2 for a in range(3)) <= 1.0
    return m


def blob_pair(shape, ncls, seed):
    """(pred, label) int32 [D, H, W]: ellipsoids of the classes 1 .. ncls - 1; the prediction is another draw whose
    blobs overlap the label's partly"""
    label, pred = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    for c in range(1, ncls):
        label[blob_mask(shape, seed * 100 + c, count=2)] = c
        pred[blob_mask(shape, seed * 100 + c, count=2) & ~blob_mask(shape, seed * 100 + 50 + c, count=1)] = c
        pred[blob_mask(shape, seed * 100 + 70 + c, count=1, fill=0.01)] = c
    return pred, label


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return ((z + y + x) & 1).astype(np.int32)


def noise(shape, seed, p=0.5):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.int32)

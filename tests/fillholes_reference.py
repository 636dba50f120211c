"""The statement of hole filling (msk_fill_holes3d, preprocess.fill_holes_*, transforms.FillHoles3D) in numpy and
scipy.ndimage.label, vectorised: no Python loop over components.

For one volume x [d, h, w]: a voxel is ZERO when x == 0 (float32: -0.0 is zero, a NaN is not).  The zero voxels form
6-connected components (scipy's default structure).  A component is a HOLE when none of its voxels lies on a face of the
volume.  Mask form: 1 where x != 0 or the voxel lies in a hole, else 0 == scipy.ndimage.binary_fill_holes(x != 0).  Label
form (integers): x, except that a hole whose non-zero 6-neighbours all carry one value c (and c in ``classes`` when given)
becomes c.  ``filled`` is the number of voxels changed."""
import numpy as np
import scipy.ndimage

BORDER, SINGLE, MIXED, EXCLUDED = "border", "single", "mixed", "excluded"


def _components(x):
    """-> (zero, lab, n, hole[n + 1], lo[n + 1], hi[n + 1]); entry 0 stands for the non-zero voxels and is no hole"""
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError("expected a 3-D volume")
    zero = x == 0
    lab, n = scipy.ndimage.label(zero)
    border = np.zeros(n + 1, bool)
    border[0] = True
    for ax in range(3):
        for face in (0, -1):
            border[np.take(lab, face, axis=ax).ravel()] = True
    lo = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
    hi = np.full(n + 1, np.iinfo(np.int64).min, np.int64)
    if np.issubdtype(x.dtype, np.integer):
        for ax in range(3):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[ax], b[ax] = slice(0, -1), slice(1, None)
            for p, q in ((tuple(a), tuple(b)), (tuple(b), tuple(a))):       # p: the zero voxel, q: its neighbour
                sel = zero[p] & ~zero[q]
                np.minimum.at(lo, lab[p][sel], x[q][sel].astype(np.int64))
                np.maximum.at(hi, lab[p][sel], x[q][sel].astype(np.int64))
    return zero, lab, n, ~border, lo, hi


def fill_mask(x):
    """-> (int32 mask, filled)"""
    zero, lab, _, hole, _, _ = _components(x)
    inside = hole[lab]
    return (~zero | inside).astype(np.int32), int(np.count_nonzero(inside))


def _fillable(hole, lo, hi, classes):
    ok = hole & (lo == hi)
    if classes is not None and len(classes):
        ok &= np.isin(lo, np.asarray(classes, np.int64))
    return ok


def fill_label(x, classes=None):
    """-> (int32 labels, filled)"""
    x = np.asarray(x)
    if not np.issubdtype(x.dtype, np.integer):
        raise TypeError("the label form takes integers")
    _, lab, _, hole, lo, hi = _components(x)
    ok = _fillable(hole, lo, hi, classes)
    sel = ok[lab]
    out = np.where(sel, lo[lab], x.astype(np.int64)).astype(np.int32)
    return out, int(np.count_nonzero(sel))


def kinds(x, classes=None):
    """the number of zero components of each of the four kinds"""
    _, _, n, hole, lo, hi = _components(x)
    hole, lo, hi = hole[1:], lo[1:], hi[1:]
    single = hole & (lo == hi)
    ok = _fillable(hole, lo, hi, classes)
    return {BORDER: int(np.count_nonzero(~hole)), SINGLE: int(np.count_nonzero(ok)),
            MIXED: int(np.count_nonzero(hole & ~single)), EXCLUDED: int(np.count_nonzero(single & ~ok))}


def fill_loop(x, classes=None, binary=False):
    """the same statement as a flood fill per component, for the small volumes of the host tests"""
    x = np.asarray(x)
    D, H, W = x.shape
    out = (x != 0).astype(np.int32) if binary else x.astype(np.int32).copy()
    seen = np.zeros(x.shape, bool)
    filled = 0
    for seed in zip(*np.nonzero(x == 0)):
        if seen[seed]:
            continue
        seen[seed] = True
        comp, stack, border, around = [], [seed], False, set()
        while stack:
            z, y, xx = stack.pop()
            comp.append((z, y, xx))
            border |= z in (0, D - 1) or y in (0, H - 1) or xx in (0, W - 1)
            for dz, dy, dx in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
                a, b, c = z + dz, y + dy, xx + dx
                if not (0 <= a < D and 0 <= b < H and 0 <= c < W):
                    continue
                if x[a, b, c] == 0:
                    if not seen[a, b, c]:
                        seen[a, b, c] = True
                        stack.append((a, b, c))
                elif not binary:
                    around.add(int(x[a, b, c]))
        if border:
            continue
        if binary:
            value = 1
        elif len(around) == 1 and (classes is None or not len(classes) or next(iter(around)) in set(int(c) for c in classes)):
            value = next(iter(around))
        else:
            continue
        for v in comp:
            out[v] = value
        filled += len(comp)
    return out, filled


# volumes shared by the CPU and GPU tests ----------------------------------------------------------------------------------
SHAPES = [(5, 9, 33), (4, 8, 32), (9, 17, 65), (1, 7, 40), (12, 1, 70)]
DENSITIES = [0.3, 0.5, 0.62, 0.75, 0.9]


def binary_noise(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.int32)


def label_noise(shape, C, seed, zeros=0.18):
    """smoothed-random labels 1..C with zeros sprinkled in: holes inside one label, between labels and at the border"""
    rng = np.random.default_rng(seed)
    f = scipy.ndimage.uniform_filter(rng.random(shape), size=5, mode="nearest")
    edges = np.quantile(f, np.linspace(0, 1, C + 1)[1:-1])
    lab = (np.digitize(f, edges) + 1).astype(np.int32)
    lab[rng.random(shape) < zeros] = 0
    return lab


def hollow_box(shape=(12, 20, 70), lo=(2, 3, 5), hi=(10, 17, 66), value=1):
    """a one-voxel shell [lo, hi) whose cavity crosses tile faces (4 x 8 x 32) on all three axes"""
    m = np.zeros(shape, np.int32)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value
    m[lo[0] + 1:hi[0] - 1, lo[1] + 1:hi[1] - 1, lo[2] + 1:hi[2] - 1] = 0
    return m


def box_with_corridor(value=1):
    """the hollow box inside a solid block, its cavity joined to the border by a one-voxel corridor with two bends that
    crosses tile faces: no hole"""
    m = np.full((12, 20, 70), value, np.int32)
    m[3:9, 4:16, 6:60] = 0
    m[5, 9, 60:67] = 0
    m[5, 9:19, 66] = 0
    m[5:12, 18, 66] = 0          # reaches the face z = 11
    return m


def box_with_diagonal_leak(value=1):
    """the same block and cavity; a second zero pocket touches the cavity only across an edge and itself reaches the
    border: 6-connectivity keeps the cavity a hole"""
    m = np.full((12, 20, 70), value, np.int32)
    m[3:9, 4:16, 6:60] = 0
    m[9:12, 16, 30] = 0          # (9, 16, 30) is diagonal to the cavity voxel (8, 15, 30)
    return m


def serpentine_corridor(shape=(12, 20, 70), reach_border=True, value=1):
    """a solid block whose interior holds cc_reference.serpentine as a one-voxel ZERO corridor (one component winding through
    every tile: long union chains); it ends on the face x = 0, or one voxel short of it"""
    from cc_reference import serpentine
    m = np.full(shape, value, np.int32)
    inner = m[1:-1, 1:-1, 1:-1]
    inner[serpentine(inner.shape) != 0] = 0
    if reach_border:
        m[1, 1, 0] = 0
    return m

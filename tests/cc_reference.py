"""Pure-numpy restatement of the reference's connected-component relabelling (medicalseg/transforms/functional.py:117-131,
SimpleITK ConnectedComponent(fullyConnected=False) + RelabelComponent(minimumObjectSize)), written without scipy: a
breadth-first search from seeds taken in raster order, 6-connectivity, components ranked by decreasing size with ties
to the component whose first voxel comes first.  tests/test_cc_host.py holds medicalseg_amd's host path to it; the
device path is held to the host path in tests/test_gpu_connected_components.py."""
import collections

import numpy as np

_STEPS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def label6(mask):
    """-> (labels, sizes): labels 1..n in order of each component's first voxel in raster order, sizes[i] of label i+1."""
    fg = np.asarray(mask) != 0
    lab = np.zeros(fg.shape, np.int64)
    sizes = []
    D, H, W = fg.shape
    for seed in zip(*np.nonzero(fg)):          # np.nonzero walks in raster (C) order
        if lab[seed]:
            continue
        cur = len(sizes) + 1
        lab[seed] = cur
        n = 0
        q = collections.deque([seed])
        while q:
            z, y, x = q.popleft()
            n += 1
            for dz, dy, dx in _STEPS:
                a, b, c = z + dz, y + dy, x + dx
                if 0 <= a < D and 0 <= b < H and 0 <= c < W and fg[a, b, c] and not lab[a, b, c]:
                    lab[a, b, c] = cur
                    q.append((a, b, c))
        sizes.append(n)
    return lab, np.asarray(sizes, np.int64)


def relabel(mask, minimum_volume=0, k=0):
    """ranks 1, 2, ... by decreasing size (stable in first-voxel order), size < minimum_volume -> 0 with the later ranks
    closing up, k > 0: ranks above k -> 0."""
    vals = np.unique(mask)
    assert len(vals) < 3, "Only binary mask is accepted, got mask with {}.".format(vals.tolist())
    lab, sizes = label6(mask)
    lut = np.zeros(len(sizes) + 1, np.int64)
    order = sorted(range(len(sizes)), key=lambda i: (-sizes[i], i))
    rank = 0
    for i in order:
        if sizes[i] >= minimum_volume:
            rank += 1
            if k <= 0 or rank <= k:
                lut[i + 1] = rank
    return lut[lab]


# masks shared by the CPU and GPU tests -------------------------------------------------------------------------
def box_blobs(shape, count, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.float32)
    for _ in range(count):
        lo = [int(rng.integers(0, max(1, s - 2))) for s in shape]
        ext = [int(rng.integers(1, max(2, s // 4 + 1))) for s in shape]
        m[lo[0]:lo[0] + ext[0], lo[1]:lo[1] + ext[1], lo[2]:lo[2] + ext[2]] = 1
    return m


def noise(shape, seed, p=0.5):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.float32)


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return ((z + y + x) % 2 == 0).astype(np.float32)


def serpentine(shape):
    """one voxel wide path filling the volume: rows along w on even h, joined at alternating ends on odd h; the planes
    joined the same way along d at alternating corners -- one component crossing every tile with deep merge chains"""
    D, H, W = shape
    m = np.zeros(shape, np.float32)
    for z in range(0, D, 2):
        for y in range(0, H, 2):
            m[z, y, :] = 1
            if y + 2 < H:
                m[z, y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = 1
        if z + 2 < D:
            last_y = ((H - 1) // 2) * 2
            m[z + 1, last_y if (z // 2) % 2 == 0 else 0, 0] = 1
    return m


def diagonal_contacts(shape):
    """voxels touching only along edges or corners: every one of them is its own component under 6-connectivity"""
    m = np.zeros(shape, np.float32)
    D, H, W = shape
    for i in range(min(D, H, W)):
        m[i, i, i] = 1                             # corner contacts along the main diagonal
    for i in range(min(H, W) - 1):
        m[D - 1, i, i] = 1                         # edge contacts in the last plane
    return m

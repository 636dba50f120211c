"""Case generators for the AUC counts (utils.metric.auc_counts on the host in tests/test_auc_host.py, csrc/msk_auc.hip on
the device in tests/test_gpu_auc.py) and the brute-force pair counter both are held to at small sizes.

A case is (kind, values, label): values float32 (1, C, *spatial), label int32 (1, 1, *spatial).  kind 'logits': the values
go through a softmax over the class axis first (numpy here, msk_softmax_c on the device); kind 'scores': they are the
scores themselves (non-negative, finite; rows need not sum to 1, every class is scored on its own column)."""
import numpy as np

GENERATORS = ("uniform", "saturated", "constant", "quantised", "separated_up", "separated_down", "special")


def spatial_of(voxels):
    """a 3-D shape with that many voxels"""
    for d in (8, 4, 2):
        if voxels % (d * d) == 0 and voxels >= d * d:
            return (d, d, voxels // (d * d))
    return (1, 1, voxels)


def labels(rng, voxels, C, all_present=True):
    lab = rng.integers(0, C, voxels).astype(np.int32)
    if all_present and voxels >= C:
        lab[rng.permutation(voxels)[:C]] = np.arange(C, dtype=np.int32)
    return lab


def case(name, shape, C, seed, all_present=True):
    """(kind, values (1, C, *shape) float32, label (1, 1, *shape) int32)"""
    rng = np.random.default_rng(seed)
    V = int(np.prod(shape))
    lab = labels(rng, V, C, all_present)
    kind = "scores"
    if name == "uniform":
        s = rng.random((V, C), dtype=np.float32)
    elif name == "saturated":           # softmax of N(0, 12^2) logits: many exact 0.0 and 1.0
        kind = "logits"
        s = (12.0 * rng.standard_normal((V, C))).astype(np.float32)
    elif name == "constant":
        s = np.full((V, C), 0.25, np.float32)
    elif name == "quantised":           # 8 levels
        s = (rng.integers(0, 8, (V, C)) / np.float32(8)).astype(np.float32)
    elif name in ("separated_up", "separated_down"):   # every positive above (below) every negative: AUC 1 (0)
        s = (0.25 * rng.random((V, C), dtype=np.float32)).astype(np.float32)
        hit = lab[:, None] == np.arange(C)[None, :]
        s = np.where(hit == (name == "separated_up"), s + np.float32(0.5), s).astype(np.float32)
    elif name == "special":             # signed zeros, denormals, the smallest normal, 1.0f and its neighbour
        vals = np.array([0.0, -0.0, 1e-45, 3e-45, 1.1754942e-38, 1.17549435e-38, 0.5, 0.99999994, 1.0], np.float32)
        s = vals[rng.integers(0, len(vals), (V, C))]
    else:
        raise KeyError(name)
    values = np.ascontiguousarray(np.moveaxis(s.reshape((1,) + tuple(shape) + (C,)), -1, 1))
    return kind, values, lab.reshape((1, 1) + tuple(shape))


def softmax(logits):
    """float32 softmax over axis 1 (the host stand-in for msk_softmax_c: same definition, not the same bits)"""
    x = logits.astype(np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def scores_of(kind, values):
    return softmax(values) if kind == "logits" else values


def brute_counts(scores, label):
    """[C, 3] {U2, n_pos, n_neg} by looking at every (positive, negative) pair: O(n_pos * n_neg), small inputs only"""
    C = scores.shape[1]
    s = np.moveaxis(scores, 1, -1).reshape(-1, C)
    lab = label.reshape(-1)
    out = np.zeros((C, 3), np.uint64)
    for c in range(C):
        p, n = s[lab == c, c], s[lab != c, c]
        u2 = 2 * int(np.count_nonzero(n[None, :] < p[:, None])) + int(np.count_nonzero(n[None, :] == p[:, None]))
        out[c] = (u2, p.size, n.size)
    return out

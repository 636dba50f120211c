"""Restatement of the hard-label metrics the way their definitions read (reference medicalseg/utils/metric.py:21-61,
110-210), written independently of medicalseg_amd/utils/metric.py: one boolean mask per class, python loops, no
bincount.  tests/test_metrics_host.py holds the package's host path to it; tests/test_gpu_metrics.py holds the device
to that host path."""
import numpy as np


def confusion(pred, label, num_classes, ignore_index=255):
    """[N, K*K + 1] counts, K = num_classes + 1: cell (r, c) = label class r and predicted class c among the voxels
    whose label is not ignore_index; class num_classes = any other value; last word = label == ignore_index"""
    pred, label = np.asarray(pred), np.asarray(label)
    n = pred.shape[0]
    K = num_classes + 1
    out = np.zeros((n, K * K + 1), dtype=np.uint64)
    for v in range(n):
        p, l = pred[v].ravel(), label[v].ravel()
        keep = l != ignore_index
        l_class = [l == r for r in range(num_classes)]
        p_class = [p == c for c in range(num_classes)]
        l_other, p_other = np.ones(l.shape, bool), np.ones(p.shape, bool)
        for m in l_class:
            l_other &= ~m
        for m in p_class:
            p_other &= ~m
        l_class.append(l_other)
        p_class.append(p_other)
        for r in range(K):
            for c in range(K):
                out[v, r * K + c] = np.count_nonzero(l_class[r] & p_class[c] & keep)
        out[v, K * K] = np.count_nonzero(~keep)
    return out


def areas(pred, label, num_classes, ignore_index=255):
    """calculate_area: pred_i = (pred == i) & (label != ignore), label_i = (label == i), intersect = pred_i & label_i"""
    pred, label = np.asarray(pred), np.asarray(label)
    if pred.ndim == 5:
        pred = pred[:, 0]
    if label.ndim == 5:
        label = label[:, 0]
    mask = label != ignore_index
    inter, pa, la = [], [], []
    for i in range(num_classes):
        pred_i = (pred == i) & mask
        label_i = label == i
        inter.append(int(np.count_nonzero(pred_i & label_i)))
        pa.append(int(np.count_nonzero(pred_i)))
        la.append(int(np.count_nonzero(label_i)))
    return np.array(inter, np.int64), np.array(pa, np.int64), np.array(la, np.int64)


def mean_iou(inter, pa, la):
    vals = []
    for i in range(len(inter)):
        union = int(pa[i]) + int(la[i]) - int(inter[i])
        vals.append(0.0 if union == 0 else int(inter[i]) / union)
    return np.array(vals), float(np.mean(vals))


def dice(inter, pa, la):
    vals = []
    for i in range(len(inter)):
        s = int(pa[i]) + int(la[i])
        vals.append(0.0 if s == 0 else (2 * int(inter[i])) / s)
    return np.array(vals), float(np.mean(vals))


def accuracy(inter, pa):
    vals = [0.0 if int(pa[i]) == 0 else int(inter[i]) / int(pa[i]) for i in range(len(inter))]
    return np.array(vals), sum(int(v) for v in inter) / sum(int(v) for v in pa)


def kappa(inter, pa, la):
    total = float(sum(int(v) for v in la))
    po = sum(int(v) for v in inter) / total
    pe = float(sum(int(p) * int(l) for p, l in zip(pa, la))) / (total * total)
    return (po - pe) / (1 - pe)


def random_case(shape, num_classes, seed, n=2, ignore_index=255, out_of_range=True, ignore_frac=0.1):
    """(pred, label) int32 [n, 1, *shape]: random classes, a share of ignored labels, and (out_of_range) negative and
    too-large values in both"""
    rng = np.random.default_rng(seed)
    full = (n, 1) + tuple(shape)
    pred = rng.integers(0, num_classes, full).astype(np.int32)
    label = rng.integers(0, num_classes, full).astype(np.int32)
    if out_of_range:
        for a in (pred, label):
            u = rng.random(full)
            a[u < 0.05] = -1
            a[(u >= 0.05) & (u < 0.08)] = num_classes
            a[(u >= 0.08) & (u < 0.10)] = num_classes + 7
            a[(u >= 0.10) & (u < 0.11)] = -2 ** 31
            a[(u >= 0.11) & (u < 0.12)] = 2 ** 31 - 1
        pred[rng.random(full) < 0.03] = ignore_index      # a prediction equal to ignore_index is just a value
    label[rng.random(full) < ignore_frac] = ignore_index
    return pred, label


def blobs(shape, num_classes, seed, n=1, foreground=0.05):
    """(pred, label) int32 [n, 1, *shape]: box blobs of classes 1.. on background 0, about `foreground` of the volume;
    the prediction is the label shifted by one voxel along the last axis"""
    rng = np.random.default_rng(seed)
    label = np.zeros((n, 1) + tuple(shape), np.int32)
    nblob = 12
    frac = (foreground / nblob) ** (1.0 / 3.0)
    for v in range(n):
        for b in range(nblob):
            ext = [max(1, int(round(s * frac))) for s in shape]
            lo = [int(rng.integers(0, s - e + 1)) for s, e in zip(shape, ext)]
            cls = 1 + b % max(num_classes - 1, 1) if num_classes > 1 else 0
            label[v, 0, lo[0]:lo[0] + ext[0], lo[1]:lo[1] + ext[1], lo[2]:lo[2] + ext[2]] = cls
    pred = np.roll(label, 1, axis=-1)
    return pred, label

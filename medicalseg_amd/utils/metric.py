"""Metrics of the evaluation loop: auc_roc on the host, or for device inputs from exact pair counts taken on the device
(auc_counts / AucScores / auc_from_counts below); the hard-label family (calculate_area, mean_iou, dice, accuracy,
kappa) from confusion counts taken on the device (second half of this file); the boundary metrics (Hausdorff distance,
HD95, average symmetric surface distance) from an exact squared Euclidean distance transform, on the device for device
inputs (last part of this file: surface_mask, edt_squared, surface_distances, surface_metrics).

auc_roc: area under the ROC curve of the softmax scores collected by ``core.val.evaluate(auc_roc=True)`` -- the quantity the
reference takes from ``sklearn.metrics.roc_auc_score`` (medicalseg/utils/metric.py:64-107): binary = AUC of the class-1
score, more classes = one-vs-rest, macro average.  Computed here from the rank statistic (Mann-Whitney U with average
ranks for ties = the trapezoidal area sklearn integrates), numpy only.

Difference to the reference, on purpose: its function insists on 4-D (N, C, H, W) arrays (it was written for 2-D
segmentation) and therefore raises on the 5-D logits of every 3-D model of this package; here any (N, C, *spatial) layout
is accepted and flattened the same way."""
import numpy as np


def _average_ranks(x):
    """1-based ranks of x with ties sharing their average rank (scipy.stats.rankdata(method='average'))"""
    order = np.argsort(x, kind="mergesort")
    xs = x[order]
    n = xs.size
    start = np.flatnonzero(np.concatenate(([True], xs[1:] != xs[:-1])))       # first index of every run of equal values
    end = np.concatenate((start[1:], [n]))
    avg = (start + end + 1) / 2.0                                             # mean of the 1-based ranks start+1 .. end
    ranks = np.empty(n, dtype=np.float64)
    ranks[order] = np.repeat(avg, end - start)
    return ranks


def binary_auc(score, positive):
    """P(score of a positive > score of a negative) + 0.5 P(equal)"""
    positive = np.asarray(positive, dtype=bool).ravel()
    score = np.asarray(score, dtype=np.float64).ravel()
    n_pos = int(positive.sum())
    n_neg = positive.size - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    r = _average_ranks(score)
    return float((r[positive].sum() - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * n_neg))


def auc_roc(logits, label, num_classes, ignore_index=None):
    """logits: softmax scores (N, C, *spatial); label: (N, 1, *spatial) or (N, *spatial) class indices.
    A device ``Tensor`` of scores with an ``IntTensor`` label (both on one device) is counted on the device
    (AucScores): the same float, and only the 3 * C + 2 count words are downloaded."""
    from ..device import IntTensor, Tensor
    if isinstance(logits, Tensor) or isinstance(label, IntTensor):
        if not (isinstance(logits, Tensor) and isinstance(label, IntTensor)):
            raise TypeError("logits and label must both be device arrays or both be host arrays")
        if ignore_index:
            raise RuntimeError('labels with ignore_index is not supported yet.')
        if logits.c != num_classes:
            raise ValueError("logits have {} channels, num_classes is {}".format(logits.c, num_classes))
        acc = AucScores(logits.dev, num_classes, logits.voxels)
        try:
            acc.add(logits, label)
            return auc_from_counts(acc.counts(), num_classes)
        finally:
            acc.free()
    logits = np.asarray(logits)
    label = np.asarray(label)
    if ignore_index or len(np.unique(label)) > num_classes:
        raise RuntimeError('labels with ignore_index is not supported yet.')
    if logits.ndim < 3:
        raise ValueError('The shape of logits is not (N, C, *spatial), it is {}'.format(logits.shape))
    C = logits.shape[1]
    scores = np.moveaxis(logits, 1, -1).reshape(-1, C)
    lab = label.reshape(-1)
    if scores.shape[0] != lab.shape[0]:
        raise ValueError('length of `logit` and `label` should be equal, but they are {} and {}.'.format(scores.shape[0],
                                                                                                    lab.shape[0]))
    if num_classes == 2:
        return binary_auc(scores[:, 1], lab == 1)
    present = np.unique(lab)
    if len(present) != C:
        raise ValueError("Number of classes in y_true not equal to the number of columns in 'y_score'")
    return float(np.mean([binary_auc(scores[:, c], lab == c) for c in range(C)]))


# ------------------------------------------------------------------------------------------------------------------
# auc_roc from exact pair counts.  With float32 scores the one-vs-rest AUC of class c is U2 / (2 * n_pos * n_neg) where
#   U2 = sum over the positives i of ( 2 * #{negatives j : s_j < s_i} + #{negatives j : s_j == s_i} )
# is an integer: twice the Mann-Whitney statistic binary_auc takes from average ranks.  On the sorted scores, with N(p) the
# negatives in front of position p, a positive inside the run of equal scores [a, b) contributes N(a) + N(b).
# auc_counts states this in numpy; csrc/msk_auc.hip (msk_auc_pack / msk_auc_counts, through AucScores) is held to it word
# for word.  auc_from_counts turns the [C, 3] words {U2, n_pos, n_neg} into the float auc_roc returns.


def _check_scores_and_labels(bad_label, bad_score):
    if bad_label:
        raise RuntimeError('labels with ignore_index is not supported yet.')
    if bad_score:
        raise ValueError("{} scores are negative or not finite: not softmax outputs".format(int(bad_score)))


def auc_counts(scores, label, num_classes):
    """[C, 3] uint64 {U2, n_pos, n_neg} per class from float32 scores (N, C, *spatial) and labels (N, 1, *spatial) or
    (N, *spatial), on the host: sort, runs of equal scores, prefix counts of the negatives.  Scores must be finite and
    >= 0 (-0.0 counts as 0.0), labels inside [0, C)."""
    scores = np.asarray(scores, dtype=np.float32)
    label = np.asarray(label)
    if scores.ndim < 2:
        raise ValueError('The shape of logits is not (N, C, *spatial), it is {}'.format(scores.shape))
    C = scores.shape[1]
    if C != num_classes:
        raise ValueError("scores have {} channels, num_classes is {}".format(C, num_classes))
    sc = np.ascontiguousarray(np.moveaxis(scores, 1, -1).reshape(-1, C))
    lab = label.reshape(-1)
    if sc.shape[0] != lab.shape[0]:
        raise ValueError('length of `logit` and `label` should be equal, but they are {} and {}.'.format(sc.shape[0],
                                                                                                    lab.shape[0]))
    bits = sc.view(np.uint32)
    bits = np.where(bits == 0x80000000, np.uint32(0), bits)
    bad_score = np.count_nonzero((bits & 0x80000000) != 0) + np.count_nonzero((bits & 0x7f800000) == 0x7f800000)
    _check_scores_and_labels(np.count_nonzero((lab < 0) | (lab >= C)), bad_score)
    out = np.zeros((C, 3), dtype=np.uint64)
    n = lab.shape[0]
    for c in range(C):
        # bits of a non-negative float are in float order; the flag rides in bit 0 (its order inside a run does not matter)
        k = np.sort((bits[:, c] << np.uint32(1)) | (lab == c).astype(np.uint32))
        positive = (k & 1).astype(bool)
        xs = k >> 1
        start = np.flatnonzero(np.concatenate(([True], xs[1:] != xs[:-1]))) if n else np.zeros(0, np.int64)
        end = np.concatenate((start[1:], [n])).astype(np.int64)
        nneg = np.concatenate(([0], np.cumsum(~positive, dtype=np.int64)))       # N(p), p = 0 .. n
        npos_run = np.add.reduceat(positive.astype(np.int64), start) if n else np.zeros(0, np.int64)
        u2 = int(np.sum(npos_run * (nneg[start] + nneg[end])))                   # <= 2 n_pos n_neg < 2^62: exact in int64
        n_neg = int(nneg[-1])
        out[c] = (u2, n - n_neg, n_neg)
    return out


def auc_from_counts(counts, num_classes):
    """The float ``auc_roc`` returns from [C, 3] {U2, n_pos, n_neg}: two classes -> AUC of class 1; more -> macro
    one-vs-rest over all classes, every one of which needs a positive (metric.py:64-107 / sklearn's conventions)."""
    c = np.asarray(counts).reshape(-1, 3)
    if c.shape[0] != num_classes:
        raise ValueError("counts have {} rows, num_classes is {}".format(c.shape[0], num_classes))

    def one(row):
        u2, n_pos, n_neg = (int(v) for v in row)
        if n_pos == 0 or n_neg == 0:
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        return float(u2) / (2.0 * n_pos * n_neg)

    if num_classes == 2:
        return one(c[1])
    if any(int(row[1]) == 0 for row in c):
        raise ValueError("Number of classes in y_true not equal to the number of columns in 'y_score'")
    return float(np.mean([one(row) for row in c]))


class AucScores:
    """The softmax scores of a whole validation set as sortable keys in persistent device buffers (not the activation
    arena), and their exact AUC counts.

    ``add(probs, label)`` appends one batch (msk_auc_pack at the current fill: no synchronisation); the buffers grow by
    a device-to-device copy when ``capacity`` (keys per class) is exceeded.  ``counts()`` sorts and counts on the device
    (msk_auc_counts) and downloads 3 * C + 2 words, the one synchronisation: the [C, 3] uint64 {U2, n_pos, n_neg} of
    ``auc_counts``.  It raises RuntimeError('labels with ignore_index is not supported yet.') when a label was outside
    [0, C) and ValueError for a negative or non-finite score.  ``add`` after ``counts()`` keeps working.

    Device memory: 4 * C * capacity bytes of keys for the lifetime of the object, and inside ``counts()`` a second
    buffer of 4 * C * fill bytes plus the histograms of the sort (about 1/16 of it): 2 * 4 * C * capacity bytes plus
    the histograms at the peak."""

    def __init__(self, dev, num_classes, capacity):
        self.dev, self.num_classes = dev, int(num_classes)
        if not 1 <= self.num_classes <= 64:
            raise ValueError("num_classes must be in [1, 64], got {}".format(num_classes))
        self.capacity = self._round(max(int(capacity), 1))
        self.fill = 0
        self.keys = self._malloc(4 * self.num_classes * self.capacity, self.capacity)
        # {U2, n_pos, n_neg} per class, then the two status words of msk_auc_pack: one download
        self.words = 3 * self.num_classes + 2
        self.res = dev.malloc(8 * self.words)
        dev.memset(self.res, 0, 8 * self.words)

    @staticmethod
    def _round(n):
        return (n + 3) & ~3       # every class stream starts on 16 bytes

    def _malloc(self, nbytes, capacity):
        from .._lib import MskError
        try:
            return self.dev.malloc(nbytes)
        except MskError as e:
            raise MskError("AucScores: {} bytes of device memory for {} classes x {} keys failed (it needs 2 x 4 x "
                           "classes x capacity = {} bytes plus the histograms): {}".format(
                               nbytes, self.num_classes, capacity, 8 * self.num_classes * capacity, e)) from None

    def _grow(self, need):
        cap = self._round(max(need, 2 * self.capacity))
        if cap >= 2 ** 31:
            cap = self._round(need)
        if cap >= 2 ** 31:
            raise ValueError("AucScores holds fewer than 2^31 scores per class, {} requested".format(need))
        new = self._malloc(4 * self.num_classes * cap, cap)
        for c in range(self.num_classes if self.fill else 0):
            self.dev.d2d(new + 4 * c * cap, self.keys + 4 * c * self.capacity, 4 * self.fill)
        self.dev.free(self.keys)
        self.keys, self.capacity = new, cap

    def add(self, probs, label):
        import ctypes as C
        from ..device import IntTensor, Tensor
        if not isinstance(probs, Tensor) or not isinstance(label, IntTensor):
            raise TypeError("AucScores.add takes a device Tensor of scores and an IntTensor label")
        if probs.dev is not self.dev or label.dev is not self.dev:
            raise ValueError("scores, label and AucScores are on different devices")
        if probs.c != self.num_classes:
            raise ValueError("scores have {} channels, num_classes is {}".format(probs.c, self.num_classes))
        v = probs.voxels
        if int(np.prod(label.shape)) != v:
            raise ValueError('length of `logit` and `label` should be equal, but they are {} and {}.'.format(
                v, int(np.prod(label.shape))))
        if self.fill + v > self.capacity:
            self._grow(self.fill + v)
        self.dev.call("msk_auc_pack", probs.msk(), C.c_void_p(label.ptr), C.c_void_p(self.keys), C.c_long(self.capacity),
                      C.c_long(self.fill), C.c_void_p(self.res + 8 * 3 * self.num_classes))
        self.fill += v

    def counts(self):
        import ctypes as C
        if self.fill == 0:
            raise ValueError("AucScores.counts: no scores were added")
        nbytes = C.c_size_t(0)
        if self.dev.lib.msk_auc_workspace(C.c_long(self.fill), self.num_classes, C.byref(nbytes)) != 0:
            from .._lib import MskError, last_error
            raise MskError("msk_auc_workspace failed: " + last_error(None))
        ws = self._malloc(nbytes.value, self.capacity)
        try:
            self.dev.call("msk_auc_counts", C.c_void_p(self.keys), C.c_long(self.capacity), C.c_long(self.fill),
                          self.num_classes, C.c_void_p(ws), nbytes, C.c_void_p(self.res))
            words = self.dev.d2h(self.res, (self.words,), np.uint64)
        finally:
            self.dev.free(ws)
        _check_scores_and_labels(int(words[-2]), int(words[-1]))
        return words[:3 * self.num_classes].reshape(self.num_classes, 3).copy()

    def free(self):
        if self.keys:
            self.dev.free(self.keys)
            self.dev.free(self.res)
        self.keys = self.res = None


# ------------------------------------------------------------------------------------------------------------------
# Hard-label metrics (reference medicalseg/utils/metric.py:21-61, 110-210): calculate_area, mean_iou, dice, accuracy,
# kappa.  Everything is derived from the CONFUSION COUNTS of a prediction against its label, one row per volume:
# K*K + 1 words with K = num_classes + 1, word r*K + c = voxels with label class r and predicted class c among the
# voxels whose label is not ignore_index (class num_classes = "other": negative or >= num_classes), last word =
# voxels whose label is ignore_index.  Device inputs are counted by msk_confusion3d (csrc/msk_metrics.hip) and only
# the counts are downloaded; numpy inputs take the same definition through np.bincount.


class ConfusionCounts:
    """[N, K*K + 1] uint64 confusion counts in a persistent device buffer (not the activation arena: it survives the
    next model forward).  Passing it back as ``confusion_counts(..., out=self)`` adds to it; ``numpy()`` downloads
    (one synchronisation)."""

    def __init__(self, dev, n, num_classes, ignore_index=255, zero=False, _view_of=None):
        self.dev, self.n, self.num_classes, self.ignore_index = dev, int(n), int(num_classes), int(ignore_index)
        self.shape = (self.n, (self.num_classes + 1) ** 2 + 1)
        self._owner = _view_of      # a view keeps its parent alive and does not free
        if _view_of is None:
            self.ptr = dev.malloc(self.shape[0] * self.shape[1] * 8)
            if zero:
                dev.memset(self.ptr, 0, self.shape[0] * self.shape[1] * 8)

    def rows(self, start, count=1):
        """rows [start, start + count) as a ConfusionCounts of their own (same memory): the ``out=`` of one batch of a
        validation set whose buffer (created with ``zero=True``) holds one row per volume"""
        start, count = int(start), int(count)
        if not (0 <= start and count >= 1 and start + count <= self.n):
            raise IndexError("rows [{}, {}) of {}".format(start, start + count, self.n))
        v = ConfusionCounts(self.dev, count, self.num_classes, self.ignore_index, _view_of=self)
        v.ptr = self.ptr + start * self.shape[1] * 8
        return v

    def numpy(self):
        return self.dev.d2h(self.ptr, self.shape, np.uint64)

    def free(self):
        if self._owner is None and self.ptr:
            self.dev.free(self.ptr)
        self.ptr = None


def _is_device(x):
    from ..device import IntTensor
    from ..preprocess import DeviceVolume
    return isinstance(x, (IntTensor, DeviceVolume))


def _volume_shape(x):
    """(N, spatial shape) of a prediction / label: [N, 1, D, H, W], [N, D, H, W] or one 3-D volume"""
    shape = tuple(int(s) for s in x.shape)
    if len(shape) == 5 and shape[1] == 1:
        shape = shape[:1] + shape[2:]
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4:
        raise ValueError("expected [N, 1, D, H, W], [N, D, H, W] or [D, H, W], got shape {}".format(tuple(x.shape)))
    return shape[0], shape[1:]


def confusion_counts(pred, label, num_classes, ignore_index=255, out=None):
    """Confusion counts of ``pred`` against ``label``, one row per volume (layout above).

    Device inputs (``IntTensor`` [N, 1, D, H, W] / [N, D, H, W], or a 3-D int32 ``DeviceVolume``; both on one
    device): one msk_confusion3d launch, no synchronisation; returns a ``ConfusionCounts``.  ``out`` (an earlier
    result with the same N, num_classes and ignore_index) is added to and returned.  numpy inputs: the same counts as
    an [N, K*K + 1] uint64 array on the host (``out``: an array that is added to in place)."""
    num_classes, ignore_index = int(num_classes), int(ignore_index)
    if not 1 <= num_classes <= 64:
        raise ValueError("num_classes must be in [1, 64], got {}".format(num_classes))
    dev_in = (_is_device(pred), _is_device(label))
    if dev_in[0] != dev_in[1]:
        raise TypeError("pred and label must both be device arrays or both be host arrays")
    if not dev_in[0]:
        pred, label = np.asarray(pred), np.asarray(label)
    (n, ps), (nl, ls) = _volume_shape(pred), _volume_shape(label)
    if (n, ps) != (nl, ls):
        raise ValueError('Shape of `pred` and `label should be equal, but there are {} and {}.'.format(
            list((n,) + ps), list((nl,) + ls)))
    K = num_classes + 1
    B = K * K + 1
    if dev_in[0]:
        import ctypes as C
        if pred.dev is not label.dev:
            raise ValueError("pred and label are on different devices")
        for x in (pred, label):
            if getattr(x, "dtype", np.dtype(np.int32)) != np.int32:
                raise TypeError("device volumes must be int32, got {}".format(x.dtype))
        if out is None:
            res, acc = ConfusionCounts(pred.dev, n, num_classes, ignore_index), 0
        else:
            if not isinstance(out, ConfusionCounts) or out.dev is not pred.dev or \
                    (out.n, out.num_classes, out.ignore_index) != (n, num_classes, ignore_index):
                raise ValueError("`out` must be a ConfusionCounts of the same device, N, num_classes and ignore_index")
            res, acc = out, 1
        pred.dev.call("msk_confusion3d", C.c_void_p(pred.ptr), C.c_void_p(label.ptr), n, C.c_long(int(np.prod(ps))),
                      num_classes, ignore_index, C.c_void_p(res.ptr), acc)
        return res
    p = pred.reshape(n, -1).astype(np.int64)
    l = label.reshape(n, -1).astype(np.int64)
    r = np.where((l >= 0) & (l < num_classes), l, num_classes)
    c = np.where((p >= 0) & (p < num_classes), p, num_classes)
    key = np.where(l == ignore_index, K * K, r * K + c)
    counts = np.stack([np.bincount(k, minlength=B) for k in key]).astype(np.uint64)
    if out is not None:
        if not isinstance(out, np.ndarray) or out.shape != counts.shape:
            raise ValueError("`out` must be an array of shape {}".format(counts.shape))
        out += counts.astype(out.dtype)
        return out
    return counts


def _host(x):
    return np.asarray(x.numpy() if hasattr(x, "numpy") else x)


def areas_from_counts(counts, num_classes, ignore_index=255, per_volume=False):
    """(intersect_area, pred_area, label_area) of the reference's calculate_area from confusion counts: int64 arrays
    of length num_classes summed over the rows, or [N, num_classes] with ``per_volume``.  label_area counts
    ``label == i`` without the ignore mask, as the reference does: the ignored voxels return to class ignore_index."""
    num_classes, ignore_index = int(num_classes), int(ignore_index)
    K = num_classes + 1
    c = _host(counts).astype(np.int64).reshape(-1, K * K + 1)
    m = c[:, :K * K].reshape(-1, K, K)
    idx = np.arange(num_classes)
    intersect = m[:, idx, idx]
    pred_area = m.sum(axis=1)[:, :num_classes]
    label_area = m.sum(axis=2)[:, :num_classes].copy()
    if 0 <= ignore_index < num_classes:
        label_area[:, ignore_index] += c[:, -1]
    if per_volume:
        return intersect, pred_area, label_area
    return intersect.sum(axis=0), pred_area.sum(axis=0), label_area.sum(axis=0)


def region_areas_from_counts(counts, num_classes, table, num_regions, per_volume=False):
    """(intersect_area, pred_area, label_area) per REGION from the same confusion counts (region-based training: the regions
    overlap, so they are no partition of the classes): int64 arrays of length num_regions summed over the rows, or
    [N, num_regions] with ``per_volume``.  Class c < num_classes belongs to region r when bit r of table[c] is set
    (RegionSpec.table()); the "other" class (a value outside [0, num_classes)) belongs to no region.  intersect counts the
    voxels whose label AND prediction lie in the region, pred_area / label_area those whose prediction / label does; the
    ignored voxels count nowhere.  Exact integers on the host (tests/mlabel_reference.py: region_areas)."""
    num_classes, num_regions = int(num_classes), int(num_regions)
    K = num_classes + 1
    table = np.asarray(table)
    c = _host(counts).astype(np.int64).reshape(-1, K * K + 1)
    m = c[:, :K * K].reshape(-1, K, K)                       # [volume, label class, predicted class]
    member = np.zeros((num_regions, K), dtype=np.int64)      # [region, class]; the last column (other) stays 0
    for cls in range(min(num_classes, table.size)):
        for r in range(num_regions):
            member[r, cls] = (int(table[cls]) >> r) & 1
    label_area = np.einsum('nlp,rl->nr', m, member)
    pred_area = np.einsum('nlp,rp->nr', m, member)
    intersect = np.einsum('nlp,rl,rp->nr', m, member, member)
    if per_volume:
        return intersect, pred_area, label_area
    return intersect.sum(axis=0), pred_area.sum(axis=0), label_area.sum(axis=0)


def calculate_area(pred, label, num_classes, ignore_index=255):
    """metric.py:21-61 -> (intersect_area, pred_area, label_area), int64 [num_classes], summed over the batch.
    Device inputs are counted on the device (one download of the counts)."""
    counts = confusion_counts(pred, label, num_classes, ignore_index)
    try:
        return areas_from_counts(counts, num_classes, ignore_index)
    finally:
        if isinstance(counts, ConfusionCounts):
            counts.free()


def _ratio(num, den):
    """num / den per class in float64, 0 where den == 0"""
    num, den = _host(num).astype(np.float64), _host(den).astype(np.float64)
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def mean_iou(intersect_area, pred_area, label_area):
    """metric.py:110-135 -> (class_iou, miou); a class with an empty union scores 0 and still enters the mean"""
    i, p, l = _host(intersect_area), _host(pred_area), _host(label_area)
    class_iou = _ratio(i, p + l - i)
    return class_iou, np.mean(class_iou)


def dice(intersect_area, pred_area, label_area):
    """metric.py:138-163 -> (class_dice, mdice); 2 |A n B| / (|A| + |B|), 0 for a class absent from both"""
    i, p, l = _host(intersect_area), _host(pred_area), _host(label_area)
    class_dice = _ratio(2 * i, p + l)
    return class_dice, np.mean(class_dice)


def accuracy(intersect_area, pred_area):
    """metric.py:166-188 -> (class_acc, macc); macc is the overall ratio sum(intersect) / sum(pred), not the class mean"""
    i, p = _host(intersect_area), _host(pred_area)
    return _ratio(i, p), np.sum(i) / np.sum(p)


def kappa(intersect_area, pred_area, label_area):
    """metric.py:191-210 Cohen's kappa (po - pe) / (1 - pe); not guarded against pe == 1, as in the reference"""
    i, p, l = _host(intersect_area), _host(pred_area), _host(label_area)
    total = np.sum(l)
    po = np.sum(i) / total
    pe = np.sum(p * l) / (total * total)
    return (po - pe) / (1 - pe)


def per_case(counts, num_classes, ignore_index=255):
    """The same metrics per volume (medical results are means over cases; the functions above pool the voxels):
    {'class_iou', 'class_dice', 'class_acc': [N, num_classes]; 'miou', 'mdice', 'acc', 'kappa': [N]} from the
    [N, K*K + 1] counts."""
    rows = areas_from_counts(counts, num_classes, ignore_index, per_volume=True)
    res = {k: [] for k in ("class_iou", "miou", "class_dice", "mdice", "class_acc", "acc", "kappa")}
    for i, p, l in zip(*rows):
        ci, mi = mean_iou(i, p, l)
        cd, md = dice(i, p, l)
        ca, ma = accuracy(i, p)
        for k, v in (("class_iou", ci), ("miou", mi), ("class_dice", cd), ("mdice", md), ("class_acc", ca), ("acc", ma),
                     ("kappa", kappa(i, p, l))):
            res[k].append(v)
    return {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}


# ------------------------------------------------------------------------------------------------------------------
# Boundary metrics: Hausdorff distance, HD95 and average symmetric surface distance (ASSD) with medpy's conventions
# (the reference has none), from an exact squared Euclidean distance transform.  Volumes are [D, H, W] with axes
# (z, y, x); spacing = (sz, sy, sx) in float64, None = (1, 1, 1); wz, wy, wx = sz*sz, sy*sy, sx*sx, rounded once.
#   surface S(M): the voxels of the boolean mask M with at least one of the six face neighbours outside M, where
#       everything beyond the volume's edge is outside (= M & ~scipy.ndimage.binary_erosion(M));
#   squared EDT of a feature set F at voxel v:  min over u in F of fl(fl(fl(wx dx^2) + fl(wy dy^2)) + fl(wz dz^2)),
#       dx, dy, dz integer index differences, every fl one float64 rounding, no fused multiply-add; +inf for empty F.
#       Rounding is monotone, so the separable evaluation (x pass: wx dx^2 of the nearest feature of the row; y pass:
#       min over y' of gx(y') + wy (y - y')^2; the same along z) gives the same bits as the brute-force minimum;
#   for class c with P = S(pred == c), L = S(label == c):  d2_pl = dist2_L at the voxels of P, d2_lp = dist2_P at the
#       voxels of L, both sorted; d = sqrt(d2);  hd = max(max d_pl, max d_lp),  hd95 = np.percentile(d_pl ++ d_lp, 95),
#       assd = (mean d_pl + mean d_lp) / 2;  all three nan when either surface is empty.
# ignore_index gets no special treatment here: a voxel labelled ignore_index belongs to no class c != ignore_index and
# therefore lies outside every mask (label == c), like any other value.
# edt_squared / surface_mask on numpy arrays ARE this specification (exact, not fast); device inputs go through
# csrc/msk_edt.hip (msk_edt3d, msk_surface_count, msk_surface_gather), which is held to the same bits.

EDT_MAX_EXTENT = 2048       # MSK_EDT_MAX_EXTENT of include/msegk.h


def _spacing_weights(spacing):
    if spacing is None:
        return np.ones(3, dtype=np.float64), None
    s = np.asarray(spacing, dtype=np.float64).reshape(-1)
    if s.shape != (3,):
        raise ValueError("spacing must be (sz, sy, sx), got {}".format(spacing))
    with np.errstate(over="ignore", invalid="ignore"):
        w = s * s
    if not (np.all(s > 0) and np.all(w >= 1e-300) and np.all(w <= 1e300)):
        raise ValueError("spacing must be positive with its square within [1e-300, 1e300], got {}".format(spacing))
    return w, s


def surface_mask(mask):
    """S(M) of a boolean [D, H, W] array: the voxels of M with a face neighbour outside M (the edge counts as outside)"""
    m = np.asarray(mask).astype(bool)
    if m.ndim != 3:
        raise ValueError("expected a [D, H, W] mask, got shape {}".format(m.shape))
    p = np.pad(m, 1, mode="constant", constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] &
             p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m & ~inner


def _edt_row_pass(f, w):
    """[n, L] bool -> w * dx^2 of the nearest True of every row (one rounding), +inf for a row without one"""
    n, L = f.shape
    x = np.arange(L, dtype=np.int64)
    far = np.int64(4 * L + 4)
    left = np.maximum.accumulate(np.where(f, x, -far), axis=1)                         # nearest feature at or left of x
    right = np.minimum.accumulate(np.where(f, x, far)[:, ::-1], axis=1)[:, ::-1]       # ... at or right of x
    dx = np.minimum(x - left, right - x)
    g = w * (dx * dx).astype(np.float64)
    g[~f.any(axis=1)] = np.inf
    return g


def _edt_line_pass(g, w, chunk=8192):
    """[n, L] float64 -> out[i, l] = min over l' of fl(g[i, l'] + fl(w (l - l')^2)), by brute force over the offsets;
    an offset k is only skipped when fl(w k^2) alone is >= every running minimum of the chunk (no candidate
    fl(g + fl(w k^2)) >= fl(w k^2) can lower any of them), which changes no bit."""
    w = float(w)
    out = np.array(g, dtype=np.float64, copy=True)
    n, L = out.shape
    live = np.flatnonzero(np.isfinite(out).any(axis=1))        # a line without a feature stays +inf
    for a in range(0, live.size, chunk):
        rows = live[a:a + chunk]
        src = out[rows]
        best = src.copy()
        for k in range(1, L):
            c = w * float(k * k)
            if c >= best.max():
                break
            np.minimum(best[:, k:], src[:, :-k] + c, out=best[:, k:])
            np.minimum(best[:, :-k], src[:, k:] + c, out=best[:, :-k])
        out[rows] = best
    return out


def _edt_squared_host(features, spacing):
    f = np.asarray(features).astype(bool)
    if f.ndim != 3:
        raise ValueError("expected a [D, H, W] feature mask, got shape {}".format(f.shape))
    (wz, wy, wx), _ = _spacing_weights(spacing)
    D, H, W = f.shape
    g = _edt_row_pass(f.reshape(D * H, W), wx).reshape(D, H, W)
    g = _edt_line_pass(g.transpose(0, 2, 1).reshape(D * W, H), wy).reshape(D, W, H).transpose(0, 2, 1)
    g = _edt_line_pass(g.transpose(1, 2, 0).reshape(H * W, D), wz).reshape(H, W, D).transpose(2, 0, 1)
    return np.ascontiguousarray(g)


def _device_volume(x, what):
    """(dev, ptr, (D, H, W)) of an int32 IntTensor [1, 1, D, H, W] / [1, D, H, W] / [D, H, W] or DeviceVolume"""
    if getattr(x, "dtype", np.dtype(np.int32)) != np.int32:
        raise TypeError("device volumes must be int32, got {}".format(x.dtype))
    n, shape = _volume_shape(x)
    if n != 1:
        raise ValueError("{}: one volume at a time, got a batch of {}".format(what, n))
    if max(shape) > EDT_MAX_EXTENT:
        raise ValueError("{}: extents up to {} per axis are supported, got {}".format(what, EDT_MAX_EXTENT, shape))
    return x.dev, x.ptr, shape


def _c_spacing(spacing):
    import ctypes as C
    _, s = _spacing_weights(spacing)
    return None if s is None else (C.c_double * 3)(*s.tolist())


def edt_squared(x, spacing=None, cls=1, surface_only=False):
    """Exact squared Euclidean distance transform (specification above) to the features of ``x``.

    numpy input: ``x`` is the boolean feature mask [D, H, W] itself (``cls`` is not used; ``surface_only`` takes
    surface_mask(x) first); returns a float64 array.  Device input (int32 ``IntTensor`` [1, 1, D, H, W] / [1, D, H, W]
    or 3-D ``DeviceVolume``): the features are the voxels with ``x == cls``, or their surface with ``surface_only``;
    one msk_edt3d call, no synchronisation; returns a float64 ``DeviceVolume`` (``numpy()``, ``free()``) holding the
    same bits.  Extents up to EDT_MAX_EXTENT per axis on the device."""
    if not _is_device(x):
        f = np.asarray(x).astype(bool)
        return _edt_squared_host(surface_mask(f) if surface_only else f, spacing)
    import ctypes as C
    from ..preprocess import DeviceVolume
    dev, ptr, (d, h, w) = _device_volume(x, "edt_squared")
    out = DeviceVolume(dev, dev.malloc(8 * d * h * w), (d, h, w), np.float64)
    try:
        dev.call("msk_edt3d", C.c_void_p(ptr), d, h, w, int(cls), 1 if surface_only else 0, _c_spacing(spacing),
                 C.c_void_p(out.ptr))
    except Exception:
        out.free()
        raise
    return out


def signed_distance(x, cls=1, spacing=None):
    """Signed distance map of class ``cls`` in the label volume ``x`` (Kervadec's one_hot2dist; tests/boundary_reference.py
    is the statement): the distance to the class outside it, ``1 -`` the distance to its complement inside it, 0 where the
    class is absent or fills the volume; float64 distances from edt_squared, rounded once to float32.

    numpy input: a [D, H, W] label array, returns a float32 array.  Device input (int32 ``IntTensor`` [1, 1, D, H, W] /
    [1, D, H, W] or 3-D ``DeviceVolume``): one msk_label_sdf call; returns a float32 ``DeviceVolume`` holding the same
    bits.  Freeing the transform's workspace waits for the stream (the loss keeps its workspace in the arena and does not)."""
    if not _is_device(x):
        lab = np.asarray(x)
        if lab.ndim != 3:
            raise ValueError("expected a [D, H, W] label volume, got shape {}".format(lab.shape))
        pos = lab == cls
        with np.errstate(invalid="ignore"):
            d_out = np.sqrt(_edt_squared_host(pos, spacing))
            d_in = np.sqrt(_edt_squared_host(~pos, spacing))
            phi = np.where(pos, 1.0 - d_in, d_out)
        return np.where(np.isfinite(phi), phi, 0.0).astype(np.float32)
    import ctypes as C
    from ..preprocess import DeviceVolume
    if not 0 <= int(cls) <= 63:
        raise ValueError("signed_distance: device volumes take classes 0 .. 63, got {}".format(cls))
    dev, ptr, (d, h, w) = _device_volume(x, "signed_distance")
    sp = _c_spacing(spacing)
    nbytes = C.c_size_t(0)
    if dev.lib.msk_sdf_workspace(d, h, w, C.byref(nbytes)) != 0:
        raise ValueError("msk_sdf_workspace refused a volume of {} x {} x {}".format(d, h, w))
    ws = dev.malloc(nbytes.value)
    out = DeviceVolume(dev, dev.malloc(4 * d * h * w), (d, h, w), np.float32)
    try:
        dev.call("msk_label_sdf", C.c_void_p(ptr), 1, d, h, w, C.c_uint64(1 << int(cls)), sp, C.c_void_p(ws),
                 C.c_size_t(nbytes.value), C.c_void_p(out.ptr))
    except Exception:
        out.free()
        raise
    finally:
        dev.free(ws)      # msk_free waits for the stream: the transform is done with it
    return out


class SurfaceDistances:
    """The two directed multisets of SQUARED surface distances of one class, sorted ascending: ``d2_pl`` (from the
    prediction's surface voxels to the label's surface) and ``d2_lp`` (the other way).  Metrics follow medpy and are
    nan when either surface is empty."""

    def __init__(self, d2_pl, d2_lp):
        self.d2_pl = np.sort(np.asarray(d2_pl, dtype=np.float64).reshape(-1))
        self.d2_lp = np.sort(np.asarray(d2_lp, dtype=np.float64).reshape(-1))

    @property
    def empty(self):
        return self.d2_pl.size == 0 or self.d2_lp.size == 0

    def distances(self):
        """(d_pl, d_lp): the square roots, still sorted"""
        return np.sqrt(self.d2_pl), np.sqrt(self.d2_lp)

    def hd(self):
        if self.empty:
            return float("nan")
        d_pl, d_lp = self.distances()
        return float(max(d_pl[-1], d_lp[-1]))

    def percentile(self, q):
        if self.empty:
            return float("nan")
        return float(np.percentile(np.concatenate(self.distances()), q))

    def hd95(self):
        return self.percentile(95)

    def assd(self):
        if self.empty:
            return float("nan")
        d_pl, d_lp = self.distances()
        return float((np.mean(d_pl) + np.mean(d_lp)) / 2)


def _surface_distances_device(pred, label, cls, spacing):
    import ctypes as C
    dev, pp, shape = _device_volume(pred, "surface_distances")
    dev_l, lp, shape_l = _device_volume(label, "surface_distances")
    if dev is not dev_l:
        raise ValueError("pred and label are on different devices")
    if shape != shape_l:
        raise ValueError('Shape of `pred` and `label should be equal, but there are {} and {}.'.format(
            list(shape), list(shape_l)))
    d, h, w = shape
    dims = (d, h, w, int(cls))
    sp = _c_spacing(spacing)
    vp = C.c_void_p
    words = dev.malloc(32)
    dist = out_p = out_l = None
    try:
        dev.call("msk_surface_count", vp(pp), *dims, vp(words))
        dev.call("msk_surface_count", vp(lp), *dims, vp(words + 8))
        n_p, n_l = (int(v) for v in dev.d2h(words, (2,), np.uint64))
        if n_p == 0 or n_l == 0:
            # a metric is nan as soon as one surface is empty; the other side's distances would all be +inf
            empty = np.zeros(0, np.float64)
            return SurfaceDistances(empty if n_p == 0 else np.full(n_p, np.inf), empty if n_l == 0 else np.full(n_l, np.inf))
        dist = dev.malloc(8 * d * h * w)
        out_p, out_l = dev.malloc(8 * n_p), dev.malloc(8 * n_l)
        dev.call("msk_edt3d", vp(lp), *dims, 1, sp, vp(dist))
        dev.call("msk_surface_gather", vp(pp), *dims, vp(dist), vp(out_p), C.c_long(n_p), vp(words + 16))
        dev.call("msk_edt3d", vp(pp), *dims, 1, sp, vp(dist))
        dev.call("msk_surface_gather", vp(lp), *dims, vp(dist), vp(out_l), C.c_long(n_l), vp(words + 24))
        d2_pl = dev.d2h(out_p, (n_p,), np.float64)
        d2_lp = dev.d2h(out_l, (n_l,), np.float64)
        got = tuple(int(v) for v in dev.d2h(words + 16, (2,), np.uint64))
        if got != (n_p, n_l):
            raise RuntimeError("surface_distances: gathered {} values, counted {}".format(got, (n_p, n_l)))
        return SurfaceDistances(d2_pl, d2_lp)
    finally:
        for ptr in (words, dist, out_p, out_l):
            if ptr:
                dev.free(ptr)


def surface_distances(pred, label, cls, spacing=None):
    """The directed squared surface distances of class ``cls`` between a hard-label prediction and its label
    (definitions above) as a ``SurfaceDistances`` (``hd()``, ``hd95()``, ``assd()``, ``percentile(q)``).

    Device inputs (int32 ``IntTensor`` [1, 1, D, H, W] / [1, D, H, W], or a 3-D ``DeviceVolume``; both on one device):
    two surface counts (one small download: an absent class ends here), then per direction one distance transform
    and one gather on the device; only the surface voxels' values are downloaded, never a volume.  numpy inputs of
    the same shapes run through the numpy specification.  ``ignore_index`` gets no special treatment."""
    dev_in = (_is_device(pred), _is_device(label))
    if dev_in[0] != dev_in[1]:
        raise TypeError("pred and label must both be device arrays or both be host arrays")
    if dev_in[0]:
        return _surface_distances_device(pred, label, cls, spacing)
    pred, label = np.asarray(pred), np.asarray(label)
    (n, ps), (nl, ls) = _volume_shape(pred), _volume_shape(label)
    if (n, ps) != (nl, ls):
        raise ValueError('Shape of `pred` and `label should be equal, but there are {} and {}.'.format(
            list((n,) + ps), list((nl,) + ls)))
    if n != 1:
        raise ValueError("surface_distances: one volume at a time, got a batch of {}".format(n))
    _spacing_weights(spacing)
    P, L = surface_mask(pred.reshape(ps) == cls), surface_mask(label.reshape(ls) == cls)
    if not P.any() or not L.any():
        return SurfaceDistances(np.full(int(P.sum()), np.inf), np.full(int(L.sum()), np.inf))
    return SurfaceDistances(_edt_squared_host(L, spacing)[P], _edt_squared_host(P, spacing)[L])


def surface_metrics(pred, label, num_classes, spacing=None, classes=None):
    """{'hd', 'hd95', 'assd'}: float64 arrays with one entry per class of ``classes`` (None = the foreground classes
    1 .. num_classes - 1) for one volume, nan where the class has no surface in ``pred`` or in ``label``; 'classes'
    holds the class indices.  Inputs as in ``surface_distances``."""
    classes = list(range(1, int(num_classes))) if classes is None else [int(c) for c in classes]
    res = {k: np.full(len(classes), np.nan, dtype=np.float64) for k in ("hd", "hd95", "assd")}
    for i, c in enumerate(classes):
        sd = surface_distances(pred, label, c, spacing)
        res["hd"][i], res["hd95"][i], res["assd"][i] = sd.hd(), sd.hd95(), sd.assd()
    res["classes"] = np.asarray(classes, dtype=np.int64)
    return res


def _nanmean(a, axis=None):
    """np.nanmean without the warning for an all-nan slice (whose mean is nan)"""
    a = np.asarray(a, dtype=np.float64)
    ok = ~np.isnan(a)
    cnt = ok.sum(axis=axis)
    tot = np.where(ok, a, 0.0).sum(axis=axis)
    return np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan)


def surface_summary(per_case):
    """What evaluate(surface_metrics=True) reports from the per-case results of ``surface_metrics`` (a list of its
    dicts, same classes): hd95 / assd = nanmean over the cases of the nanmean over the classes, class_hd95 /
    class_assd = nanmean over the cases per class, surface_nan = nan entries of the [cases, classes] hd95 table."""
    h = np.stack([np.asarray(r["hd95"], dtype=np.float64) for r in per_case])
    a = np.stack([np.asarray(r["assd"], dtype=np.float64) for r in per_case])
    return {"hd95": float(_nanmean(_nanmean(h, axis=1))), "assd": float(_nanmean(_nanmean(a, axis=1))),
            "class_hd95": _nanmean(h, axis=0), "class_assd": _nanmean(a, axis=0),
            "surface_nan": int(np.isnan(h).sum())}

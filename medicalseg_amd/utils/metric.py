"""Metrics of the evaluation loop: auc_roc on the host, or for device inputs from exact pair counts taken on the device
(auc_counts / AucScores / auc_from_counts below); the hard-label family (calculate_area, mean_iou, dice, accuracy,
kappa) from confusion counts taken on the device (second half of this file).

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

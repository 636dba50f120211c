"""Device side of the loss: one fused statistics kernel + one backward kernel shared by
CrossEntropyLoss and DiceLoss, the BCELoss pair beside them, and the scalar objects the training loop manipulates
(``sum(loss_list)``, ``coef * loss``, ``loss.backward()``, ``loss.numpy()[0]``;
reference core/train.py:135-139,158)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ...device import IntTensor, LazyArray, Tensor, to_tensor


def label_pyramid(labels: IntTensor, extents) -> list:
    """The label [N, D, H, W] down-sampled by nearest neighbour to every (od, oh, ow) of `extents` (1 .. 8 of them) in one launch
    of msk_label_pyramid: per axis i = ((2 o + 1) * in) // (2 * out), the values passed through as they are
    (tests/pyramid_reference.py).  The levels come from the activation arena: they live until the next model forward, like
    the loss records."""
    dev = labels.dev
    extents = [tuple(int(v) for v in e) for e in extents]
    n, d, h, w = labels.shape
    levels = [IntTensor(dev, dev.arena.alloc(n * od * oh * ow * 4), (n, od, oh, ow), dev.arena.gen) for od, oh, ow in extents]
    ext = (C.c_int32 * (3 * len(extents)))(*[v for e in extents for v in e])
    dst = (C.c_void_p * len(levels))(*[t.ptr for t in levels])
    dev.call("msk_label_pyramid", C.c_void_p(labels.ptr), n, d, h, w, len(levels), ext, dst)
    return levels


_PYRAMID = {"key": None, "levels": None}


def label_for(logits: Tensor, labels) -> IntTensor:
    """The label a loss scores `logits` against: `labels` itself when the extents agree; for a head that its model returned at
    the head's own extent (Tensor.native_head) the level of the label pyramid with that extent.  The first request after a
    forward builds the levels of all heads of that model in one launch; they are kept per (label pointer, label shape, extents,
    arena generation), one entry.  One launch per step therefore needs the SAME device label at every loss, as core/train.py and
    loss_computation hand it over (one to_tensor per batch): a host array given to each loss separately is uploaded, and its
    pyramid built, once per loss, and two native models scored alternately inside one arena generation rebuild it at every
    change -- correct either way, only more launches."""
    labels = to_tensor(labels, logits.dev)
    if tuple(labels.shape) == (logits.n, logits.d, logits.h, logits.w):
        return labels
    mark = logits.native_head
    if mark is None or len(labels.shape) != 4 or labels.shape[0] != logits.n:
        raise ValueError(f"label shape {labels.shape} does not match logits {logits.shape}")
    extents, index = mark
    key = (labels.ptr, tuple(labels.shape), extents, logits.dev.arena.gen)
    if _PYRAMID["key"] != key:
        _PYRAMID["levels"] = label_pyramid(labels, extents)
        _PYRAMID["key"] = key
    return _PYRAMID["levels"][index]


class LossNode:
    """Fused CE + Dice evaluation for one (logits, labels) pair."""

    def __init__(self, logits: Tensor, labels: IntTensor):
        if tuple(labels.shape) != (logits.n, logits.d, logits.h, logits.w):
            raise ValueError(f"label shape {labels.shape} does not match logits {logits.shape}")
        self.logits, self.labels = logits, labels
        self.dev = logits.dev
        self.C = logits.c
        self.weights_ptr = None
        self.ignore_index = 255
        self.dice_softmax = False      # DiceLoss(sigmoid_norm=False)
        self.dice_weight_ptr = None    # DiceLoss(weight=[...]) on the device
        self.out_ptr = None
        self.stats_ptr = None
        self.evaluated_with = None

    def evaluate(self):
        key = (self.weights_ptr, self.dice_softmax, self.dice_weight_ptr)
        if self.evaluated_with == (key, self.ignore_index) and self.out_ptr is not None:
            return
        dev, Cn = self.dev, self.C
        if self.out_ptr is None:
            self.out_ptr = dev.arena.alloc((2 + Cn) * 4)
            self.stats_ptr = dev.arena.alloc((3 * Cn + 2) * 8)
        w = self.weights_ptr
        if w is None:  # Dice alone: CE term unused, any weights do
            w = dev.arena.alloc(Cn * 4)
            dev.h2d(w, np.ones(Cn, dtype=np.float32))
            self._dummy_w = w
        dev.call("msk_loss_fwd_ex", self.logits.msk(), C.c_void_p(self.labels.ptr), C.c_void_p(w),
                 int(self.ignore_index), int(self.dice_softmax), C.c_void_p(self.dice_weight_ptr),
                 C.c_void_p(self.out_ptr), C.c_void_p(self.stats_ptr))
        self.evaluated_with = (key, self.ignore_index)

    def backward(self, coef_ce: float, coef_dice: float):
        self.evaluate()
        dev = self.dev
        w = self.weights_ptr if self.weights_ptr is not None else self._dummy_w
        dz = self.logits.empty_like()
        dev.call("msk_loss_bwd_ex", self.logits.msk(), C.c_void_p(self.labels.ptr), C.c_void_p(w),
                 int(self.ignore_index), int(self.dice_softmax), C.c_void_p(self.dice_weight_ptr),
                 C.c_void_p(self.stats_ptr), C.c_float(coef_ce), C.c_float(coef_dice), dz.msk())
        self.logits.grad = dz
        self.logits.grad_written = True
        return dz


def node_for(logits: Tensor, labels) -> LossNode:
    labels = label_for(logits, labels)
    key = (labels.ptr, tuple(labels.shape))
    node = _NODE_CACHE.get((id(logits), logits.ptr, logits.gen) + key)
    if node is None or node.logits is not logits:
        if len(_NODE_CACHE) > 8:
            _NODE_CACHE.clear()
        node = LossNode(logits, labels)
        _NODE_CACHE[(id(logits), logits.ptr, logits.gen) + key] = node
    return node


_NODE_CACHE = {}


class BCENode:
    """BCELoss evaluation for one (logits, labels, settings) tuple: msk_bce_fwd / msk_bce_bwd.  out[0] is the loss (the
    record has 2 + C floats like LossNode's, so the train loop's snapshot copies both kinds alike)."""

    def __init__(self, logits: Tensor, labels: IntTensor, ignore_index: int, weight_mode: int, pos_weight_mode: int,
                 pos_weight: float):
        if tuple(labels.shape) != (logits.n, logits.d, logits.h, logits.w):
            raise ValueError(f"label shape {labels.shape} does not match logits {logits.shape}")
        self.logits, self.labels = logits, labels
        self.dev = logits.dev
        self.C = logits.c
        self.ignore_index = int(ignore_index)
        self.weight_mode, self.pos_weight_mode, self.pos_weight = int(weight_mode), int(pos_weight_mode), float(pos_weight)
        self.out_ptr = None
        self.stats_ptr = None

    def evaluate(self):
        if self.out_ptr is not None:
            return
        dev = self.dev
        out = dev.arena.alloc((2 + self.C) * 4)
        stats = dev.arena.alloc(8 * 8)
        dev.call("msk_bce_fwd", self.logits.msk(), C.c_void_p(self.labels.ptr), self.ignore_index, self.weight_mode,
                 self.pos_weight_mode, C.c_float(self.pos_weight), C.c_void_p(out), C.c_void_p(stats))
        self.out_ptr, self.stats_ptr = out, stats

    def backward(self, coef: float, dz: Tensor | None = None) -> Tensor:
        """coef * dBCE/dlogits written into a new tensor, or added into `dz` (the CE / Dice gradient of the same logits)."""
        self.evaluate()
        accumulate = dz is not None
        if dz is None:
            dz = self.logits.empty_like()
        self.dev.call("msk_bce_bwd", self.logits.msk(), C.c_void_p(self.labels.ptr), self.ignore_index,
                      C.c_void_p(self.stats_ptr), C.c_float(coef), int(accumulate), dz.msk())
        self.logits.grad = dz
        self.logits.grad_written = True
        return dz


def bce_node_for(logits: Tensor, labels, ignore_index, weight_mode, pos_weight_mode, pos_weight) -> BCENode:
    labels = label_for(logits, labels)
    key = (id(logits), logits.ptr, logits.gen, labels.ptr, tuple(labels.shape), int(ignore_index), int(weight_mode),
           int(pos_weight_mode), float(pos_weight))
    node = _BCE_CACHE.get(key)
    if node is None or node.logits is not logits:
        if len(_BCE_CACHE) > 8:
            _BCE_CACHE.clear()
        node = BCENode(logits, labels, ignore_index, weight_mode, pos_weight_mode, pos_weight)
        _BCE_CACHE[key] = node
    return node


_BCE_CACHE = {}

REGION_ACTIVATIONS = {"softmax": 0, "sigmoid": 1}
REGION_DICE, REGION_TVERSKY = 0, 1


class RegionNode:
    """Masked soft Dice / Tversky (the 'dice' term, out[1]) and the focal / CE term (the 'ce' term, out[0]) for one
    (logits, labels, settings) tuple: msk_region_loss_fwd / msk_region_loss_bwd, one statistics pass and one gradient pass
    for both terms.  out[2:] is the per-class Dice; the record has 2 + C floats like LossNode's.  `settings` is the tuple
    (ignore_index, activation, squared_pred, batch_dice, do_bg, mode, smooth, alpha, beta, focal_on, gamma) in the order of the
    C ABI; `weight_ptr` is the device vector of per-class focal weights or None.  With several ranks the batch-Dice sums are
    those of this rank's batch."""

    def __init__(self, logits: Tensor, labels: IntTensor, settings, weight_ptr=None):
        if tuple(labels.shape) != (logits.n, logits.d, logits.h, logits.w):
            raise ValueError(f"label shape {labels.shape} does not match logits {logits.shape}")
        self.logits, self.labels = logits, labels
        self.dev = logits.dev
        self.C = logits.c
        self.settings = tuple(settings)
        self.weight_ptr = weight_ptr
        self.groups = 1 if self.settings[3] else logits.n
        self.out_ptr = None
        self.stats_ptr = None

    def _args(self):
        ign, act, sq, batch, bg, mode, smooth, alpha, beta, focal, gamma = self.settings
        return (self.logits.msk(), C.c_void_p(self.labels.ptr), int(ign), int(act), int(sq), int(batch), int(bg), int(mode),
                C.c_float(smooth), C.c_float(alpha), C.c_float(beta), int(focal), C.c_float(gamma), C.c_void_p(self.weight_ptr))

    def evaluate(self):
        if self.out_ptr is not None:
            return
        dev = self.dev
        out = dev.arena.alloc((2 + self.C) * 4)
        stats = dev.arena.alloc((5 * self.groups * self.C + 2) * 8)
        dev.call("msk_region_loss_fwd", *self._args(), C.c_void_p(out), C.c_void_p(stats))
        self.out_ptr, self.stats_ptr = out, stats

    def backward(self, coef_f: float, coef_r: float, dz: Tensor | None = None) -> Tensor:
        """coef_f dL_f/dlogits + coef_r dL_r/dlogits written into a new tensor, or added into `dz` (the CE / Dice gradient of
        the same logits)."""
        self.evaluate()
        accumulate = dz is not None
        if dz is None:
            dz = self.logits.empty_like()
        self.dev.call("msk_region_loss_bwd", *self._args(), C.c_void_p(self.stats_ptr), C.c_float(coef_f), C.c_float(coef_r),
                      int(accumulate), dz.msk())
        self.logits.grad = dz
        self.logits.grad_written = True
        return dz


def region_node_for(logits: Tensor, labels, settings, weight_ptr=None) -> RegionNode:
    """The node of (logits, labels, settings): two region losses on one logits tensor share it (one forward and one backward
    pass) only if every setting agrees."""
    labels = label_for(logits, labels)
    settings = tuple(settings)
    key = (id(logits), logits.ptr, logits.gen, labels.ptr, tuple(labels.shape), settings, weight_ptr)
    node = _REGION_CACHE.get(key)
    if node is None or node.logits is not logits:
        if len(_REGION_CACHE) > 8:
            _REGION_CACHE.clear()
        node = RegionNode(logits, labels, settings, weight_ptr)
        _REGION_CACHE[key] = node
    return node


_REGION_CACHE = {}

# which float of a node's out record a term reads
TERM_SLOT = {"ce": 0, "dice": 1, "bce": 0}


class Scalar:
    """A scalar loss = sum_i coef_i * term_i, term = (LossNode | RegionNode, 'ce'|'dice') or (BCENode, 'bce').  Values stay on
    the device until ``numpy()``/``float()`` (one sync), so the train loop can defer host
    syncs to log boundaries."""

    def __init__(self, terms):
        self.terms = list(terms)  # [(coef, node, which)]

    # arithmetic used by MixedLoss / loss_computation / sum()
    def __mul__(self, k):
        k = float(k)
        return Scalar([(c * k, n, w) for c, n, w in self.terms])

    __rmul__ = __mul__

    def __add__(self, other):
        if isinstance(other, (int, float)):
            if other != 0:
                raise TypeError("only sum()'s zero start value can be added to a loss")
            return self
        return Scalar(self.terms + other.terms)

    __radd__ = __add__

    def __truediv__(self, k):
        return self * (1.0 / float(k))

    def value(self) -> float:
        tot = 0.0
        for c, node, which in self.terms:
            node.evaluate()
            v = node.dev.d2h(node.out_ptr, (2,), np.float32)
            tot += c * float(v[TERM_SLOT[which]])
        return tot

    def numpy(self):
        return np.array([self.value()], dtype=np.float32)

    def item(self):
        return self.value()

    __float__ = value

    def backward(self):
        # coefficients per node, the nodes grouped per logits tensor: the CE / Dice node writes dL/dlogits, every BCE or
        # region node on the same logits adds into it (or writes it when it is the first)
        per_logits = {}
        for c, node, which in self.terms:
            group = per_logits.setdefault(id(node.logits), {})
            g = group.setdefault(id(node), [node, 0.0, 0.0])
            if which == "dice":
                g[2] += c
            else:
                g[1] += c
        # dL/dlogits per evaluated output, then ONE backward per producing model: a
        # multi-output model (VNetDeepSup.num_outputs = 4) receives the list in forward order
        producers = {}
        for group in per_logits.values():
            dz = None
            for node, cce, cdice in group.values():
                if isinstance(node, LossNode):
                    dz = node.backward(cce, cdice)
            for node, coef, cdice in group.values():
                if isinstance(node, BCENode):
                    dz = node.backward(coef, dz)
                elif isinstance(node, RegionNode):
                    dz = node.backward(coef, cdice, dz)
            logits = next(iter(group.values()))[0].logits
            prod = logits.producer
            if prod is not None:
                producers.setdefault(id(prod), (prod, {}))[1][getattr(logits, "out_index", 0)] = dz
        for prod, grads in producers.values():
            n_out = getattr(prod, "num_outputs", 1)
            if n_out == 1:
                prod.backward(grads[0])
            else:
                prod.backward([grads.get(i) for i in range(n_out)])

    def detach(self):
        return self

    def __repr__(self):
        return f"Scalar({self.value():.6f})"


def per_channel_dice(node: LossNode) -> LazyArray:
    node.evaluate()
    return LazyArray(node.dev, node.out_ptr + 8, node.C)

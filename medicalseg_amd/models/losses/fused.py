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


class Node:
    """One evaluation of (logits, labels, settings) by a pair of fused kernels.  The record `out_ptr` has 2 + C floats for
    every kind: the two terms, then the per-class Dice (the train loop's snapshot copies all kinds alike).  A kind supplies
    stats_doubles(), _forward(), _backward(coef_a, coef_b, accumulate, dz), SLOTS and `writes`."""
    writes = False     # True: backward WRITES dL/dlogits and cannot add into one; such a node runs first on its logits
    SLOTS = {}         # term name -> the float of the record it reads; slot 0 takes coef_a, slot 1 coef_b in backward

    def __init__(self, logits: Tensor, labels: IntTensor):
        if tuple(labels.shape) != (logits.n, logits.d, logits.h, logits.w):
            raise ValueError(f"label shape {labels.shape} does not match logits {logits.shape}")
        self.logits, self.labels = logits, labels
        self.dev = logits.dev
        self.C = logits.c
        self.out_ptr = None
        self.stats_ptr = None
        self.evaluated_with = None

    def slot(self, which: str) -> int:
        return self.SLOTS[which]

    def _key(self):
        """the settings a later caller may still change; evaluate() runs the forward again when they differ"""
        return ()

    def evaluate(self):
        key = self._key()
        if self.evaluated_with == key:
            return
        if self.out_ptr is None:
            self.out_ptr = self.dev.arena.alloc((2 + self.C) * 4)
            self.stats_ptr = self.dev.arena.alloc(self.stats_doubles() * 8)
        self._forward()
        self.evaluated_with = key

    def backward(self, coef_a: float, coef_b: float, dz: Tensor | None = None) -> Tensor:
        """coef_a d(term of slot 0)/dlogits + coef_b d(term of slot 1)/dlogits written into a new tensor (dz None), or added
        into `dz`, the gradient the earlier nodes of the same logits left."""
        assert dz is None or not self.writes
        self.evaluate()
        accumulate = dz is not None
        if dz is None:
            dz = self.logits.empty_like()
        self._backward(coef_a, coef_b, int(accumulate), dz)
        return self._publish(dz)

    def _publish(self, dz: Tensor) -> Tensor:
        self.logits.grad = dz
        self.logits.grad_written = True
        return dz


class LossNode(Node):
    """Fused CE + Dice evaluation for one (logits, labels) pair: msk_loss_fwd_ex / msk_loss_bwd_ex.  CrossEntropyLoss and
    DiceLoss share the node and each hands over its own settings."""
    writes = True
    SLOTS = {"ce": 0, "dice": 1}

    def __init__(self, logits: Tensor, labels: IntTensor, settings=()):
        assert not settings, "LossNode takes its settings through set_ce / set_dice: two losses share one node"
        super().__init__(logits, labels)
        self.weights_ptr = None
        self.ignore_index = 255
        self.dice_softmax = False      # DiceLoss(sigmoid_norm=False)
        self.dice_weight_ptr = None    # DiceLoss(weight=[...]) on the device

    def set_ce(self, weights_ptr, ignore_index):
        self.weights_ptr, self.ignore_index = weights_ptr, ignore_index

    def set_dice(self, softmax: bool, weight_ptr=None):
        """weight_ptr None leaves the vector an earlier DiceLoss on this node gave"""
        self.dice_softmax = softmax
        if weight_ptr is not None:
            self.dice_weight_ptr = weight_ptr

    def stats_doubles(self):
        return 3 * self.C + 2

    def _key(self):
        return ((self.weights_ptr, self.dice_softmax, self.dice_weight_ptr), self.ignore_index)

    def _args(self, w):
        return (self.logits.msk(), C.c_void_p(self.labels.ptr), C.c_void_p(w), int(self.ignore_index), int(self.dice_softmax),
                C.c_void_p(self.dice_weight_ptr))

    def _forward(self):
        w = self.weights_ptr
        if w is None:  # Dice alone: CE term unused, any weights do
            w = self.dev.arena.alloc(self.C * 4)
            self.dev.h2d(w, np.ones(self.C, dtype=np.float32))
            self._dummy_w = w
        self.dev.call("msk_loss_fwd_ex", *self._args(w), C.c_void_p(self.out_ptr), C.c_void_p(self.stats_ptr))

    def _backward(self, coef_ce, coef_dice, accumulate, dz):
        w = self.weights_ptr if self.weights_ptr is not None else self._dummy_w
        self.dev.call("msk_loss_bwd_ex", *self._args(w), C.c_void_p(self.stats_ptr), C.c_float(coef_ce), C.c_float(coef_dice),
                      dz.msk())


class BCENode(Node):
    """BCELoss evaluation: msk_bce_fwd / msk_bce_bwd.  out[0] is the loss.  `settings` is (ignore_index, weight_mode,
    pos_weight_mode, pos_weight)."""
    SLOTS = {"bce": 0}

    def __init__(self, logits: Tensor, labels: IntTensor, settings):
        super().__init__(logits, labels)
        self.ignore_index, self.weight_mode, self.pos_weight_mode, self.pos_weight = settings

    def stats_doubles(self):
        return 8

    def _forward(self):
        self.dev.call("msk_bce_fwd", self.logits.msk(), C.c_void_p(self.labels.ptr), self.ignore_index, self.weight_mode,
                      self.pos_weight_mode, C.c_float(self.pos_weight), C.c_void_p(self.out_ptr), C.c_void_p(self.stats_ptr))

    def _backward(self, coef, _, accumulate, dz):
        self.dev.call("msk_bce_bwd", self.logits.msk(), C.c_void_p(self.labels.ptr), self.ignore_index,
                      C.c_void_p(self.stats_ptr), C.c_float(coef), accumulate, dz.msk())


REGION_ACTIVATIONS = {"softmax": 0, "sigmoid": 1}
REGION_DICE, REGION_TVERSKY = 0, 1


class RegionNode(Node):
    """Masked soft Dice / Tversky (the 'dice' term, out[1]) and the focal / CE term (the 'ce' term, out[0]):
    msk_region_loss_fwd / msk_region_loss_bwd, one statistics pass and one gradient pass for both terms.  out[2:] is the
    per-class Dice.  `settings` is the tuple (ignore_index, activation, squared_pred, batch_dice, do_bg, mode, smooth, alpha,
    beta, focal_on, gamma) in the order of the C ABI, then the device vector of per-class focal weights or None: two region
    losses on one logits tensor share a node only if every one of them agrees.  With several ranks the batch-Dice sums are
    those of this rank's batch."""
    SLOTS = {"ce": 0, "dice": 1}

    def __init__(self, logits: Tensor, labels: IntTensor, settings):
        super().__init__(logits, labels)
        self.settings, self.weight_ptr = tuple(settings[:-1]), settings[-1]
        self.groups = 1 if self.settings[3] else logits.n

    def stats_doubles(self):
        return 5 * self.groups * self.C + 2

    def _args(self):
        ign, act, sq, batch, bg, mode, smooth, alpha, beta, focal, gamma = self.settings
        return (self.logits.msk(), C.c_void_p(self.labels.ptr), int(ign), int(act), int(sq), int(batch), int(bg), int(mode),
                C.c_float(smooth), C.c_float(alpha), C.c_float(beta), int(focal), C.c_float(gamma), C.c_void_p(self.weight_ptr))

    def _forward(self):
        self.dev.call("msk_region_loss_fwd", *self._args(), C.c_void_p(self.out_ptr), C.c_void_p(self.stats_ptr))

    def _backward(self, coef_f, coef_r, accumulate, dz):
        self.dev.call("msk_region_loss_bwd", *self._args(), C.c_void_p(self.stats_ptr), C.c_float(coef_f), C.c_float(coef_r),
                      accumulate, dz.msk())


class MultiLabelNode(Node):
    """Sigmoid Dice + BCE over label regions (the 'bce' term, out[0], and the 'dice' term, out[1]; out[2:] is the per-region
    Dice): msk_mlabel_loss_fwd / msk_mlabel_loss_bwd, one statistics pass and one gradient pass for both terms.  The channels
    of the logits are the regions; the label stays one int32 per voxel.  `settings` is (ignore_index, squared_pred, batch_dice,
    smooth, table pointer, table length): the device table of uint32 that maps a label value to the bit mask of its regions
    (RegionSpec.device_table).  With several ranks the sums are those of this rank's batch."""
    SLOTS = {"bce": 0, "dice": 1}

    def __init__(self, logits: Tensor, labels: IntTensor, settings):
        super().__init__(logits, labels)
        self.ignore_index, self.squared_pred, self.batch_dice, self.smooth, self.table_ptr, self.table_len = settings
        self.groups = 1 if self.batch_dice else logits.n

    def stats_doubles(self):
        return 5 * self.groups * self.C + 2

    def _args(self):
        return (self.logits.msk(), C.c_void_p(self.labels.ptr), int(self.ignore_index), C.c_void_p(self.table_ptr),
                int(self.table_len), int(self.squared_pred), int(self.batch_dice), C.c_float(self.smooth))

    def _forward(self):
        self.dev.call("msk_mlabel_loss_fwd", *self._args(), C.c_void_p(self.out_ptr), C.c_void_p(self.stats_ptr))

    def _backward(self, coef_bce, coef_dice, accumulate, dz):
        self.dev.call("msk_mlabel_loss_bwd", *self._args(), C.c_void_p(self.stats_ptr), C.c_float(coef_bce), C.c_float(coef_dice),
                      accumulate, dz.msk())


class TopKNode(Node):
    """Top-k cross entropy (the 'topk' term, out[0]): msk_topk_ce_fwd / msk_topk_ce_bwd.  `settings` is (ignore_index, k,
    weight_ptr): k the percentage of the valid voxels that count, weight_ptr the device vector of per-class weights or None.
    The workspace (the per-voxel losses the backward pass compares against the threshold) and the record come from the
    activation arena: they live until the next model forward, like the other records.  K, the threshold and the tie weight
    stay on the device.  With several ranks the selection is that of this rank's batch."""
    SLOTS = {"topk": 0}

    def __init__(self, logits: Tensor, labels: IntTensor, settings):
        super().__init__(logits, labels)
        self.ignore_index, self.k, self.weight_ptr = settings
        self.ws_ptr = None

    def stats_doubles(self):
        return 8

    def _args(self):
        return (self.logits.msk(), C.c_void_p(self.labels.ptr), int(self.ignore_index), C.c_void_p(self.weight_ptr))

    def _forward(self):
        if self.ws_ptr is None:
            nbytes = C.c_size_t(0)
            voxels = self.logits.n * self.logits.d * self.logits.h * self.logits.w
            if self.dev.lib.msk_topk_workspace(C.c_long(voxels), C.byref(nbytes)) != 0:
                raise ValueError("msk_topk_workspace refused %d voxels" % voxels)
            self.ws_ptr = self.dev.arena.alloc(nbytes.value)
        self.dev.call("msk_topk_ce_fwd", *self._args(), C.c_float(self.k), C.c_void_p(self.ws_ptr), C.c_void_p(self.out_ptr),
                      C.c_void_p(self.stats_ptr))

    def _backward(self, coef, _, accumulate, dz):
        self.dev.call("msk_topk_ce_bwd", *self._args(), C.c_void_p(self.ws_ptr), C.c_void_p(self.stats_ptr), C.c_float(coef),
                      accumulate, dz.msk())


LOVASZ_PRESENT, LOVASZ_ALL, LOVASZ_LIST = 0, 1, 2


class LovaszNode(Node):
    """Lovasz-Softmax (the 'lovasz' term, out[0]; out[1] is the number of counted (group, class) pairs, out[2:] the per-class
    means): msk_lovasz_fwd / msk_lovasz_bwd.  `settings` is (ignore_index, class_mode, class_mask, per_image): class_mode one of
    LOVASZ_PRESENT / LOVASZ_ALL / LOVASZ_LIST, class_mask the bits of the listed classes.  The workspace (the sorted keys, the
    permutation and the dL/de planes the backward pass reads) and the record come from the activation arena: they live until the
    next model forward, like the other records.  With several ranks the sort is that of this rank's batch."""
    SLOTS = {"lovasz": 0}

    def __init__(self, logits: Tensor, labels: IntTensor, settings):
        super().__init__(logits, labels)
        self.ignore_index, self.class_mode, self.class_mask, self.per_image = settings
        self.groups = logits.n if self.per_image else 1
        self.ws_ptr = None
        self.ws_bytes = 0

    def stats_doubles(self):
        return 4 * self.groups * self.C + 2

    def _args(self):
        return (self.logits.msk(), C.c_void_p(self.labels.ptr), int(self.ignore_index))

    def _forward(self):
        if self.ws_ptr is None:
            nbytes = C.c_size_t(0)
            voxels = self.logits.n * self.logits.d * self.logits.h * self.logits.w // self.groups
            if self.dev.lib.msk_lovasz_workspace(C.c_long(voxels), self.C, self.groups, C.byref(nbytes)) != 0:
                raise ValueError("msk_lovasz_workspace refused %d groups of %d voxels and %d classes" % (self.groups, voxels, self.C))
            self.ws_ptr, self.ws_bytes = self.dev.arena.alloc(nbytes.value), nbytes.value
        self.dev.call("msk_lovasz_fwd", *self._args(), int(self.class_mode), C.c_uint64(self.class_mask), int(self.per_image),
                      C.c_void_p(self.ws_ptr), C.c_size_t(self.ws_bytes), C.c_void_p(self.out_ptr), C.c_void_p(self.stats_ptr))

    def _backward(self, coef, _, accumulate, dz):
        self.dev.call("msk_lovasz_bwd", *self._args(), int(self.per_image), C.c_void_p(self.ws_ptr), C.c_size_t(self.ws_bytes),
                      C.c_void_p(self.stats_ptr), C.c_float(coef), accumulate, dz.msk())


class BoundaryNode(Node):
    """Boundary loss (the 'boundary' term, out[0]; out[1] is the mean of the absolute terms, out[2:] the per-class means):
    msk_label_sdf, then msk_boundary_loss_fwd / msk_boundary_loss_bwd.  `settings` is (ignore_index, class_mask, spacing):
    class_mask the bits of the classes whose signed distance maps count, spacing a (sz, sy, sx) tuple or None.  The maps are
    built on the device from THIS node's labels (a native deep-supervision head: its own level of the label pyramid) once per
    forward; they and the transform's workspace come from the activation arena and live until the next model forward, like the
    other records.  With several ranks the sums are those of this rank's batch."""
    SLOTS = {"boundary": 0}

    def __init__(self, logits: Tensor, labels: IntTensor, settings):
        super().__init__(logits, labels)
        self.ignore_index, self.class_mask, self.spacing = settings
        self.phi_ptr = None
        self.ws_ptr = None
        self.ws_bytes = 0

    def stats_doubles(self):
        return 3 + self.C

    def _args(self):
        return (self.logits.msk(), C.c_void_p(self.labels.ptr), int(self.ignore_index), C.c_uint64(self.class_mask),
                C.c_void_p(self.phi_ptr))

    def _forward(self):
        t = self.logits
        if self.phi_ptr is None:
            nbytes = C.c_size_t(0)
            if self.dev.lib.msk_sdf_workspace(t.d, t.h, t.w, C.byref(nbytes)) != 0:
                raise ValueError("msk_sdf_workspace refused a volume of %d x %d x %d" % (t.d, t.h, t.w))
            planes = t.n * bin(self.class_mask).count("1")
            self.phi_ptr = self.dev.arena.alloc(planes * t.d * t.h * t.w * 4)
            self.ws_ptr, self.ws_bytes = self.dev.arena.alloc(nbytes.value), nbytes.value
        spacing = None if self.spacing is None else (C.c_double * 3)(*self.spacing)
        self.dev.call("msk_label_sdf", C.c_void_p(self.labels.ptr), t.n, t.d, t.h, t.w, C.c_uint64(self.class_mask), spacing,
                      C.c_void_p(self.ws_ptr), C.c_size_t(self.ws_bytes), C.c_void_p(self.phi_ptr))
        self.dev.call("msk_boundary_loss_fwd", *self._args(), C.c_void_p(self.out_ptr), C.c_void_p(self.stats_ptr))

    def _backward(self, coef, _, accumulate, dz):
        self.dev.call("msk_boundary_loss_bwd", *self._args(), C.c_void_p(self.stats_ptr), C.c_float(coef), accumulate, dz.msk())


_CACHE = {}     # kind -> {key: node}


def node_for(kind, logits: Tensor, labels, settings=()):
    """The node of class `kind` for (logits, labels, settings); a second loss with the same three shares it, and with it the
    forward and the backward pass.  More than 8 nodes of a kind empty that kind's cache alone: the four heads of a
    deep-supervision model scored by two kinds of node stay cached through their step."""
    labels = label_for(logits, labels)
    settings = tuple(settings)
    key = (id(logits), logits.ptr, logits.gen, labels.ptr, tuple(labels.shape)) + settings
    cache = _CACHE.setdefault(kind, {})
    node = cache.get(key)
    if node is None or node.logits is not logits:
        if len(cache) > 8:
            cache.clear()
        node = cache[key] = kind(logits, labels, settings)
    return node


class Scalar:
    """A scalar loss = sum_i coef_i * term_i, term = (node, 'ce' | 'dice' | 'bce' | 'topk' | 'boundary' | 'lovasz'): the float node.slot(which) of the node's
    record.  Values stay on the device until ``numpy()``/``float()`` (one sync), so the train loop can defer host
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
            tot += c * float(v[node.slot(which)])
        return tot

    def numpy(self):
        return np.array([self.value()], dtype=np.float32)

    def item(self):
        return self.value()

    __float__ = value

    def backward(self):
        # coefficients per node and slot, the nodes grouped per logits tensor in term order
        per_logits = {}
        for c, node, which in self.terms:
            group = per_logits.setdefault(id(node.logits), {})
            group.setdefault(id(node), [node, 0.0, 0.0])[1 + node.slot(which)] += c
        # dL/dlogits per evaluated output: the node that writes it first, every other node of the same logits adds into it
        # (or writes it when it is the first).  Then ONE backward per producing model: a multi-output model
        # (VNetDeepSup.num_outputs = 4) receives the list in forward order
        producers = {}
        for group in per_logits.values():
            dz = None
            for node, coef_a, coef_b in sorted(group.values(), key=lambda g: not g[0].writes):
                dz = node.backward(coef_a, coef_b, None if node.writes else dz)
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

"""Inference helpers (reference medicalseg/core/infer.py:62-94): forward + argmax."""
import collections.abc
import ctypes as C
import math

import numpy as np

from .. import nn
from ..device import IntTensor, Tensor, to_tensor


def get_reverse_list(ori_shape, transforms):
    """infer.py:21-40: [('resize', shape before that Resize3D), ...] in application order."""
    reverse_list = []
    d, h, w = ori_shape[0], ori_shape[1], ori_shape[2]
    for op in (transforms or []):
        if op.__class__.__name__ in ['Resize3D']:
            reverse_list.append(('resize', (d, h, w)))
            d, h, w = op.size[0], op.size[1], op.size[2]
    return reverse_list


def reverse_transform(pred, ori_shape, transforms, mode='trilinear'):
    """infer.py:43-59: undo the Resize3D ops of the val transforms on the logits, last one first, with
    F.interpolate(mode='trilinear', align_corners=False) -- the resize kernel of the deep-supervision heads
    (msk_interp_trilinear_fwd).  The reference's own call site passes mode='bilinear', which Paddle rejects for
    5-D input; the function's default mode is what is built, and 'bilinear' is read as it."""
    if mode not in ('trilinear', 'bilinear'):
        raise ValueError("reverse_transform supports mode='trilinear' only, got %r" % (mode,))
    for kind, (d, h, w) in get_reverse_list(ori_shape, transforms)[::-1]:
        if kind != 'resize':
            raise Exception("Unexpected info '{}' in im_info".format(kind))
        if (d, h, w) == (pred.d, pred.h, pred.w):
            continue
        out = Tensor.empty(pred.dev, pred.n, int(d), int(h), int(w), pred.c)
        pred.dev.call("msk_interp_trilinear_fwd", pred.msk(), out.msk())
        pred = out
    return pred


def inference(model, im, ori_shape=None, transforms=None, regions=None):
    """Returns (pred int32 [N,1,D,H,W] on device, logits Tensor); with `ori_shape` different from the logits' and
    Resize3D ops in `transforms`, the logits are resized back first (infer.py:88-90).

    regions (region-based training: a RegionSpec with class_order, e.g. DiceBCERegionLoss.region_spec): the channels are
    sigmoid regions, and the prediction is rebuilt from the thresholded logits in the spec's order (msk_regions_to_label, after
    the resize back) instead of the argmax.

    An eval-mode model runs its conv -> BN -> PReLU units as single folded convolutions here
    (nn.fused_inference); a model left in training mode runs the ordinary kernels."""
    with nn.fused_inference():
        logit = _forward(model, im)
    return _finish(logit, ori_shape, transforms, regions)


# ---- what the three prediction paths (inference, aug_inference, sliding_window_inference) share ------------------------------
def _forward(model, x):
    """model(x)[0], the full-resolution logits"""
    logits = model(x)
    if not isinstance(logits, collections.abc.Sequence):
        raise TypeError("The type of logits must be one of collections.abc.Sequence, e.g. list, tuple. "
                        "But received {}".format(type(logits)))
    return logits[0]


def _new_pred(logit):
    """an int32 [N,1,D,H,W] prediction for `logit` in the activation arena, not yet written"""
    dev = logit.dev
    return IntTensor(dev, dev.arena.alloc(logit.voxels * 4), (logit.n, 1, logit.d, logit.h, logit.w), dev.arena.gen)


def _finish(logit, ori_shape, transforms, regions=None):
    """-> (pred, logit): the logits (or probabilities) resized back when `ori_shape` differs from their extent, then their
    argmax, or with `regions` (a RegionSpec) the label map rebuilt from the thresholded region logits"""
    if ori_shape is not None and tuple(ori_shape) != tuple(logit.shape[2:]):
        logit = reverse_transform(logit, ori_shape, transforms, mode='bilinear')
    if regions is not None:
        return regions.to_label(logit), logit
    pred = _new_pred(logit)
    logit.dev.call("msk_argmax_c", logit.msk(), C.c_void_p(pred.ptr))
    return pred, logit


def _kept(dev, key, n, d, h, w, c):
    """The persistent device tensor under `key` in dev.kept, outside the activation arena (every model forward resets the
    arena): allocated on first use, reused while the shape asked for is the one kept, freed and replaced when it is not.  A
    key that contains the shape therefore keeps one buffer per shape, a key without it one buffer."""
    shape = (int(n), int(d), int(h), int(w), int(c))
    t = dev.kept.get(key)
    if t is not None and (t.n, t.d, t.h, t.w, t.c) != shape:
        dev.free(dev.kept.pop(key).ptr)
        t = None
    if t is None:
        t = dev.kept[key] = Tensor.empty(dev, *shape, arena=False)
    return t


def _release(dev, family):
    """free what dev.kept holds under the keys (family, ...), in the order it was allocated, and nothing else"""
    for key in [k for k in dev.kept if k[0] == family]:
        v = dev.kept.pop(key)
        for p in (v[1] if isinstance(v, tuple) else [v.ptr]):      # (plan, table pointers), or a Tensor
            dev.free(p)


def _copy_into(kept, t):
    """`t` copied into the kept buffer of its shape (msk_flip_axes mirroring no axis) -> kept"""
    t.dev.call("msk_flip_axes", t.msk(), kept.msk(), 0)
    return kept


def _restamp(kept):
    """A kept buffer stamped like an activation of the last forward: stale after the next one, a new object per call."""
    return Tensor(kept.dev, kept.ptr, kept.n, kept.d, kept.h, kept.w, kept.c, kept.c, kept.dev.arena.gen)


# ----------------------------------------------------------------------------------------
# test-time augmentation (the reference's infer.py ends with "todo: add aug inference"; the 2D library it was cut from has
# aug_inference(scales, flip_horizontal, flip_vertical))
# ----------------------------------------------------------------------------------------
def tta_passes(scales=1.0, flip_axes=()):
    """The forward passes of one augmented prediction as an ordered list of (scale, mask): the scales in the given order (a
    bare number is one scale), within a scale every subset of `flip_axes` in increasing mask order, mask 0 first.  Axis
    numbers are 0/1/2 = D/H/W, bit a of the mask mirrors axis a (msk_flip_axes)."""
    if isinstance(scales, (int, float)):
        scales = [scales]
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError("tta_passes: scales is empty")
    for s in scales:
        if not s > 0.0:
            raise ValueError("tta_passes: scales must be positive, got %r" % (s,))
    axes = list(flip_axes)
    for a in axes:
        if not isinstance(a, (int, np.integer)) or isinstance(a, bool) or a < 0 or a > 2:
            raise ValueError("tta_passes: flip_axes are 0, 1 or 2 (D, H, W), got %r" % (a,))
    if len(set(axes)) != len(axes):
        raise ValueError("tta_passes: duplicate axis in flip_axes %r" % (tuple(axes),))
    bits = sum(1 << a for a in axes)
    masks = [m for m in range(8) if m & ~bits == 0]
    return [(s, m) for s in scales for m in masks]


def tta_size(shape, scale):
    """Extent of a rescaled pass: int(dim * scale + 0.5) per axis (the 2D library's rule), at least 1."""
    return tuple(max(1, int(int(v) * float(scale) + 0.5)) for v in shape)


def _tta_buffer(dev, role, n, d, h, w, c):
    """A persistent device tensor per (role, shape), outside the activation arena: every model forward resets the arena, and
    the accumulator, the kept plain logits and the mirrored / resized inputs have to outlive one.  After the first
    aug_inference at a shape no call allocates device memory; tta_release frees the buffers."""
    return _kept(dev, ("tta", role, int(n), int(d), int(h), int(w), int(c)), n, d, h, w, c)


def tta_release(dev):
    """Free the persistent buffers of aug_inference on `dev` (they are kept per shape, for the device's lifetime otherwise)."""
    _release(dev, "tta")


def aug_inference(model, im, ori_shape=None, transforms=None, scales=1.0, flip_axes=(), with_plain=False, regions=None):
    """Flip- and scale-averaged prediction: one forward per pass of tta_passes(scales, flip_axes), the softmax of every pass
    mirrored back and summed on the device in pass order (msk_tta_accumulate: no mirrored copy, no probabilities in
    between), then the mean and its argmax (msk_tta_finish).  A pass at scale != 1 resizes `im` to tta_size with the
    trilinear kernel of reverse_transform, and its logits back to `im`'s extent, before they are accumulated.

    Returns (pred IntTensor [N,1,D,H,W], probs Tensor).  `probs` is the MEAN softmax over the passes; the 2D library's
    aug_inference returns their sum, which has the same argmax.  With `ori_shape` different from `im`'s extent and Resize3D
    ops in `transforms`, the mean probabilities are resized back (reverse_transform) and the argmax is taken after that.
    with_plain=True adds a third value: the logits of the unscaled, unmirrored pass at `im`'s extent -- what `inference`
    computes before its reverse_transform -- and needs 1.0 among `scales`.

    Runs in one nn.fused_inference scope.  The returned tensors are valid until the next forward, as inference()'s are.
    A model's own errors at sizes it cannot run (a scaled extent its strides do not divide) propagate unchanged.

    What is averaged are softmax probabilities, which region-based (sigmoid) channels do not have: `regions` raises ValueError
    (sliding_window_inference(mirror_axes=...) averages logits and takes regions)."""
    if regions is not None:
        raise ValueError("aug_inference averages softmax probabilities and does not support regions; "
                         "use sliding_window_inference(mirror_axes=..., regions=...)")
    passes = tta_passes(scales, flip_axes)
    if with_plain and (1.0, 0) not in passes:
        raise ValueError("aug_inference(with_plain=True) needs 1.0 among scales, got %r" % (scales,))
    if not isinstance(im, Tensor):
        im = to_tensor(im)
    dev = im.dev
    extent = (im.d, im.h, im.w)
    acc = plain = None
    with nn.fused_inference():
        for k, (scale, mask) in enumerate(passes):
            x = im
            if scale != 1.0:
                x = _tta_buffer(dev, "resized", im.n, *tta_size(extent, scale), im.c)
                dev.call("msk_interp_trilinear_fwd", im.msk(), x.msk())
            if mask:
                xf = _tta_buffer(dev, "mirrored", x.n, x.d, x.h, x.w, x.c)
                dev.call("msk_flip_axes", x.msk(), xf.msk(), mask)
                x = xf
            logit = _forward(model, x)
            if scale != 1.0:
                back = Tensor.empty(dev, logit.n, extent[0], extent[1], extent[2], logit.c)
                dev.call("msk_interp_trilinear_fwd", logit.msk(), back.msk())
                logit = back
            if acc is None:
                acc = _tta_buffer(dev, "acc", logit.n, logit.d, logit.h, logit.w, logit.c)
            if with_plain and plain is None and scale == 1.0 and mask == 0:
                plain = _copy_into(_tta_buffer(dev, "plain", logit.n, logit.d, logit.h, logit.w, logit.c), logit)
            dev.call("msk_tta_accumulate", logit.msk(), mask, acc.msk(), 1 if k == 0 else 0)
    if plain is not None:
        plain = _restamp(plain)
    probs = Tensor.empty(dev, acc.n, acc.d, acc.h, acc.w, acc.c)
    if ori_shape is not None and tuple(ori_shape) != tuple(probs.shape[2:]):
        dev.call("msk_tta_finish", acc.msk(), len(passes), probs.msk(), None)
        pred, probs = _finish(probs, ori_shape, transforms)
    else:                      # nothing to resize: the mean and its argmax in one pass
        pred = _new_pred(probs)
        dev.call("msk_tta_finish", acc.msk(), len(passes), probs.msk(), C.c_void_p(pred.ptr))
    return (pred, probs, plain) if with_plain else (pred, probs)


# ----------------------------------------------------------------------------------------
# sliding-window inference: the net on overlapping roi_size windows at native resolution, blended with a window weight that
# falls off towards the window border (the reference has it in its nnunet subtree only, not in the VNet path)
# ----------------------------------------------------------------------------------------
class SlidingPlan:
    """Everything of a sliding-window prediction that depends only on geometry: one volume extent (D, H, W), one roi_size
    (rd, rh, rw).  Per axis, with `size` the volume extent and `r` the window extent:

      padded extent   P = max(size, r); a volume smaller than the window is padded with before = (r - size) // 2 voxels in
                      front and the rest behind.  The padding is implicit (msk_sw_gather fills it, msk_sw_accumulate skips it).
      window starts   in padded coordinates: [0] if P == r, else interval = max(1, int(r * (1 - overlap))),
                      num = ceil((P - r) / interval) + 1, start_i = min(i * interval, P - r).
      profile         g[k], float64: 1 ('constant') or exp(-0.5 * ((k - (r - 1) / 2) / (sigma_scale * r)) ** 2) ('gaussian').
      coverage        S[p] = sum over the windows that contain p of g[p - start_i], float64, in window order.
      table           T[i][k] = float32(g[k] / S[start_i + k]), one row per window start.

    The windows are the full product of the three start lists and the 3-D weight is the product of the three profiles, so
    the 3-D coverage is the product of the three S: normalising per axis normalises the blend, and no weight-sum volume, no
    division and no finish pass exist anywhere.

    Attributes: shape, roi_size, overlap, mode, sigma_scale, padded, before, starts (three lists), tables (three float32
    arrays [len(starts[a]), roi_size[a]]).  ValueError: overlap outside [0, 1), a non-positive roi_size or shape, an unknown
    mode, a coverage of zero or a table entry that is zero, subnormal or not finite (a sigma_scale so small that the profile
    underflows)."""

    def __init__(self, shape, roi_size, overlap=0.5, mode='gaussian', sigma_scale=0.125):
        shape, roi_size = tuple(shape), tuple(roi_size)
        if len(shape) != 3 or len(roi_size) != 3:
            raise ValueError("SlidingPlan: shape and roi_size are (D, H, W) triples, got %r and %r" % (shape, roi_size))
        for v in shape + roi_size:
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1:
                raise ValueError("SlidingPlan: shape and roi_size must be positive integers, got %r and %r" % (shape, roi_size))
        overlap = float(overlap)
        if not 0.0 <= overlap < 1.0:
            raise ValueError("SlidingPlan: overlap must satisfy 0 <= overlap < 1, got %r" % (overlap,))
        if mode not in ('constant', 'gaussian'):
            raise ValueError("SlidingPlan: mode is 'constant' or 'gaussian', got %r" % (mode,))
        if mode == 'gaussian' and not float(sigma_scale) > 0.0:
            raise ValueError("SlidingPlan: sigma_scale must be positive, got %r" % (sigma_scale,))
        self.shape = tuple(int(v) for v in shape)
        self.roi_size = tuple(int(v) for v in roi_size)
        self.overlap, self.mode, self.sigma_scale = overlap, mode, float(sigma_scale)
        self.padded, self.before, self.starts, self.tables = [], [], [], []
        tiny = np.finfo(np.float32).tiny
        for size, r in zip(self.shape, self.roi_size):
            P = max(size, r)
            if P == r:
                starts = [0]
            else:
                interval = max(1, int(r * (1 - overlap)))
                num = -(-(P - r) // interval) + 1
                starts = [min(i * interval, P - r) for i in range(num)]
            with np.errstate(all='ignore'):
                if mode == 'constant':
                    g = np.ones(r, np.float64)
                else:
                    # math.exp, the C library's: numpy's vector exp may differ from it in the last bit
                    g = np.array([math.exp(-0.5 * ((k - (r - 1) / 2) / (self.sigma_scale * r)) ** 2) for k in range(r)])
                S = np.zeros(P, np.float64)
                for s in starts:
                    S[s:s + r] += g
                if not (S != 0).all():
                    raise ValueError("SlidingPlan: a voxel has zero window weight (sigma_scale = %r underflows at extent %d)"
                                     % (sigma_scale, r))
                T = np.stack([(g / S[s:s + r]).astype(np.float32) for s in starts])
            if not (np.isfinite(T).all() and (T >= tiny).all()):
                raise ValueError("SlidingPlan: a window weight is zero, subnormal or not finite (sigma_scale = %r at extent %d)"
                                 % (sigma_scale, r))
            self.padded.append(P)
            self.before.append((r - size) // 2 if size < r else 0)
            self.starts.append(starts)
            self.tables.append(T)
        self.padded, self.before = tuple(self.padded), tuple(self.before)

    @property
    def key(self):
        return (self.shape, self.roi_size, self.overlap, self.mode, self.sigma_scale)

    def windows(self, n=1):
        """The windows of a batch of n volumes in order: batch item slowest, then the d, h and w starts, w fastest; each is
        (n, id, ih, iw), indices into the three start lists."""
        nd, nh, nw = (len(s) for s in self.starts)
        return [(b, i, j, k) for b in range(int(n)) for i in range(nd) for j in range(nh) for k in range(nw)]

    def origin(self, window):
        """(n, d0, h0, w0): the window's first voxel in VOLUME coordinates, start - before per axis; may be negative, and the
        window may run past the end of the volume"""
        b, i, j, k = window
        return (b, self.starts[0][i] - self.before[0], self.starts[1][j] - self.before[1], self.starts[2][k] - self.before[2])


def _sw_buffer(dev, role, n, d, h, w, c):
    """The persistent device tensor of a role (the patch batch, the accumulator, the kept input) outside the activation arena:
    they have to outlive the forwards.  One per role: a call at the same shape reuses it and allocates nothing, a call at
    another shape frees it first -- native-resolution volumes differ in extent, and a whole-volume accumulator per distinct
    extent (0.9 GB at 300 x 512 x 512, C = 3) would otherwise stay for the device's lifetime.  sliding_release frees them."""
    return _kept(dev, ("sw", role), n, d, h, w, c)


def _sw_plan(dev, shape, roi_size, overlap, mode, sigma_scale):
    """-> (SlidingPlan, [td, th, tw] device pointers): the plan of a geometry and its three tables, uploaded once"""
    key = ("sw", "plan", tuple(int(v) for v in shape), tuple(roi_size), float(overlap), mode, float(sigma_scale))
    hit = dev.kept.get(key)
    if hit is None:
        plan = SlidingPlan(shape, roi_size, overlap, mode, sigma_scale)
        ptrs = []
        for T in plan.tables:
            p = dev.malloc(T.nbytes)
            dev.h2d(p, T)
            ptrs.append(p)
        hit = dev.kept[key] = (plan, ptrs)
    return hit


def sliding_release(dev):
    """Free the persistent buffers and plan tables of sliding_window_inference on `dev`.  The buffers are one per role (see
    _sw_buffer); the plans with their three small device tables are kept per geometry, for the device's lifetime otherwise.
    The `logits` an earlier call returned IS the accumulator freed here: it must not be used after a release (its liveness
    check cannot know; until the next forward it still passes)."""
    _release(dev, "sw")


def sliding_window_inference(model, im, roi_size, overlap=0.5, mode='gaussian', sigma_scale=0.125, sw_batch_size=1, cval=0.0,
                             ori_shape=None, transforms=None, mirror_axes=(), regions=None):
    """Window-by-window prediction at native resolution: the net runs on the overlapping `roi_size` windows of SlidingPlan
    (`overlap`, implicit padding with `cval` where the volume is smaller than the window), sw_batch_size windows per forward
    (the last batch may be smaller), and the outputs are blended on the device with the plan's normalised window weights
    (mode 'gaussian' or 'constant'): msk_sw_gather -> model(patches)[0] -> msk_sw_accumulate per batch, in window order.

    Returns (pred IntTensor [N,1,D,H,W], logits Tensor [N,C,D,H,W]), the pair inference() returns, so a caller can swap one
    for the other.  What is blended are the LOGITS (the network's output), not probabilities: evaluate's loss and mdice need
    whole-volume logits, and the softmax / AUC / argmax downstream then work unchanged.  `logits` is the persistent
    accumulator itself, stamped with the arena generation of the last forward: no copy, valid until the next forward, as
    inference()'s are.  With `ori_shape` different from `im`'s extent and Resize3D ops in `transforms`, the blended logits are
    resized back (reverse_transform) and the argmax is taken after that, as inference() does.

    Runs in one nn.fused_inference scope.  The plan with its device tables, the patch batch, the accumulator and (if `im`
    lives in the activation arena, which every forward resets) a copy of `im` are persistent buffers: a second call at the
    same shapes allocates no device memory, a call at other shapes frees and replaces the buffers whose shape changed (so
    `logits` of an earlier call is gone then, as it is after the next forward); sliding_release frees them.

    mirror_axes (0/1/2 = D/H/W; nnU-Net's mirroring inside the sliding window): every window is also shown to the net mirrored
    about the WINDOW along every subset of the axes -- the K = 1, 2, 4 or 8 masks of tta_passes(1.0, mirror_axes), mask 0
    first -- and the mean of the K outputs, mirrored back, is what is blended (tests/sliding_mirror_reference.py).  The passes
    are the list [(window, mask) for window in windows for mask in masks]; sw_batch_size then counts PASSES per forward, and a
    window's passes may straddle two forwards: msk_sw_gather_mirrored -> model(patches)[0] -> one
    msk_sw_accumulate_mirrored(scale = 1 / K) per batch.  Every pass is one add at a fixed place in the sequence, so the
    result does not depend on sw_batch_size.  Without mirror_axes the calls are those described above, unchanged.

    regions (a RegionSpec with class_order): the prediction is rebuilt from the thresholded blended logits
    (msk_regions_to_label) instead of their argmax, as in inference(); what is blended and mirrored stays the logits."""
    if not isinstance(sw_batch_size, (int, np.integer)) or isinstance(sw_batch_size, bool) or sw_batch_size < 1:
        raise ValueError("sliding_window_inference: sw_batch_size must be a positive integer, got %r" % (sw_batch_size,))
    masks = [m for _, m in tta_passes(1.0, mirror_axes)]
    mirrored = len(masks) > 1
    if not isinstance(im, Tensor):
        im = to_tensor(im)
    dev = im.dev
    plan, (td, th, tw) = _sw_plan(dev, (im.d, im.h, im.w), roi_size, overlap, mode, sigma_scale)
    rd, rh, rw = plan.roi_size
    if im.gen is not None:          # an activation: the first forward would reset the arena under it
        im = _copy_into(_sw_buffer(dev, "im", im.n, im.d, im.h, im.w, im.c), im)
    work = [(wd, m) for wd in plan.windows(im.n) for m in masks]          # the passes: one per window without mirror_axes
    batch = min(int(sw_batch_size), len(work))
    patches = _sw_buffer(dev, "patches", batch, rd, rh, rw, im.c)
    rows = [C.c_int(len(s)) for s in plan.starts]
    acc = None
    with nn.fused_inference():
        for k in range(0, len(work), batch):
            group = work[k:k + batch]
            origins = np.array([plan.origin(wd) + wd[1:] + (m,) for wd, m in group], np.int32)
            x = patches if len(group) == batch else Tensor(dev, patches.ptr, len(group), rd, rh, rw, im.c)
            if mirrored:
                corners = np.ascontiguousarray(origins[:, [0, 1, 2, 3, 7]])
                dev.call("msk_sw_gather_mirrored", im.msk(), x.msk(), corners.ctypes.data_as(C.c_void_p), C.c_float(cval))
            else:
                origins = np.ascontiguousarray(origins[:, :7])
                corners = np.ascontiguousarray(origins[:, :4])
                dev.call("msk_sw_gather", im.msk(), x.msk(), corners.ctypes.data_as(C.c_void_p), C.c_float(cval))
            logit = _forward(model, x)
            if (logit.n, logit.d, logit.h, logit.w) != (len(group), rd, rh, rw):
                raise ValueError("sliding_window_inference: the model maps a window batch of extent %r to %r; the logits "
                                 "must keep the window's extent" % ((len(group), rd, rh, rw), (logit.n, logit.d, logit.h, logit.w)))
            if acc is None:
                acc = _sw_buffer(dev, "acc", im.n, im.d, im.h, im.w, logit.c)
                dev.memset(acc.ptr, 0, acc.voxels * acc.c * 4)
            if mirrored:        # the kernel finds a window's passes among the rows and adds them in one launch
                dev.call("msk_sw_accumulate_mirrored", logit.msk(), origins.ctypes.data_as(C.c_void_p), C.c_void_p(td), rows[0],
                         C.c_void_p(th), rows[1], C.c_void_p(tw), rows[2], C.c_float(1.0 / len(masks)), acc.msk())
            else:
                dev.call("msk_sw_accumulate", logit.msk(), origins.ctypes.data_as(C.c_void_p), C.c_void_p(td), rows[0],
                         C.c_void_p(th), rows[1], C.c_void_p(tw), rows[2], acc.msk())
    return _finish(_restamp(acc), ori_shape, transforms, regions)

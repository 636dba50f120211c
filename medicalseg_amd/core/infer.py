"""Inference helpers (reference medicalseg/core/infer.py:62-94): forward + argmax."""
import collections.abc
import ctypes as C

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


def inference(model, im, ori_shape=None, transforms=None):
    """Returns (pred int32 [N,1,D,H,W] on device, logits Tensor); with `ori_shape` different from the logits' and
    Resize3D ops in `transforms`, the logits are resized back first (infer.py:88-90).

    An eval-mode model runs its conv -> BN -> PReLU units as single folded convolutions here
    (nn.fused_inference); a model left in training mode runs the ordinary kernels."""
    with nn.fused_inference():
        logits = model(im)
    if not isinstance(logits, collections.abc.Sequence):
        raise TypeError("The type of logits must be one of collections.abc.Sequence, e.g. list, tuple. "
                        "But received {}".format(type(logits)))
    logit = logits[0]
    if ori_shape is not None and tuple(ori_shape) != tuple(logit.shape[2:]):
        logit = reverse_transform(logit, ori_shape, transforms, mode='bilinear')
    dev = logit.dev
    ptr = dev.arena.alloc(logit.voxels * 4)
    dev.call("msk_argmax_c", logit.msk(), C.c_void_p(ptr))
    pred = IntTensor(dev, ptr, (logit.n, 1, logit.d, logit.h, logit.w), dev.arena.gen)
    return pred, logit


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
    cache = dev.__dict__.setdefault("_tta_buffers", {})
    key = (role, int(n), int(d), int(h), int(w), int(c))
    t = cache.get(key)
    if t is None:
        t = cache[key] = Tensor.empty(dev, n, d, h, w, c, arena=False)
    return t


def tta_release(dev):
    """Free the persistent buffers of aug_inference on `dev` (they are kept per shape, for the device's lifetime otherwise)."""
    for t in dev.__dict__.pop("_tta_buffers", {}).values():
        dev.free(t.ptr)


def aug_inference(model, im, ori_shape=None, transforms=None, scales=1.0, flip_axes=(), with_plain=False):
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
    A model's own errors at sizes it cannot run (a scaled extent its strides do not divide) propagate unchanged."""
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
            logits = model(x)
            if not isinstance(logits, collections.abc.Sequence):
                raise TypeError("The type of logits must be one of collections.abc.Sequence, e.g. list, tuple. "
                                "But received {}".format(type(logits)))
            logit = logits[0]
            if scale != 1.0:
                back = Tensor.empty(dev, logit.n, extent[0], extent[1], extent[2], logit.c)
                dev.call("msk_interp_trilinear_fwd", logit.msk(), back.msk())
                logit = back
            if acc is None:
                acc = _tta_buffer(dev, "acc", logit.n, logit.d, logit.h, logit.w, logit.c)
            if with_plain and plain is None and scale == 1.0 and mask == 0:
                plain = _tta_buffer(dev, "plain", logit.n, logit.d, logit.h, logit.w, logit.c)
                dev.call("msk_flip_axes", logit.msk(), plain.msk(), 0)
            dev.call("msk_tta_accumulate", logit.msk(), mask, acc.msk(), 1 if k == 0 else 0)
    if plain is not None:      # stamped like an activation of the last forward: stale after the next one, a new object per call
        plain = Tensor(dev, plain.ptr, plain.n, plain.d, plain.h, plain.w, plain.c, plain.c, dev.arena.gen)
    probs = Tensor.empty(dev, acc.n, acc.d, acc.h, acc.w, acc.c)
    resize = ori_shape is not None and tuple(ori_shape) != tuple(probs.shape[2:])
    if resize:
        dev.call("msk_tta_finish", acc.msk(), len(passes), probs.msk(), None)
        probs = reverse_transform(probs, ori_shape, transforms, mode='bilinear')
    ptr = dev.arena.alloc(probs.voxels * 4)
    if resize:
        dev.call("msk_argmax_c", probs.msk(), C.c_void_p(ptr))
    else:
        dev.call("msk_tta_finish", acc.msk(), len(passes), probs.msk(), C.c_void_p(ptr))
    pred = IntTensor(dev, ptr, (probs.n, 1, probs.d, probs.h, probs.w), dev.arena.gen)
    return (pred, probs, plain) if with_plain else (pred, probs)

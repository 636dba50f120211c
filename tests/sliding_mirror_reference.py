"""The numpy statement of mirroring inside sliding-window inference (core/infer.py sliding_window_inference(mirror_axes=...),
msk_sw_gather_mirrored / msk_sw_accumulate_mirrored of csrc/msk_sliding.hip), on top of sliding_reference (plan, crop, the
unmirrored blend) and tta_reference (flip).

Masks are msk_flip_axes': bit 0 = D, bit 1 = H, bit 2 = W, m_a(i) = r_a - 1 - i where bit a is set and i where it is not, r_a
the WINDOW's extent.  A volume smaller than the window has asymmetric implicit padding: the mirror is about the window.
Passes: every subset of the chosen axes in increasing mask order, mask 0 first (K = 1, 2, 4 or 8); the work list is
[(window, mask) for window in windows for mask in masks]; scale = float32(1 / K), an exact power of two.
Gather:  patch = flip(crop_with_padding(vol, window, cval), mask): the padding is mirrored with the content.
Blend, float32, one rounding per operation, never an FMA, over the work list in order; for every voxel of the window inside the
volume, at window-local (z, y, x) in the VOLUME frame, and every channel c:
    w   = (Td[id][z] * Th[ih][y]) * Tw[iw][x]              tables indexed un-mirrored
    ws  = w * scale
    acc = acc + (ws * logit_pass[m_D(z)][m_H(y)][m_W(x)][c])
Every pass is one add at a fixed place in the sequence: the result does not depend on how the passes are batched.  All arrays are
NCDHW."""
import numpy as np

import sliding_reference as R
import tta_reference as T


def masks_of(mirror_axes):
    bits = sum(1 << a for a in mirror_axes)
    return [m for m in range(8) if m & ~bits == 0]


def work(plan, n, masks):
    """the passes in order: (window, mask)"""
    return [(wd, m) for wd in plan.windows(n) for m in masks]


def gather(vol, plan, window, mask, cval=0.0):
    """the window of an NCDHW volume as pass `mask` sees it -> [C, rd, rh, rw]"""
    return T.flip(R.crop(vol, plan, window, cval)[None], mask)[0]


def gathers(vol, plan, masks, cval=0.0):
    """every pass of the volume batch, in work order"""
    return [gather(vol, plan, wd, m, cval) for wd, m in work(plan, np.asarray(vol).shape[0], masks)]


def blend(pass_logits, plan, passes, scale, n=1, acc=None):
    """pass_logits[i]: [C, rd, rh, rw] logits of pass i in ITS (mirrored) frame; passes[i] = (window, mask); scale: the factor
    of every pass -> acc [n, C, D, H, W].  `acc`: start from this array instead of zeros (it is not modified)."""
    assert len(pass_logits) == len(passes)
    scale = np.float32(scale)
    c = np.asarray(pass_logits[0]).shape[0]
    acc = np.zeros((n, c) + plan.shape, np.float32) if acc is None else np.array(acc, np.float32)
    td, th, tw = plan.tables
    for lg, (wd, mask) in zip(pass_logits, passes):
        lg = T.flip(np.asarray(lg, np.float32)[None], mask)[0]                 # lg[m_D(z)][m_H(y)][m_W(x)] at (z, y, x)
        b, d0, h0, w0 = plan.origin(wd)
        wzy = (td[wd[1]][:, None] * th[wd[2]][None, :]).astype(np.float32)
        w = (wzy[:, :, None] * tw[wd[3]][None, None, :]).astype(np.float32)
        ws = (w * scale).astype(np.float32)
        (z0, z1), (y0, y1), (x0, x1) = (R._overlap(o, r, s) for o, r, s in zip((d0, h0, w0), plan.roi, plan.shape))
        part = (ws[None, z0:z1, y0:y1, x0:x1] * lg[:, z0:z1, y0:y1, x0:x1]).astype(np.float32)
        view = acc[b, :, d0 + z0:d0 + z1, h0 + y0:h0 + y1, w0 + x0:w0 + x1]
        view[...] = (view + part).astype(np.float32)
    return acc


def predict(f, vol, plan, mirror_axes, cval=0.0):
    """the whole statement with a host model f (NCDHW -> NCDHW, applied to every pass on its own) -> blended logits"""
    vol = np.asarray(vol, np.float32)
    masks = masks_of(mirror_axes)
    passes = work(plan, vol.shape[0], masks)
    out = [f(gather(vol, plan, wd, m, cval)[None])[0] for wd, m in passes]
    return blend(out, plan, passes, np.float32(1) / np.float32(len(masks)), vol.shape[0])

"""Device counterparts of medicalseg/models/losses/loss_utils.py."""
import ctypes as C

import numpy as np

from ...device import Tensor


def class_weights(tensor: Tensor):
    """w_c = sum(1 - softmax_c) / sum(softmax_c) over all voxels (reference
    loss_utils.py:31-40); returns a persistent device pointer (the reference caches it)."""
    dev = tensor.dev
    ptr = dev.small(tensor.c)
    dev.call("msk_class_weights", tensor.msk(), C.c_void_p(ptr))
    return ptr


def device_weights(dev, weight: np.ndarray, held, small=False):
    """The per-class vector `weight` (float32) on `dev`, uploaded once per device.  `held` is what the last call returned (or
    None); returns the (device, pointer) pair to hold on to.  small: the buffer comes from dev.small (zeroed, kept in the
    device's list) instead of dev.malloc."""
    if held is None or held[0] is not dev:
        ptr = dev.small(weight.size) if small else dev.malloc(max(weight.size, 4) * 4)
        dev.h2d(ptr, weight)
        held = (dev, ptr)
    return held


def flatten(tensor: Tensor):
    """(N, C, D, H, W) -> (C, N*D*H*W) on the host (reference loss_utils.py:18-28); only for
    inspection -- the fused loss kernel never materialises it."""
    a = tensor.numpy()
    return np.moveaxis(a, 1, 0).reshape(a.shape[1], -1)

"""Shared helpers for the GPU parity tests (call the C ABI through medicalseg_amd).

Every buffer these helpers hand out sits between two red zones inside one device allocation:

    base | GUARD bytes of SENTINEL | payload (nbytes, rounded up to 256) | GUARD bytes of SENTINEL

and a tensor with a voxel stride wider than its channel count (``ld > c``) has its pad channels filled with a known bit
pattern as well.  ``assert_redzones_intact()`` reads all of that back and compares it bit for bit, so a kernel that stores
outside its tensor turns into an assertion that names the buffer; a kernel that loads outside its tensor, or a view read as
dense, pulls the quiet-NaN SENTINEL into its arithmetic and fails the parity check; and an output element that is never
written reads back as NaN (``t_empty`` without ``fill``).  GPU test modules run the check after every test through the
``redzone_check`` fixture below (imported into the module; it is autouse there).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

# 64 KiB on each side: the widest row a kernel stores at once is a 32-voxel tile at 256 channels (32 KiB), this is twice that;
# and a multiple of 256, so the payload keeps the allocator's alignment and no float4 / alignment dispatch predicate changes.
GUARD = 64 * 1024
ALIGN = 256
SENTINEL_BITS = 0x7FC0BEEF          # quiet NaN with a recognisable payload
SENTINEL = np.array([SENTINEL_BITS], dtype=np.uint32).view(np.float32)[0]

_registry = []                      # one dict per guarded allocation not checked yet, see dmalloc()
_bases = {}                         # payload pointer -> base of every guarded allocation still allocated (dfree)


def dev():
    from medicalseg_amd.device import get_device
    return get_device()


def _tensor(*args):
    from medicalseg_amd.device import Tensor
    return Tensor(*args)


def _roundup(n, m):
    return (int(n) + m - 1) // m * m


def _call_site():
    f = sys._getframe(1)
    here = os.path.abspath(__file__)
    while f is not None and os.path.abspath(f.f_code.co_filename) == here:
        f = f.f_back
    if f is None:
        return "?"
    return "%s:%d in %s" % (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


def _guarded(nbytes, label, write=None, tensor=None):
    """One allocation GUARD + roundup(nbytes, 256) + GUARD, SENTINEL everywhere except what `write` (called with the payload
    as a flat float32 host view, or None) puts into the payload, sent in one h2d.  Returns the payload pointer."""
    d = dev()
    nbytes = int(nbytes)
    total = GUARD + _roundup(nbytes, ALIGN) + GUARD
    host = np.full(total // 4, SENTINEL_BITS, dtype=np.uint32)
    if write is not None and nbytes:
        write(host[GUARD // 4:(GUARD + nbytes) // 4].view(np.float32))
    base = d.malloc(total)
    d.h2d(base, host)
    _registry.append({"base": base, "offset": GUARD, "nbytes": nbytes, "total": total,
                      "label": label or _call_site(), "tensor": tensor})
    _bases[base + GUARD] = base
    return base + GUARD


def dmalloc(nbytes, label=None):
    """Guarded device allocation of nbytes (payload SENTINEL-filled); the tail red zone starts at payload + nbytes."""
    return _guarded(nbytes, label or "%s dmalloc(%d)" % (_call_site(), int(nbytes)))


def _bits(value):
    return int(np.array([value], dtype=np.float32).view(np.uint32)[0])


def t_from_ncdhw(a, ld=None):
    """numpy NCDHW -> persistent device Tensor (NDHWC, optional wider voxel stride; the pad channels hold SENTINEL)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, c, D, H, W = a.shape
    ld = ld or c

    def write(payload):
        payload.reshape(n, D, H, W, ld)[..., :c] = np.moveaxis(a, 1, -1)

    label = "%s t_from_ncdhw(shape=%s, c=%d, ld=%d)" % (_call_site(), (n, D, H, W), c, ld)
    ptr = _guarded(n * D * H * W * ld * 4, label, write, {"vox": n * D * H * W, "c": c, "ld": ld, "pad_bits": SENTINEL_BITS})
    return _tensor(dev(), ptr, n, D, H, W, c, ld, None)


def t_empty(n, c, D, H, W, ld=None, fill=None, pads_owned=True):
    """Device Tensor whose payload (pad channels included) holds `fill`, or SENTINEL when fill is None: an output element
    that no kernel writes then shows as NaN.  pads_owned=False: the test writes the pad channels through a second Tensor,
    so only the guards are checked."""
    ld = ld or c
    vox = n * D * H * W
    write = None if fill is None else (lambda payload: payload.fill(fill))
    pad_bits = SENTINEL_BITS if fill is None else _bits(fill)
    label = "%s t_empty(shape=%s, c=%d, ld=%d)" % (_call_site(), (n, D, H, W), c, ld)
    tensor = {"vox": vox, "c": c, "ld": ld, "pad_bits": pad_bits} if pads_owned else None
    ptr = _guarded(vox * ld * 4, label, write, tensor)
    return _tensor(dev(), ptr, n, D, H, W, c, ld, None)


def t_to_ncdhw(t):
    d = dev()
    full = d.d2h(t.ptr - 0, (t.n, t.d, t.h, t.w, t.ld), np.float32) if t.ld == t.c else None
    if full is not None:
        return np.moveaxis(full, -1, 1).copy()
    return t.numpy()


def vec(a):
    """1-D float array -> device pointer"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    a = a.reshape(-1)

    def write(payload):
        payload[:] = a

    return _guarded(a.nbytes, "%s vec(%d)" % (_call_site(), a.size), write)


def vec_back(ptr, n, dtype=np.float32):
    return dev().d2h(ptr, (n,), dtype)


def vp(ptr):
    return C.c_void_p(ptr) if ptr else None


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _describe(label, side, byte_offsets):
    return "%s: %s red zone corrupted: %d word(s), first at payload%+d, last at payload%+d" % (
        label, side, len(byte_offsets), int(byte_offsets[0]), int(byte_offsets[-1]))


def _check(d, e):
    """Messages for the corrupted red zones of one registered allocation (empty when intact)."""
    bad = []
    payload = e["base"] + e["offset"]
    head = d.d2h(e["base"], (GUARD // 4,), np.uint32)
    idx = np.flatnonzero(head != SENTINEL_BITS)
    if idx.size:
        bad.append(_describe(e["label"], "head", idx * 4 - GUARD))
    start = _roundup(e["nbytes"], 4)                      # a payload that ends inside a word owns that word
    tail = d.d2h(payload + start, ((e["total"] - e["offset"] - start) // 4,), np.uint32)
    idx = np.flatnonzero(tail != SENTINEL_BITS)
    if idx.size:
        bad.append(_describe(e["label"], "tail", idx * 4 + start))
    t = e["tensor"]
    if t is not None and t["ld"] > t["c"]:
        full = d.d2h(payload, (t["vox"], t["ld"]), np.uint32)
        v, ch = np.nonzero(full[:, t["c"]:] != t["pad_bits"])
        if v.size:
            bad.append(_describe(e["label"], "pad", (v * t["ld"] + t["c"] + ch) * 4))
    return bad


def assert_redzones_intact():
    """Read back both guards of every allocation made since the last check, and the pad channels of the tensors among them,
    compare them as uint32 with what was put there, and forget the allocations (they are not freed: module-scoped objects
    may still hold the pointers).  Raises AssertionError naming buffer, side (head / tail / pad), first and last corrupted
    offset in bytes relative to the payload, and the count."""
    if not _registry:
        return
    entries = list(_registry)
    del _registry[:]
    d = dev()
    d.sync()
    bad = [m for e in entries for m in _check(d, e)]
    assert not bad, "\n".join(bad)


def dfree(ptr):
    """Free a guarded allocation by its payload pointer (msk_free of the whole allocation) after checking its red zones.
    A pointer these helpers did not hand out, or one freed before, is an error."""
    assert ptr in _bases, "dfree(0x%x): not the payload of a live guarded allocation" % ptr
    d = dev()
    bad = []
    for e in [e for e in _registry if e["base"] + e["offset"] == ptr]:
        d.sync()
        bad = _check(d, e)
        _registry.remove(e)
    d.free(_bases.pop(ptr))
    assert not bad, "\n".join(bad)


@pytest.fixture(autouse=True)
def redzone_check():
    """Autouse in every module that imports it (`from helpers import redzone_check`): checks the guards after each test."""
    yield
    assert_redzones_intact()

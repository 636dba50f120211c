"""Device versions of tools/preprocess_utils (reference geometry.py:31-69, values.py:37-87):
same function names, arguments and return values; inputs are host arrays (as the
reference's `Prep.load_save` hands them over, tools/prepare.py:200-259), staged through
pinned-host -> device copies, processed by HIP kernels, and returned as host arrays.
``*_device`` variants keep data on the GPU for in-loop use."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from ._lib import MskError
from .device import get_device


class DeviceVolume:
    """A 3-D float32/int32 volume on the device (persistent allocation); also the small records device ops hand to each
    other (int32 patch records, float64 intensity statistics)."""

    def __init__(self, dev, ptr, shape, dtype):
        self.dev, self.ptr, self.shape, self.dtype = dev, ptr, tuple(int(s) for s in shape), np.dtype(dtype)
        self.pooled = False

    @property
    def size(self):
        return int(np.prod(self.shape))

    def numpy(self):
        return self.dev.d2h(self.ptr, self.shape, self.dtype)

    def free(self):
        if self.ptr:
            if self.pooled:
                _pool_release(self.dev, self.ptr, self.size * self.dtype.itemsize)
            else:
                self.dev.free(self.ptr)
            self.ptr = None


# Stream-ordered recycling of augmentation buffers: every op is enqueued on the context's single
# stream, so a buffer released by one op can be handed to a later op without synchronising
# (hipFree would stall the loader on the whole training stream).  The free lists are the device object's own (Device.pool).
def _pool_alloc(dev, nbytes):
    free = dev.pool.get(int(nbytes))
    return free.pop() if free else dev.malloc(nbytes)


def _pool_release(dev, ptr, nbytes):
    dev.pool.setdefault(int(nbytes), []).append(ptr)


def _pooled_volume(dev, shape, dtype) -> DeviceVolume:
    shape = tuple(int(v) for v in shape)
    v = DeviceVolume(dev, _pool_alloc(dev, int(np.prod(shape)) * np.dtype(dtype).itemsize), shape, dtype)
    v.pooled = True
    return v


def _new_volume(dev, shape, dtype, pooled) -> DeviceVolume:
    """a volume from the pool, or one of its own allocation (``free()`` is hipFree then, which synchronises)"""
    if pooled:
        return _pooled_volume(dev, shape, dtype)
    shape = tuple(int(v) for v in shape)
    return DeviceVolume(dev, dev.malloc(int(np.prod(shape)) * np.dtype(dtype).itemsize), shape, dtype)


@contextlib.contextmanager
def _pooled_outputs(dev, *specs):
    """The output volumes of one device op, a (shape, dtype) each, taken from the pool in the order given (None: no such
    output, yielded as None); a body that raises -- the library refused the call -- hands them back."""
    outs = []
    try:
        for spec in specs:
            outs.append(None if spec is None else _pooled_volume(dev, *spec))
        yield outs
    except BaseException:
        for v in outs:
            if v is not None:
                v.free()
        raise


@contextlib.contextmanager
def _pooled_scratch(dev, nbytes):
    """Scratch of one device op from the pool, handed back whatever happens: every later op is enqueued behind this one on
    the same stream.  ``nbytes`` None: the op needs none, yields None."""
    ptr = None if nbytes is None else _pool_alloc(dev, nbytes)
    try:
        yield ptr
    finally:
        if ptr is not None:
            _pool_release(dev, ptr, nbytes)


def _workspace_bytes(dev, query, *args):
    """the scratch size one of the library's msk_*_workspace queries (they take no context) asks for"""
    nbytes = C.c_size_t(0)
    if getattr(dev.lib, query)(*args, C.byref(nbytes)) != 0:
        from ._lib import last_error
        raise MskError(query + " failed: " + last_error(None))
    return nbytes.value


def _dt(vol):
    return 0 if vol.dtype == np.float32 else 1


def _check_order(vol, order):
    if order not in (0, 1, 3):
        raise ValueError("only orders 0, 1 and 3 are built, got order {}".format(order))
    if order == 3 and vol.dtype != np.float32:
        raise ValueError("order 3 is built for float32 volumes only (labels are resampled with order 0)")


def _spline_device(vol: DeviceVolume, box, size, pooled) -> DeviceVolume:
    """scipy.ndimage.zoom(order=3, mode='nearest') of the crop box (i, j, k, d, h, w) of a float32 volume
    (msk_spline_resample3d: tests/spline_reference.py's statement bit for bit); the float64 workspace comes from the pool."""
    dev = vol.dev
    box = [int(v) for v in box]
    size = tuple(int(s) for s in size)
    nbytes = _workspace_bytes(dev, "msk_spline_workspace", *box[3:])
    out = _new_volume(dev, size, np.float32, pooled)
    try:
        with _pooled_scratch(dev, nbytes) as work:
            dev.call("msk_spline_resample3d", C.c_void_p(vol.ptr), *vol.shape, *box, C.c_void_p(out.ptr), *size,
                     C.c_void_p(work), C.c_size_t(nbytes))
    except BaseException:
        out.free()
        raise
    return out


def flip_device(vol: DeviceVolume, axis: int) -> DeviceVolume:
    """functional.py:80-88 flip_3d on the device."""
    out = _pooled_volume(vol.dev, vol.shape, vol.dtype)
    vol.dev.call("msk_flip3d", C.c_void_p(vol.ptr), C.c_void_p(out.ptr), *vol.shape, int(axis), _dt(vol))
    return out


def rotate_device(vol: DeviceVolume, r_plane, angle, order=1, cval=0) -> DeviceVolume:
    """functional.py:91-100 rotate_3d (scipy.ndimage.rotate, reshape=False) on the device."""
    out = _pooled_volume(vol.dev, vol.shape, vol.dtype)
    vol.dev.call("msk_rotate3d", C.c_void_p(vol.ptr), C.c_void_p(out.ptr), *vol.shape, int(r_plane[0]), int(r_plane[1]),
                 C.c_double(float(angle)), int(order), C.c_double(float(cval)), _dt(vol))
    return out


def resized_crop_device(vol: DeviceVolume, i, j, k, d, h, w, size, order) -> DeviceVolume:
    """functional.py:103-110 resized_crop_3d (crop box, then zoom to `size`) on the device."""
    _check_order(vol, order)
    if order == 3:
        return _spline_device(vol, (i, j, k, d, h, w), size, True)
    out = _pooled_volume(vol.dev, size, vol.dtype)
    vol.dev.call("msk_crop_resample3d", C.c_void_p(vol.ptr), *vol.shape, int(i), int(j), int(k), int(d), int(h), int(w),
                 C.c_void_p(out.ptr), *out.shape, int(order), _dt(vol))
    return out


def max_normalize_device(vol: DeviceVolume) -> DeviceVolume:
    """transforms/transform.py:67-69 in place: im / im.max() when the maximum is positive."""
    vol.dev.call("msk_max_norm", C.c_void_p(vol.ptr), C.c_void_p(vol.ptr), C.c_size_t(vol.size))
    return vol


def connected_components_device(x, minimum_volume=0, k=0):
    """transforms/functional.py:117-131 connected_component (+ transform.py:343-396) on the device: the 6-connected
    foreground components of every volume numbered 1, 2, ... by decreasing size (ties: first voxel in raster order),
    components smaller than ``minimum_volume`` set to 0, with ``k > 0`` only the k largest kept.  Bitwise equal to
    transforms.transform._connected_components per volume, as int32 instead of uint32.

    x: a 3-D float32 / int32 ``DeviceVolume`` -> a new int32 ``DeviceVolume`` (pooled, like the other device ops); or an
    ``IntTensor`` [N, 1, D, H, W] (core.infer.inference's prediction) -> a new ``IntTensor`` in the activation arena
    (valid until the next model forward, like the prediction), each of the N volumes labelled on its own.  The input is
    not modified.  Synchronises once, to read the per-volume status words: a volume with three or more distinct values
    raises the host path's AssertionError."""
    from .device import IntTensor
    mv = int(min(max(np.ceil(minimum_volume), 0), 2 ** 31 - 1))   # integer sizes: size >= v  <=>  size >= ceil(v)
    k = int(k)
    if isinstance(x, DeviceVolume):
        if len(x.shape) != 3:
            raise ValueError("expected a 3-D volume, got shape {}".format(x.shape))
        n, (d, h, w), dtype = 1, x.shape, _dt(x)
        out = _pooled_volume(x.dev, x.shape, np.int32)
        out_ptr = out.ptr
    elif isinstance(x, IntTensor):
        if len(x.shape) != 5 or x.shape[1] != 1:
            raise ValueError("expected an [N, 1, D, H, W] label tensor, got shape {}".format(x.shape))
        n, _, d, h, w = x.shape
        dtype = 1
        out = IntTensor(x.dev, x.dev.arena.alloc(int(np.prod(x.shape)) * 4), x.shape, x.dev.arena.gen)
        out_ptr = out.ptr
    else:
        raise TypeError("connected_components_device takes a DeviceVolume or an IntTensor, got {}".format(type(x)))
    dev = x.dev
    with _pooled_scratch(dev, 4 * n) as st:
        dev.call("msk_connected_components3d", C.c_void_p(x.ptr), C.c_void_p(out_ptr), n, d, h, w, dtype, mv, k,
                 C.c_void_p(st), None)
        status = dev.d2h(st, (n,), np.int32)
    if status.any():
        if isinstance(out, DeviceVolume):
            out.free()
        if (status & 2).any():
            raise MskError("msk_connected_components3d: an iteration bound was hit (status {})".format(status.tolist()))
        i = int(np.flatnonzero(status & 1)[0])
        vol = x.numpy() if isinstance(x, DeviceVolume) else x.numpy()[i, 0]
        vals = np.unique(vol)
        raise AssertionError("Only binary mask is accepted, got mask with {}.".format(vals.tolist()))
    return out


# ---- hole filling (scipy.ndimage.binary_fill_holes = nnU-Net's create_nonzero_mask; MONAI's FillHoles) -------------------------
FILL_MASK, FILL_LABEL, FILL_NONE = 0, 1, 2       # MSK_FILL_*
FILL_MAX_CLASSES = 64


def _fill_classes(classes, binary):
    """the ``classes`` argument as an int32 array (empty: any value)"""
    cls = np.zeros(0, np.int32) if classes is None else np.atleast_1d(np.asarray(classes)).astype(np.int32).reshape(-1)
    if cls.size > FILL_MAX_CLASSES:
        raise ValueError("at most {} classes, got {}".format(FILL_MAX_CLASSES, cls.size))
    if binary and cls.size:
        raise ValueError("binary=True fills every hole of the non-zero mask and takes no classes")
    return cls


def fill_holes_device(x, classes=None, binary=False):
    """msk_fill_holes3d: the enclosed holes of every volume filled on the device (tests/fillholes_reference.py is the statement).
    The zero voxels (value == 0; float32: -0.0 is zero, a NaN is not) form 6-connected components; one that touches no face of
    the volume is a hole.  ``binary=True``: the int32 mask 1 where x != 0 or in a hole, else 0 -- exactly
    scipy.ndimage.binary_fill_holes(x != 0).  ``binary=False`` (int32 only, MONAI's FillHoles): x with every hole whose non-zero
    6-neighbours all carry ONE value c set to c, when c is in ``classes`` (None: any value; at most 64); a hole between
    different values stays 0.

    x: a 3-D float32 (``binary=True`` only) / int32 ``DeviceVolume`` -> a new pooled int32 ``DeviceVolume``; or an
    ``IntTensor`` [N, 1, D, H, W] -> a new ``IntTensor`` in the activation arena (valid until the next model forward), each of
    the N volumes on its own.  The input is not modified.  Synchronises once, to read the per-volume status words (4 bytes
    each): an iteration bound that was hit raises MskError."""
    from .device import IntTensor
    cls = _fill_classes(classes, binary)
    if isinstance(x, DeviceVolume):
        if len(x.shape) != 3:
            raise ValueError("expected a 3-D volume, got shape {}".format(x.shape))
        if x.dtype not in (np.float32, np.int32):
            raise TypeError("fill_holes_device takes a float32 or int32 volume, got {}".format(x.dtype))
        if x.dtype == np.float32 and not binary:
            raise ValueError("a float32 volume has no label form: pass binary=True for the filled non-zero mask")
        n, (d, h, w), dtype = 1, x.shape, _dt(x)
        out = _pooled_volume(x.dev, x.shape, np.int32)
    elif isinstance(x, IntTensor):
        if len(x.shape) != 5 or x.shape[1] != 1:
            raise ValueError("expected an [N, 1, D, H, W] label tensor, got shape {}".format(x.shape))
        n, _, d, h, w = x.shape
        dtype = 1
        out = IntTensor(x.dev, x.dev.arena.alloc(int(np.prod(x.shape)) * 4), x.shape, x.dev.arena.gen)
    else:
        raise TypeError("fill_holes_device takes a DeviceVolume or an IntTensor, got {}".format(type(x)))
    dev = x.dev
    try:
        with _pooled_scratch(dev, 4 * n) as st:
            dev.call("msk_fill_holes3d", C.c_void_p(x.ptr), C.c_void_p(out.ptr), n, d, h, w, dtype,
                     FILL_MASK if binary else FILL_LABEL, cls.ctypes.data_as(C.c_void_p) if cls.size else None, int(cls.size),
                     C.c_void_p(st), None)
            status = dev.d2h(st, (n,), np.int32)
        if status.any():
            raise MskError("msk_fill_holes3d: an iteration bound was hit (status {})".format(status.tolist()))
    except BaseException:
        if isinstance(out, DeviceVolume):
            out.free()
        raise
    return out


def _fill_holes_volume(x, cls, binary):
    """one 3-D host volume -> int32, the statement of tests/fillholes_reference.py vectorised over the components"""
    import scipy.ndimage
    zero = x == 0
    lab, n = scipy.ndimage.label(zero)
    hole = np.ones(n + 1, bool)
    hole[0] = False                                    # entry 0: the non-zero voxels
    for ax in range(3):
        for face in (0, -1):
            hole[np.take(lab, face, axis=ax).ravel()] = False
    if binary:
        return (~zero | hole[lab]).astype(np.int32)
    lo = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
    hi = np.full(n + 1, np.iinfo(np.int64).min, np.int64)
    for ax in range(3):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        for p, q in ((tuple(a), tuple(b)), (tuple(b), tuple(a))):   # p: the zero voxel, q: its neighbour along the axis
            sel = zero[p] & ~zero[q]
            np.minimum.at(lo, lab[p][sel], x[q][sel].astype(np.int64))
            np.maximum.at(hi, lab[p][sel], x[q][sel].astype(np.int64))
    ok = hole & (lo == hi)
    if cls.size:
        ok &= np.isin(lo, cls.astype(np.int64))
    return np.where(ok[lab], lo[lab], x.astype(np.int64)).astype(np.int32)


def fill_holes_host(x, classes=None, binary=False) -> np.ndarray:
    """fill_holes_device in numpy and scipy.ndimage.label, the same values: a [D, H, W] volume or a batch [N, 1, D, H, W],
    every volume on its own -> int32 of the same shape"""
    cls = _fill_classes(classes, binary)
    x = np.asarray(x)
    if x.ndim == 5 and x.shape[1] == 1:
        if not x.shape[0]:
            raise ValueError("empty batch")
        return np.stack([fill_holes_host(v[0], classes, binary)[None] for v in x])
    if x.ndim != 3:
        raise ValueError("expected a 3-D volume or an [N, 1, D, H, W] batch, got shape {}".format(x.shape))
    if not binary and not np.issubdtype(x.dtype, np.integer):
        raise ValueError("a float32 volume has no label form: pass binary=True for the filled non-zero mask")
    return _fill_holes_volume(x, cls, binary)


def fill_holes(x, classes=None, binary=False, on_device=True) -> np.ndarray:
    """fill_holes_device for a host array [D, H, W] (uploaded, filled, downloaded) -> int32; ``on_device`` False takes
    fill_holes_host, which gives the same values"""
    if not on_device:
        return fill_holes_host(x, classes, binary)
    _fill_classes(classes, binary)
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError("expected a 3-D volume, got shape {}".format(x.shape))
    if np.issubdtype(x.dtype, np.integer):
        vol = upload(x.astype(np.int32))
    elif binary:
        vol = upload(x.astype(np.float32))
    else:
        raise ValueError("a float32 volume has no label form: pass binary=True for the filled non-zero mask")
    try:
        out = fill_holes_device(vol, classes, binary)
    finally:
        vol.free()
    res = out.numpy()
    out.free()
    return res


def nonzero_mask_device(vol: DeviceVolume, fill_holes=True) -> DeviceVolume:
    """nnU-Net's create_nonzero_mask, binary_fill_holes(x != 0), as a new pooled int32 volume of 0 / 1 ready for mode='mask'
    (``fill_holes`` False: x != 0 alone).  Downloads the 4-byte status word of fill_holes_device.  One channel: nnU-Net ORs the
    mask over the modalities of a case."""
    if not isinstance(vol, DeviceVolume) or len(vol.shape) != 3:
        raise TypeError("nonzero_mask_device takes a 3-D DeviceVolume")
    if fill_holes:
        return fill_holes_device(vol, binary=True)
    if vol.dtype not in (np.float32, np.int32):
        raise TypeError("nonzero_mask_device takes a float32 or int32 volume, got {}".format(vol.dtype))
    with _pooled_outputs(vol.dev, (vol.shape, np.int32)) as (out,), _pooled_scratch(vol.dev, 4) as st:
        # MSK_FILL_NONE is the apply pass alone: no search, so no bound can be hit and the status word is not read
        vol.dev.call("msk_fill_holes3d", C.c_void_p(vol.ptr), C.c_void_p(out.ptr), 1, *vol.shape, _dt(vol), FILL_NONE, None, 0,
                     C.c_void_p(st), None)
    return out


def nonzero_mask_host(volume, fill_holes=True) -> np.ndarray:
    """nonzero_mask_device in numpy: int32 0 / 1"""
    v = np.asarray(volume)
    if v.ndim != 3:
        raise ValueError("expected a 3-D volume, got shape {}".format(v.shape))
    return fill_holes_host(v, binary=True) if fill_holes else (v != 0).astype(np.int32)


def patch_select_device(label: DeviceVolume, roi, num_classes, classes, words) -> DeviceVolume:
    """msk_patch_select: choose patch origins in a device label volume -> the ``sel`` records, an int32 ``DeviceVolume``
    [n_patches, 8] (d0, h0, w0, cls, cz, cy, cx, 0) from the stream-ordered pool (``free()`` hands it back).

    ``classes``: the strictly ascending candidate classes; ``words``: six 32-bit integers per patch (force_fg, w_cls, w_rank,
    w_d, w_h, w_w), one patch or a sequence of up to 16.  The workspace comes from the pool and goes back to it (every later
    op is enqueued behind this one on the same stream).  Nothing is downloaded and nothing synchronises: the host never learns
    the origin.  With ``classes`` empty (or no patch forcing foreground) the volume is not read, so an image may stand in
    for a missing label."""
    dev = label.dev
    d, h, w = label.shape
    words = np.ascontiguousarray(np.asarray(words, dtype=np.uint64).astype(np.uint32).reshape(-1, 6))
    cls = np.ascontiguousarray(np.asarray(list(classes), dtype=np.int32).reshape(-1))
    nbytes = _workspace_bytes(dev, "msk_patch_workspace", C.c_long(d * h * w), int(num_classes))
    with _pooled_outputs(dev, ((len(words), 8), np.int32)) as (sel,), _pooled_scratch(dev, nbytes) as ws:
        dev.call("msk_patch_select", C.c_void_p(label.ptr), d, h, w, int(num_classes), cls.ctypes.data_as(C.c_void_p), len(cls),
                 int(roi[0]), int(roi[1]), int(roi[2]), words.ctypes.data_as(C.c_void_p), len(words), C.c_void_p(ws),
                 C.c_void_p(sel.ptr), None)
    return sel


def patch_crop_device(vol: DeviceVolume, sel: DeviceVolume, roi, pad=0, index=0) -> DeviceVolume:
    """msk_patch_crop: the patch of ``vol`` at the origin of record ``index`` of ``sel`` (patch_select_device), read on the
    device -> a pooled ``DeviceVolume`` of extent ``roi`` and vol's dtype; voxels outside the volume are ``pad``."""
    if not 0 <= int(index) < sel.shape[0]:
        raise ValueError("patch_crop_device: record {} of {}".format(index, sel.shape[0]))
    with _pooled_outputs(vol.dev, (roi, vol.dtype)) as (out,):
        bits = int(np.array([pad], dtype=vol.dtype).view(np.uint32)[0])
        vol.dev.call("msk_patch_crop", C.c_void_p(vol.ptr), *vol.shape, C.c_void_p(sel.ptr + 32 * int(index)), C.c_void_p(out.ptr),
                     int(roi[0]), int(roi[1]), int(roi[2]), C.c_uint32(bits))
    return out


def affine_patch_device(img: DeviceVolume, label, sel: DeviceVolume, roi, matrix, pad=0, label_pad=0, index=0, field=None):
    """msk_affine_patch: the patch of ``img`` (float32) and, unless ``label`` is None, of ``label`` (int32) whose sampling grid
    is centred on the patch of record ``index`` of ``sel`` (patch_select_device; read on the device) and turned and scaled by
    the 3x3 ``matrix`` (rows: source axes, columns: patch axes) -> one pooled ``DeviceVolume`` of extent ``roi``, or two.  The
    image is read trilinearly with ``pad`` outside the volume, the label by nearest neighbour with ``label_pad``, from the
    same coordinates, in one launch.  Nothing is downloaded and nothing synchronises.

    ``field``: a float32 ``DeviceVolume`` of shape ``(3,) + roi`` (elastic_field_device) that displaces the grid before the
    matrix, msk_affine_patch_elastic; without it the call is msk_affine_patch."""
    _float_volume(img, "affine_patch_device")
    if field is not None and (not isinstance(field, DeviceVolume) or field.dtype != np.float32 or
                              tuple(field.shape) != (3,) + tuple(int(r) for r in roi)):
        raise TypeError("affine_patch_device takes a float32 DeviceVolume of shape (3,) + roi as the field")
    if label is not None and (not isinstance(label, DeviceVolume) or label.dtype != np.int32 or label.shape != img.shape):
        raise TypeError("affine_patch_device takes an int32 DeviceVolume of the image's shape as the label")
    if not 0 <= int(index) < sel.shape[0]:
        raise ValueError("affine_patch_device: record {} of {}".format(index, sel.shape[0]))
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float32).reshape(9))
    name, extra = ("msk_affine_patch", ()) if field is None else ("msk_affine_patch_elastic", (C.c_void_p(field.ptr),))
    with _pooled_outputs(img.dev, (roi, np.float32), None if label is None else (roi, np.int32)) as (out, out_label):
        img.dev.call(name, C.c_void_p(img.ptr), C.c_void_p(label.ptr) if label is not None else None, *img.shape,
                     C.c_void_p(sel.ptr + 32 * int(index)), m.ctypes.data_as(C.c_void_p), *extra, C.c_void_p(out.ptr),
                     C.c_void_p(out_label.ptr) if label is not None else None, int(roi[0]), int(roi[1]), int(roi[2]),
                     C.c_float(float(pad)), int(label_pad))
    return out if label is None else (out, out_label)


INTENSITY_NOISE, INTENSITY_SCALE, INTENSITY_CONTRAST, INTENSITY_GAMMA, INTENSITY_RESTORE = range(5)   # MSK_INTENSITY_*
GAUSS_MAX_SIGMA = 2.0   # radius int(4 sigma + 0.5) <= 8, the widest msk_gauss_blur3d takes
ELASTIC_MIN_SIGMA, ELASTIC_MAX_SIGMA = 0.5, 16.0   # radius 2 .. 64, what msk_elastic_field takes
ELASTIC_MAX_ALPHA = 4096.0


def gauss_taps(sigma, max_sigma=GAUSS_MAX_SIGMA) -> np.ndarray:
    """The 2r+1 float32 weights of one blurred axis, r = int(4 sigma + 0.5) (scipy.ndimage.gaussian_filter's kernel at
    truncate 4, computed in float64 and rounded once); empty when r == 0.  The host path and the device path of the blur use
    these same numbers; ``max_sigma`` is the limit of the kernel the taps are for (the elastic field's is ELASTIC_MAX_SIGMA)."""
    sigma = float(sigma)
    if not 0.0 <= sigma <= max_sigma:
        raise ValueError("sigma must be in [0, {}], got {}".format(max_sigma, sigma))
    r = int(4.0 * sigma + 0.5)
    if r == 0:
        return np.zeros(0, np.float32)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * k * k)
    return (w / w.sum()).astype(np.float32)


def elastic_axes_mask(axes) -> int:
    """bit a set for every source axis a of ``axes``, a subset of (0, 1, 2) without repeats"""
    axes = [int(a) for a in axes]
    if any(a not in (0, 1, 2) for a in axes) or len(set(axes)) != len(axes):
        raise ValueError("axes must be a subset of (0, 1, 2), got {}".format(axes))
    return sum(1 << a for a in axes)


def elastic_field_device(dev, roi, sigma, alpha, seed, axes=(0, 1, 2)) -> DeviceVolume:
    """msk_elastic_field: the displacement field of an elastic deformation, alpha * (uniform counter noise smoothed by a
    Gaussian of ``sigma`` in [0.5, 16] along W, H and D with zeros outside the patch), as a pooled float32 ``DeviceVolume`` of
    shape ``(3,) + roi`` (``free()`` hands it back) for affine_patch_device's ``field``.  A component whose axis is not in
    ``axes`` is zero.  The scratch volume comes from the pool and goes back to it.  Nothing is downloaded and nothing
    synchronises."""
    roi = tuple(int(r) for r in roi)
    if len(roi) != 3:
        raise ValueError("roi must have three extents, got {}".format(roi))
    sigma, alpha = float(sigma), float(alpha)
    if not ELASTIC_MIN_SIGMA <= sigma <= ELASTIC_MAX_SIGMA:
        raise ValueError("sigma must be in [{}, {}], got {}".format(ELASTIC_MIN_SIGMA, ELASTIC_MAX_SIGMA, sigma))
    taps = gauss_taps(sigma, ELASTIC_MAX_SIGMA)
    mask = elastic_axes_mask(axes)
    shape = (3,) + roi
    with _pooled_outputs(dev, (shape, np.float32)) as (field,), _pooled_scratch(dev, int(np.prod(shape)) * 4) as tmp:
        dev.call("msk_elastic_field", C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), *roi, taps.ctypes.data_as(C.c_void_p),
                 (len(taps) - 1) // 2, C.c_float(alpha), mask, C.c_void_p(field.ptr), C.c_void_p(tmp))
    return field


def _float_volume(vol, what):
    if not isinstance(vol, DeviceVolume) or vol.dtype != np.float32:
        raise TypeError("{} takes a float32 DeviceVolume".format(what))


def intensity_stats_device(vol: DeviceVolume) -> DeviceVolume:
    """msk_intensity_stats: the record {min, max, sum, sumsq} of a float32 volume as four float64 in a pooled device buffer
    (a ``DeviceVolume`` of shape (4,), ``free()`` hands it back), in the fixed summation order of tests/intensity_reference.py.
    The workspace comes from the pool and goes back to it (every later op is enqueued behind this one on the same stream).
    Nothing is downloaded and nothing synchronises: the record is read by msk_intensity_apply on the device."""
    _float_volume(vol, "intensity_stats_device")
    dev = vol.dev
    nbytes = _workspace_bytes(dev, "msk_intensity_stats_workspace", C.c_long(vol.size))
    with _pooled_outputs(dev, ((4,), np.float64)) as (rec,), _pooled_scratch(dev, nbytes) as ws:
        dev.call("msk_intensity_stats", C.c_void_p(vol.ptr), C.c_long(vol.size), C.c_void_p(ws), C.c_void_p(rec.ptr))
    return rec


def intensity_apply_device(vol: DeviceVolume, mode, params, stats_a=None, stats_b=None, seed=0, inplace=True) -> DeviceVolume:
    """msk_intensity_apply: one streaming pass over a float32 volume, in place (returns ``vol``) or into a new pooled volume.
    ``mode``: INTENSITY_NOISE (params: std; ``seed``), INTENSITY_SCALE (factor), INTENSITY_CONTRAST (factor, preserve_range;
    ``stats_a``), INTENSITY_GAMMA (gamma, invert; ``stats_a``), INTENSITY_RESTORE (``stats_a`` of the volume before,
    ``stats_b`` of ``vol``).  The records are intensity_stats_device's and are read on the device: nothing synchronises."""
    _float_volume(vol, "intensity_apply_device")
    p = np.zeros(4, np.float32)
    params = np.asarray(params, np.float32).reshape(-1)
    p[:params.size] = params
    with _pooled_outputs(vol.dev, None if inplace else (vol.shape, vol.dtype)) as (out,):
        out = vol if inplace else out
        vol.dev.call("msk_intensity_apply", C.c_void_p(vol.ptr), C.c_void_p(out.ptr), C.c_long(vol.size), int(mode),
                     p.ctypes.data_as(C.c_void_p), C.c_void_p(stats_a.ptr) if stats_a is not None else None,
                     C.c_void_p(stats_b.ptr) if stats_b is not None else None, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))
    return out


def gauss_blur_device(vol: DeviceVolume, sigma) -> DeviceVolume:
    """msk_gauss_blur3d: separable Gaussian blur (scipy's mode='reflect', truncate 4) of a float32 volume into a new pooled
    volume; ``sigma`` a scalar or one value per axis (D, H, W), 0 skips an axis, at most 2.  The scratch volume comes from the
    pool and goes back to it."""
    _float_volume(vol, "gauss_blur_device")
    if len(vol.shape) != 3:
        raise ValueError("expected a 3-D volume, got shape {}".format(vol.shape))
    sig = [float(sigma)] * 3 if np.isscalar(sigma) else [float(s) for s in sigma]
    if len(sig) != 3:
        raise ValueError("sigma must be a scalar or three values, got {}".format(sigma))
    taps = [gauss_taps(s) for s in sig]
    dev = vol.dev
    args = []
    for t in taps:
        args += [t.ctypes.data_as(C.c_void_p) if len(t) else None, (len(t) - 1) // 2 if len(t) else 0]
    nbytes = vol.size * 4 if sum(len(t) > 0 for t in taps) >= 2 else None   # one blurred axis needs no scratch volume
    with _pooled_outputs(dev, (vol.shape, vol.dtype)) as (out,), _pooled_scratch(dev, nbytes) as tmp:
        dev.call("msk_gauss_blur3d", C.c_void_p(vol.ptr), C.c_void_p(out.ptr), *vol.shape, *args, C.c_void_p(tmp) if tmp else None)
    return out


# ---- non-zero cropping, percentile clipping and z-scoring (nnU-Net's crop_to_nonzero, CTNormalization, ZScoreNormalization;
#      MONAI's ScaleIntensityRangePercentiles / NormalizeIntensity(nonzero=True)) --------------------------------------------------
MASK_MODES = {"all": 0, "nonzero": 1, "mask": 2}       # MSK_MASK_*
NORM_CLIP, NORM_ZSCORE, NORM_MASK_OUT = 1, 2, 4        # MSK_NORM_*
FG_FIELDS = ("n_valid", "min", "max", "sum", "sumsq", "mean", "std", "p_lo", "p_hi", "a_lo", "b_lo", "g_lo", "a_hi", "b_hi", "g_hi")


def _mask_mode(mode, mask):
    if mode not in MASK_MODES:
        raise ValueError("mode must be one of 'all', 'nonzero', 'mask', got {!r}".format(mode))
    if (mode == "mask") != (mask is not None):
        raise ValueError("mode 'mask' takes a mask and the other modes take none")
    return MASK_MODES[mode]


def _percentile_pair(percentiles):
    q = [float(v) for v in percentiles]
    if len(q) != 2 or not 0.0 <= q[0] <= q[1] <= 100.0:
        raise ValueError("percentiles must be two values 0 <= lo <= hi <= 100, got {}".format(percentiles))
    return q


def _norm_params(stats, lo, hi, mean, std, clip, zscore):
    """the four doubles {lo, hi, mean, std} of the apply pass from explicit values (None when a record supplies them)"""
    if not (clip or zscore):
        raise ValueError("at least one of clip and zscore must be on")
    given = [v is not None for v in (lo, hi, mean, std)]
    if stats is not None:
        if any(given):
            raise ValueError("give a statistics record or explicit values, not both")
        return None
    if clip and not (given[0] and given[1]):
        raise ValueError("clip needs lo and hi (or a statistics record)")
    if zscore and not (given[2] and given[3]):
        raise ValueError("zscore needs mean and std (or a statistics record)")
    p = np.array([lo if clip else 0.0, hi if clip else 0.0, mean if zscore else 0.0, std if zscore else 1.0], np.float64)
    if clip and not p[0] <= p[1]:
        raise ValueError("lo must not exceed hi, got {} > {}".format(lo, hi))
    return p


def _mask_volume(vol, mask, what):
    if not isinstance(mask, DeviceVolume) or mask.dtype != np.int32 or mask.size != vol.size:
        raise TypeError("{} takes an int32 DeviceVolume of the volume's size as the mask".format(what))


def nonzero_bbox_device(vol: DeviceVolume) -> DeviceVolume:
    """msk_nonzero_bbox: the record {d0, h0, w0, d1, h1, w1, count, 0} of the non-zero voxels of a float32 (x != 0) or int32
    volume as eight int32 in a pooled device buffer (``free()`` hands it back); the upper corner is exclusive, an empty volume
    gives zeros.  Holes do not change a bounding box, so this is the box of nnU-Net's hole-filled non-zero mask.  Nothing is
    downloaded and nothing synchronises."""
    if not isinstance(vol, DeviceVolume) or len(vol.shape) != 3:
        raise TypeError("nonzero_bbox_device takes a 3-D DeviceVolume")
    with _pooled_outputs(vol.dev, ((8,), np.int32)) as (box,):
        vol.dev.call("msk_nonzero_bbox", C.c_void_p(vol.ptr), *vol.shape, _dt(vol), C.c_void_p(box.ptr))
    return box


def crop_to_nonzero_device(img: DeviceVolume, label=None):
    """nnU-Net's crop_to_nonzero: ``(img, label, box)`` cut to the bounding box of the image's non-zero voxels (the existing
    identity crop, msk_crop_resample3d at order 0) as NEW pooled volumes; the inputs stay the caller's.  ``box`` is the
    downloaded record of nonzero_bbox_device as a host array.  SYNCHRONISES once: the 32-byte record is downloaded because the
    output shape depends on it.  A volume without a non-zero voxel is returned whole (the same objects)."""
    if label is not None and (not isinstance(label, DeviceVolume) or label.shape != img.shape):
        raise TypeError("crop_to_nonzero_device takes a DeviceVolume of the image's shape as the label")
    rec = nonzero_bbox_device(img)
    box = rec.numpy()
    rec.free()
    if box[6] == 0:
        return img, label, box
    lo, ext = [int(v) for v in box[:3]], [int(v) for v in box[3:6] - box[:3]]
    out = resized_crop_device(img, *lo, *ext, ext, 0)
    try:
        out_label = None if label is None else resized_crop_device(label, *lo, *ext, ext, 0)
    except BaseException:
        out.free()
        raise
    return out, out_label, box


def fg_stats_device(vol: DeviceVolume, mask=None, mode="all", percentiles=(0.5, 99.5)) -> DeviceVolume:
    """msk_fg_stats: the record FG_FIELDS of the valid voxels of a float32 volume (``mode`` 'all'; 'nonzero': x != 0;
    'mask': ``mask`` > 0, an int32 volume -- nonzero_mask_device gives nnU-Net's hole-filled non-zero mask) as sixteen float64 in a pooled device buffer:
    count, exact min / max, the float64 sums in msk_intensity_stats' fixed order, mean, std and the two ``percentiles`` by
    numpy's default method, every field exact (tests/normalize_reference.py).  The workspace comes from the pool and goes back
    to it.  Nothing is downloaded and nothing synchronises: clip_zscore_device reads the record on the device."""
    _float_volume(vol, "fg_stats_device")
    mm = _mask_mode(mode, mask)
    if mask is not None:
        _mask_volume(vol, mask, "fg_stats_device")
    q = _percentile_pair(percentiles)
    dev = vol.dev
    nbytes = _workspace_bytes(dev, "msk_fg_stats_workspace", C.c_long(vol.size))
    with _pooled_outputs(dev, ((16,), np.float64)) as (rec,), _pooled_scratch(dev, nbytes) as ws:
        dev.call("msk_fg_stats", C.c_void_p(vol.ptr), C.c_void_p(mask.ptr) if mask is not None else None, C.c_long(vol.size), mm,
                 C.c_double(q[0]), C.c_double(q[1]), C.c_void_p(ws), C.c_void_p(rec.ptr))
    return rec


def clip_zscore_device(vol: DeviceVolume, stats=None, lo=None, hi=None, mean=None, std=None, mask=None, mode="all", clip=True,
                       zscore=True, outside=None, inplace=True) -> DeviceVolume:
    """msk_clip_zscore: one streaming pass, in place (returns ``vol``) or into a new pooled volume: clip to [lo, hi], then
    (x - mean) / max(std, 1e-8) as a multiplication by the float64 reciprocal.  The four values come from ``stats`` (a
    fg_stats_device record: its percentiles, mean and std, read on the device, nothing synchronises) or are given (nnU-Net's CT
    plan: dataset-level values).  ``clip`` / ``zscore`` switch the two steps; with ``outside`` set, a voxel that is not valid
    under ``mode`` / ``mask`` becomes that value (nnU-Net: 0), otherwise it is transformed like every other voxel."""
    _float_volume(vol, "clip_zscore_device")
    mm = _mask_mode(mode, mask)
    if mask is not None:
        _mask_volume(vol, mask, "clip_zscore_device")
    if stats is not None and (not isinstance(stats, DeviceVolume) or stats.dtype != np.float64 or stats.size != 16):
        raise TypeError("clip_zscore_device takes a fg_stats_device record as stats")
    p = _norm_params(stats, lo, hi, mean, std, clip, zscore)
    flags = (NORM_CLIP if clip else 0) | (NORM_ZSCORE if zscore else 0) | (NORM_MASK_OUT if outside is not None else 0)
    with _pooled_outputs(vol.dev, None if inplace else (vol.shape, vol.dtype)) as (out,):
        out = vol if inplace else out
        vol.dev.call("msk_clip_zscore", C.c_void_p(vol.ptr), C.c_void_p(mask.ptr) if mask is not None else None, C.c_long(vol.size),
                     mm, C.c_void_p(stats.ptr) if stats is not None else None, p.ctypes.data_as(C.c_void_p) if p is not None else None,
                     flags, C.c_float(0.0 if outside is None else float(outside)), C.c_void_p(out.ptr))
    return out


# The numpy host path: tests/normalize_reference.py's statement bit for bit, for callers that want no device.
def _sort_keys(x):
    b = x.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unsort_keys(k):
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _valid_host(x, mm, mask):
    if mm == 0:
        return np.ones(x.size, bool)
    if mm == 1:
        return x != 0
    m = np.ascontiguousarray(mask, np.int32).reshape(-1)
    if m.size != x.size:
        raise ValueError("the mask must have the volume's size")
    return m > 0


def fg_stats_host(image, mask=None, mode="all", percentiles=(0.5, 99.5)) -> np.ndarray:
    """fg_stats_device's record computed in numpy, bit for bit the same: sixteen float64 (FG_FIELDS and a zero)"""
    from .transforms.transform import _ordered_sum
    mm = _mask_mode(mode, mask)
    q = _percentile_pair(percentiles)
    x = np.ascontiguousarray(image, np.float32).reshape(-1)
    valid = _valid_host(x, mm, mask)
    nv = int(np.count_nonzero(valid))
    rec = np.zeros(16, np.float64)
    if nv == 0:
        return rec
    s = _unsort_keys(np.sort(_sort_keys(x[valid]))).astype(np.float64)
    d = np.where(valid, x.astype(np.float64), 0.0)
    n64 = np.float64(nv)
    rec[0], rec[1], rec[2] = n64, s[0], s[-1]
    rec[3], rec[4] = _ordered_sum(d), _ordered_sum(d * d)
    rec[5] = rec[3] / n64
    rec[6] = np.sqrt(max(rec[4] / n64 - rec[5] * rec[5], np.float64(0.0)))
    for t, qq in enumerate(q):
        h = np.float64(nv - 1) * (np.float64(qq) / np.float64(100.0))
        i = int(np.floor(h))
        g = h - np.floor(h)
        a, b = s[i], s[min(i + 1, nv - 1)]
        dd = b - a
        rec[7 + t] = b - dd * (np.float64(1.0) - g) if g >= 0.5 else a + dd * g
        rec[9 + 3 * t:12 + 3 * t] = [a, b, g]
    return rec


def clip_zscore_host(image, stats=None, lo=None, hi=None, mean=None, std=None, mask=None, mode="all", clip=True, zscore=True,
                     outside=None) -> np.ndarray:
    """clip_zscore_device in numpy, bit for bit the same; ``stats`` is a fg_stats_host record"""
    mm = _mask_mode(mode, mask)
    p = _norm_params(stats, lo, hi, mean, std, clip, zscore)
    if p is None:
        p = np.array([stats[7], stats[8], stats[5], stats[6]], np.float64)
    x = np.ascontiguousarray(image, np.float32)
    y = x
    if clip:
        lo32, hi32 = np.float32(p[0]), np.float32(p[1])
        y = np.where(y < lo32, lo32, y)
        y = np.where(y > hi32, hi32, y)
    if zscore:
        inv = np.float32(np.float64(1.0) / max(p[3], np.float64(1e-8)))
        y = (y - np.float32(p[2])).astype(np.float32) * inv
    if outside is not None:
        y = np.where(_valid_host(x.reshape(-1), mm, mask).reshape(x.shape), y, np.float32(outside))
    return np.array(y, np.float32)


def nonzero_bbox_host(volume) -> np.ndarray:
    """nonzero_bbox_device's record in numpy: eight int32"""
    v = np.asarray(volume)
    if v.ndim != 3:
        raise ValueError("expected a 3-D volume, got shape {}".format(v.shape))
    nz = np.nonzero(v != 0)
    box = np.zeros(8, np.int32)
    if nz[0].size:
        box[:3] = [c.min() for c in nz]
        box[3:6] = [c.max() + 1 for c in nz]
        box[6] = nz[0].size
    return box


def _zscore_settings(percentiles, mode):
    """(percentiles of the record, clip on?, outside value) of a z-score call: outside the mask voxels become 0, as in nnU-Net"""
    return (percentiles if percentiles is not None else (0.0, 100.0)), percentiles is not None, (None if mode == "all" else 0.0)


def ct_normalize(image, lo, hi, mean, std, on_device=True):
    """nnU-Net's CTNormalization with the plan's dataset-level values: clip to [lo, hi], then (x - mean) / max(std, 1e-8).
    ``on_device`` False takes the numpy host path, which gives the same bits."""
    if not on_device:
        return clip_zscore_host(image, lo=lo, hi=hi, mean=mean, std=std)
    _norm_params(None, lo, hi, mean, std, True, True)
    return _on_host_array(lambda v: clip_zscore_device(v, lo=lo, hi=hi, mean=mean, std=std), image)


def _check_fill_mode(fill_holes, mode):
    if fill_holes and mode != "nonzero":
        raise ValueError("fill_holes=True fills the holes of the non-zero mask and needs mode 'nonzero', got {!r}".format(mode))


def zscore_normalize(image, percentiles=None, mode="all", mask=None, on_device=True, fill_holes=False):
    """nnU-Net's ZScoreNormalization per volume: mean and std of the valid voxels (``mode`` 'all', 'nonzero' or 'mask' with an
    integer ``mask``), after clipping to the two ``percentiles`` of the valid voxels when they are given (MONAI's
    ScaleIntensityRangePercentiles in front of NormalizeIntensity); with a mask the voxels outside it become 0.
    ``mode='nonzero'`` alone is x != 0; with ``fill_holes=True`` (a [D, H, W] volume) it is nnU-Net's mask,
    binary_fill_holes(x != 0): a zero voxel enclosed by the body is part of the statistics and is z-scored.  That is mode 'mask'
    on nonzero_mask_device / nonzero_mask_host, whose device form downloads its 4-byte status word.
    ``on_device`` False takes the numpy host path, which gives the same bits."""
    _mask_mode(mode, mask)
    _check_fill_mode(fill_holes, mode)
    q, clip, outside = _zscore_settings(percentiles, mode)
    _percentile_pair(q)
    if not on_device:
        if fill_holes:
            mask, mode = nonzero_mask_host(np.asarray(image, dtype=np.float32)), "mask"
        rec = fg_stats_host(image, mask, mode, q)
        return clip_zscore_host(image, stats=rec, mask=mask, mode=mode, clip=clip, outside=outside)
    if fill_holes and np.ndim(image) != 3:
        raise ValueError("expected a 3-D volume, got shape {}".format(np.shape(image)))
    vol = upload(np.asarray(image, dtype=np.float32))
    mvol = None
    try:
        if fill_holes:
            mvol, mode = nonzero_mask_device(vol), "mask"
        elif mask is not None:
            mvol = upload(np.asarray(mask).astype(np.int32))
        rec = fg_stats_device(vol, mvol, mode, q)
        out = clip_zscore_device(vol, stats=rec, mask=mvol, mode=mode, clip=clip, outside=outside).numpy()
        rec.free()
    finally:
        vol.free()
        if mvol is not None:
            mvol.free()
    return out


def crop_to_nonzero(image, label=None, on_device=True):
    """nnU-Net's crop_to_nonzero on host arrays -> (image, label, box): both cut to the bounding box of the image's non-zero
    voxels, box = {d0, h0, w0, d1, h1, w1, count, 0}; an empty volume is returned whole.  ``on_device`` False slices in numpy."""
    image = np.asarray(image)
    if label is not None and np.asarray(label).shape != image.shape:
        raise ValueError("the label must have the image's shape")
    if on_device:
        vol = upload(image)
        rec = nonzero_bbox_device(vol)
        box = rec.numpy()
        rec.free()
        vol.free()
    else:
        box = nonzero_bbox_host(image)
    if box[6] == 0:
        return image, label, box
    sl = tuple(slice(int(a), int(b)) for a, b in zip(box[:3], box[3:6]))
    return image[sl], (None if label is None else np.asarray(label)[sl]), box


class ForegroundFingerprint:
    """nnU-Net's dataset fingerprint, the exact part of it: per case the statistics of the image voxels under the label's
    foreground (label > 0), gathered on the device; the records stay there until ``result()`` downloads them once.

    Dataset-pooled percentiles are not a function of per-case records and are out of scope: a caller who wants them runs
    fg_stats_device on a concatenated flat buffer of the cases' voxels."""

    def __init__(self, percentiles=(0.5, 99.5)):
        self.percentiles = tuple(_percentile_pair(percentiles))
        self._records = []

    def add(self, img_vol: DeviceVolume, label_vol: DeviceVolume):
        """enqueue fg_stats_device with the label as the mask; nothing synchronises"""
        self._records.append(fg_stats_device(img_vol, label_vol, "mask", self.percentiles))

    def result(self):
        """download the records (one synchronisation per call) -> a dict: pooled ``n``, ``min``, ``max``, ``mean`` and ``std``
        from the n / sum / sumsq summed over the cases in float64 in case order, and the per-case records and percentiles"""
        recs = np.stack([r.numpy() for r in self._records]) if self._records else np.zeros((0, 16), np.float64)
        seen = recs[recs[:, 0] > 0]
        n = s = ss = np.float64(0.0)
        for r in recs:
            n, s, ss = n + r[0], s + r[3], ss + r[4]
        out = {"n": int(n), "records": recs, "percentiles": recs[:, 7:9].copy(), "min": None, "max": None, "mean": None, "std": None}
        if n > 0:
            mean = s / n
            out.update(min=float(seen[:, 1].min()), max=float(seen[:, 2].max()), mean=float(mean),
                       std=float(np.sqrt(max(ss / n - mean * mean, np.float64(0.0)))))
        return out

    def free(self):
        for r in self._records:
            r.free()
        self._records = []


def _upload(image, dev, pooled) -> DeviceVolume:
    dev = dev or get_device()
    a = np.asarray(image)
    if a.ndim != 3:
        raise ValueError("expected a 3-D volume, got shape {}".format(a.shape))
    a = np.ascontiguousarray(a, dtype=np.int32 if np.issubdtype(a.dtype, np.integer) else np.float32)
    v = _new_volume(dev, a.shape, a.dtype, pooled)
    dev.h2d(v.ptr, a)
    return v


def upload_pooled(image, dev=None) -> DeviceVolume:
    """Host volume -> pooled device buffer (loader path of the device augmentations)."""
    return _upload(image, dev, True)


def upload(image, dev=None) -> DeviceVolume:
    """Host volume (integers as int32, anything else as float32) -> device volume of its own allocation."""
    return _upload(image, dev, False)


def resample_device(vol: DeviceVolume, new_shape, order=1, pooled=False) -> DeviceVolume:
    dev = vol.dev
    new_shape = tuple(int(s) for s in new_shape)
    _check_order(vol, order)
    if order == 3:
        return _spline_device(vol, (0, 0, 0) + vol.shape, new_shape, pooled)
    res = _new_volume(dev, new_shape, vol.dtype, pooled)
    dev.call("msk_resample3d", C.c_void_p(vol.ptr), *vol.shape, C.c_void_p(res.ptr), *new_shape, int(order), _dt(vol))
    return res


def resample(image, spacing=None, new_spacing=[1.0, 1.0, 1.0], new_shape=None, order=1):
    """reference geometry.py:31-69 -> (array, new_spacing)."""
    image = np.asarray(image)
    if new_shape is None:
        spacing = np.array([spacing[0], spacing[1], spacing[2]])
        new_shape = np.round(image.shape * spacing / new_spacing)
    else:
        new_shape = np.array(new_shape)
        if spacing is not None and len(spacing) == 4:
            spacing = spacing[1:]
        new_spacing = tuple((image.shape / new_shape) * spacing) if spacing is not None else None
    src_dtype = image.dtype
    vol = upload(image)
    out = resample_device(vol, [int(s) for s in new_shape], order)
    res = out.numpy()
    vol.free()
    out.free()
    if res.dtype != src_dtype and (np.issubdtype(src_dtype, np.integer) or src_dtype == np.float64):
        res = res.astype(src_dtype)
    return res, new_spacing


def HUnorm_device(vol: DeviceVolume, HU_min=-1200, HU_max=600, HU_nan=-2000) -> DeviceVolume:
    """reference values.py:67-87, in place."""
    vol.dev.call("msk_hu_norm", C.c_void_p(vol.ptr), C.c_void_p(vol.ptr), C.c_size_t(vol.size), C.c_float(HU_min),
                 C.c_float(HU_max), C.c_float(HU_nan))
    return vol


def normalize_device(vol: DeviceVolume, min_val=None, max_val=None) -> DeviceVolume:
    """reference values.py:54-64, in place."""
    use = 0 if (min_val is None and max_val is None) else 1
    vol.dev.call("msk_minmax_norm", C.c_void_p(vol.ptr), C.c_void_p(vol.ptr), C.c_size_t(vol.size), use,
                 C.c_float(min_val or 0.0), C.c_float(max_val or 0.0))
    return vol


def _on_host_array(op, image, *args):
    """a float32 copy of `image` through one in-place device op and back"""
    vol = upload(np.asarray(image, dtype=np.float32))
    out = op(vol, *args).numpy()
    vol.free()
    return out


def HUnorm(image, HU_min=-1200, HU_max=600, HU_nan=-2000):
    """reference values.py:67-87."""
    return _on_host_array(HUnorm_device, image, HU_min, HU_max, HU_nan)


def normalize(image, min_val=None, max_val=None):
    """reference values.py:54-64."""
    return _on_host_array(normalize_device, image, min_val, max_val)


def max_normalize(image):
    """transforms/transform.py:67-69: im/im.max() if max > 0, plus the channel axis."""
    return np.expand_dims(_on_host_array(max_normalize_device, image), axis=0)


def label_remap(label, map_dict=None):
    """reference values.py:37-51 (sequential key -> value passes)."""
    vol = upload(np.asarray(label).astype(np.int32))
    dev = vol.dev
    keys = np.array(list(map_dict.keys()), dtype=np.int32)
    vals = np.array(list(map_dict.values()), dtype=np.int32)
    kp, vp = dev.malloc(max(keys.nbytes, 4)), dev.malloc(max(vals.nbytes, 4))
    if len(keys):
        dev.h2d(kp, keys)
        dev.h2d(vp, vals)
    dev.call("msk_label_remap", C.c_void_p(vol.ptr), C.c_size_t(vol.size), C.c_void_p(kp), C.c_void_p(vp), len(keys))
    out = vol.numpy().astype(np.asarray(label).dtype)
    vol.free()
    dev.free(kp)
    dev.free(vp)
    return out


class DevicePipeline:
    """In-loop preprocessing that never returns to the host: raw volume -> pinned staging buffer ->
    asynchronous H2D copy -> HIP kernels -> model input tensor.

    Mirrors the op lists of the reference's prepare scripts
    (tools/prepare_lung_coronavirus.py:81-90: [HUnorm, resample(128^3, order 1)];
    tools/prepare_mri_spine_seg.py:71-80: [normalize(0, 2650), resample([512,512,12], 1)]) followed by
    Compose's max-normalisation (transforms/transform.py:67-69).  Labels take `resample(order=0)`.

        pipe = DevicePipeline()
        x = pipe.image(raw).HUnorm().resample([128, 128, 128], 1).max_normalize().tensor()
        y = pipe.label(raw_label).resample([128, 128, 128], 0).int_tensor()
    """

    def __init__(self, dev=None, pooled=False):
        """pooled: device buffers come from (and intermediate ones return to) the stream-ordered pool instead of
        hipMalloc / hipFree per op -- hipFree synchronises the whole device, which an in-loop pipeline running BESIDE a
        training step (a second Device() = a second stream, tools/bench_workloads.py --inloop-preprocess) cannot afford;
        the caller hands a finished sample's buffers back with release()."""
        self.dev = dev or get_device()
        self._pinned = [None, 0]
        self.pooled = bool(pooled)

    def release(self, *tensors):
        """return the buffers of finished samples (tensor() / int_tensor() results) to the pool: the NEXT op enqueued on this
        pipeline's stream may overwrite them, so order that stream behind their last reader first (Device.wait_for)"""
        for t in tensors:
            if t is not None and getattr(t, "_pool_bytes", 0):
                _pool_release(self.dev, t.ptr, t._pool_bytes)
                t._pool_bytes = 0

    def _stage(self, a: np.ndarray) -> DeviceVolume:
        dev = self.dev
        a = np.ascontiguousarray(a)
        if self._pinned[1] < a.nbytes:
            if self._pinned[0]:
                dev.sync()
                dev.call("msk_pinned_free", C.c_void_p(self._pinned[0]))
            p = C.c_void_p()
            dev.call("msk_pinned_alloc", C.c_size_t(a.nbytes), C.byref(p))
            self._pinned = [p.value, a.nbytes]
        else:
            dev.sync()  # the previous copy out of the staging buffer must have drained
        C.memmove(self._pinned[0], a.ctypes.data, a.nbytes)
        vol = _new_volume(dev, a.shape, a.dtype, self.pooled)
        dev.call("msk_h2d_async", C.c_void_p(vol.ptr), C.c_void_p(self._pinned[0]), C.c_size_t(a.nbytes))
        return vol

    def from_pinned(self, pinned_ptr: int, shape, dtype=np.float32) -> "_Chain":
        """a raw volume that already sits in PINNED host memory (msk_pinned_alloc: a loader that reads into pinned buffers):
        one asynchronous copy, no staging memmove and no host synchronisation -- the caller keeps the buffer unchanged until the
        copy has run"""
        dev = self.dev
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * 4
        vol = _new_volume(dev, shape, dtype, self.pooled)
        dev.call("msk_h2d_async", C.c_void_p(vol.ptr), C.c_void_p(pinned_ptr), C.c_size_t(nbytes))
        return _Chain(self, vol)

    def image(self, raw) -> "_Chain":
        return _Chain(self, self._stage(np.asarray(raw, dtype=np.float32)))

    def label(self, raw) -> "_Chain":
        return _Chain(self, self._stage(np.asarray(raw).astype(np.int32)))


class _Chain:
    def __init__(self, pipe, vol):
        self.pipe, self.vol = pipe, vol

    def HUnorm(self, HU_min=-1200, HU_max=600, HU_nan=-2000):
        HUnorm_device(self.vol, HU_min, HU_max, HU_nan)
        return self

    def normalize(self, min_val=None, max_val=None):
        normalize_device(self.vol, min_val, max_val)
        return self

    def resample(self, new_shape, order=1):
        out = resample_device(self.vol, new_shape, order, pooled=self.pipe.pooled)
        old, self.vol = self.vol, out
        # the source is still being read by the enqueued kernel: free() synchronises first
        old.free()
        return self

    def max_normalize(self):
        max_normalize_device(self.vol)
        return self

    def crop_to_nonzero(self):
        """cut to the bounding box of the non-zero voxels (crop_to_nonzero_device: one 32-byte download, the chain's only
        synchronisation); the record stays in ``self.box``"""
        out, _, self.box = crop_to_nonzero_device(self.vol)
        if out is not self.vol:
            old, self.vol = self.vol, out
            old.free()
        return self

    def ct_normalize(self, lo, hi, mean, std):
        """nnU-Net's CTNormalization with the plan's values, in place"""
        clip_zscore_device(self.vol, lo=lo, hi=hi, mean=mean, std=std)
        return self

    def zscore(self, percentiles=None, mode="all", fill_holes=False):
        """nnU-Net's ZScoreNormalization of this volume, in place: statistics of all voxels or of the non-zero ones (outside
        them the result is 0), after clipping to the two ``percentiles`` when given; the record never leaves the device.
        ``fill_holes=True`` with mode 'nonzero' normalises under nnU-Net's hole-filled mask (nonzero_mask_device: zero voxels
        enclosed by the body are inside); that downloads the 4-byte status word of the hole filling, and the mask goes back to
        the pool afterwards"""
        if mode not in ("all", "nonzero"):
            raise ValueError("a chain z-scores over 'all' or 'nonzero' voxels, got {!r}".format(mode))
        _check_fill_mode(fill_holes, mode)
        q, clip, outside = _zscore_settings(percentiles, mode)
        mask = nonzero_mask_device(self.vol) if fill_holes else None
        mode = "mask" if fill_holes else mode
        rec = None
        try:
            rec = fg_stats_device(self.vol, mask, mode, q)
            clip_zscore_device(self.vol, stats=rec, mask=mask, mode=mode, clip=clip, outside=outside)
        finally:
            if rec is not None:
                rec.free()
            if mask is not None:
                mask.free()
        return self

    def tensor(self):
        """[1, 1, D, H, W] model input (one channel: NDHWC and NCDHW coincide); keeps the buffer."""
        from .device import Tensor
        d, h, w = self.vol.shape
        t = Tensor(self.vol.dev, self.vol.ptr, 1, d, h, w, 1, 1, None)
        t._pool_bytes = self.vol.size * 4 if self.vol.pooled else 0      # DevicePipeline.release
        return t

    def int_tensor(self):
        from .device import IntTensor
        t = IntTensor(self.vol.dev, self.vol.ptr, (1,) + tuple(self.vol.shape))
        t._pool_bytes = self.vol.size * 4 if self.vol.pooled else 0
        return t

    def numpy(self):
        return self.vol.numpy()

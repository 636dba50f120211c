"""Loader-side augmentation with the reference's class names, constructor arguments and
RANDOM-NUMBER STREAMS (medicalseg/transforms/transform.py:28-396): under the same
``random.seed`` / ``np.random.seed`` every class draws the same crop boxes, angles, planes and
flip axes as the reference's (pinned by tests/golden/transforms_golden.npz), so a YAML file and
a seed reproduce the reference's augmentation sequence.

Two execution paths share the parameter sampling:
  * host arrays (numpy in, numpy out) -- scipy, like the reference;
  * device volumes (``preprocess.DeviceVolume`` in and out) -- the HIP kernels msk_flip3d,
    msk_rotate3d, msk_crop_resample3d, selected with
    ``Compose(..., device=True)`` / ``device_aug: True`` on a dataset.

``Compose`` ends with the per-volume max normalisation and the channel axis (:64-69).
"""
import collections.abc
import numbers
import random

import numpy as np
import scipy.ndimage

from ..cvlibs import manager


def _on_device(x):
    from ..preprocess import DeviceVolume
    return isinstance(x, DeviceVolume)


def _swap(old, new):
    """Release the input buffer of a device op (stream-ordered pool) and pass the result on."""
    if old is not new:
        old.free()
    return new


class Compose:
    def __init__(self, transforms, device=False):
        if not isinstance(transforms, list):
            raise TypeError('The transforms must be a list!')
        self.transforms = transforms
        self.device = bool(device)

    def __call__(self, im, label=None):
        if isinstance(im, str):
            im = np.load(im)
        if isinstance(label, str):
            label = np.load(label)
        if im is None:
            raise ValueError("Can't read the image file")
        if self.device and not _on_device(im):
            from ..preprocess import upload_pooled
            im = upload_pooled(np.asarray(im, dtype=np.float32))
            if label is not None:
                label = upload_pooled(np.asarray(label).astype(np.int32))
        for op in self.transforms:
            outputs = op(im, label)
            im = outputs[0]
            if len(outputs) == 2:
                label = outputs[1]
        if _on_device(im):
            from ..preprocess import max_normalize_device
            return (max_normalize_device(im), label)  # [D,H,W] on the device == [1,D,H,W] (one channel)
        im = np.expand_dims(im, axis=0)
        if im.max() > 0:
            im = im / im.max()
        return (im, label)


def _zoom_to(img, size, order):
    """functional.py:49-58: ndimage.zoom(img, size/shape, mode='nearest', order)."""
    factors = np.array(size) / np.array(img.shape[:3])
    return scipy.ndimage.zoom(img, factors, mode="nearest", order=order)


def _resize(img, size, order):
    """functional.py:25-58 resize_3d: an int size fixes the SHORTEST side and keeps the aspect."""
    d, h, w = img.shape[:3]
    if isinstance(size, int):
        short = min(d, h, w)
        if short == size:
            return img
        size = (int(size * d / short), int(size * h / short), int(size * w / short))
    if _on_device(img):
        from ..preprocess import resized_crop_device
        return resized_crop_device(img, 0, 0, 0, d, h, w, size, order)
    return _zoom_to(img, size, order)


@manager.TRANSFORMS.add_component
class Resize3D:
    def __init__(self, size, order=1):
        if isinstance(size, int):
            self.size = size
        elif isinstance(size, collections.abc.Iterable) and len(size) == 3:
            self.size = tuple(size)
        else:
            raise ValueError('Unknown inputs for size: {}'.format(size))
        self.order = order

    def __call__(self, img, label=None):
        out = _resize(img, self.size, self.order)
        img = _swap(img, out) if _on_device(img) else out
        if label is not None:
            out = _resize(label, self.size, 0)
            label = _swap(label, out) if _on_device(label) else out
        return img, label


@manager.TRANSFORMS.add_component
class RandomRotation3D:
    """One random in-plane rotation; the reference rotates image AND label with order 1,
    cval 0 (transform.py:162-167 -> functional.py:91 defaults), reproduced here."""

    def __init__(self, degrees, rotate_planes=[[0, 1], [0, 2], [1, 2]]):
        if isinstance(degrees, numbers.Number):
            if degrees < 0:
                raise ValueError("If degrees is a single number, it must be positive.")
            self.degrees = (-degrees, degrees)
        else:
            if len(degrees) != 2:
                raise ValueError("If degrees is a sequence, it must be of len 2.")
            self.degrees = degrees
        self.rotate_planes = rotate_planes

    def get_params(self, degrees):
        angle = random.uniform(degrees[0], degrees[1])
        r_plane = self.rotate_planes[random.randint(0, len(self.rotate_planes) - 1)]
        return angle, r_plane

    @staticmethod
    def _rotate(vol, r_plane, angle):
        if _on_device(vol):
            from ..preprocess import rotate_device
            return _swap(vol, rotate_device(vol, r_plane, angle, order=1, cval=0))
        return scipy.ndimage.rotate(vol, angle=angle, axes=r_plane, order=1, cval=0, reshape=False)

    def __call__(self, img, label=None):
        angle, r_plane = self.get_params(self.degrees)
        img = self._rotate(img, r_plane, angle)
        if label is not None:
            label = self._rotate(label, r_plane, angle)
        return img, label


@manager.TRANSFORMS.add_component
class RandomFlip3D:
    def __init__(self, prob=0.5, flip_axis=[0, 1, 2]):
        self.prob = prob
        self.flip_axis = flip_axis

    @staticmethod
    def _flip(vol, axis):
        if _on_device(vol):
            from ..preprocess import flip_device
            return _swap(vol, flip_device(vol, axis))
        return np.flip(vol, axis)

    def __call__(self, img, label=None):
        # the axis is drawn BEFORE the coin (transform.py:193-199)
        if isinstance(self.flip_axis, (tuple, list)):
            flip_axis = self.flip_axis[random.randint(0, len(self.flip_axis) - 1)]
        else:
            flip_axis = self.flip_axis
        if random.random() < self.prob:
            img = self._flip(img, flip_axis)
            if label is not None:
                label = self._flip(label, flip_axis)
        return img, label


CropBox = collections.namedtuple('CropBox', ['i', 'j', 'k', 'd', 'h', 'w'])


@manager.TRANSFORMS.add_component
class RandomResizedCrop3D:
    """Random crop box (volume ``scale`` x the input, aspect jitter ``ratio``) resized to ``size``;
    image with order ``interpolation``, label with order 0.  ``pre_crop`` first cuts a box of about
    ``size`` (optionally inside the label's non-zero bounding box) -- transform.py:207-339."""

    def __init__(self, size, scale=(0.8, 1.2), ratio=(3. / 4., 4. / 3.), interpolation=1, pre_crop=False,
                 nonzero_mask=False):
        if isinstance(size, (tuple, list)):
            assert len(size) == 3, \
                "Size must contain THREE number when it is a tuple or list, got {}.".format(len(size))
            self.size = size
        elif isinstance(size, int):
            self.size = (size, size, size)
        else:
            raise ValueError("Size must be an int, list or tuple, got {}.".format(type(size)))
        self.interpolation = interpolation
        self.scale = scale
        self.ratio = ratio
        self.pre_crop = pre_crop
        self.nonzero_mask = nonzero_mask

    def get_params(self, img, scale, ratio):
        """Up to ten attempts (transform.py:246-276): target volume and aspect -> (d, h), w = full
        width, an optional shuffle of the three sides, accepted when the box fits; else the
        centred cube of the shortest side."""
        D, H, W = img.shape[0], img.shape[1], img.shape[2]
        for _ in range(10):
            target = random.uniform(*scale) * (D * H * W)
            aspect = random.uniform(*ratio)
            d = int(round((target * aspect) ** (1 / 3)))
            h = int(round((target / aspect) ** (1 / 3)))
            w = W
            if random.random() < 0.5:
                d, h, w = random.sample([d, h, w], k=3)
            if w <= W and h <= H and d <= D:
                i = random.randint(0, D - d)
                j = random.randint(0, H - h)
                k = random.randint(0, W - w)
                return CropBox(i, j, k, d, h, w)
        side = min(D, H, W)
        return CropBox((D - side) // 2, (H - side) // 2, (W - side) // 2, side, side, side)

    def _pre_crop_box(self, img, label):
        """transform.py:288-318: numpy's global RNG draws the box (3 uniforms, then 3 randints)."""
        crop = (np.random.uniform(low=self.scale[0], high=self.scale[1], size=3) * self.size).round().astype("int")
        if self.nonzero_mask:
            if _on_device(label):
                # the 32-byte record instead of the whole label; an empty label fails as np.min of nothing does on the host
                from ..preprocess import nonzero_bbox_device
                rec = nonzero_bbox_device(label)
                box = rec.numpy()
                rec.free()
                if box[6] == 0:
                    raise ValueError("zero-size array to reduction operation minimum which has no identity")
                lo, hi = box[:3].astype(int), box[3:6].astype(int)
            else:
                nz = np.where(label != 0)
                lo = np.array([int(np.min(c)) for c in nz])
                hi = np.array([int(np.max(c)) + 1 for c in nz])
        else:
            lo = np.zeros(3, dtype=int)
            hi = np.array(img.shape[:3])
        ext = hi - lo
        cz, cy, cx = np.minimum(ext, crop)
        z0 = np.random.randint(ext[0] - cz + 1) + lo[0]
        y0 = np.random.randint(ext[1] - cy + 1) + lo[1]
        x0 = np.random.randint(ext[2] - cx + 1) + lo[2]
        return int(z0), int(y0), int(x0), int(cz), int(cy), int(cx)

    @staticmethod
    def _crop(vol, box):
        z0, y0, x0, cz, cy, cx = box
        if _on_device(vol):
            from ..preprocess import resized_crop_device
            return _swap(vol, resized_crop_device(vol, z0, y0, x0, cz, cy, cx, (cz, cy, cx), 0))  # identity zoom
        return vol[z0:z0 + cz, y0:y0 + cy, x0:x0 + cx]

    def _resized_crop(self, vol, p, order):
        if _on_device(vol):
            from ..preprocess import resized_crop_device
            return _swap(vol, resized_crop_device(vol, p.i, p.j, p.k, p.d, p.h, p.w, self.size, order))
        return _zoom_to(vol[p.i:p.i + p.d, p.j:p.j + p.h, p.k:p.k + p.w], self.size, order)

    def __call__(self, img, label=None):
        if self.pre_crop:
            box = self._pre_crop_box(img, label)
            img = self._crop(img, box)
            if label is not None:
                label = self._crop(label, box)
        p = self.get_params(img, self.scale, self.ratio)
        img = self._resized_crop(img, p, self.interpolation)
        if label is not None:
            label = self._resized_crop(label, p, 0)
        return img, label


def _patch_origin(roi, dim, pos=None, word=0):
    """One axis of a patch origin: a volume no larger than the patch is centred (SlidingPlan's padding: (roi - dim) // 2
    voxels in front); else the patch is centred on `pos` and pushed inside, or, without a centre, starts at
    (word * (dim - roi + 1)) >> 32 -- word a 32-bit integer, so every start is hit and none lies outside."""
    if dim <= roi:
        return -((roi - dim) // 2)
    if pos is None:
        return (int(word) * (dim - roi + 1)) >> 32
    return min(max(pos - roi // 2, 0), dim - roi)


def _patch_select_host(label, roi, num_classes, classes, words):
    """The patch record (d0, h0, w0, cls, cz, cy, cx, 0) msk_patch_select computes, from a host label (or None) and the six
    words (force_fg, w_cls, w_rank, w_d, w_h, w_w); shape is the volume's when there is no label."""
    force, w_cls, w_rank = int(words[0]), int(words[1]), int(words[2])
    if force and label is not None and len(classes):
        lab = np.asarray(label).reshape(-1)
        inside = lab[(lab >= 0) & (lab < num_classes)]
        counts = np.bincount(inside, minlength=num_classes)
        present = [c for c in classes if counts[c] > 0]
        if present:
            cls = int(present[(w_cls * len(present)) >> 32])
            r = (w_rank * int(counts[cls])) >> 32
            centre = [int(v) for v in np.unravel_index(int(np.flatnonzero(lab == cls)[r]), label.shape)]
            return [_patch_origin(ro, dim, c) for ro, dim, c in zip(roi, label.shape, centre)] + [cls] + centre + [0]
    return None


def _patch_crop_host(vol, origin, roi, pad):
    out = np.full(tuple(roi), pad, dtype=vol.dtype)
    src, dst = [], []
    for o, ro, dim in zip(origin, roi, vol.shape):
        lo, hi = max(o, 0), min(o + ro, dim)
        src.append(slice(lo, hi))
        dst.append(slice(lo - o, hi - o))
    out[tuple(dst)] = vol[tuple(src)]
    return out


@manager.TRANSFORMS.add_component
class RandomPatchCrop3D:
    """A fixed-size patch cut at the volume's own resolution, the sampler patch-trained 3D nets use (nnU-Net, MONAI's
    RandCropByPosNegLabel): with probability ``fg_prob`` the patch is centred on a voxel of a randomly chosen class of
    ``classes`` that occurs in the label (every such class equally likely, every voxel of it equally likely), pushed inside the
    volume; otherwise, and when there is no label or none of the classes occurs, its origin is uniform over the positions
    inside the volume.  An axis shorter than the patch is centred and padded with ``pad_value`` (image) / ``label_pad``
    (label).  Volumes of any size come out as ``size``, which is what batching needs.  Not in the reference.

    ``classes=None`` means 1 .. num_classes - 1.  ``label_pad=255``, the datasets' ``ignore_index``, keeps the padding out of
    the loss; the default 0 counts it as background.

    Random stream: every call draws exactly one ``random.random()`` (the coin) and then five ``random.getrandbits(32)``
    (class, rank, and one word per axis), whatever the data and the outcome, so the host and the device path cut the same
    patch under the same seed.  On device volumes the choice is made by msk_patch_select on the device: the label is never
    downloaded and nothing synchronises."""

    def __init__(self, size, num_classes, fg_prob=1. / 3., classes=None, pad_value=0, label_pad=0):
        if isinstance(size, int):
            size = (size, size, size)
        if not isinstance(size, (tuple, list)) or len(size) != 3 or any(int(s) < 1 for s in size):
            raise ValueError("Size must be an int or three positive numbers, got {}.".format(size))
        self.size = tuple(int(s) for s in size)
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= 256:
            raise ValueError("num_classes must be in [1, 256], got {}.".format(num_classes))
        self.fg_prob = float(fg_prob)
        self.classes = list(range(1, self.num_classes)) if classes is None else [int(c) for c in classes]
        if len(self.classes) > 32 or any(not 0 <= c < self.num_classes for c in self.classes) or \
                any(b <= a for a, b in zip(self.classes, self.classes[1:])):
            raise ValueError("classes must be at most 32 strictly ascending classes inside [0, num_classes), got {}.".format(classes))
        self.pad_value = pad_value
        self.label_pad = int(label_pad)

    def get_params(self, have_label=True):
        """the six words of msk_patch_select: force_fg, w_cls, w_rank, w_d, w_h, w_w"""
        coin = random.random()
        words = [random.getrandbits(32) for _ in range(5)]
        return [int(have_label and coin < self.fg_prob)] + words

    def select(self, shape, label, words):
        """host path: the record (d0, h0, w0, cls, cz, cy, cx, 0)"""
        rec = _patch_select_host(label, self.size, self.num_classes, self.classes, words)
        if rec is None:
            rec = [_patch_origin(ro, dim, None, w) for ro, dim, w in zip(self.size, shape, words[3:6])] + [-1, -1, -1, -1, 0]
        return rec

    def _device_crops(self, img, label, sel):
        """the plain patch of the image and of the label (or None) at the origin of the record `sel`"""
        from ..preprocess import patch_crop_device
        return (patch_crop_device(img, sel, self.size, self.pad_value),
                None if label is None else patch_crop_device(label, sel, self.size, self.label_pad))

    def _device_call(self, img, label, words, cut):
        """device path: msk_patch_select, then cut(img, label, sel) -> (patch, label patch or None); the record goes back to
        the pool whether or not the cut is refused, the inputs only once both patches exist"""
        from ..preprocess import patch_select_device
        sel = patch_select_device(img if label is None else label, self.size, self.num_classes,
                                  [] if label is None else self.classes, words)
        try:
            out, out_label = cut(img, label, sel)
        finally:
            sel.free()
        return _swap(img, out), None if label is None else _swap(label, out_label)

    def __call__(self, img, label=None):
        words = self.get_params(label is not None)
        if _on_device(img):
            return self._device_call(img, label, words, self._device_crops)
        origin = self.select(img.shape[:3], label, words)[:3]
        img = _patch_crop_host(img, origin, self.size, self.pad_value)
        if label is not None:
            label = _patch_crop_host(label, origin, self.size, self.label_pad)
        return img, label


# ---- intensity augmentation (nnU-Net / batchgenerators' set; not in the reference) -----------------------------------------
# Host paths: numpy evaluations of tests/intensity_reference.py's statement, float32 throughout.  Device paths: msk_intensity.hip
# through preprocess.intensity_stats_device / intensity_apply_device / gauss_blur_device; the statistics stay on the device.
_MASK64 = 0xFFFFFFFFFFFFFFFF


def _lanes_then_tree(terms):
    """float64 [groups, k, 256] -> [groups]: lane l adds its k terms in order, then the tree v[l] += v[l+s], s = 128 .. 1"""
    acc = np.zeros((terms.shape[0], 256), np.float64)
    for j in range(terms.shape[1]):
        acc = acc + terms[:, j, :]
    s = 128
    while s >= 1:
        acc = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    return acc[:, 0]


def _ordered_sum(v):
    """msk_intensity_stats' float64 sum: chunks of 4096 (256 lanes x 16 strided terms, then the tree), then the chunk values
    by the same scheme; missing elements count as +0.0"""
    nc = -(-v.size // 4096)
    pad = np.zeros(nc * 4096, np.float64)
    pad[:v.size] = v
    p = _lanes_then_tree(pad.reshape(nc, 16, 256))
    rows = -(-nc // 256)
    pad = np.zeros(rows * 256, np.float64)
    pad[:nc] = p
    return float(_lanes_then_tree(pad.reshape(1, rows, 256))[0])


def _stats_host(x):
    """the record {min, max, sum, sumsq} of msk_intensity_stats, bit for bit"""
    d = np.asarray(x, np.float32).reshape(-1).astype(np.float64)
    return np.array([d.min(), d.max(), _ordered_sum(d), _ordered_sum(d * d)], np.float64)


def _splitmix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _noise_host(x, std, seed):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = _splitmix64(_splitmix64(np.uint64(int(seed) & _MASK64)) + np.arange(x.size, dtype=np.uint64))
    u1 = ((h >> np.uint64(40)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
    z = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(2.0 * np.pi) * u2)
    return x + np.float32(std) * z.reshape(x.shape)


def _contrast_host(x, factor, preserve_range):
    x = np.asarray(x, np.float32)
    rec = _stats_host(x)
    m = np.float32(rec[2] / np.float64(x.size))
    y = ((x - m) * np.float32(factor)) + m
    if preserve_range:
        y = np.minimum(np.maximum(y, np.float32(rec[0])), np.float32(rec[1]))
    return y


def _gamma_host(x, gamma, invert, rec):
    x = np.asarray(x, np.float32)
    s = np.float32(-1.0 if invert else 1.0)
    mn, mx = (-np.float32(rec[1]), -np.float32(rec[0])) if invert else (np.float32(rec[0]), np.float32(rec[1]))
    rg = mx - mn
    return s * (np.power((s * x - mn) / (rg + np.float32(1e-7)), np.float32(gamma)) * rg + mn)


def _moments(rec, n):
    mean = rec[2] / np.float64(n)
    var = max(rec[3] / np.float64(n) - mean * mean, 0.0)
    return np.float32(mean), np.float32(np.sqrt(var))


def _restore_host(x, rec_a, rec_b):
    mean_a, sd_a = _moments(rec_a, x.size)
    mean_b, sd_b = _moments(rec_b, x.size)
    return (x - mean_b) / (sd_b + np.float32(1e-8)) * sd_a + mean_a


def _blur_host(x, sigmas):
    from ..preprocess import gauss_taps
    y = np.asarray(x, np.float32)
    for axis, sigma in enumerate(sigmas):
        w = gauss_taps(sigma)
        if not len(w):
            continue
        r, n = (len(w) - 1) // 2, y.shape[axis]
        acc = None
        for k in range(-r, r + 1):
            m = np.mod(np.arange(n) + k, 2 * n)
            term = w[k + r] * np.take(y, np.where(m < n, m, 2 * n - 1 - m), axis=axis)
            acc = term if acc is None else acc + term
        y = acc
    return y


# ---- order-3 resampling on the host: tests/spline_reference.py's statement, float64, one rounding per operator -------------
_SPLINE_PAD = 12
_SPLINE_HORIZON = 47
_SPLINE_Z = np.sqrt(np.float64(3.0)) - np.float64(2.0)
_SPLINE_GAIN = (1.0 - _SPLINE_Z) * (1.0 - 1.0 / _SPLINE_Z)
_SPLINE_LAST = _SPLINE_Z / (_SPLINE_Z * _SPLINE_Z - 1.0)


def _spline_taps(n_in, n_out):
    scale = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(0.0)
    cc = np.arange(n_out, dtype=np.float64) * scale + np.float64(_SPLINE_PAD)
    f = np.floor(cc)
    t = cc - f
    u = 1.0 - t
    w0 = ((u * u) * u) / 6.0
    w1 = (((t * t) * (t - 2.0)) * 3.0 + 4.0) / 6.0
    w2 = (((u * u) * (u - 2.0)) * 3.0 + 4.0) / 6.0
    return f.astype(np.int64) - 1, (w0, w1, w2, ((1.0 - w0) - w1) - w2)


def _spline_zoom_host(x, out_shape):
    """scipy.ndimage.zoom(order=3, mode='nearest') of a float32 volume as msk_spline_resample3d computes it, bit for bit:
    12 edge voxels of padding, the recursive prefilter along each axis (the loop runs along the line, the slices span all
    lines), then 4 x 4 x 4 taps, d outermost and w innermost."""
    z = _SPLINE_Z
    p = np.pad(np.asarray(x, np.float32).astype(np.float64), _SPLINE_PAD, mode="edge")
    for axis in range(3):
        c = np.moveaxis(p, axis, 0)
        n = c.shape[0]
        zn1 = np.float64(1.0)
        for _ in range(n - 1):
            zn1 = zn1 * z
        c *= _SPLINE_GAIN
        zi = z
        c0 = c[0] + zn1 * c[n - 1]
        for i in range(1, min(n - 2, _SPLINE_HORIZON) + 1):
            c0 = c0 + zi * (c[i] + zn1 * c[n - 1 - i])
            zi = zi * z
        c[0] = c0 * (1.0 / (1.0 - zn1 * zn1))
        for i in range(1, n):
            c[i] = c[i] + z * c[i - 1]
        c[n - 1] = _SPLINE_LAST * (c[n - 1] + z * c[n - 2])
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
    out_shape = tuple(int(s) for s in out_shape)
    (sd, wd), (sh, wh), (sw, ww) = (_spline_taps(x.shape[a], out_shape[a]) for a in range(3))
    acc = np.zeros(out_shape, np.float64)
    for a in range(4):
        for b in range(4):
            for k in range(4):
                taps = p[(sd + a)[:, None, None], (sh + b)[None, :, None], (sw + k)[None, None, :]]
                acc = acc + ((taps * wd[a][:, None, None]) * wh[b][None, :, None]) * ww[k][None, None, :]
    return acc.astype(np.float32)


def _nearest_zoom_host(x, out_shape):
    """msk_resample3d order 0 (scipy.ndimage.zoom(order=0, mode='nearest')): the voxel at floor(o (n_in-1)/(n_out-1) + 0.5)"""
    idx = []
    for n_in, n_out in zip(x.shape, out_shape):
        scale = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(0.0)
        i = np.floor(np.arange(int(n_out), dtype=np.float64) * scale + 0.5).astype(np.int64)
        idx.append(np.clip(i, 0, n_in - 1))
    return x[idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]


def _check_prob(prob):
    prob = float(prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError("prob must be in [0, 1], got {}.".format(prob))
    return prob


def _check_range(rng, name, lowest=None, highest=None):
    if isinstance(rng, numbers.Number):
        rng = (rng, rng)
    if not isinstance(rng, (tuple, list)) or len(rng) != 2:
        raise ValueError("{} must be a (low, high) pair, got {}.".format(name, rng))
    lo, hi = float(rng[0]), float(rng[1])
    if not lo <= hi or (lowest is not None and lo < lowest) or (highest is not None and hi > highest):
        raise ValueError("{} must be an ordered range inside [{}, {}], got {}.".format(name, lowest, highest, rng))
    return (lo, hi)


def _value(rng, u):
    return rng[0] + (rng[1] - rng[0]) * u


def _branch_value(rng, coin, u):
    """batchgenerators' draw for contrast and gamma: below 1 on one side of the coin, above on the other"""
    lo, hi = rng
    return _value((lo, 1.0) if coin < 0.5 and lo < 1 else (max(lo, 1.0), hi), u)


@manager.TRANSFORMS.add_component
class RandomGaussianNoise3D:
    """With probability ``prob``: image + std * z, z standard normal from the counter RNG of msk_intensity_apply (splitmix64 of
    the voxel's raster index, Box-Muller), std uniform in ``std``.  The label passes through.  Not in the reference.

    Random stream, whatever the coin: ``random.random()`` (coin), ``random.random()`` (std), ``random.getrandbits(64)``."""

    def __init__(self, prob=0.1, std=(0.0, 0.1)):
        self.prob = _check_prob(prob)
        self.std = _check_range(std, "std", lowest=0.0)

    def get_params(self):
        coin, u, seed = random.random(), random.random(), random.getrandbits(64)
        return coin < self.prob, float(np.float32(_value(self.std, u))), seed

    def __call__(self, img, label=None):
        fire, std, seed = self.get_params()
        if fire:
            if _on_device(img):
                from ..preprocess import INTENSITY_NOISE, intensity_apply_device
                intensity_apply_device(img, INTENSITY_NOISE, [std], seed=seed)
            else:
                img = _noise_host(img, std, seed)
        return img, label


@manager.TRANSFORMS.add_component
class RandomGaussianBlur3D:
    """With probability ``prob``: a separable Gaussian blur (scipy's mode='reflect', truncate 4), sigma uniform in ``sigma``
    (at most 2), one value for all axes or, with ``per_axis``, one per axis.  The label passes through.  Not in the reference.

    Random stream, whatever the coin: ``random.random()`` (coin) and three more; without ``per_axis`` the first of the three
    sets every axis."""

    def __init__(self, prob=0.2, sigma=(0.5, 1.0), per_axis=False):
        from ..preprocess import GAUSS_MAX_SIGMA
        self.prob = _check_prob(prob)
        self.sigma = _check_range(sigma, "sigma", lowest=0.0, highest=GAUSS_MAX_SIGMA)
        self.per_axis = bool(per_axis)

    def get_params(self):
        coin = random.random()
        u = [random.random() for _ in range(3)]
        if not self.per_axis:
            u = [u[0]] * 3
        return coin < self.prob, [_value(self.sigma, v) for v in u]

    def __call__(self, img, label=None):
        fire, sigmas = self.get_params()
        if fire:
            if _on_device(img):
                from ..preprocess import gauss_blur_device
                img = _swap(img, gauss_blur_device(img, sigmas))
            else:
                img = _blur_host(img, sigmas)
        return img, label


@manager.TRANSFORMS.add_component
class RandomBrightness3D:
    """With probability ``prob``: image * factor, factor uniform in ``factor`` (nnU-Net's multiplicative brightness).  The
    label passes through.  Not in the reference.  Random stream, whatever the coin: ``random.random()`` twice."""

    def __init__(self, prob=0.15, factor=(0.75, 1.25)):
        self.prob = _check_prob(prob)
        self.factor = _check_range(factor, "factor")

    def get_params(self):
        coin, u = random.random(), random.random()
        return coin < self.prob, float(np.float32(_value(self.factor, u)))

    def __call__(self, img, label=None):
        fire, factor = self.get_params()
        if fire:
            if _on_device(img):
                from ..preprocess import INTENSITY_SCALE, intensity_apply_device
                intensity_apply_device(img, INTENSITY_SCALE, [factor])
            else:
                img = np.asarray(img, np.float32) * np.float32(factor)
        return img, label


@manager.TRANSFORMS.add_component
class RandomContrast3D:
    """With probability ``prob``: (image - mean) * factor + mean, clamped to the image's own [min, max] with
    ``preserve_range`` (batchgenerators' ContrastAugmentationTransform: a second coin picks the part of ``factor`` below or
    above 1).  The mean is msk_intensity_stats' ordered float64 sum / n on both paths.  The label passes through.  Not in the
    reference.  Random stream, whatever the coin: ``random.random()`` three times (coin, branch, value)."""

    def __init__(self, prob=0.15, factor=(0.75, 1.25), preserve_range=True):
        self.prob = _check_prob(prob)
        self.factor = _check_range(factor, "factor", lowest=0.0)
        self.preserve_range = bool(preserve_range)

    def get_params(self):
        coin, branch, u = random.random(), random.random(), random.random()
        return coin < self.prob, float(np.float32(_branch_value(self.factor, branch, u)))

    def __call__(self, img, label=None):
        fire, factor = self.get_params()
        if fire:
            if _on_device(img):
                from ..preprocess import INTENSITY_CONTRAST, intensity_apply_device, intensity_stats_device
                rec = intensity_stats_device(img)
                intensity_apply_device(img, INTENSITY_CONTRAST, [factor, float(self.preserve_range)], stats_a=rec)
                rec.free()
            else:
                img = _contrast_host(img, factor, self.preserve_range)
        return img, label


@manager.TRANSFORMS.add_component
class RandomGamma3D:
    """With probability ``prob``: batchgenerators' augment_gamma -- the image (negated first with ``invert``) is scaled to
    [0, 1] by its own range, raised to gamma (drawn like RandomContrast3D's factor), scaled back (and negated back); with
    ``retain_stats`` the result is then shifted and scaled to the mean and standard deviation the image had before.  The
    label passes through.  Not in the reference.  Random stream, whatever the coin: ``random.random()`` three times."""

    def __init__(self, prob=0.3, gamma=(0.7, 1.5), invert=False, retain_stats=True):
        self.prob = _check_prob(prob)
        self.gamma = _check_range(gamma, "gamma", lowest=0.0)
        if self.gamma[0] <= 0.0:
            raise ValueError("gamma must be positive, got {}.".format(gamma))
        self.invert = bool(invert)
        self.retain_stats = bool(retain_stats)

    def get_params(self):
        coin, branch, u = random.random(), random.random(), random.random()
        return coin < self.prob, float(np.float32(_branch_value(self.gamma, branch, u)))

    def __call__(self, img, label=None):
        fire, gamma = self.get_params()
        if fire:
            if _on_device(img):
                from ..preprocess import INTENSITY_GAMMA, INTENSITY_RESTORE, intensity_apply_device, intensity_stats_device
                before = intensity_stats_device(img)
                intensity_apply_device(img, INTENSITY_GAMMA, [gamma, float(self.invert)], stats_a=before)
                if self.retain_stats:
                    after = intensity_stats_device(img)
                    intensity_apply_device(img, INTENSITY_RESTORE, [], stats_a=before, stats_b=after)
                    after.free()
                before.free()
            else:
                img = np.asarray(img, np.float32)
                before = _stats_host(img)
                img = _gamma_host(img, gamma, self.invert, before)
                if self.retain_stats:
                    img = _restore_host(img, before, _stats_host(img))
        return img, label


@manager.TRANSFORMS.add_component
class RandomLowResolution3D:
    """With probability ``prob``: nnU-Net's SimulateLowResolutionTransform -- the image is shrunk to
    ``max(1, round(n * zoom))`` voxels per axis with order 0 (nearest) and brought back to its extent with order 3 (cubic
    B-spline), zoom uniform in ``zoom`` (inside (0, 1]), one value for all axes or, with ``per_axis``, one per axis.  Both
    steps use this project's ``scipy.ndimage.zoom(mode='nearest')`` geometry (corner-aligned coordinates); batchgenerators
    resizes with skimage's pixel-centre map, so the voxels differ from its output although the recipe is the same.  The label
    passes through.  Not in the reference.

    Random stream, whatever the coin and the data: ``random.random()`` (coin), then one more, or three with ``per_axis``.
    Host arrays go through ``_nearest_zoom_host`` / ``_spline_zoom_host``, device volumes through
    ``preprocess.resample_device`` with order 0 and then 3; both are tests/spline_reference.py's statement bit for bit, so
    one ``random.seed`` gives one result on either path."""

    def __init__(self, prob=0.25, zoom=(0.5, 1.0), per_axis=False):
        self.prob = _check_prob(prob)
        self.zoom = _check_range(zoom, "zoom", lowest=0.0, highest=1.0)
        if self.zoom[0] <= 0.0:
            raise ValueError("zoom must be positive, got {}.".format(zoom))
        self.per_axis = bool(per_axis)

    def get_params(self):
        coin = random.random()
        u = [random.random() for _ in range(3 if self.per_axis else 1)]
        if not self.per_axis:
            u = u * 3
        return coin < self.prob, [_value(self.zoom, v) for v in u]

    def __call__(self, img, label=None):
        fire, zooms = self.get_params()
        if fire:
            shape = tuple(int(s) for s in img.shape[:3])
            small = tuple(max(1, int(round(n * z))) for n, z in zip(shape, zooms))
            if _on_device(img):
                from ..preprocess import resample_device
                low = resample_device(img, small, 0, pooled=True)
                out = resample_device(low, shape, 3, pooled=True)
                low.free()
                img = _swap(img, out)
            else:
                img = _spline_zoom_host(_nearest_zoom_host(np.asarray(img, np.float32), small), shape)
        return img, label


def _connected_components(binary_mask, minimum_volume=0):
    """functional.py:117-131 (SimpleITK ConnectedComponent + RelabelComponent): face-connected
    components relabelled 1, 2, ... by decreasing size, components smaller than
    ``minimum_volume`` dropped.  SimpleITK is absent from this image; scipy.ndimage.label uses
    the same 6-connectivity."""
    vals = np.unique(binary_mask)
    assert len(vals) < 3, "Only binary mask is accepted, got mask with {}.".format(vals.tolist())
    lab, n = scipy.ndimage.label(np.asarray(binary_mask) != 0)
    if n == 0:
        return lab.astype(np.uint32)
    sizes = np.bincount(lab.ravel())[1:]
    order = np.argsort(-sizes, kind="stable")
    lut = np.zeros(n + 1, dtype=np.uint32)
    rank = 1
    for comp in order:
        if sizes[comp] >= minimum_volume:
            lut[comp + 1] = rank
            rank += 1
    return lut[lab]


def _cc_on_device(x):
    from ..device import IntTensor
    return _on_device(x) or isinstance(x, IntTensor)


def _cc_device(x, minimum_volume=0, k=0):
    """a DeviceVolume is released like the other device ops' inputs (_swap); an IntTensor (inference()'s prediction,
    arena memory) is left as it is"""
    from ..preprocess import connected_components_device
    out = connected_components_device(x, minimum_volume, k)
    return _swap(x, out) if _on_device(x) else out


# ---- rotated and scaled patch crop (nnU-Net's spatial augmentation without the elastic part; not in the reference) ---------
def _affine_matrix(angles_deg, scales):
    """M = Rd . Rh . Rw . diag(scales): right-handed rotations about the D, H and W axes, angles in degrees, computed in
    float64 and rounded to float32 once (tests/affine_reference.py).  Rows are source axes, columns patch axes."""
    import math
    c = [math.cos(math.radians(float(a))) for a in angles_deg]
    s = [math.sin(math.radians(float(a))) for a in angles_deg]
    rd = np.array([[1.0, 0.0, 0.0], [0.0, c[0], -s[0]], [0.0, s[0], c[0]]], np.float64)
    rh = np.array([[c[1], 0.0, s[1]], [0.0, 1.0, 0.0], [-s[1], 0.0, c[1]]], np.float64)
    rw = np.array([[c[2], -s[2], 0.0], [s[2], c[2], 0.0], [0.0, 0.0, 1.0]], np.float64)
    return (rd @ rh @ rw @ np.diag(np.asarray(scales, np.float64))).astype(np.float32)


def _affine_gather(vol, idx, outside):
    ok = np.ones(idx[0].shape, bool)
    clipped = []
    for i, n in zip(idx, vol.shape):
        ok &= (i >= 0) & (i < n)
        clipped.append(np.clip(i, 0, n - 1))
    return np.where(ok, vol[tuple(clipped)], outside)


def _affine_patch_host(img, label, origin, roi, m, pad, label_pad, field=None):
    """msk_affine_patch in numpy, float32 throughout, every operation rounded on its own: the grid of the patch, centred on
    origin + roi // 2, through the matrix; the image trilinearly (W, then H, then D; ``pad`` outside the volume), the label
    at floor(p + 0.5) (``label_pad`` outside).  Equal to tests/affine_reference.py bit for bit.  With ``field`` (float32
    [3, rd, rh, rw], _elastic_field_host) the offsets are displaced before the matrix, msk_affine_patch_elastic: equal to
    tests/elastic_reference.py bit for bit."""
    img = np.asarray(img, np.float32)
    m = np.asarray(m, np.float32).reshape(3, 3)
    oz, oy, ox = ((np.arange(r) - r // 2).astype(np.float32).reshape(sh)
                  for r, sh in zip(roi, ((-1, 1, 1), (1, -1, 1), (1, 1, -1))))
    if field is not None:
        field = np.asarray(field, np.float32)
        oz, oy, ox = oz + field[0], oy + field[1], ox + field[2]
    p = [((m[a, 0] * oz + m[a, 1] * oy) + m[a, 2] * ox) + np.float32(int(origin[a]) + int(roi[a]) // 2) for a in range(3)]
    f = [np.floor(v) for v in p]
    t = [v - fl for v, fl in zip(p, f)]
    i0 = [fl.astype(np.int64) for fl in f]
    pad = np.float32(pad)

    def lerp(a, b, w):
        return a + w * (b - a)

    def along_w(dz, dy):
        return lerp(_affine_gather(img, (i0[0] + dz, i0[1] + dy, i0[2]), pad),
                    _affine_gather(img, (i0[0] + dz, i0[1] + dy, i0[2] + 1), pad), t[2])
    out = lerp(lerp(along_w(0, 0), along_w(0, 1), t[1]), lerp(along_w(1, 0), along_w(1, 1), t[1]), t[0])
    if label is None:
        return out, None
    near = [np.floor(v + np.float32(0.5)).astype(np.int64) for v in p]
    return out, _affine_gather(np.asarray(label), near, np.asarray(label).dtype.type(label_pad))


@manager.TRANSFORMS.add_component
class RandomAffinePatchCrop3D(RandomPatchCrop3D):
    """RandomPatchCrop3D whose patch is, with probability ``rotate_prob``, rotated about all three axes and, with
    probability ``scale_prob``, zoomed -- nnU-Net's spatial augmentation: the sampling grid of the patch is built around the
    chosen centre, turned and scaled, and the volume is read once (the image trilinearly, the label by nearest neighbour from
    the same coordinates), so the cost follows the patch and there is one interpolation.  Not in the reference.

    ``degrees``: a number d (every axis in [-d, d]), a (low, high) pair for every axis, or three pairs for the rotations
    about D, H and W -- ``[[-15, 15], [0, 0], [0, 0]]`` turns a thin slab in-plane only.  ``scale``: a range inside
    [0.25, 4]; a value above 1 reads a larger region, so the content shrinks; a second coin picks the part of the range below
    or above 1 (nnU-Net's rule), and ``per_axis_scale`` draws one value per axis instead of one for all.

    Random stream: the parent's six draws, then always nine ``random.random()``: the rotate coin, three angles, the scale
    coin, the branch coin, three scales (without ``per_axis_scale`` only the first is used).  When neither coin hits the
    patch is the parent's: the same select and the same plain crops, and msk_affine_patch is not launched.  On device volumes msk_patch_select and msk_affine_patch run back to back:
    the origin never visits the host and nothing synchronises."""

    def __init__(self, size, num_classes, fg_prob=1. / 3., classes=None, pad_value=0, label_pad=0, rotate_prob=0.2, degrees=30,
                 scale_prob=0.2, scale=(0.7, 1.4), per_axis_scale=False):
        super().__init__(size, num_classes, fg_prob, classes, pad_value, label_pad)
        self.rotate_prob = _check_prob(rotate_prob)
        self.scale_prob = _check_prob(scale_prob)
        if isinstance(degrees, numbers.Number):
            if degrees < 0:
                raise ValueError("If degrees is a single number, it must be positive.")
            degrees = (-degrees, degrees)
        if isinstance(degrees, (tuple, list)) and len(degrees) == 3 and all(isinstance(d, (tuple, list)) for d in degrees):
            per_axis = list(degrees)
        else:
            per_axis = [degrees] * 3
        try:
            self.degrees = [_check_range(d, "degrees", lowest=-180.0, highest=180.0) for d in per_axis]
        except TypeError:
            raise ValueError("degrees must be a number, a (low, high) pair or three pairs, got {}.".format(degrees))
        self.scale = _check_range(scale, "scale", lowest=0.25, highest=4.0)
        self.per_axis_scale = bool(per_axis_scale)

    def _device_affine(self, img, label, sel, m):
        from ..preprocess import affine_patch_device
        if label is None:
            return affine_patch_device(img, None, sel, self.size, m, self.pad_value), None
        return affine_patch_device(img, label, sel, self.size, m, self.pad_value, self.label_pad)

    def get_matrix(self):
        """the nine draws -> the float32 matrix, or None when neither coin hit"""
        u = [random.random() for _ in range(9)]
        rotate, scale = u[0] < self.rotate_prob, u[4] < self.scale_prob
        if not rotate and not scale:
            return None
        angles = [_value(rng, v) for rng, v in zip(self.degrees, u[1:4])] if rotate else [0.0, 0.0, 0.0]
        su = u[6:9] if self.per_axis_scale else [u[6]] * 3
        scales = [_branch_value(self.scale, u[5], v) for v in su] if scale else [1.0, 1.0, 1.0]
        return _affine_matrix(angles, scales)

    def __call__(self, img, label=None):
        words = self.get_params(label is not None)
        m = self.get_matrix()
        if _on_device(img):
            if m is None:                    # neither coin hit: the parent's two crops, msk_affine_patch is not launched
                return self._device_call(img, label, words, self._device_crops)
            return self._device_call(img, label, words, lambda *a: self._device_affine(*a, m))
        origin = self.select(img.shape[:3], label, words)[:3]
        if m is None:
            return (_patch_crop_host(img, origin, self.size, self.pad_value),
                    None if label is None else _patch_crop_host(label, origin, self.size, self.label_pad))
        return _affine_patch_host(img, label, origin, self.size, m, self.pad_value, self.label_pad)


# ---- elastic deformation of that patch (batchgenerators' SpatialTransform(do_elastic_deform=True); not in the reference) -----
def _elastic_field_host(roi, sigma, alpha, seed, axes=(0, 1, 2)):
    """msk_elastic_field in numpy, float32 throughout: [3, rd, rh, rw] = alpha * (counter noise in [-1, 1) smoothed along W, H
    and D by gauss_taps(sigma) with zeros outside the patch; all 2r+1 terms of a line added in order, every multiply and add
    rounded on its own).  A component whose axis is not in ``axes`` is zero.  Equal to tests/elastic_reference.py bit for bit."""
    from ..preprocess import ELASTIC_MAX_SIGMA, gauss_taps
    roi = tuple(int(r) for r in roi)
    n = int(np.prod(roi))
    w = gauss_taps(sigma, ELASTIC_MAX_SIGMA)
    r = (len(w) - 1) // 2
    with np.errstate(over="ignore"):
        h = _splitmix64(_splitmix64(np.uint64(int(seed) & _MASK64)) + np.arange(3 * n, dtype=np.uint64))
    x = ((h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).reshape((3,) + roi)
    for a in range(3):
        if a not in axes:
            x[a] = 0.0
    for axis in (3, 2, 1):
        padding = [(0, 0)] * 4
        padding[axis] = (r, r)
        xp = np.moveaxis(np.pad(x, padding), axis, -1)
        length = x.shape[axis]
        acc = w[0] * xp[..., :length]
        for k in range(1, 2 * r + 1):
            acc = acc + w[k] * xp[..., k:k + length]
        x = np.moveaxis(acc, -1, axis)
    return np.ascontiguousarray(np.float32(alpha) * x)


@manager.TRANSFORMS.add_component
class RandomElasticAffinePatchCrop3D(RandomAffinePatchCrop3D):
    """RandomAffinePatchCrop3D whose sampling grid is, with probability ``elastic_prob``, also deformed elastically --
    batchgenerators' ``SpatialTransform(do_elastic_deform=True)``, MONAI's ``Rand3DElastic``: uniform noise per axis, smoothed
    by a Gaussian of ``elastic_sigma`` voxels and scaled by ``elastic_alpha``, displaces the zero-centred grid before it is
    rotated, scaled and moved to the chosen centre, and the volume is still read once.  The defaults are nnU-Net v1's.
    ``elastic_axes``: the source axes that are displaced; ``(1, 2)`` keeps a thin slab from being displaced across slices.
    Not in the reference.

    Random stream: the parent's six draws and nine ``random.random()``, then always ``random.random()`` (the coin),
    ``random.random()`` (alpha), ``random.random()`` (sigma) and ``random.getrandbits(64)`` (the seed of the counter noise),
    whatever the coins and the data.  Without an elastic hit the call is the parent's: its select, then plain crops or
    msk_affine_patch; neither elastic kernel is launched.  With an elastic hit and no matrix the identity matrix is used.  On
    device volumes msk_patch_select, msk_elastic_field and msk_affine_patch_elastic run back to back: nothing is downloaded
    and nothing synchronises."""

    def __init__(self, size, num_classes, fg_prob=1. / 3., classes=None, pad_value=0, label_pad=0, rotate_prob=0.2, degrees=30,
                 scale_prob=0.2, scale=(0.7, 1.4), per_axis_scale=False, elastic_prob=0.2, elastic_alpha=(0., 900.),
                 elastic_sigma=(9., 13.), elastic_axes=(0, 1, 2)):
        from ..preprocess import ELASTIC_MAX_ALPHA, ELASTIC_MAX_SIGMA, ELASTIC_MIN_SIGMA, elastic_axes_mask
        super().__init__(size, num_classes, fg_prob, classes, pad_value, label_pad, rotate_prob, degrees, scale_prob, scale,
                         per_axis_scale)
        self.elastic_prob = _check_prob(elastic_prob)
        self.elastic_alpha = _check_range(elastic_alpha, "elastic_alpha", lowest=0.0, highest=ELASTIC_MAX_ALPHA)
        self.elastic_sigma = _check_range(elastic_sigma, "elastic_sigma", lowest=ELASTIC_MIN_SIGMA, highest=ELASTIC_MAX_SIGMA)
        if not isinstance(elastic_axes, (tuple, list)):
            raise ValueError("elastic_axes must be a subset of (0, 1, 2), got {}.".format(elastic_axes))
        elastic_axes_mask(elastic_axes)
        self.elastic_axes = tuple(sorted(int(a) for a in elastic_axes))
        if 3 * self.size[0] * self.size[1] * self.size[2] >= 2 ** 31:
            raise ValueError("the displacement field of a {} patch has 2^31 elements or more.".format(self.size))

    def get_elastic(self):
        """the four draws -> (alpha, sigma, seed), both float32 values, or None without a hit"""
        coin, ua, us, seed = random.random(), random.random(), random.random(), random.getrandbits(64)
        if not coin < self.elastic_prob:
            return None
        return float(np.float32(_value(self.elastic_alpha, ua))), float(np.float32(_value(self.elastic_sigma, us))), seed

    def _device_elastic(self, img, label, sel, m, alpha, sigma, seed):
        from ..preprocess import affine_patch_device, elastic_field_device
        field = elastic_field_device(img.dev, self.size, sigma, alpha, seed, self.elastic_axes)
        try:
            if label is None:
                return affine_patch_device(img, None, sel, self.size, m, self.pad_value, field=field), None
            return affine_patch_device(img, label, sel, self.size, m, self.pad_value, self.label_pad, field=field)
        finally:
            field.free()                     # stream-ordered: the sampling kernel is enqueued in front of the next user

    def __call__(self, img, label=None):
        words = self.get_params(label is not None)
        m = self.get_matrix()
        hit = self.get_elastic()
        if hit is None:                      # the parent's call from here on
            if _on_device(img):
                if m is None:
                    return self._device_call(img, label, words, self._device_crops)
                return self._device_call(img, label, words, lambda *a: self._device_affine(*a, m))
            origin = self.select(img.shape[:3], label, words)[:3]
            if m is None:
                return (_patch_crop_host(img, origin, self.size, self.pad_value),
                        None if label is None else _patch_crop_host(label, origin, self.size, self.label_pad))
            return _affine_patch_host(img, label, origin, self.size, m, self.pad_value, self.label_pad)
        if m is None:
            m = np.eye(3, dtype=np.float32)
        if _on_device(img):
            return self._device_call(img, label, words, lambda *a: self._device_elastic(*a, m, *hit))
        origin = self.select(img.shape[:3], label, words)[:3]
        field = _elastic_field_host(self.size, hit[1], hit[0], hit[2], self.elastic_axes)
        return _affine_patch_host(img, label, origin, self.size, m, self.pad_value, self.label_pad, field)


@manager.TRANSFORMS.add_component
class BinaryMaskToConnectComponent:
    """numpy masks: the scipy path, uint32 labels.  A ``DeviceVolume`` or an ``IntTensor`` [N, 1, D, H, W] (the
    prediction of core.infer.inference) takes the HIP path (preprocess.connected_components_device, every volume on its
    own): int32 labels with the same values, on the device."""

    def __init__(self, minimum_volume=0):
        self.minimum_volume = minimum_volume

    def _label(self, vol):
        if _cc_on_device(vol):
            return _cc_device(vol, self.minimum_volume)
        return _connected_components(vol, self.minimum_volume)

    def __call__(self, pred, label=None):
        pred = self._label(pred)
        if label is not None:
            label = self._label(label)
        return pred, label


@manager.TRANSFORMS.add_component
class TopkLargestConnectComponent:
    """numpy masks: the scipy path, uint32 labels.  A ``DeviceVolume`` or an ``IntTensor`` [N, 1, D, H, W] takes the HIP
    path (preprocess.connected_components_device): int32 labels with the same values, on the device."""

    def __init__(self, k=1):
        self.k = k

    def __call__(self, pred, label=None):
        if _cc_on_device(pred):
            keep = int(np.floor(self.k))   # ranks r with r > k are dropped: k = 2.5 keeps 1 and 2
            pred = _cc_device(pred, 0, max(keep, 0))
            if keep < 1:   # the host path zeroes every label (still after the binary check)
                n = pred.size if _on_device(pred) else int(np.prod(pred.shape))
                pred.dev.memset(pred.ptr, 0, 4 * n)
            return pred, label
        pred = _connected_components(pred)
        pred[pred > self.k] = 0
        return pred, label


@manager.TRANSFORMS.add_component
class FillHoles3D:
    """MONAI's FillHoles for label volumes (not in the reference): a 6-connected region of zeros that touches no face of the
    volume and whose non-zero neighbours all carry one value c becomes c, when c is in ``classes`` (None: any value; at most
    64); a hole between different values stays 0.  On a binary mask this is scipy.ndimage.binary_fill_holes.  numpy volumes
    [D, H, W] (or [N, 1, D, H, W]) take the host path (preprocess.fill_holes_host) and keep their dtype; a ``DeviceVolume`` or
    an ``IntTensor`` [N, 1, D, H, W] takes the HIP path (preprocess.fill_holes_device, every volume on its own, one download
    of the status words): int32 with the same values, on the device.  Composes with TopkLargestConnectComponent as a
    ``pred_transform``."""

    def __init__(self, classes=None):
        from ..preprocess import _fill_classes
        self.classes = None if classes is None else [int(c) for c in _fill_classes(classes, False)]

    def _fill(self, vol):
        from ..preprocess import fill_holes_device, fill_holes_host
        if _cc_on_device(vol):
            out = fill_holes_device(vol, self.classes)
            return _swap(vol, out) if _on_device(vol) else out
        vol = np.asarray(vol)
        return fill_holes_host(vol, self.classes).astype(vol.dtype)

    def __call__(self, pred, label=None):
        pred = self._fill(pred)
        if label is not None:
            label = self._fill(label)
        return pred, label

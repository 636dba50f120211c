"""The statement of order-3 resampling: what msk_spline_resample3d, preprocess.resample_device(order=3) and
transforms.transform._spline_zoom_host compute, bit for bit, and what agrees with
``scipy.ndimage.zoom(x, out / in, order=3, mode='nearest')`` (grid_mode=False) within 1e-12 * max|x| on float64 input.

numpy, float64.  Every numpy expression below is one elementwise operation per operator, so every multiply and every add is
rounded on its own, in the order the parentheses give; the loops run along a line and the slices span all lines.

What is fixed here, in code:

* Constants: ``Z = sqrt(3) - 2`` (the pole), ``GAIN = (1 - Z) * (1 - 1 / Z)``, ``LAST = Z / (Z * Z - 1)``, all float64
  arithmetic on the host.
* Powers of z: ``z^(n-1)`` is ``zn1 = 1; zn1 = zn1 * Z`` repeated n - 1 times, on the host (it underflows to 0 for long
  lines, as it must); ``rden = 1 / (1 - zn1 * zn1)`` too, and the initial value is MULTIPLIED by it.  ``z^i`` inside the
  initialisation is the running product ``zi = zi * Z`` starting at ``zi = Z``.  Nothing calls pow.
* Initialisation sum: ``min(n - 2, HORIZON)`` terms with HORIZON = 47, in ascending i, each term
  ``zi * (c[i] + zn1 * c[n-1-i])``; ``|Z|^48 = 3.5e-28``.
* The padded input: 12 edge voxels per side of the volume GIVEN (a crop box is cut out first, as the reference does).
* Axes 0, 1, 2 in turn.
* Coordinates: ``cc = o * scale + 12`` with ``scale = (n_in - 1) / (n_out - 1)`` (0 when n_out == 1), taps
  ``floor(cc) - 1 .. floor(cc) + 2``; weights from ``t = cc - floor(cc)``, ``u = 1 - t``:
  ``w0 = ((u*u)*u)/6``, ``w1 = (((t*t)*(t-2))*3 + 4)/6``, ``w2 = (((u*u)*(u-2))*3 + 4)/6``, ``w3 = ((1 - w0) - w1) - w2``.
* The 64 taps: ``acc = 0``; for a (axis 0), b (axis 1), c (axis 2) in 0..3, c innermost:
  ``acc = acc + ((p * wd[a]) * wh[b]) * ww[c]``.  The result is ``acc`` cast to float32 (round to nearest even).
"""
import os

import numpy as np

PAD = 12
HORIZON = 47
Z = np.sqrt(np.float64(3.0)) - np.float64(2.0)
GAIN = (1.0 - Z) * (1.0 - 1.0 / Z)
LAST = Z / (Z * Z - 1.0)


def axis_constants(n):
    """(z^(n-1), 1 / (1 - z^(2(n-1)))) of a line of n samples"""
    zn1 = np.float64(1.0)
    for _ in range(n - 1):
        zn1 = zn1 * Z
    return zn1, 1.0 / (1.0 - zn1 * zn1)


def prefilter_axis(p, axis):
    """the recursive filter along one axis of the float64 array p, in place"""
    c = np.moveaxis(p, axis, 0)                    # a view: c[i] is sample i of every line
    n = c.shape[0]
    zn1, rden = axis_constants(n)
    c *= GAIN
    zi = Z
    c0 = c[0] + zn1 * c[n - 1]
    for i in range(1, min(n - 2, HORIZON) + 1):
        c0 = c0 + zi * (c[i] + zn1 * c[n - 1 - i])
        zi = zi * Z
    c[0] = c0 * rden
    for i in range(1, n):
        c[i] = c[i] + Z * c[i - 1]
    c[n - 1] = LAST * (c[n - 1] + Z * c[n - 2])
    for i in range(n - 2, -1, -1):
        c[i] = Z * (c[i + 1] - c[i])


def prefilter(x):
    """float64 coefficients of x padded by 12 edge voxels per side"""
    p = np.pad(np.asarray(x).astype(np.float64), PAD, mode="edge")
    for axis in range(3):
        prefilter_axis(p, axis)
    return p


def axis_taps(n_in, n_out):
    """first tap [n_out] and weights [4, n_out] along one axis"""
    scale = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(0.0)
    cc = np.arange(n_out, dtype=np.float64) * scale + np.float64(PAD)
    f = np.floor(cc)
    t = cc - f
    u = 1.0 - t
    w0 = ((u * u) * u) / 6.0
    w1 = (((t * t) * (t - 2.0)) * 3.0 + 4.0) / 6.0
    w2 = (((u * u) * (u - 2.0)) * 3.0 + 4.0) / 6.0
    w3 = ((1.0 - w0) - w1) - w2
    return f.astype(np.int64) - 1, np.stack([w0, w1, w2, w3])


def spline_zoom_f64(x, out_shape):
    """the statement before the cast: float64 [out_shape]"""
    x = np.asarray(x)
    assert x.ndim == 3 and len(out_shape) == 3
    p = prefilter(x)
    (sd, wd), (sh, wh), (sw, ww) = (axis_taps(x.shape[a], int(out_shape[a])) for a in range(3))
    acc = np.zeros(tuple(int(s) for s in out_shape), dtype=np.float64)
    for a in range(4):
        for b in range(4):
            for c in range(4):
                taps = p[(sd + a)[:, None, None], (sh + b)[None, :, None], (sw + c)[None, None, :]]
                acc = acc + ((taps * wd[a][:, None, None]) * wh[b][None, :, None]) * ww[c][None, None, :]
    return acc


def spline_zoom(x, out_shape):
    """the statement: float32 [out_shape]"""
    return spline_zoom_f64(x, out_shape).astype(np.float32)


def spline_crop_zoom(x, box, out_shape):
    """crop box (i, j, k, d, h, w) first, then zoom: functional.py:103-110"""
    i, j, k, d, h, w = (int(v) for v in box)
    return spline_zoom(np.asarray(x)[i:i + d, j:j + h, k:k + w], out_shape)


# ---- the goldens captured from the reference, and the tolerance they are held to ----------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spline_golden.npz")


def golden_cases():
    """(name, input, output shape, expected) of every case in golden/spline_golden.npz: the reference's own
    resize_3d(order=3) and resample(order=3), see golden/make_spline_golden.py"""
    g = np.load(GOLDEN)
    names = sorted(k[:-4] for k in g.files if k.endswith("_out"))
    assert len(names) == 9
    return [(n, g[n + "_img"], g[n + "_out"].shape, g[n + "_out"]) for n in names]


def assert_within_golden_tolerance(got, img, want, name):
    """one float32 rounding apart at most: 2^-23 |golden| + 1e-12 max|x|"""
    assert got.shape == want.shape and got.dtype == np.float32, name
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 2.0 ** -23 * np.abs(want.astype(np.float64)) + 1e-12 * np.abs(img).max()
    print(name, "max err / bound", float((err / bound).max()), "unequal", int((got != want).sum()), "of", want.size)
    assert (err <= bound).all(), name
    return int((got != want).sum())

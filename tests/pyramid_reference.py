"""The statement of msk_label_pyramid (medicalseg_amd/csrc/msk_pyramid.hip), in numpy integers.

For a label [N, D, H, W] and a level of extent (od, oh, ow):

    out[n, z, y, x] = label[n, iz, iy, ix],      per axis  i = ((2 * o + 1) * in) // (2 * out)

i.e. the source voxel that holds the centre of output voxel o when both grids cover the same extent (the geometry of
``interpolate(align_corners=False)``, mode 'nearest-exact').  No floating point is involved, so an axis without an integer stride
(12 -> 9) is as well defined as 16 -> 8.  The values are copied as they are: 255 (ignore_index), negative numbers and anything
else pass through."""
import numpy as np


def src_index(n_in: int, n_out: int) -> np.ndarray:
    """the source index of every output index along one axis"""
    o = np.arange(int(n_out), dtype=np.int64)
    return ((2 * o + 1) * int(n_in)) // (2 * int(n_out))


def pyramid_level(label: np.ndarray, extent) -> np.ndarray:
    label = np.asarray(label)
    _, d, h, w = label.shape
    od, oh, ow = (int(v) for v in extent)
    iz, iy, ix = src_index(d, od), src_index(h, oh), src_index(w, ow)
    return np.ascontiguousarray(label[:, iz[:, None, None], iy[None, :, None], ix[None, None, :]])


def label_pyramid(label: np.ndarray, extents) -> list:
    return [pyramid_level(label, e) for e in extents]

"""msk_label_pyramid on the device (medicalseg_amd/csrc/msk_pyramid.hip) against the integer statement
tests/pyramid_reference.py: np.array_equal everywhere, the values are copied, not computed.  Source and destinations sit between
red zones (tests/helpers.py), and a destination starts as the sentinel pattern, so a voxel the kernel skips shows as well."""
import ctypes as C

import numpy as np
import pytest

import pyramid_reference as R
from helpers import SENTINEL_BITS, dev, dmalloc, redzone_check, vec, vec_back  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

ERR = -1      # msk_fail: the library's argument-error status

CASES = [
    (2, (16, 16, 16), [(8, 8, 8), (4, 4, 4), (2, 2, 2)]),                       # isotropic, three levels
    (1, (32, 32, 12), [(16, 16, 9), (8, 8, 8), (4, 4, 4)]),                     # the MRI geometry; ow = 9: 4-byte stores
    (1, (7, 5, 9), [(3, 2, 4), (1, 1, 1)]),                                      # odd extents
    (1, (16, 16, 16), [(16, 16, 16)]),                                           # one level, out == in
    (1, (16, 16, 16), [(16, 16, 16), (8, 8, 8), (4, 4, 4), (2, 2, 2), (1, 1, 1), (5, 7, 3), (16, 1, 12), (9, 16, 6)]),   # L = 8
    (3, (9, 33, 40), [(9, 17, 40), (4, 33, 20), (2, 8, 37)]),                    # several workgroups per level, partial last quads
]


def _labels(rng, n, shape):
    y = rng.integers(0, 20, (n,) + shape).astype(np.int32)
    y[rng.random(y.shape) < 0.1] = 255
    flat = y.reshape(-1)
    flat[rng.integers(0, flat.size, 8)] = -1
    flat[rng.integers(0, flat.size, 8)] = 2 ** 31 - 1
    flat[0], flat[-1] = -(2 ** 31), 2 ** 31 - 1
    return y


def _upload(y):
    return vec(np.ascontiguousarray(y).reshape(-1).view(np.float32))      # the bits as they are


def _raw(label_ptr, n, shape, extents, dst_ptrs):
    """the bare C call -> its return code"""
    d = dev()
    ext = (C.c_int32 * max(3 * len(extents), 1))(*[int(v) for e in extents for v in e]) if extents is not None else None
    dst = (C.c_void_p * max(len(dst_ptrs), 1))(*dst_ptrs) if dst_ptrs is not None else None
    return d.lib.msk_label_pyramid(d.ctx, C.c_void_p(label_ptr) if label_ptr else None, n, shape[0], shape[1], shape[2],
                                   len(extents) if extents is not None else 1, ext, dst)


def _count(n, e):
    return n * e[0] * e[1] * e[2]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%s-L%d" % (c[0], "x".join(map(str, c[1])), len(c[2])))
def test_levels_match_the_statement(case):
    n, shape, extents = case
    y = _labels(np.random.default_rng(len(extents) * 100 + shape[2]), n, shape)
    assert (y == 255).any() and (y == -1).any() and (y == 2 ** 31 - 1).any()
    src = _upload(y)
    dst = [dmalloc(_count(n, e) * 4) for e in extents]
    assert _raw(src, n, shape, extents, dst) == 0
    want = R.label_pyramid(y, extents)
    for p, e, w in zip(dst, extents, want):
        got = vec_back(p, _count(n, e), np.int32).reshape((n,) + e)
        assert np.array_equal(got, w), e
    assert np.array_equal(vec_back(src, y.size, np.int32).reshape(y.shape), y)          # the source is read only


def test_the_wrapper_returns_arena_levels():
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models.losses.fused import label_pyramid
    y = _labels(np.random.default_rng(1), 2, (16, 16, 16))
    extents = [(2, 2, 2), (4, 4, 4), (8, 8, 8)]
    levels = label_pyramid(to_tensor(y), extents)
    for lv, w in zip(levels, R.label_pyramid(y, extents)):
        assert lv.gen == dev().arena.gen and np.array_equal(lv.numpy(), w)


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_a_destination_off_the_16_byte_grid_takes_the_4_byte_stores(offset):
    n, shape, extents = 2, (16, 16, 16), [(8, 8, 8), (4, 4, 4)]          # ow % 4 == 0 on both levels
    y = _labels(np.random.default_rng(offset), n, shape)
    src = _upload(y)
    counts = [_count(n, e) for e in extents]
    bufs = [dmalloc(c * 4 + offset) for c in counts]                      # the tail red zone starts right behind the level
    assert _raw(src, n, shape, extents, [bufs[0] + offset, bufs[1]]) == 0
    want = R.label_pyramid(y, extents)
    assert np.array_equal(vec_back(bufs[0] + offset, counts[0], np.int32), want[0].reshape(-1))
    assert np.all(vec_back(bufs[0], offset // 4, np.uint32) == SENTINEL_BITS)           # nothing in front of it was written
    assert np.array_equal(vec_back(bufs[1], counts[1], np.int32), want[1].reshape(-1))  # the aligned level next to it


def test_argument_errors_launch_nothing():
    d = dev()
    n, shape = 1, (8, 8, 8)
    y = _labels(np.random.default_rng(2), n, shape)
    src = _upload(y)
    e = (4, 4, 4)
    out = dmalloc(_count(n, e) * 4)
    assert _raw(src, n, shape, [e], [out]) == 0
    good = vec_back(out, _count(n, e), np.int32).copy()
    dst = dmalloc(_count(n, shape) * 4)

    def untouched():
        d.sync()
        return np.all(vec_back(dst, _count(n, shape), np.uint32) == SENTINEL_BITS)

    bad = [
        ("2^31 voxels", lambda: _raw(src, 2, (1024, 1024, 1024), [(1, 1, 1)], [dst])),
        ("more than 2^31 voxels", lambda: _raw(src, 8, (32768, 32768, 8), [(1, 1, 1)], [dst])),
        ("2^64 voxels: a 64-bit product would wrap to 0", lambda: _raw(src, 2 ** 19, (32768, 32768, 32768), [(1, 1, 1)], [dst])),
        ("an axis longer than 32768", lambda: _raw(src, 1, (1, 1, 32769), [(1, 1, 1)], [dst])),
        ("no level", lambda: _raw(src, n, shape, [], [dst])),
        ("nine levels", lambda: _raw(src, n, shape, [(1, 1, 1)] * 9, [dst] * 9)),
        ("extent 0", lambda: _raw(src, n, shape, [(4, 0, 4)], [dst])),
        ("negative extent", lambda: _raw(src, n, shape, [(4, 4, -1)], [dst])),
        ("extent above the source's", lambda: _raw(src, n, shape, [(8, 8, 9)], [dst])),
        ("a later level's extent above the source's", lambda: _raw(src, n, shape, [(4, 4, 4), (9, 8, 8)], [dst, dst])),
        ("empty label", lambda: _raw(src, 0, shape, [(4, 4, 4)], [dst])),
        ("null label", lambda: _raw(None, n, shape, [e], [dst])),
        ("null extents", lambda: _raw(src, n, shape, None, [dst])),
        ("null destination table", lambda: _raw(src, n, shape, [e], None)),
        ("null destination", lambda: _raw(src, n, shape, [e], [None])),
        ("null second destination", lambda: _raw(src, n, shape, [e, e], [dst, None])),
        ("destination is the label", lambda: _raw(src, n, shape, [shape], [src])),
        ("destination inside the label", lambda: _raw(src, n, shape, [e], [src + y.nbytes - 4])),
        ("destination ends inside the label", lambda: _raw(src + 16, n, (8, 8, 4), [(8, 8, 4)], [src])),
        ("second destination overlaps the label", lambda: _raw(src, n, shape, [e, e], [dst, src + 64])),
    ]
    for what, call in bad:
        assert call() == ERR, what
        assert d.lib.msk_last_error(d.ctx), what
        assert untouched(), what
    assert np.array_equal(vec_back(src, y.size, np.int32).reshape(y.shape), y)
    # the context still works, and a destination that ends where the label starts is no overlap
    both = dmalloc(y.nbytes + _count(n, e) * 4)
    d.d2d(both + _count(n, e) * 4, src, y.nbytes)
    assert _raw(both + _count(n, e) * 4, n, shape, [e], [both]) == 0
    assert np.array_equal(vec_back(both, _count(n, e), np.int32), good)

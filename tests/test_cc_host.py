"""Connected-component transforms without a GPU: the C ABI surface of msk_connected_components3d, the dispatch of
BinaryMaskToConnectComponent / TopkLargestConnectComponent to the device path (through a stand-in, no kernel runs),
and the independent BFS restatement (tests/cc_reference.py) against the host path the GPU is held to."""
import os
import re

import numpy as np
import pytest

import cc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_ctypes_table_carry_the_entry_point():
    import ctypes as C

    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    m = re.search(r"int\s+msk_connected_components3d\s*\(([^)]*)\)", txt)
    assert m, "msegk.h does not declare msk_connected_components3d"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 12
    res, args = _lib.SIGNATURES["msk_connected_components3d"]
    assert res is C.c_int and len(args) == 12
    # ctx, src, dst pointers; n d h w dtype minimum_volume k ints; status, counts pointers
    assert args[:3] == [C.c_void_p] * 3 and args[3:10] == [C.c_int] * 7 and args[10:] == [C.c_void_p] * 2


class _Dev:
    def __init__(self):
        self.memsets = []

    def memset(self, ptr, value, nbytes):
        self.memsets.append((ptr, value, nbytes))


@pytest.fixture
def stand_in(monkeypatch):
    """replaces preprocess.connected_components_device; records its calls and returns a new object of the input's kind"""
    from medicalseg_amd import preprocess
    from medicalseg_amd.device import IntTensor
    calls = []

    def fake(x, minimum_volume=0, k=0):
        calls.append((x, minimum_volume, k))
        if isinstance(x, preprocess.DeviceVolume):
            return preprocess.DeviceVolume(x.dev, 2000 + len(calls), x.shape, np.int32)
        return IntTensor(x.dev, 3000 + len(calls), x.shape)

    monkeypatch.setattr(preprocess, "connected_components_device", fake)
    return calls


def _volume(dev, ptr=100):
    from medicalseg_amd.preprocess import DeviceVolume
    v = DeviceVolume(dev, ptr, (4, 5, 6), np.float32)
    v.freed = False

    def free():
        v.freed = True
    v.free = free
    return v


def test_binary_mask_transform_routes_device_volumes(stand_in):
    from medicalseg_amd.preprocess import DeviceVolume
    from medicalseg_amd.transforms import transform as T
    dev = _Dev()
    pred, label = _volume(dev, 100), _volume(dev, 200)
    out_p, out_l = T.BinaryMaskToConnectComponent(minimum_volume=7)(pred, label)
    assert [(c[0], c[1], c[2]) for c in stand_in] == [(pred, 7, 0), (label, 7, 0)]
    assert isinstance(out_p, DeviceVolume) and isinstance(out_l, DeviceVolume)
    assert out_p.ptr != pred.ptr and pred.freed and label.freed   # the inputs go back to the pool (_swap)


def test_binary_mask_transform_routes_int_tensors(stand_in):
    from medicalseg_amd.device import IntTensor
    from medicalseg_amd.transforms import transform as T
    dev = _Dev()
    pred = IntTensor(dev, 100, (3, 1, 4, 5, 6))
    out_p, out_l = T.BinaryMaskToConnectComponent(minimum_volume=2)(pred)
    assert stand_in == [(pred, 2, 0)] and out_l is None
    assert isinstance(out_p, IntTensor) and out_p.ptr != pred.ptr and out_p.shape == pred.shape


def test_topk_transform_routes_device_inputs(stand_in):
    from medicalseg_amd.device import IntTensor
    from medicalseg_amd.transforms import transform as T
    dev = _Dev()
    pred, label = _volume(dev, 100), _volume(dev, 200)
    out_p, out_l = T.TopkLargestConnectComponent(k=3)(pred, label)
    assert stand_in == [(pred, 0, 3)] and out_l is label and pred.freed and not label.freed
    t = IntTensor(dev, 300, (2, 1, 4, 5, 6))
    T.TopkLargestConnectComponent(k=2.5)(t)
    assert stand_in[-1] == (t, 0, 2)                 # ranks > 2.5 dropped: the two largest stay
    assert dev.memsets == []
    out, _ = T.TopkLargestConnectComponent(k=0)(t)
    assert stand_in[-1] == (t, 0, 0)
    assert dev.memsets == [(out.ptr, 0, 4 * 2 * 4 * 5 * 6)]   # k < 1 zeroes every label, as pred[pred > 0] = 0 does


def test_numpy_inputs_keep_the_scipy_path(stand_in):
    from medicalseg_amd.transforms import transform as T
    m = R.box_blobs((6, 7, 8), 4, 0)
    p, _ = T.BinaryMaskToConnectComponent()(m)
    q, _ = T.TopkLargestConnectComponent(k=1)(m)
    assert stand_in == []
    assert p.dtype == np.uint32 and q.dtype == np.uint32
    np.testing.assert_array_equal(p, R.relabel(m))


def test_reference_checks_itself_on_known_masks():
    lab, sizes = R.label6(R.checkerboard((3, 4, 5)))
    assert len(sizes) == 30 and (sizes == 1).all()
    _, sizes = R.label6(R.serpentine((5, 7, 9)))
    assert len(sizes) == 1
    d = R.diagonal_contacts((4, 5, 6))
    _, sizes = R.label6(d)
    assert len(sizes) == int((d != 0).sum()) - 1     # (D-1, D-1, D-1) lies on both lines; (D-1, D-2, D-2) touches (D-2, D-2, D-2)
    m = np.zeros((1, 1, 9), np.float32)
    m[0, 0, [0, 1, 3, 5, 6, 7]] = 1                    # sizes 2, 1, 3: ranks by size, ties by first voxel
    np.testing.assert_array_equal(R.relabel(m)[0, 0], [2, 2, 0, 3, 0, 1, 1, 1, 0])
    np.testing.assert_array_equal(R.relabel(m, minimum_volume=2)[0, 0], [2, 2, 0, 0, 0, 1, 1, 1, 0])
    np.testing.assert_array_equal(R.relabel(m, k=1)[0, 0], [0, 0, 0, 0, 0, 1, 1, 1, 0])


@pytest.mark.parametrize("seed", range(6))
def test_host_path_matches_the_bfs_restatement(seed):
    from medicalseg_amd.transforms.transform import _connected_components
    rng = np.random.default_rng(seed)
    shape = tuple(int(s) for s in rng.integers(1, 12, 3))
    masks = [R.noise(shape, seed, p) for p in (0.3, 0.5, 0.7)]
    masks += [R.box_blobs(shape, 5, seed), R.checkerboard(shape), R.serpentine(shape), R.diagonal_contacts(shape),
              np.zeros(shape, np.float32), np.ones(shape, np.float32), 2 * R.noise(shape, seed + 100)]
    for m in masks:
        for mv in (0, 1, 3, 1000):
            np.testing.assert_array_equal(_connected_components(m, mv), R.relabel(m, mv))
        top = _connected_components(m)
        top[top > 2] = 0
        np.testing.assert_array_equal(top, R.relabel(m, k=2))


def test_non_binary_message_matches_the_host_path():
    from medicalseg_amd.transforms.transform import _connected_components
    m = np.zeros((2, 3, 4), np.float32)
    m[0, 0, :3] = [1, 2, 3]
    with pytest.raises(AssertionError) as host:
        _connected_components(m)
    with pytest.raises(AssertionError) as ref:
        R.relabel(m)
    assert str(host.value) == str(ref.value) == "Only binary mask is accepted, got mask with [0.0, 1.0, 2.0, 3.0]."

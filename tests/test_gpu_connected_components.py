"""msk_connected_components3d (medicalseg_amd/csrc/msk_ccl.hip) through preprocess.connected_components_device and the
two transform classes: labels bitwise equal to the host path transforms.transform._connected_components (itself held
to the BFS restatement tests/cc_reference.py in tests/test_cc_host.py), volume by volume, in float32 and int32."""
import numpy as np
import pytest

import cc_reference as R

pytestmark = pytest.mark.gpu


def _host(m, minimum_volume=0, k=0):
    from medicalseg_amd.transforms.transform import _connected_components
    lab = _connected_components(m, minimum_volume).astype(np.int64)
    if k > 0:
        lab[lab > k] = 0
    return lab


def _device(m, minimum_volume=0, k=0):
    from medicalseg_amd import preprocess as pp
    v = pp.upload_pooled(m)
    out = pp.connected_components_device(v, minimum_volume, k)
    res = out.numpy()
    assert res.dtype == np.int32 and res.shape == m.shape
    assert np.array_equal(v.numpy(), m), "the input volume was modified"
    v.free()
    out.free()
    return res


def _check(m, minimum_volume=0, k=0):
    want = _host(m, minimum_volume, k)
    for dt in (np.float32, np.int32):
        got = _device(m.astype(dt), minimum_volume, k)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError("%s %s mv=%s k=%s: %d voxels differ, first %s: got %d want %d (%d components)" % (
                m.shape, np.dtype(dt).name, minimum_volume, k, len(bad), tuple(bad[0]), got[tuple(bad[0])],
                want[tuple(bad[0])], want.max()))


def _corners(shape):
    m = np.zeros(shape, np.float32)
    D, H, W = shape
    for z in (0, D - 1):
        for y in (0, H - 1):
            for x in (0, W - 1):
                m[z, y, x] = 1
    return m


SMALL = (33, 37, 70)   # several tiles along every axis, partial tiles at every far face


@pytest.mark.parametrize("name", ["empty", "full", "corners", "diagonal", "blobs", "noise", "checkerboard", "serpentine"])
def test_masks_match_host(name):
    s = SMALL
    m = {"empty": lambda: np.zeros(s, np.float32), "full": lambda: np.ones(s, np.float32),
         "corners": lambda: _corners(s), "diagonal": lambda: R.diagonal_contacts(s),
         "blobs": lambda: R.box_blobs(s, 12, 1), "noise": lambda: R.noise(s, 2),
         "checkerboard": lambda: R.checkerboard(s), "serpentine": lambda: R.serpentine(s)}[name]()
    _check(m)


@pytest.mark.parametrize("shape", [(7, 13, 130), (1, 1, 4096), (4096, 1, 1), (3, 300, 5), (1, 1, 1), (4, 8, 32)])
def test_odd_shapes(shape):
    for m in (R.noise(shape, 3), R.checkerboard(shape), R.serpentine(shape), _corners(shape), np.ones(shape, np.float32)):
        _check(m)


@pytest.mark.parametrize("shape", [(128, 128, 128), (12, 512, 512)])
def test_benchmark_shapes(shape):
    _check(R.box_blobs(shape, 12, 4))
    _check(R.noise(shape, 5))
    _check(R.checkerboard(shape))


def test_serpentine_128():
    _check(R.serpentine((128, 128, 128)))


def test_non_unit_foreground_values():
    m = R.noise(SMALL, 6)
    _check(2 * m)            # {0, 2}
    _check(1 + m)            # {1, 2}: every voxel is foreground
    _check(-m)               # {-1, 0}; -0.0 is background


@pytest.mark.parametrize("mv", [0, 1, 5, 10 ** 9])
def test_minimum_volume(mv):
    m = R.noise(SMALL, 7, 0.45)
    _check(m, minimum_volume=mv)
    _check(R.box_blobs(SMALL, 12, 8), minimum_volume=mv)


@pytest.mark.parametrize("k", [1, 3, 10 ** 6])
def test_top_k(k):
    _check(R.noise(SMALL, 9), k=k)
    _check(R.box_blobs(SMALL, 12, 10), minimum_volume=5, k=k)


def test_non_binary_mask_raises_host_message():
    from medicalseg_amd import preprocess as pp
    for dt in (np.float32, np.int32):
        m = R.noise(SMALL, 11).astype(dt)
        m[5, 6, 7] = 3
        with pytest.raises(AssertionError) as host:
            _host(m)
        v = pp.upload_pooled(m)
        with pytest.raises(AssertionError) as dev:
            pp.connected_components_device(v)
        assert str(dev.value) == str(host.value)
        v.free()
    # the batched form names the offending volume's values
    from medicalseg_amd.device import to_tensor
    b = np.stack([R.noise(SMALL, 12), R.noise(SMALL, 13) * 4]).astype(np.int32)[:, None]
    b[1, 0, 0, 0, 0] = 7
    with pytest.raises(AssertionError, match=r"got mask with \[0, 4, 7\]"):
        pp.connected_components_device(to_tensor(b))


def test_batched_int_tensor_labels_each_volume_alone():
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.device import to_tensor
    vols = [R.box_blobs(SMALL, 8, 20), R.noise(SMALL, 21), np.ones(SMALL, np.float32)]
    vols[0][-1] = 1          # foreground on the last plane of volume 0 touches volume 1's first plane in memory
    vols[1][0] = 1
    b = np.stack(vols).astype(np.int32)[:, None]
    t = to_tensor(b)
    for mv, k in ((0, 0), (3, 0), (0, 2)):
        out = pp.connected_components_device(t, mv, k)
        assert out.shape == t.shape and out.ptr != t.ptr
        got = out.numpy()
        for i in range(3):
            assert np.array_equal(got[i, 0], _host(vols[i], mv, k)), (i, mv, k)
    assert np.array_equal(t.numpy(), b), "the input tensor was modified"


def test_repeat_runs_are_bitwise_identical():
    m = R.noise((128, 128, 128), 30)
    a, b = _device(m), _device(m)
    assert np.array_equal(a, b)


def test_transform_classes_device_vs_numpy():
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.preprocess import DeviceVolume
    from medicalseg_amd.transforms import transform as T
    pred, label = R.noise(SMALL, 40, 0.4), R.box_blobs(SMALL, 10, 41)
    for op in (T.BinaryMaskToConnectComponent(), T.BinaryMaskToConnectComponent(minimum_volume=4),
               T.TopkLargestConnectComponent(k=1), T.TopkLargestConnectComponent(k=3), T.TopkLargestConnectComponent(k=0)):
        hp, hl = op(pred.copy(), label.copy())
        dp, dl = op(pp.upload_pooled(pred), pp.upload_pooled(label.astype(np.int32)))
        assert isinstance(dp, DeviceVolume) and isinstance(dl, DeviceVolume)
        assert np.array_equal(dp.numpy(), hp), op
        assert np.array_equal(dl.numpy(), hl), op
        dp.free()
        dl.free()


def test_inference_then_top1_component():
    from medicalseg_amd import models
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import IntTensor, to_tensor
    from medicalseg_amd.transforms import transform as T
    rng = np.random.default_rng(50)
    model = models.VNet(num_classes=2)
    model.eval()
    x = rng.standard_normal((2, 1, 32, 32, 32)).astype(np.float32)
    pred, _ = infer.inference(model, to_tensor(x))
    host_pred = pred.numpy()
    out, _ = T.TopkLargestConnectComponent(k=1)(pred)
    assert isinstance(out, IntTensor)
    got = out.numpy()
    assert np.array_equal(pred.numpy(), host_pred)
    for i in range(2):
        want, _ = T.TopkLargestConnectComponent(k=1)(host_pred[i, 0])
        assert np.array_equal(got[i, 0], want), i

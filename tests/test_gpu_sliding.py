"""Sliding-window inference on the device (medicalseg_amd/csrc/msk_sliding.hip, core/infer.py sliding_window_inference,
evaluate(sliding_window=...)) against the numpy statement of tests/sliding_reference.py.  Everything is compared with
np.array_equal: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import sliding_reference as R

pytestmark = pytest.mark.gpu


class Owned:
    """device tensors outside the arena and the input pool, freed on exit"""

    def __enter__(self):
        from medicalseg_amd.device import get_device
        self.dev, self.ptrs = get_device(), []
        return self

    def __exit__(self, *exc):
        self.dev.sync()
        for p in self.ptrs:
            self.dev.free(p)
        return False

    def empty(self, n, d, h, w, c):
        from medicalseg_amd.device import Tensor
        t = Tensor.empty(self.dev, n, d, h, w, c, arena=False)
        self.ptrs.append(t.ptr)
        return t

    def upload(self, ncdhw):
        a = np.ascontiguousarray(np.moveaxis(np.asarray(ncdhw, np.float32), 1, -1))
        t = self.empty(*a.shape)
        self.dev.h2d(t.ptr, a)
        return t

    def floats(self, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        p = self.dev.malloc(arr.nbytes)
        self.ptrs.append(p)
        self.dev.h2d(p, arr)
        return p


def _plans(shape, roi, overlap, mode):
    """the product's plan (whose tables go to the device) and the statement's"""
    from medicalseg_amd.core.infer import SlidingPlan
    return SlidingPlan(shape, roi, overlap=overlap, mode=mode), R.Plan(shape, roi, overlap, mode)


def _origins(plan, windows, table_rows=True):
    rows = [plan.origin(w) + (w[1:] if table_rows else ()) for w in windows]
    return np.ascontiguousarray(np.array(rows, np.int32))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _batches(count):
    return sorted({1, min(3, count), count})


def _accumulate(dev, plan, tables, logits_t, windows, acc_t):
    o = _origins(plan, windows)
    dev.call("msk_sw_accumulate", logits_t.msk(), _ptr(o), C.c_void_p(tables[0]), len(plan.starts[0]), C.c_void_p(tables[1]),
             len(plan.starts[1]), C.c_void_p(tables[2]), len(plan.starts[2]), acc_t.msk())


# ---- msk_sw_gather -----------------------------------------------------------------------------------------------------------
GATHER_CASES = [  # (n, volume, roi, overlap, cin, cval)
    (2, (5, 7, 9), (4, 4, 4), 0.5, 1, 0.0), (2, (5, 7, 9), (4, 4, 4), 0.5, 2, 0.0),
    (1, (2, 6, 10), (4, 4, 8), 0.5, 1, 0.0), (1, (2, 6, 10), (4, 4, 8), 0.5, 1, -3.5), (1, (2, 6, 10), (4, 4, 8), 0.5, 4, -3.5),
    (1, (2, 3, 300), (2, 2, 260), 0.25, 1, 0.0), (1, (2, 3, 300), (2, 2, 260), 0.25, 2, 1.0),
    (1, (4, 4, 4), (4, 4, 8), 0.5, 2, -3.5)]                                   # padded on w by whole quads


@pytest.mark.parametrize("n,shape,roi,overlap,cin,cval", GATHER_CASES)
def test_gather_equals_numpy_crop_with_padding(n, shape, roi, overlap, cin, cval):
    plan, ref = _plans(shape, roi, overlap, 'constant')
    x = R.volume(n, shape, cin, 1)
    windows = plan.windows(n)
    want = np.stack(R.crops(x, ref, cval))
    assert len(windows) == len(want)
    with Owned() as o:
        vol = o.upload(x)
        for batch in _batches(len(windows)):
            for k in range(0, len(windows), batch):
                group = windows[k:k + batch]
                dst = o.upload(np.full((len(group), cin) + roi, np.nan, np.float32))
                o.dev.call("msk_sw_gather", vol.msk(), dst.msk(), _ptr(_origins(plan, group, False)), C.c_float(cval))
                got = dst.numpy()
                assert np.array_equal(got.view(np.uint32), want[k:k + batch].view(np.uint32)), (batch, k)
        assert np.array_equal(vol.numpy(), x)


def test_gather_on_channel_slice_views():
    n, shape, roi = 1, (2, 6, 10), (4, 4, 8)
    plan, ref = _plans(shape, roi, 0.5, 'constant')
    wide = R.volume(n, shape, 4, 2)
    windows = plan.windows(n)
    with Owned() as o:
        vol = o.upload(wide)
        fill = np.full((len(windows), 3) + roi, 7.0, np.float32)
        dst = o.upload(fill)
        o.dev.call("msk_sw_gather", vol.channel_slice(1, 3).msk(), dst.channel_slice(1, 3).msk(), _ptr(_origins(plan, windows, False)),
                   C.c_float(-3.5))
        want = fill.copy()
        want[:, 1:3] = np.stack(R.crops(wide[:, 1:3], ref, -3.5))
        assert np.array_equal(dst.numpy(), want)                                # the channels around the view are untouched


@pytest.mark.parametrize("shape,roi,overlap", [((2, 6, 10), (4, 4, 8), 0.5), ((5, 7, 9), (4, 4, 4), 0.5), ((2, 3, 300), (2, 2, 260), 0.25)])
def test_gather_with_a_view_on_one_side_only(shape, roi, overlap):
    """a channel-slice view as the source of DENSE patches whose rows are whole quads (what sliding_window_inference does
    with a slice of a multi-modal volume: its patch buffer is always dense), and a dense source into a view"""
    n, c = 1, 2
    plan, ref = _plans(shape, roi, overlap, 'constant')
    assert (roi[2] * c) % 4 == 0
    wide = R.volume(n, shape, 5, 3)
    windows = plan.windows(n)
    o4 = _origins(plan, windows, False)
    with Owned() as o:
        vol = o.upload(wide)
        dst = o.upload(np.full((len(windows), c) + roi, np.nan, np.float32))
        o.dev.call("msk_sw_gather", vol.channel_slice(2, 2 + c).msk(), dst.msk(), _ptr(o4), C.c_float(-3.5))
        want = np.stack(R.crops(wide[:, 2:2 + c], ref, -3.5))
        assert np.array_equal(dst.numpy().view(np.uint32), want.view(np.uint32))
        dense = o.upload(wide[:, 2:2 + c])
        fill = np.full((len(windows), c + 2) + roi, 7.0, np.float32)
        into = o.upload(fill)
        o.dev.call("msk_sw_gather", dense.msk(), into.channel_slice(1, 1 + c).msk(), _ptr(o4), C.c_float(-3.5))
        got = into.numpy()
        assert np.array_equal(got[:, 1:1 + c].view(np.uint32), want.view(np.uint32))
        assert (got[:, 0] == 7.0).all() and (got[:, 1 + c] == 7.0).all()


def test_sliding_window_inference_of_a_channel_slice():
    """one modality of a multi-modal volume, as a view, through the whole call"""
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    shape, roi = (5, 7, 9), (4, 4, 4)
    wide = R.volume(1, shape, 3, 44)
    ref = R.Plan(shape, roi, 0.5, 'gaussian')
    pred, logits = infer.sliding_window_inference(_stub(R.ramp_model), to_tensor(wide).channel_slice(1, 2), roi, sw_batch_size=4)
    want = R.blend(R.model_on_windows(R.ramp_model, wide[:, 1:2], ref), ref, 1)
    assert np.array_equal(logits.numpy(), want)
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))


# ---- msk_sw_accumulate -------------------------------------------------------------------------------------------------------
ACC_CASES = [  # (n, volume, roi, overlap, c)
    (2, (5, 7, 9), (4, 4, 4), 0.5, 1), (2, (5, 7, 9), (4, 4, 4), 0.5, 3),      # unaligned starts 0, 2, 4, 5
    (1, (2, 6, 10), (4, 4, 8), 0.5, 20),                                       # padding on d, whole quads
    (1, (2, 6, 10), (4, 4, 8), 0.5, 2),                                        # whole quads with two voxels per quad; w0 = 2 is one
    (1, (2, 3, 300), (2, 2, 260), 0.25, 3),                                    # long rows, unaligned
    (1, (2, 3, 300), (2, 2, 260), 0.25, 4),                                    # long rows, whole quads
    (1, (4, 4, 4), (4, 4, 8), 0.5, 2),                                         # padded on w: whole quads from x0 = 2 on
    (1, (8, 8, 8), (4, 4, 4), 0.0, 3)]                                         # every weight is 1


@pytest.mark.parametrize("mode", ['gaussian', 'constant'])
@pytest.mark.parametrize("n,shape,roi,overlap,c", ACC_CASES)
def test_accumulate_equals_blend(n, shape, roi, overlap, c, mode):
    plan, ref = _plans(shape, roi, overlap, mode)
    windows = plan.windows(n)
    lg = R.window_logits(ref, n, c, 10)
    want = R.blend(lg, ref, n)
    if (5, 7, 9) == shape:
        assert plan.starts[2] == [0, 2, 4, 5]
    if overlap == 0.0:                                                          # the logits placed side by side
        for wd, l_ in zip(windows, lg):
            _, d0, h0, w0 = plan.origin(wd)
            assert np.array_equal(want[wd[0], :, d0:d0 + roi[0], h0:h0 + roi[1], w0:w0 + roi[2]], l_)
    stacked = np.stack(lg)
    with Owned() as o:
        tables = [o.floats(t) for t in plan.tables]
        for batch in _batches(len(windows)):
            acc = o.upload(np.zeros((n, c) + shape, np.float32))
            for k in range(0, len(windows), batch):
                _accumulate(o.dev, plan, tables, o.upload(stacked[k:k + batch]), windows[k:k + batch], acc)
            got = acc.numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), batch


def test_accumulate_on_channel_slice_views():
    n, shape, roi, c = 2, (5, 7, 9), (4, 4, 4), 3
    plan, ref = _plans(shape, roi, 0.5, 'gaussian')
    windows = plan.windows(n)
    lg = R.window_logits(ref, n, c, 20)
    wide = np.concatenate([R.volume(len(windows), roi, 2, 21), np.stack(lg)], axis=1)            # the logits are channels 2..4
    base = np.full((n, c + 2) + shape, 7.0, np.float32)
    with Owned() as o:
        tables = [o.floats(t) for t in plan.tables]
        acc = o.upload(base)
        _accumulate(o.dev, plan, tables, o.upload(wide).channel_slice(2, 2 + c), windows, acc.channel_slice(1, 1 + c))
        got = acc.numpy()
        assert np.array_equal(got[:, 1:1 + c], R.blend(lg, ref, n, acc=base[:, 1:1 + c]))
        assert (got[:, 0] == 7.0).all() and (got[:, 1 + c] == 7.0).all()       # the channels around the view are untouched


def test_argument_errors_launch_nothing():
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import NULL_TENSOR, MskError
    n, shape, roi, c = 2, (5, 7, 9), (4, 4, 4), 3
    plan, ref = _plans(shape, roi, 0.5, 'gaussian')
    nd, nh, nw = (len(s) for s in plan.starts)
    with Owned() as o:
        dev = o.dev
        td, th, tw = (C.c_void_p(o.floats(t)) for t in plan.tables)
        x = R.volume(n, shape, c, 30)
        vol = o.upload(x)
        patches = o.upload(np.full((2, c) + roi, np.nan, np.float32))
        acc = o.upload(np.full((n, c) + shape, np.nan, np.float32))
        lg = o.upload(R.volume(2, roi, c, 31))
        other_c = o.upload(R.volume(2, roi, c + 1, 32))

        def g(*rows):
            return _ptr(np.ascontiguousarray(np.array(rows, np.int32)))
        ok4, ok7 = [(0, 0, 0, 0), (1, 1, 3, 5)], [(0, 0, 0, 0, 0, 0, 0), (1, 1, 3, 5, 1, 2, 3)]
        tabs = (td, nd, th, nh, tw, nw)
        bad = [("msk_sw_gather", (vol.msk(), other_c.msk(), g(*ok4), C.c_float(0))),                      # channel mismatch
               ("msk_sw_gather", (vol.msk(), patches.msk(), g((0, 0, 0, 0), (2, 0, 0, 0)), C.c_float(0))),   # n outside the batch
               ("msk_sw_gather", (vol.msk(), patches.msk(), g((0, 0, 0, 0), (-1, 0, 0, 0)), C.c_float(0))),
               ("msk_sw_gather", (vol.msk(), patches.msk(), g((0, 0, 0, 0), (0, 5, 0, 0)), C.c_float(0))),   # beside the volume
               ("msk_sw_gather", (vol.msk(), patches.msk(), g((0, 0, 0, 0), (0, 0, -4, 0)), C.c_float(0))),
               ("msk_sw_gather", (vol.msk(), patches.msk(), g((0, 0, 0, 0), (0, 0, 0, 9)), C.c_float(0))),
               ("msk_sw_gather", (vol.msk(), patches.msk(), None, C.c_float(0))),
               ("msk_sw_gather", (vol.msk(), NULL_TENSOR, g(*ok4), C.c_float(0))),
               ("msk_sw_gather", (vol.msk(), vol.msk(), g(*ok4), C.c_float(0))),                           # in place
               ("msk_sw_accumulate", (other_c.msk(), g(*ok7)) + tabs + (acc.msk(),)),                     # channel mismatch
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (2, 1, 3, 5, 1, 2, 3))) + tabs + (acc.msk(),)),    # n outside the batch
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (1, 1, 3, 5, nd, 2, 3))) + tabs + (acc.msk(),)),   # table rows
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (1, 1, 3, 5, 1, nh, 3))) + tabs + (acc.msk(),)),
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (1, 1, 3, 5, 1, 2, nw))) + tabs + (acc.msk(),)),
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (1, 1, 3, 5, -1, 2, 3))) + tabs + (acc.msk(),)),
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (1, -4, 3, 5, 1, 2, 3))) + tabs + (acc.msk(),)),   # beside the volume
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (1, 1, 7, 5, 1, 2, 3))) + tabs + (acc.msk(),)),
               ("msk_sw_accumulate", (lg.msk(), g(ok7[0], (1, 1, 3, -4, 1, 2, 3))) + tabs + (acc.msk(),)),
               ("msk_sw_accumulate", (lg.msk(), g(*ok7), None, nd, th, nh, tw, nw, acc.msk())),
               ("msk_sw_accumulate", (lg.msk(), g(*ok7), td, 0, th, nh, tw, nw, acc.msk())),
               ("msk_sw_accumulate", (lg.msk(), None) + tabs + (acc.msk(),)),
               ("msk_sw_accumulate", (lg.msk(), g(*ok7)) + tabs + (NULL_TENSOR,)),
               ("msk_sw_accumulate", (acc.msk(), g(*ok7)) + tabs + (acc.msk(),))]                         # acc is the logits
        for name, args in bad:
            rc = getattr(dev.lib, name)(dev.ctx, *args)
            assert rc != 0, (name, args[1:])
            assert _lib.last_error(dev.ctx), name
            with pytest.raises(MskError, match=name):
                dev.call(name, *args)
        assert np.isnan(acc.numpy()).all() and np.isnan(patches.numpy()).all()  # a valid first window was not launched either
        assert np.array_equal(vol.numpy(), x)
        # ... and the same calls with valid arguments run
        dev.call("msk_sw_gather", vol.msk(), patches.msk(), g(*ok4), C.c_float(0))
        dev.call("msk_sw_accumulate", lg.msk(), g(*ok7), *tabs, acc.msk())
        assert not np.isnan(patches.numpy()).any()


# ---- sliding_window_inference ------------------------------------------------------------------------------------------------
def _stub(f, calls=None):
    from medicalseg_amd.device import to_tensor

    def model(x):
        a = x.numpy()
        if calls is not None:
            calls.append(a)
        return [to_tensor(f(a))]
    return model


@pytest.mark.parametrize("n,shape,roi,overlap,mode,batch,cval", [
    (2, (5, 7, 9), (4, 4, 4), 0.5, 'gaussian', 3, 0.0), (2, (5, 7, 9), (4, 4, 4), 0.5, 'gaussian', 5, 0.0),
    (1, (2, 6, 10), (4, 4, 8), 0.5, 'constant', 1, -3.5), (1, (2, 6, 10), (4, 4, 8), 0.25, 'gaussian', 100, -3.5)])
def test_sliding_window_inference_plumbing_with_a_host_stub(n, shape, roi, overlap, mode, batch, cval):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    ref = R.Plan(shape, roi, overlap, mode)
    x = R.volume(n, shape, 1, 40)
    want_windows = R.crops(x, ref, cval)
    calls = []
    pred, logits = infer.sliding_window_inference(_stub(R.ramp_model, calls), to_tensor(x), roi, overlap=overlap, mode=mode,
                                                  sw_batch_size=batch, cval=cval)
    # the stub was shown exactly the expected windows, in order, batched as stated
    sizes = [len(a) for a in calls]
    b = min(batch, len(want_windows))
    assert sizes == [b] * (len(want_windows) // b) + ([len(want_windows) % b] if len(want_windows) % b else [])
    assert np.array_equal(np.concatenate(calls), np.stack(want_windows))
    want = R.blend([R.ramp_model(p[None])[0] for p in want_windows], ref, n)
    assert logits.shape == (n, 3) + shape and pred.shape == (n, 1) + shape
    assert np.array_equal(logits.numpy(), want)
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))


def test_constant_mode_exactness_reproduces_on_the_device():
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    x = R.integer_volume(2, (12, 8, 16), 3)
    pred, logits = infer.sliding_window_inference(_stub(R.pointwise_model), to_tensor(x), (8, 4, 8), overlap=0.5, mode='constant',
                                                  sw_batch_size=4)
    want = R.pointwise_model(x)
    assert np.array_equal(logits.numpy(), want)                                # the blend IS the model of the whole volume
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))


def _vnet(seed=5):
    from medicalseg_amd.models import VNet
    rng = np.random.default_rng(seed)
    model = VNet(num_classes=3)
    state = model.state_dict()
    for k_, v in state.items():                      # non-trivial running statistics and slopes
        if k_.endswith("._mean"):
            state[k_] = rng.standard_normal(v.shape).astype(np.float32) * 0.1
        elif k_.endswith("._variance"):
            state[k_] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif "relu" in k_ and k_.endswith("_weight"):
            state[k_] = rng.uniform(0.1, 0.4, v.shape).astype(np.float32)
    model.set_state_dict(state)
    model.eval()
    return model


@pytest.fixture(scope="module")
def vnet():
    return _vnet()


def _mem_free(dev):
    free, total = C.c_size_t(), C.c_size_t()
    dev.sync()
    dev.call("msk_mem_info", C.byref(free), C.byref(total))
    return free.value


def _hand_composition(vnet, x, ref, batch):
    """crop on the host, inference() per window batch with the SAME batching (kernel choice may depend on N), blend"""
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    windows = R.crops(x, ref)
    out = []
    for k in range(0, len(windows), batch):
        _, logit = infer.inference(vnet, to_tensor(np.stack(windows[k:k + batch])))
        out.extend(logit.numpy())
    return R.blend(out, ref, x.shape[0])


@pytest.mark.parametrize("batch", [1, 2])
def test_sliding_window_inference_of_a_real_net_equals_the_hand_composition(vnet, batch):
    from medicalseg_amd._lib import MskError
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import Tensor, to_tensor
    x = R.volume(1, (16, 16, 24), 1, 42)
    ref = R.Plan((16, 16, 24), (16, 16, 16), 0.5, 'gaussian')
    assert len(ref.windows(1)) == 2
    want = _hand_composition(vnet, x, ref, batch)
    im = to_tensor(x)
    pred, logits = infer.sliding_window_inference(vnet, im, (16, 16, 16), sw_batch_size=batch)
    assert np.array_equal(logits.numpy(), want)
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))
    # a second call at the same shapes allocates no device memory
    dev = logits.dev
    before = _mem_free(dev)
    pred2, logits2 = infer.sliding_window_inference(vnet, im, (16, 16, 16), sw_batch_size=batch)
    assert np.array_equal(logits2.numpy(), want) and np.array_equal(pred2.numpy()[:, 0], np.argmax(want, axis=1))
    assert _mem_free(dev) == before
    # the tensors of the first call belong to an earlier forward
    with pytest.raises(MskError, match="stale"):
        logits.numpy()
    # an input that lives in the activation arena (every forward resets it) is kept aside first
    act = Tensor.empty(dev, 1, 16, 16, 24, 1)
    dev.h2d(act.ptr, x)
    _, logits3 = infer.sliding_window_inference(vnet, act, (16, 16, 16), sw_batch_size=batch)
    assert np.array_equal(logits3.numpy(), want)


def test_sliding_release_frees_the_buffers(vnet):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    im = to_tensor(R.volume(1, (16, 16, 24), 1, 43))
    dev = im.dev
    infer.tta_release(dev)
    infer.sliding_release(dev)
    assert not dev.kept
    infer.aug_inference(vnet, to_tensor(R.volume(1, (16, 16, 16), 1, 44)), flip_axes=(2,))
    tta = dict(dev.kept)
    assert tta and all(key[0] == "tta" for key in tta)
    infer.sliding_window_inference(vnet, im, (16, 16, 16))
    assert any(key[0] == "sw" for key in dev.kept) and len(dev.kept) > len(tta)
    infer.sliding_release(dev)
    assert dev.kept == tta                                                       # the other path's buffers stay
    infer.tta_release(dev)
    assert not dev.kept
    pred, logits = infer.sliding_window_inference(vnet, im, (16, 16, 16))        # and they come back on demand
    assert logits.shape == (1, 3, 16, 16, 24)


# ---- evaluate ----------------------------------------------------------------------------------------------------------------
def _eval_setup(shape):
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    ds = SyntheticCT(num_samples=2, shape=shape, num_classes=3, mode="val")
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    return ds, losses


def test_evaluate_with_sliding_window_is_the_loop_by_hand(vnet):
    from medicalseg_amd import nn
    from medicalseg_amd.core import evaluate, infer
    from medicalseg_amd.datasets import DataLoader
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import loss_computation, metric
    ds, losses = _eval_setup((16, 16, 24))
    got = evaluate(vnet, ds, losses, print_detail=False, hard_metrics=True, sliding_window=(16, 16, 16))
    mdice, counts = 0.0, None
    with nn.fused_inference():
        for it, (im, label, idx) in enumerate(DataLoader(ds, batch_size=1, shuffle=False, drop_last=False, num_workers=0)):
            label_t = to_tensor(label.astype('int32'))
            pred, logits = infer.sliding_window_inference(vnet, to_tensor(im), (16, 16, 16))
            assert logits.shape == (1, 3, 16, 16, 24)
            _, pcd = loss_computation(logits, label_t, losses)
            mdice += np.mean(np.asarray(pcd))
            if counts is None:
                counts = metric.ConfusionCounts(pred.dev, 2, 3, 255, zero=True)
            metric.confusion_counts(pred, label_t, 3, 255, out=counts.rows(it, len(label)))
    c = counts.numpy()
    counts.free()
    areas = metric.areas_from_counts(c, 3, 255)
    class_iou, miou = metric.mean_iou(*areas)
    class_dice, hdice = metric.dice(*areas)
    assert got["mdice"] == float(mdice / 2)
    assert got["miou"] == float(miou) and got["dice"] == float(hdice)
    assert np.array_equal(got["class_iou"], class_iou) and np.array_equal(got["class_dice"], class_dice)
    assert got["acc"] == float(metric.accuracy(areas[0], areas[1])[1]) and got["kappa"] == float(metric.kappa(*areas))
    # the other arguments reach sliding_window_inference
    two = evaluate(vnet, ds, losses, print_detail=False, hard_metrics=True, sliding_window=(16, 16, 16), sw_batch_size=2,
                   sw_overlap=0.5, sw_mode='gaussian')
    assert set(two) == set(got) and np.isfinite(two["mdice"])
    const = evaluate(vnet, ds, losses, print_detail=False, sliding_window=(16, 16, 16), sw_mode='constant')
    assert const["mdice"] != got["mdice"]
    with pytest.raises(ValueError):
        evaluate(vnet, ds, losses, print_detail=False, sliding_window=(16, 16, 16), aug_eval=True)


def test_evaluate_without_sliding_window_is_what_it_was(vnet):
    """the plain loop by hand (16^3 volumes: one forward of the whole volume needs extents VNet's strides divide); the sw_*
    arguments without a roi change nothing"""
    from medicalseg_amd import nn
    from medicalseg_amd.core import evaluate, infer
    from medicalseg_amd.datasets import DataLoader
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import loss_computation
    ds, losses = _eval_setup((16, 16, 16))
    mdice = 0.0
    with nn.fused_inference():
        for im, label, idx in DataLoader(ds, batch_size=1, shuffle=False, drop_last=False, num_workers=0):
            pred, logits = infer.inference(vnet, to_tensor(im), ori_shape=label.shape[-3:], transforms=ds.transforms.transforms)
            _, pcd = loss_computation(logits, to_tensor(label.astype('int32')), losses)
            mdice += np.mean(np.asarray(pcd))
    want = {"mdice": float(mdice / 2)}
    assert evaluate(vnet, ds, losses, print_detail=False) == want
    assert evaluate(vnet, ds, losses, print_detail=False, sliding_window=None, sw_overlap=0.25, sw_mode='constant',
                    sw_batch_size=3) == want
    # a roi that covers the whole volume is one window whose weights are exactly 1: the same logits, the same result
    assert evaluate(vnet, ds, losses, print_detail=False, sliding_window=(16, 16, 16)) == want

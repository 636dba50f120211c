"""Mirroring inside sliding-window inference on the device (msk_sw_gather_mirrored / msk_sw_accumulate_mirrored of
medicalseg_amd/csrc/msk_sliding.hip, core/infer.py sliding_window_inference(mirror_axes=...), evaluate(sw_mirror_axes=...))
against the numpy statement of tests/sliding_mirror_reference.py.  Every comparison is np.array_equal on the uint32 view: no
tolerance anywhere.  The kernel tests use the red-zoned buffers of tests/helpers.py."""
import ctypes as C

import numpy as np
import pytest

import sliding_mirror_reference as M
import sliding_reference as R
import tta_reference as T
from helpers import redzone_check, t_empty, t_from_ncdhw, vec  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

ASYM = (1, (3, 5, 6), (4, 8, 8), 0.5)        # padding before / after: 0 / 1 on D, 1 / 2 on H, 1 / 1 on W


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _plans(shape, roi, overlap, mode):
    """the product's plan (whose tables go to the device) and the statement's"""
    from medicalseg_amd.core.infer import SlidingPlan
    return SlidingPlan(shape, roi, overlap=overlap, mode=mode), R.Plan(shape, roi, overlap, mode)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _rows(plan, passes, cols):
    """host origins: cols 5 = (n, d0, h0, w0, mask), 8 = (n, d0, h0, w0, id, ih, iw, mask), 4 / 7 = the unmirrored forms"""
    rows = [plan.origin(wd) + (wd[1:] if cols >= 7 else ()) + ((m,) if cols in (5, 8) else ()) for wd, m in passes]
    return np.ascontiguousarray(np.array(rows, np.int32))


def _sub(t, k, count):
    """items k .. k + count of a batch tensor, as a tensor"""
    from medicalseg_amd.device import Tensor
    return Tensor(t.dev, t.ptr + 4 * k * t.d * t.h * t.w * t.ld, count, t.d, t.h, t.w, t.c, t.ld, None)


def _batches(count):
    return sorted({1, min(3, count), count})


def _tables(plan):
    return [(C.c_void_p(vec(t)), len(s)) for t, s in zip(plan.tables, plan.starts)]


def _tab_args(tables):
    return tuple(v for pair in tables for v in pair)


def _accumulate(dev, plan, tables, logits_t, passes, scale, acc_t):
    dev.call("msk_sw_accumulate_mirrored", logits_t.msk(), _ptr(_rows(plan, passes, 8)), *_tab_args(tables), C.c_float(scale),
             acc_t.msk())


def _pass_logits(count, roi, c, seed):
    return [T.logits_case((1,) + tuple(roi) + (c,), seed + i)[0] for i in range(count)]


# ---- msk_sw_gather_mirrored --------------------------------------------------------------------------------------------------
GATHER_CASES = [  # (n, volume, roi, overlap, cin, cval): those of test_gpu_sliding.py and the asymmetric padding
    (2, (5, 7, 9), (4, 4, 4), 0.5, 1, 0.0), (2, (5, 7, 9), (4, 4, 4), 0.5, 2, 0.0),
    (1, (2, 6, 10), (4, 4, 8), 0.5, 1, 0.0), (1, (2, 6, 10), (4, 4, 8), 0.5, 1, -3.5), (1, (2, 6, 10), (4, 4, 8), 0.5, 4, -3.5),
    (1, (2, 3, 300), (2, 2, 260), 0.25, 1, 0.0), (1, (2, 3, 300), (2, 2, 260), 0.25, 2, 1.0),
    (1, (4, 4, 4), (4, 4, 8), 0.5, 2, -3.5),
    ASYM + (2, -3.5)]


@pytest.mark.parametrize("n,shape,roi,overlap,cin,cval", GATHER_CASES)
def test_gather_equals_the_statement(n, shape, roi, overlap, cin, cval):
    plan, ref = _plans(shape, roi, overlap, 'constant')
    if shape == ASYM[1]:
        assert [(r - s) // 2 for r, s in zip(roi, shape)] == [0, 1, 1] and [r - s for r, s in zip(roi, shape)] == [1, 3, 2]
    x = R.volume(n, shape, cin, 1)
    passes = M.work(ref, n, list(range(8)))                                     # every mask, mixed within one call
    want = np.stack(M.gathers(x, ref, list(range(8)), cval))
    assert len(passes) == len(want)
    vol = t_from_ncdhw(x)
    for batch in _batches(len(passes)):
        dst = t_empty(len(passes), cin, *roi)
        for k in range(0, len(passes), batch):
            group = passes[k:k + batch]
            vol.dev.call("msk_sw_gather_mirrored", vol.msk(), _sub(dst, k, len(group)).msk(), _ptr(_rows(plan, group, 5)), C.c_float(cval))
        assert _same(dst.numpy(), want), batch
    assert _same(vol.numpy(), x)


# ---- msk_sw_accumulate_mirrored ----------------------------------------------------------------------------------------------
ACC_CASES = [  # (n, volume, roi, overlap, c): those of test_gpu_sliding.py and the asymmetric padding
    (2, (5, 7, 9), (4, 4, 4), 0.5, 1), (2, (5, 7, 9), (4, 4, 4), 0.5, 3),
    (1, (2, 6, 10), (4, 4, 8), 0.5, 20), (1, (2, 6, 10), (4, 4, 8), 0.5, 2),
    (1, (2, 3, 300), (2, 2, 260), 0.25, 3), (1, (2, 3, 300), (2, 2, 260), 0.25, 4),
    (1, (4, 4, 4), (4, 4, 8), 0.5, 2),
    (1, (8, 8, 8), (4, 4, 4), 0.0, 3),
    ASYM + (3,)]
AXES_OF_K = {1: (), 2: (2,), 4: (0, 2), 8: (0, 1, 2)}


@pytest.mark.parametrize("mode", ['gaussian', 'constant'])
@pytest.mark.parametrize("n,shape,roi,overlap,c", ACC_CASES)
def test_accumulate_equals_the_statement(n, shape, roi, overlap, c, mode):
    plan, ref = _plans(shape, roi, overlap, mode)
    tables = _tables(plan)
    for K, axes in AXES_OF_K.items():
        passes = M.work(ref, n, M.masks_of(axes))
        scale = np.float32(1) / np.float32(K)
        lg = _pass_logits(len(passes), roi, c, 10 + K)
        want = M.blend(lg, ref, passes, scale, n)
        src = t_from_ncdhw(np.stack(lg))
        for batch in _batches(len(passes)):          # one row per call, 3 rows (runs straddle calls), all rows in one call
            acc = t_from_ncdhw(np.zeros((n, c) + shape, np.float32))
            for k in range(0, len(passes), batch):
                group = passes[k:k + batch]
                _accumulate(src.dev, plan, tables, _sub(src, k, len(group)), group, scale, acc)
            assert _same(acc.numpy(), want), (K, batch)


def test_a_run_longer_than_eight_rows_is_split():
    n, shape, roi, c = 1, (4, 4, 8), (4, 4, 8), 2                               # one window
    plan, ref = _plans(shape, roi, 0.5, 'gaussian')
    wd = plan.windows(n)[0]
    passes = [(wd, m) for m in (0, 4, 1, 5, 2, 6, 3, 7, 7, 0, 4)]
    lg = _pass_logits(len(passes), roi, c, 50)
    want = M.blend(lg, ref, passes, 0.25, n)
    acc = t_from_ncdhw(np.zeros((n, c) + shape, np.float32))
    _accumulate(acc.dev, plan, _tables(plan), t_from_ncdhw(np.stack(lg)), passes, 0.25, acc)
    assert _same(acc.numpy(), want)


# ---- equalities with the existing kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape,roi,overlap,c", [ACC_CASES[1], ACC_CASES[2], ACC_CASES[3], ACC_CASES[0], ACC_CASES[8]])
def test_equalities_with_the_unmirrored_kernels(n, shape, roi, overlap, c):
    plan, ref = _plans(shape, roi, overlap, 'gaussian')
    windows = plan.windows(n)
    plain = [(wd, 0) for wd in windows]
    tables = _tables(plan)
    # gather, masks all 0
    x = R.volume(n, shape, c, 2)
    vol = t_from_ncdhw(x)
    d = vol.dev
    a, b = t_empty(len(windows), c, *roi), t_empty(len(windows), c, *roi)
    d.call("msk_sw_gather", vol.msk(), a.msk(), _ptr(_rows(plan, plain, 4)), C.c_float(-3.5))
    d.call("msk_sw_gather_mirrored", vol.msk(), b.msk(), _ptr(_rows(plan, plain, 5)), C.c_float(-3.5))
    assert _same(a.numpy(), b.numpy())
    # accumulate, masks all 0 and scale 1
    lg = np.stack(_pass_logits(len(windows), roi, c, 60))
    src = t_from_ncdhw(lg)
    acc0, acc1 = (t_from_ncdhw(np.zeros((n, c) + shape, np.float32)) for _ in range(2))
    d.call("msk_sw_accumulate", src.msk(), _ptr(_rows(plan, plain, 7)), *_tab_args(tables), acc0.msk())
    _accumulate(d, plan, tables, src, plain, 1.0, acc1)
    assert _same(acc0.numpy(), acc1.numpy())
    # one pass per window with mask m and scale 1: msk_flip_axes of the logits, then msk_sw_accumulate
    for mask in range(1, 8):
        flipped = t_empty(len(windows), c, *roi)
        d.call("msk_flip_axes", src.msk(), flipped.msk(), mask)
        acc0, acc1 = (t_from_ncdhw(np.zeros((n, c) + shape, np.float32)) for _ in range(2))
        d.call("msk_sw_accumulate", flipped.msk(), _ptr(_rows(plan, plain, 7)), *_tab_args(tables), acc0.msk())
        _accumulate(d, plan, tables, src, [(wd, mask) for wd in windows], 1.0, acc1)
        assert _same(acc0.numpy(), acc1.numpy()), mask


# ---- channel-slice views -----------------------------------------------------------------------------------------------------
def test_gather_on_channel_slice_views():
    n, shape, roi, c = 1, (2, 6, 10), (4, 4, 8), 2
    plan, ref = _plans(shape, roi, 0.5, 'constant')
    wide = R.volume(n, shape, 4, 2)
    masks = list(range(8))
    passes = M.work(ref, n, masks)
    want = np.stack(M.gathers(wide[:, 1:1 + c], ref, masks, -3.5))
    o5 = _ptr(_rows(plan, passes, 5))
    vol = t_from_ncdhw(wide)
    dst = t_empty(len(passes), c + 1, *roi, fill=7.0)                           # a view on both sides
    vol.dev.call("msk_sw_gather_mirrored", vol.channel_slice(1, 1 + c).msk(), dst.channel_slice(1, 1 + c).msk(), o5, C.c_float(-3.5))
    got = dst.numpy()
    assert _same(got[:, 1:], want) and (got[:, 0] == 7.0).all()                 # the channel beside the view is untouched
    dense = t_empty(len(passes), c, *roi)                                       # a view as the source of dense patches
    vol.dev.call("msk_sw_gather_mirrored", vol.channel_slice(1, 1 + c).msk(), dense.msk(), o5, C.c_float(-3.5))
    assert _same(dense.numpy(), want)
    into = t_empty(len(passes), c + 2, *roi, fill=7.0)                          # a dense source into a view
    vol.dev.call("msk_sw_gather_mirrored", t_from_ncdhw(wide[:, 1:1 + c]).msk(), into.channel_slice(1, 1 + c).msk(), o5, C.c_float(-3.5))
    got = into.numpy()
    assert _same(got[:, 1:1 + c], want) and (got[:, 0] == 7.0).all() and (got[:, 1 + c] == 7.0).all()
    assert _same(vol.numpy(), wide)


def test_accumulate_on_channel_slice_views():
    n, shape, roi, c = 2, (5, 7, 9), (4, 4, 4), 3
    plan, ref = _plans(shape, roi, 0.5, 'gaussian')
    passes = M.work(ref, n, M.masks_of((0, 1, 2)))
    lg = _pass_logits(len(passes), roi, c, 20)
    wide = np.concatenate([R.volume(len(passes), roi, 2, 21), np.stack(lg)], axis=1)              # the logits are channels 2..4
    base = np.full((n, c + 2) + shape, 7.0, np.float32)
    tables = _tables(plan)
    want = M.blend(lg, ref, passes, 0.125, n, acc=base[:, 1:1 + c])
    src = t_from_ncdhw(wide)
    acc = t_from_ncdhw(base)
    _accumulate(acc.dev, plan, tables, src.channel_slice(2, 2 + c), passes, 0.125, acc.channel_slice(1, 1 + c))
    got = acc.numpy()
    assert _same(got[:, 1:1 + c], want)
    assert (got[:, 0] == 7.0).all() and (got[:, 1 + c] == 7.0).all()           # the channels around the view are untouched
    dense = t_from_ncdhw(base[:, 1:1 + c])                                      # a view on the logits' side only, and on acc's only
    _accumulate(acc.dev, plan, tables, src.channel_slice(2, 2 + c), passes, 0.125, dense)
    assert _same(dense.numpy(), want)
    acc = t_from_ncdhw(base)
    _accumulate(acc.dev, plan, tables, t_from_ncdhw(np.stack(lg)), passes, 0.125, acc.channel_slice(1, 1 + c))
    got = acc.numpy()
    assert _same(got[:, 1:1 + c], want) and (got[:, 0] == 7.0).all() and (got[:, 1 + c] == 7.0).all()
    assert _same(src.numpy(), wide)


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import NULL_TENSOR, MskError
    n, shape, roi, c = 2, (5, 7, 9), (4, 4, 4), 3
    plan, ref = _plans(shape, roi, 0.5, 'gaussian')
    tables = _tables(plan)
    (td, nd), (th, nh), (tw, nw) = tables
    x = R.volume(n, shape, c, 30)
    vol = t_from_ncdhw(x)
    dev = vol.dev
    patches = t_empty(2, c, *roi)
    acc = t_empty(n, c, *shape)
    lg = t_from_ncdhw(R.volume(2, roi, c, 31))
    other_c = t_from_ncdhw(R.volume(2, roi, c + 1, 32))
    one = C.c_float(1.0)

    def g(*rows):
        return _ptr(np.ascontiguousarray(np.array(rows, np.int32)))
    ok5, ok8 = [(0, 0, 0, 0, 3), (1, 1, 3, 5, 4)], [(0, 0, 0, 0, 0, 0, 0, 3), (1, 1, 3, 5, 1, 2, 3, 4)]
    tabs = _tab_args(tables)
    G, A = "msk_sw_gather_mirrored", "msk_sw_accumulate_mirrored"
    bad = [(G, (vol.msk(), patches.msk(), g(ok5[0], (1, 1, 3, 5, 8)), C.c_float(0))),                     # mask 8
           (G, (vol.msk(), patches.msk(), g(ok5[0], (1, 1, 3, 5, -1)), C.c_float(0))),                    # mask -1
           (G, (vol.msk(), other_c.msk(), g(*ok5), C.c_float(0))),                                        # channel mismatch
           (G, (vol.msk(), patches.msk(), g(ok5[0], (2, 0, 0, 0, 0)), C.c_float(0))),                     # n outside the batch
           (G, (vol.msk(), patches.msk(), g(ok5[0], (0, 5, 0, 0, 0)), C.c_float(0))),                     # beside the volume
           (G, (vol.msk(), patches.msk(), None, C.c_float(0))),
           (G, (vol.msk(), NULL_TENSOR, g(*ok5), C.c_float(0))),
           (G, (vol.msk(), vol.msk(), g(*ok5), C.c_float(0))),                                            # in place
           (A, (lg.msk(), g(ok8[0], (1, 1, 3, 5, 1, 2, 3, 8))) + tabs + (one, acc.msk())),                # mask 8
           (A, (lg.msk(), g(ok8[0], (1, 1, 3, 5, 1, 2, 3, -1))) + tabs + (one, acc.msk())),               # mask -1
           (A, (lg.msk(), g(*ok8)) + tabs + (C.c_float(0.0), acc.msk())),                                 # scale 0
           (A, (lg.msk(), g(*ok8)) + tabs + (C.c_float(float('nan')), acc.msk())),                        # scale NaN
           (A, (lg.msk(), g(*ok8)) + tabs + (C.c_float(-0.5), acc.msk())),
           (A, (lg.msk(), g(*ok8)) + tabs + (C.c_float(float('inf')), acc.msk())),
           (A, (other_c.msk(), g(*ok8)) + tabs + (one, acc.msk())),                                       # channel mismatch
           (A, (lg.msk(), g(ok8[0], (2, 1, 3, 5, 1, 2, 3, 0))) + tabs + (one, acc.msk())),                # n outside the batch
           (A, (lg.msk(), g(ok8[0], (1, 1, 3, 5, nd, 2, 3, 0))) + tabs + (one, acc.msk())),               # table row
           (A, (lg.msk(), g(ok8[0], (1, -4, 3, 5, 1, 2, 3, 0))) + tabs + (one, acc.msk())),               # beside the volume
           (A, (lg.msk(), g(*ok8), None, nd, th, nh, tw, nw, one, acc.msk())),
           (A, (lg.msk(), None) + tabs + (one, acc.msk())),
           (A, (lg.msk(), g(*ok8)) + tabs + (one, NULL_TENSOR)),
           (A, (acc.msk(), g(*ok8)) + tabs + (one, acc.msk()))]                                           # acc is the logits
    for name, args in bad:
        rc = getattr(dev.lib, name)(dev.ctx, *args)
        assert rc != 0, (name, args[1:])
        assert _lib.last_error(dev.ctx), name
        with pytest.raises(MskError, match=name):
            dev.call(name, *args)
    assert np.isnan(acc.numpy()).all() and np.isnan(patches.numpy()).all()      # a valid first row was not launched either
    assert _same(vol.numpy(), x)
    # ... and the same calls with valid arguments run
    dev.call(G, vol.msk(), patches.msk(), g(*ok5), C.c_float(0))
    dev.call(A, lg.msk(), g(*ok8), *tabs, one, acc.msk())
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


@pytest.mark.parametrize("axes,batch", [((0, 2), 3), ((0, 2), 100), ((0, 1, 2), 5)])
def test_sliding_window_inference_plumbing_with_a_host_stub(axes, batch):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    n, shape, roi = 1, (5, 7, 9), (4, 4, 4)
    ref = R.Plan(shape, roi, 0.5, 'gaussian')
    x = R.volume(n, shape, 1, 40)
    masks = M.masks_of(axes)
    want_passes = M.gathers(x, ref, masks)
    calls = []
    pred, logits = infer.sliding_window_inference(_stub(R.ramp_model, calls), to_tensor(x), roi, sw_batch_size=batch, mirror_axes=axes)
    # the stub was shown exactly the statement's mirrored windows, in order, batched as stated
    count = len(want_passes)
    b = min(batch, count)
    assert [len(a) for a in calls] == [b] * (count // b) + ([count % b] if count % b else [])
    assert _same(np.concatenate(calls), np.stack(want_passes))
    want = M.predict(R.ramp_model, x, ref, axes)
    assert logits.shape == (n, 3) + shape and pred.shape == (n, 1) + shape
    assert _same(logits.numpy(), want)
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))
    assert not np.array_equal(want, R.blend(R.model_on_windows(R.ramp_model, x, ref), ref, n))     # the mirrors do something


@pytest.mark.parametrize("axes", [(2,), (0, 1), (0, 1, 2)])
def test_constant_mode_exactness_reproduces_on_the_device(axes):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    x = R.integer_volume(2, (12, 8, 16), 3)
    pred, logits = infer.sliding_window_inference(_stub(R.pointwise_model), to_tensor(x), (8, 4, 8), overlap=0.5, mode='constant',
                                                  sw_batch_size=4, mirror_axes=axes)
    want = R.pointwise_model(x)
    assert np.array_equal(logits.numpy(), want)                                # the blend IS the model of the whole volume
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))


def test_no_mirror_axes_is_the_call_of_before(monkeypatch):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import Device, to_tensor
    shape, roi = (5, 7, 9), (4, 4, 4)
    x = R.volume(2, shape, 1, 41)
    names = []
    real = Device.call

    def recording(self, name, *args):
        names.append(name)
        return real(self, name, *args)
    infer.sliding_window_inference(_stub(R.ramp_model), to_tensor(x), roi, sw_batch_size=5)      # the buffers exist from here on
    monkeypatch.setattr(Device, "call", recording)
    _, logits = infer.sliding_window_inference(_stub(R.ramp_model), to_tensor(x), roi, sw_batch_size=5)
    before, first = logits.numpy(), list(names)
    del names[:]
    _, logits = infer.sliding_window_inference(_stub(R.ramp_model), to_tensor(x), roi, sw_batch_size=5, mirror_axes=())
    assert _same(logits.numpy(), before)
    assert names == first and "msk_sw_gather" in names and "msk_sw_accumulate" in names
    assert "msk_sw_gather_mirrored" not in names and "msk_sw_accumulate_mirrored" not in names
    del names[:]
    infer.sliding_window_inference(_stub(R.ramp_model), to_tensor(x), roi, sw_batch_size=5, mirror_axes=(1,))
    assert "msk_sw_gather_mirrored" in names and "msk_sw_accumulate_mirrored" in names
    assert "msk_sw_gather" not in names and "msk_sw_accumulate" not in names and "msk_flip_axes" not in names


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


def _hand_composition(vnet, x, ref, axes, batch):
    """crop and flip on the host, inference() per pass batch with the SAME batching (kernel choice may depend on N), then the
    statement's blend"""
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    masks = M.masks_of(axes)
    passes = M.work(ref, x.shape[0], masks)
    shown = M.gathers(x, ref, masks)
    out = []
    for k in range(0, len(shown), batch):
        _, logit = infer.inference(vnet, to_tensor(np.stack(shown[k:k + batch])))
        out.extend(logit.numpy())
    return M.blend(out, ref, passes, np.float32(1) / np.float32(len(masks)), x.shape[0])


@pytest.mark.parametrize("batch", [3, 8])
def test_sliding_window_inference_of_a_real_net_equals_the_hand_composition(vnet, batch):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    x = R.volume(1, (16, 16, 24), 1, 42)
    ref = R.Plan((16, 16, 24), (16, 16, 16), 0.5, 'gaussian')
    assert len(M.work(ref, 1, M.masks_of((0, 1, 2)))) == 16
    want = _hand_composition(vnet, x, ref, (0, 1, 2), batch)
    im = to_tensor(x)
    pred, logits = infer.sliding_window_inference(vnet, im, (16, 16, 16), sw_batch_size=batch, mirror_axes=(0, 1, 2))
    assert _same(logits.numpy(), want)
    assert np.array_equal(pred.numpy()[:, 0], np.argmax(want, axis=1))
    # a second call at the same shapes allocates no device memory
    dev = logits.dev
    before = _mem_free(dev)
    pred2, logits2 = infer.sliding_window_inference(vnet, im, (16, 16, 16), sw_batch_size=batch, mirror_axes=(0, 1, 2))
    assert _same(logits2.numpy(), want) and np.array_equal(pred2.numpy()[:, 0], np.argmax(want, axis=1))
    assert _mem_free(dev) == before


# ---- evaluate ----------------------------------------------------------------------------------------------------------------
def test_evaluate_with_sw_mirror_axes_is_the_loop_by_hand(vnet):
    from medicalseg_amd import nn
    from medicalseg_amd.core import evaluate, infer
    from medicalseg_amd.datasets import DataLoader, SyntheticCT
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation, metric
    ds = SyntheticCT(num_samples=2, shape=(16, 16, 24), num_classes=3, mode="val")
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    plain = evaluate(vnet, ds, losses, print_detail=False, hard_metrics=True, sliding_window=(16, 16, 16))
    got = evaluate(vnet, ds, losses, print_detail=False, hard_metrics=True, sliding_window=(16, 16, 16), sw_mirror_axes=(0, 2))
    mdice, plain_mdice, counts = 0.0, 0.0, None
    with nn.fused_inference():
        for it, (im, label, idx) in enumerate(DataLoader(ds, batch_size=1, shuffle=False, drop_last=False, num_workers=0)):
            label_t = to_tensor(label.astype('int32'))
            _, logits = infer.sliding_window_inference(vnet, to_tensor(im), (16, 16, 16))
            plain_mdice += np.mean(np.asarray(loss_computation(logits, label_t, losses)[1]))
            pred, logits = infer.sliding_window_inference(vnet, to_tensor(im), (16, 16, 16), mirror_axes=(0, 2))
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
    # evaluate without the new keyword returns what it returned before, and the mirrors change the logits
    assert plain["mdice"] == float(plain_mdice / 2) and set(plain) == set(got)
    assert evaluate(vnet, ds, losses, print_detail=False, hard_metrics=True, sliding_window=(16, 16, 16), sw_mirror_axes=())["mdice"] \
        == plain["mdice"]
    assert got["mdice"] != plain["mdice"]
    with pytest.raises(ValueError):
        evaluate(vnet, ds, losses, print_detail=False, sliding_window=(16, 16, 16), sw_mirror_axes=(0, 2), aug_eval=True)
    with pytest.raises(ValueError):
        evaluate(vnet, ds, losses, print_detail=False, sw_mirror_axes=(0, 2))

"""Gradient clipping and Nesterov momentum on the device (medicalseg_amd/csrc/msk_clip.hip: msk_grad_clip_coef,
msk_sgd_momentum_clip, msk_adam_clip; optimizer.Momentum / Adam with grad_clip / use_nesterov) against the numpy statement of
tests/clip_reference.py.

The sum of squares is compared bit for bit; the norm and the coefficient within one ulp of their format (they are single IEEE
operations on that sum); the updates at the tolerance tests/test_gpu_ops.py uses for msk_sgd_momentum / msk_adam; and a clip
that does not bite with np.array_equal against those two entry points.  Every buffer is red-zoned (tests/helpers.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import clip_reference as R
from helpers import SENTINEL_BITS, dev, dfree, dmalloc, redzone_check, rel_err, vec  # noqa: F401  (redzone_check: autouse here)

pytestmark = pytest.mark.gpu

# a tail-only chunk, an exact chunk, one element over, and 257 chunks: the finish pass takes a second row
N_LIST = [1, 3, 4, 4095, 4096, 4097, 10007, 1048581]
# 2053 chunks: every lane of the finish pass takes one eight-deep round of loads, lanes 0..4 one more term
N_FINISH = 2052 * 4096 + 7
V = C.c_void_p
F = C.c_float
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _grad(n, scale):
    a = (np.random.default_rng(n + 29).standard_normal(n) * scale).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _sumsq(n, scale):
    return R.sumsq(_grad(n, scale))


def _want(n, scale, gs, clip_norm):
    """the statement's record from the shared sum"""
    S = _sumsq(n, scale)
    norm = np.float64(np.float32(gs)) * np.sqrt(np.float64(S))
    return np.array([S, norm, np.float64(R.coef_of(norm, clip_norm)), 0.0], np.float64)


def _workspace(n):
    b = C.c_size_t(0)
    assert dev().lib.msk_grad_clip_workspace(C.c_size_t(n), C.byref(b)) == 0 and b.value == -(-n // 4096) * 8
    return dmalloc(b.value)


def _coef(g, n, gs, clip_norm, ws, rec):
    dev().call("msk_grad_clip_coef", V(g), C.c_size_t(n), F(gs), F(clip_norm), V(ws), V(rec))


def _ulp_apart(a, b, dtype):
    a, b = dtype(a), dtype(b)
    return abs(float(a) - float(b)) <= float(np.spacing(np.abs(b)))


# ---- msk_grad_clip_coef --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_record_equals_the_statement(scale):
    d = dev()
    bites = 0
    for n in N_LIST + [N_FINISH]:
        g = vec(_grad(n, scale))
        ws, rec = _workspace(n), dmalloc(32)
        for gs in (1.0, 0.5):
            norm = float(_want(n, scale, gs, INF)[1])
            for clip_norm in (1e9, INF, float(np.float32(norm / 4))):
                _coef(g, n, gs, clip_norm, ws, rec)                                # the same workspace and record again
                got, want = d.d2h(rec, (4,), np.float64), _want(n, scale, gs, clip_norm)
                what = (n, scale, gs, clip_norm, got.tolist(), want.tolist())
                assert got[0] == want[0] and got[3] == 0.0, what                   # S bit for bit
                assert _ulp_apart(got[1], want[1], np.float64), what
                assert got[2] == float(np.float32(got[2])) and _ulp_apart(got[2], want[2], np.float32), what
                if clip_norm >= 1e9:
                    assert got[2] == 1.0, what
                elif norm > 0:
                    assert want[2] < 1.0 and got[2] < 1.0 and abs(got[2] - 0.25) < 1e-6, what
                    bites += 1
        assert np.array_equal(d.d2h(g, (n,), np.float32), _grad(n, scale))
        for p in (g, ws, rec):
            dfree(p)
    assert bites == 2 * (len(N_LIST) + 1)


def test_coef_and_intensity_stats_share_one_sum():
    """msk_grad_clip_coef and msk_intensity_stats are two instantiations of one reduction: the same sum of squares, bit for bit"""
    d = dev()
    for n in N_LIST + [N_FINISH]:
        g = vec(_grad(n, 1e-3))
        b = C.c_size_t(0)
        assert d.lib.msk_intensity_stats_workspace(C.c_long(n), C.byref(b)) == 0
        ws, rec, ws_stats, stats = _workspace(n), dmalloc(32), dmalloc(b.value), dmalloc(32)
        _coef(g, n, 1.0, INF, ws, rec)
        d.call("msk_intensity_stats", V(g), C.c_long(n), V(ws_stats), V(stats))
        S, want = float(d.d2h(rec, (4,), np.float64)[0]), float(d.d2h(stats, (4,), np.float64)[3])
        assert S == want and S > 0, (n, S, want)
        for p in (g, ws, rec, ws_stats, stats):
            dfree(p)


def test_coef_argument_errors_launch_nothing():
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import MskError
    d = dev()
    n = 10007
    host = np.empty(n + 4, np.float32)
    host[:] = 1.0
    g = vec(host)
    ws, rec = _workspace(n), dmalloc(32)
    sz = C.c_size_t
    bad = [(V(g + 4), sz(n), F(1), F(12), V(ws), V(rec)),                          # grad only 4-byte aligned
           (V(g), sz(n), F(1), F(0), V(ws), V(rec)),                               # clip_norm 0, negative, NaN
           (V(g), sz(n), F(1), F(-1), V(ws), V(rec)),
           (V(g), sz(n), F(1), F(float("nan")), V(ws), V(rec)),
           (V(g), sz(0), F(1), F(12), V(ws), V(rec)),
           (V(g), sz(2 ** 31), F(1), F(12), V(ws), V(rec)),
           (None, sz(n), F(1), F(12), V(ws), V(rec)),
           (V(g), sz(n), F(1), F(12), None, V(rec)),
           (V(g), sz(n), F(1), F(12), V(ws), None),
           (V(g), sz(n), F(1), F(12), V(ws + 4), V(rec)),
           (V(g), sz(n), F(1), F(12), V(ws), V(rec + 4))]
    for args in bad:
        assert d.lib.msk_grad_clip_coef(d.ctx, *args) != 0, args
        assert _lib.last_error(d.ctx)
    with pytest.raises(MskError, match="msk_grad_clip_coef"):
        d.call("msk_grad_clip_coef", *bad[1])
    b = sz(5)
    assert d.lib.msk_grad_clip_workspace(sz(0), C.byref(b)) != 0 and d.lib.msk_grad_clip_workspace(sz(2 ** 31), C.byref(b)) != 0
    pv = dmalloc(16)
    for args in [(V(g), V(g), V(pv + 4)), (V(g + 4), V(g), V(pv))]:                 # misaligned velocity / param
        assert d.lib.msk_sgd_momentum_clip(d.ctx, *args, sz(4), F(0.1), F(0.9), F(0), F(1), 0, None, F(-INF), F(INF)) != 0
    assert d.lib.msk_sgd_momentum_clip(d.ctx, V(g), V(g), V(pv), sz(4), F(0.1), F(0.9), F(0), F(1), 0, None, F(1), F(-1)) != 0
    assert d.lib.msk_sgd_momentum_clip(d.ctx, V(g), V(g), V(pv), sz(4), F(0.1), F(0.9), F(0), F(1), 0, V(rec + 4), F(-1), F(1)) != 0
    # nothing was launched
    assert (d.d2h(rec, (8,), np.uint32) == SENTINEL_BITS).all() and (d.d2h(ws, (6,), np.uint32) == SENTINEL_BITS).all()
    assert (d.d2h(pv, (4,), np.uint32) == SENTINEL_BITS).all() and np.array_equal(d.d2h(g, (n + 4,), np.float32), host)
    # ... and the same call with valid arguments runs
    _coef(g, n, 1.0, 12.0, ws, rec)
    got = d.d2h(rec, (4,), np.float64)
    assert got[0] == float(n) and got[2] == float(np.float32(12.0 / np.sqrt(np.float64(n))))


# ---- msk_sgd_momentum_clip -------------------------------------------------------------------------------------------------------
LR, MU, WD = 0.01, 0.9, 1e-4


@functools.lru_cache(maxsize=None)
def _pgv(n):
    rng = np.random.default_rng(n + 3)
    out = tuple(rng.standard_normal(n).astype(np.float32) for _ in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def _sgd_clip(p, g, v, n, gs, nesterov, rec, lo, hi):
    dev().call("msk_sgd_momentum_clip", V(p), V(g), V(v), C.c_size_t(n), F(LR), F(MU), F(WD), F(gs), int(nesterov),
               V(rec) if rec else None, F(lo), F(hi))


SGD_CASES = [("global norm", 1.0, False, True, None), ("nesterov", 1.0, True, False, None), ("clamp", 1.0, False, False, 0.5),
             ("all three", 0.5, True, True, 0.5)]


@pytest.mark.parametrize("n", [10007, 3])
@pytest.mark.parametrize("name,gs,nesterov,clip,bound", SGD_CASES, ids=[c[0] for c in SGD_CASES])
def test_sgd_momentum_clip_matches_the_statement(name, gs, nesterov, clip, bound, n):
    d = dev()
    p, g, v = _pgv(n)
    pp, gp, vp_ = vec(p), vec(g), vec(v)
    rec, coef = None, 1.0
    if clip:                                                   # the record goes from one kernel to the other on the device
        want = R.record(g, gs, 1.0)
        clip_norm = float(np.float32(want[1] / 4))
        want = R.record(g, gs, clip_norm)
        coef = want[2]
        assert coef < 1.0
        ws, rec = _workspace(n), dmalloc(32)
        _coef(gp, n, gs, clip_norm, ws, rec)
    if bound:                                                  # +-0.5 sigma of the gradient the clamp sees: g is standard normal
        bound = float(np.float32(bound * float(np.float32(np.float32(gs) * np.float32(coef)))))
    lo, hi = (-bound, bound) if bound else (-INF, INF)
    _sgd_clip(pp, gp, vp_, n, gs, nesterov, rec, lo, hi)
    p2, v2 = R.sgd_step(p, g, v, LR, MU, WD, gs, nesterov, coef, *((lo, hi) if bound else (None, None)))
    ev, ep = rel_err(d.d2h(vp_, (n,), np.float32), v2), rel_err(d.d2h(pp, (n,), np.float32), p2)
    print("%s n = %d: velocity %.3e, param %.3e" % (name, n, ev, ep))
    assert ev < 1e-6 and ep < 1e-6
    assert np.array_equal(d.d2h(gp, (n,), np.float32), g)
    # the option changed something: the plain step is further away than the tolerance
    p0, v0 = R.sgd_step(p, g, v, LR, MU, WD, gs)
    assert rel_err(p0, p2) > 1e-4
    if bound and n > 3:
        gc = np.abs(R.clipped(g, gs, coef))
        assert (gc > bound).any() and (gc < bound).any()       # the clamp did bind, and not everywhere


@pytest.mark.parametrize("n", [10007, 3])
def test_sgd_momentum_clip_that_does_not_bite_is_bitwise_sgd_momentum(n):
    d = dev()
    p, g, v = _pgv(n)
    gp = vec(g)
    ws, rec = _workspace(n), dmalloc(32)
    _coef(gp, n, 0.5, INF, ws, rec)                            # a record whose coef is 1
    assert d.d2h(rec, (4,), np.float64)[2] == 1.0
    pa, va = vec(p), vec(v)
    d.call("msk_sgd_momentum", V(pa), V(gp), V(va), C.c_size_t(n), F(LR), F(MU), F(WD), F(0.5))
    want_p, want_v = d.d2h(pa, (n,), np.float32), d.d2h(va, (n,), np.float32)
    assert not np.array_equal(want_p, p)
    for r in (None, rec):
        pb, vb = vec(p), vec(v)
        _sgd_clip(pb, gp, vb, n, 0.5, False, r, -INF, INF)
        assert np.array_equal(d.d2h(pb, (n,), np.float32), want_p) and np.array_equal(d.d2h(vb, (n,), np.float32), want_v)


# ---- msk_adam_clip ---------------------------------------------------------------------------------------------------------------
def _adam_args(n, t, b1, b2):
    return (C.c_size_t(n), F(2e-3), F(0.9), F(0.999), F(1e-8), C.c_double(b1 ** t), C.c_double(b2 ** t), F(1e-4), F(0.5))


def test_adam_clip_matches_the_statement_over_five_steps():
    d = dev()
    n = 10007
    rng = np.random.default_rng(4)
    p = rng.standard_normal(n).astype(np.float32)
    pp, m1p, m2p = vec(p), vec(np.zeros(n)), vec(np.zeros(n))
    ws, rec = _workspace(n), dmalloc(32)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))        # the kernel holds them as float32 (tests/test_gpu_ops.py)
    p64, m1, m2 = p.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n).astype(np.float32)
        gp = vec(g)
        clip_norm = float(np.float32(R.record(g, 0.5, 1.0)[1] / 3))
        coef = R.record(g, 0.5, clip_norm)[2]
        assert coef < 1.0
        _coef(gp, n, 0.5, clip_norm, ws, rec)
        d.call("msk_adam_clip", V(pp), V(gp), V(m1p), V(m2p), *_adam_args(n, t, b1, b2), V(rec), F(-0.25), F(0.25))
        p64, m1, m2 = R.adam_step(p64, g, m1, m2, t, 2e-3, 0.9, 0.999, 1e-8, 1e-4, 0.5, coef, -0.25, 0.25)
        err = rel_err(d.d2h(pp, (n,), np.float32), p64)
        print("adam step %d: param %.3e" % (t, err))
        assert err < 1e-6
        dfree(gp)
    assert rel_err(d.d2h(m1p, (n,), np.float32), m1) < 1e-6 and rel_err(d.d2h(m2p, (n,), np.float32), m2) < 1e-6
    gc = np.abs(R.clipped(g, 0.5, coef))
    assert (gc > 0.25).any() and (gc < 0.25).any()


def test_adam_clip_that_does_not_bite_is_bitwise_adam():
    d = dev()
    n = 10007
    rng = np.random.default_rng(8)
    p = rng.standard_normal(n).astype(np.float32)
    bufs = [[vec(p), vec(np.zeros(n)), vec(np.zeros(n))] for _ in range(3)]
    ws, rec = _workspace(n), dmalloc(32)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    for t in range(1, 4):
        gp = vec(rng.standard_normal(n).astype(np.float32))
        _coef(gp, n, 0.5, 1e9, ws, rec)
        d.call("msk_adam", V(bufs[0][0]), V(gp), V(bufs[0][1]), V(bufs[0][2]), *_adam_args(n, t, b1, b2))
        d.call("msk_adam_clip", V(bufs[1][0]), V(gp), V(bufs[1][1]), V(bufs[1][2]), *_adam_args(n, t, b1, b2), None, F(-INF), F(INF))
        d.call("msk_adam_clip", V(bufs[2][0]), V(gp), V(bufs[2][1]), V(bufs[2][2]), *_adam_args(n, t, b1, b2), V(rec), F(-INF), F(INF))
        dfree(gp)
    want = [d.d2h(b, (n,), np.float32) for b in bufs[0]]
    assert not np.array_equal(want[0], p)
    for other in bufs[1:]:
        for b, w in zip(other, want):
            assert np.array_equal(d.d2h(b, (n,), np.float32), w)


# ---- whole net -------------------------------------------------------------------------------------------------------------------
def _step_errors(p, g, v, got_p, got_v, *step_args):
    """rel_err (tests/helpers.py: max |got - want| / max |want|) of param and velocity against R.sgd_step, evaluated block by
    block -- the statement is elementwise -- so that the float64 temporaries of 45.6 M elements stay in the cache"""
    num, den = [0.0, 0.0], [0.0, 0.0]
    for i in range(0, p.size, 1 << 18):
        sl = slice(i, i + (1 << 18))
        want = R.sgd_step(p[sl], g[sl], v[sl], *step_args)
        for k, got in enumerate((got_p[sl], got_v[sl])):
            num[k] = max(num[k], float(np.abs(got.astype(np.float64) - want[k]).max()))
            den[k] = max(den[k], float(np.abs(want[k]).max()))
    return num[0] / (den[0] + 1e-30), num[1] / (den[1] + 1e-30)


def _build(ncls, K, S, seed):
    from medicalseg_amd.models import VNet
    from oracle import vnet_numpy as O
    model = VNet(elu=False, in_channels=1, num_classes=ncls, kernel_size=K, stride_size=S)
    missing, unexpected = model.set_state_dict(O.init_params(seed, 1, ncls, K, S))
    assert not missing and not unexpected
    return model


def test_optimizer_options_on_the_whole_net():
    """The 16^3 model and the loop of test_gpu_model.test_eager_optimizer_is_bitwise_the_plain_order, four steps:
    (a) plain Momentum, eager off; (b) grad_clip=ClipGradByGlobalNorm(1e9): equal to (a) in every loss, parameter, velocity and
    BatchNorm buffer -- the side-stream join, the whole-arena update and the re-pack of the convolution weights; (c) a clip at
    a third of the first step's norm plus Nesterov: the statement applied to the downloaded arena, step by step.

    The loop is that test's but for the seed of the batches (0, there 5).  At 16^3 the deep levels normalise 2 x 1^3 voxels per
    channel, so part of the gradient is rounding noise amplified by 1 / sqrt(var + eps): the norm has a floor near 1.8 - 2.1 that
    every batch shows and, on some batches, a multiple of it on top.  Measured over four steps with ClipGradByGlobalNorm(1e9):
    seed 5: 6.25 6.22 3.93 22.2; seed 0: 2.21 2.45 2.85 10.2; seed 1: 16.3 2.07 3.53 9.94.  With seed 5 a third of the first norm
    (2.08) sits ON the floor, and run (c) measured 6.25, 2.00: its second step would not be clipped whatever the code does.
    The first batch of seed 0 is at the floor itself, so a third of its norm (0.74) is below anything a later step can show
    (run (c) with seed 0 measured 2.21 2.54 6.96 7.77), and the clip bites in every step with a margin above two."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    d = dev()
    shape, ncls, K, S, N = (16, 16, 16), 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4, 2
    lr0, mu, wd = 1e-2, 0.9, 1e-4
    results, first_norm = [], None
    for run in "abc":
        rng = np.random.default_rng(0)
        nn.Dropout3D._site_counter = 0
        model = _build(ncls, K, S, seed=6)
        sched = optim.lr.PolynomialDecay(lr0, decay_steps=100, end_lr=0, power=0.9)
        kw = {}
        if run == "b":
            kw = dict(grad_clip=optim.ClipGradByGlobalNorm(1e9))
        elif run == "c":
            clip_norm = float(np.float32(first_norm / 3))
            kw = dict(grad_clip=optim.ClipGradByGlobalNorm(clip_norm), use_nesterov=True)
        opt = optim.Momentum(sched, parameters=model.parameters(), momentum=mu, weight_decay=wd, **kw)
        if run != "a":
            assert opt.enable_eager(model) is False and opt.grad_norm() is None
        losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
        model.train()
        model.set_dropout_masks(None)
        nn.Dropout3D.step, nn.Dropout3D.seed = 0, 3
        a = model.arena
        vals = []
        for step in range(4):
            x = rng.standard_normal((N, 1) + shape).astype(np.float32)
            y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
            logits = model(x)
            loss_list, per = loss_computation(logits, to_tensor(y), losses)
            loss = sum(loss_list)
            loss.backward()
            if run == "c":
                p, g, v = (d.d2h(ptr, (a.count,), np.float32) for ptr in (a.value_ptr, a.grad_ptr, opt.velocity_ptr))
                lr = opt.get_lr()
            opt.step()
            if run == "b" and step == 0:
                first_norm = opt.grad_norm()
                assert first_norm > 0
            if run == "c":
                want = R.record(g, a.grad_scale, clip_norm)
                assert want[2] < 1.0, (step, want.tolist())
                assert _ulp_apart(opt.grad_norm(), want[1], np.float64), (step, opt.grad_norm(), want.tolist())
                ep, ev = _step_errors(p, g, v, d.d2h(a.value_ptr, (a.count,), np.float32),
                                      d.d2h(opt.velocity_ptr, (a.count,), np.float32), lr, mu, wd, a.grad_scale, True, want[2])
                print("step %d: norm %.6g coef %.6g, velocity %.3e, param %.3e" % (step, want[1], want[2], ev, ep))
                assert ev < 1e-6 and ep < 1e-6
                del p, g, v
            sched.step()
            model.clear_gradients()
            vals.append(float(loss))
        if run != "c":
            results.append((vals, model.state_dict(), d.d2h(opt.velocity_ptr, (a.count,), np.float32)))
    (va, sda, vela), (vb, sdb, velb) = results
    assert va == vb, (va, vb)
    assert any("_mean" in k for k in sda)                              # the BatchNorm buffers are in there
    for k in sda:
        assert np.array_equal(sda[k], sdb[k]), k
    assert np.array_equal(vela, velb) and np.abs(vela).max() > 0

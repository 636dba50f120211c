"""Every tensor-taking op of the C ABI on CHANNEL-SLICE VIEWS (the model's zero-copy concat: ld > c, pointer offset 4 * c0),
against the float64 oracle, with the tolerances stated at the top of tests/test_gpu_ops.py (convolutions: _conv_tol(K);
elementwise / BN: 1e-5 of max|ref|; loss: the bounds of test_loss_fwd_bwd / test_dice_options / tests/test_gpu_bce.py).

Two view flavours per op:
  aligned    ld = c + 16 (c rounded up to a multiple of 4 first), channel offset 16 -- the product's concat pattern; every
             float4 predicate (ld % 4, pointer & 15) still holds, so the vector kernels are still chosen: the convolution
             cases assert the kernel names of the dense run of the same shape (DECLINES lists the kernels that legitimately
             want dense tensors, with the predicate).
  unaligned  ld = c + 3, channel offset 1 -- msk_tensor permits any 4-byte-aligned pointer and any ld >= c.  The op gives
             the oracle's answer through its scalar path, or returns an error (MskError); UNALIGNED states which per op.
  ld_odd     ld = c + 18, channel offset 16, for the cases whose channel counts are multiples of 4: the pointer IS 16-byte
             aligned and only ld % 4 fails, so a float4 predicate that looks at the pointer alone is caught (unaligned breaks
             both at once).  Same expectation per op as unaligned.

The operands sit inside wider buffers whose other channels hold helpers.SENTINEL (a quiet NaN): a float4 load that pulls in the
neighbouring channels, or a view read as dense, poisons the result; a store outside the view is seen bit for bit
(_Place.check) and in the red zones (helpers.redzone_check after every test)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bce_reference as R
import helpers
from helpers import (GUARD, SENTINEL, SENTINEL_BITS, assert_redzones_intact, dev, dmalloc, redzone_check, rel_err,  # noqa: F401
                     t_empty, t_from_ncdhw, vec, vec_back, vp)

pytestmark = pytest.mark.gpu

from oracle import vnet_numpy as O  # noqa: E402

FLAVOURS = {"aligned": (16, 16), "unaligned": (1, 3), "ld_odd": (16, 18)}     # (channel offset, ld - c; aligned: ld - roundup(c, 4))


def _flavours(*channels):
    return ["aligned", "unaligned"] + (["ld_odd"] if all(c % 4 == 0 for c in channels) else [])


def _cross(cases, channels):
    """(case, flavour) pairs: every case in both flavours, and in ld_odd where channels(case) are all multiples of 4."""
    return [(case, f) for case in cases for f in _flavours(*channels(case))]
ANSWER, ERROR, DECLINE = "answer", "error", "declines (returns 1, nothing launched); the calls it stands for give the answer"

# What each op does with an UNALIGNED (offset 1 channel, ld = c + 3) or LD_ODD (offset 16, ld = c + 18) view: the oracle's answer (scalar kernels), MskError, or --
# for an entry point whose contract has a "not eligible" return -- that return with every output untouched.
UNALIGNED = {
    "msk_conv3d_fwd": ANSWER, "msk_conv3d_dgrad": ANSWER, "msk_conv3d_wgrad": ANSWER,
    "msk_convT3d_fwd": ANSWER, "msk_convT3d_dgrad": ANSWER, "msk_convT3d_wgrad": ANSWER,
    "msk_conv3d_fwd_act": ANSWER, "msk_conv3d_bwd_bnact": ANSWER,
    "msk_convT3d_bwd_bnact": DECLINE,   # msk_gconv_ks_fwd_bnbwd: yld % 4 || dld % 4 || (y | dout) & 15 -> 0 -> "1 = not eligible" (msegk.h)
    "msk_bn_stats": ANSWER, "msk_affine_act_fwd": ANSWER, "msk_affine_act_bwd_reduce": ANSWER, "msk_affine_act_bwd_apply": ANSWER,
    "msk_affine_act_join_fwd": ANSWER,
    "msk_add_act_join_bwd": ERROR,      # MSK_REQUIRE: "join backward needs float4-aligned tensors with C % 4 == 0" (also any C % 4 != 0)
    "msk_elu_fwd": ANSWER, "msk_elu_bwd": ANSWER, "msk_copy_scale": ANSWER, "msk_channel_sum": ANSWER, "msk_argmax_c": ANSWER,
    "msk_softmax_c": ANSWER,
    "msk_loss_fwd": ANSWER, "msk_loss_bwd": ANSWER, "msk_loss_fwd_ex": ANSWER, "msk_loss_bwd_ex": ANSWER,
    "msk_bce_fwd": ANSWER, "msk_bce_bwd": ANSWER,
    "msk_interp_trilinear_fwd": ANSWER, "msk_interp_trilinear_bwd": ANSWER,
}


def _conv_tol(K):                                          # tests/test_gpu_ops.py
    return 8e-6 * np.sqrt(K / 1000.0 + 1.0)


def _desc(k, s, p):
    from medicalseg_amd._lib import MskConvDesc
    return MskConvDesc(*k, *s, *p)


def _msk_error():
    from medicalseg_amd._lib import MskError
    return MskError


class _Place:
    """Puts operands where a flavour says: dense tensors (flavour None), or channel slices of wider SENTINEL-filled buffers."""

    def __init__(self, flavour):
        self.flavour = flavour
        self.wides = []

    def inp(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if self.flavour is None:
            return t_from_ncdhw(a)
        off, extra = FLAVOURS[self.flavour]
        n, c = a.shape[:2]
        ld = ((c + 3) // 4 * 4 if self.flavour == "aligned" else c) + extra
        host = np.full((n, ld) + a.shape[2:], SENTINEL, dtype=np.float32)
        host[:, off:off + c] = a
        wide = t_from_ncdhw(host)
        self.wides.append((wide, off, c))
        return wide.channel_slice(off, off + c)

    def out(self, shape, init=None):
        """An output: every element SENTINEL (an unwritten one reads back as NaN), or `init` for an accumulate target."""
        return self.inp(np.full(shape, SENTINEL, np.float32) if init is None else init)

    def check(self):
        """The channels of the wider buffers that are not part of a view still hold SENTINEL, bit for bit."""
        for wide, off, c in self.wides:
            raw = dev().d2h(wide.ptr, (wide.n * wide.d * wide.h * wide.w, wide.ld), np.uint32)
            keep = np.ones(wide.ld, bool)
            keep[off:off + c] = False
            bad = np.argwhere(raw[:, keep] != SENTINEL_BITS)
            assert bad.size == 0, "%d neighbour channel words overwritten, first at voxel %d" % (len(bad), bad[0][0])


def _profiled(d, fn):
    d.set_option("prof_only_halo", 0)
    d.set_option("prof_shapes", 0)
    d.prof_reset()
    d.prof_enable(True)
    try:
        out = fn()
        d.sync()
    finally:
        d.prof_enable(False)
    return out, set(d.prof_report())


# ---------------------------------------------------------------------------------------------------------------------------
# red-zone plumbing on the device
# ---------------------------------------------------------------------------------------------------------------------------
def test_guarded_payloads_keep_the_allocator_alignment():
    """GUARD is a multiple of 256, so no float4 / 16-byte dispatch predicate changes under the guarded helpers."""
    t = t_empty(1, 3, 2, 3, 5, ld=5)
    for ptr in (dmalloc(12), vec(np.zeros(7)), t.ptr, t_from_ncdhw(np.zeros((1, 2, 3, 3, 3), np.float32)).ptr):
        assert ptr % 256 == 0
    assert np.isnan(t.numpy()).all()                          # an unfilled tensor holds SENTINEL


def test_a_corrupted_tail_guard_is_reported():
    """One float written (host copy, no kernel) right after a 40-byte payload, inside the test's own allocation."""
    d = dev()
    p = vec(np.zeros(10))
    d.h2d(p + 40, np.array([1.0], np.float32))
    with pytest.raises(AssertionError, match=r"tail red zone corrupted: 1 word\(s\), first at payload\+40,"):
        assert_redzones_intact()
    assert helpers._registry == []


# ---------------------------------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------------------------------
K5, K3, K2, K1 = (5, 5, 5), (3, 3, 3), (2, 2, 2), (1, 1, 1)
S1, P0, P1, P2 = (1, 1, 1), (0, 0, 0), (1, 1, 1), (2, 2, 2)
CONV_VIEW_CASES = {
    # name: (transposed, Cin, Cout, k, s, p, (N, D, H, W), conv_impl)
    "halo_mfma_32_32": (0, 32, 32, K5, S1, P2, (1, 4, 6, 33), 0),
    "wino5_64_40": (0, 64, 40, K5, S1, P2, (1, 4, 8, 32), 10),           # WINO_CASES; Cout not a multiple of 32
    "wino3_16_24": (0, 16, 24, K3, S1, P1, (1, 6, 8, 16), 10),           # WINO3_CASES; ragged planes
    "foldn_32_3": (0, 32, 3, K5, S1, P2, (1, 6, 8, 33), 0),              # out_tr.conv1; its data gradient is the tight-K class 3 -> 32
    "c1_1_16": (0, 1, 16, K5, S1, P2, (1, 5, 9, 17), 0),                 # in_tr.conv1
    "ks_down_16_32": (0, 16, 32, K2, K2, P0, (2, 6, 8, 10), 0),
    "ks_up_64_16": (1, 64, 16, K2, K2, P0, (1, 3, 5, 7), 0),
    "aniso_down_16_32": (0, 16, 32, (2, 2, 4), (2, 2, 1), P0, (1, 8, 8, 12), 0),
    "aniso_up_64_16": (1, 64, 16, (2, 2, 4), (2, 2, 1), P0, (1, 4, 4, 9), 0),
    "pw_thin_32_3": (0, 32, 3, K1, S1, P0, (2, 5, 11, 7), 0),
    "pw_mid_20_20": (0, 20, 20, K1, S1, P0, (2, 4, 5, 6), 0),
    "odd_5_7": (0, 5, 7, (3, 2, 1), (2, 1, 1), (1, 0, 0), (1, 7, 6, 5), 0),   # reference kernels
}

# Kernels that legitimately decline an ALIGNED view and change the profile tags, by case and op: (tags of the dense run that
# go, tags that come, predicate).  None does: the dispatch predicates ask for ld % 4 == 0 and a 16-byte pointer, not for ld == c.
DECLINES = {}

# Kernels that decline every view (they want ld == c) but run under the SAME tag as the kernel that takes it, so the tag
# comparison cannot see them: (entry point, tag, dense-only kernel, its predicate, kernel a view gets instead).
DENSE_ONLY_SAME_TAG = [
    ("msk_conv3d_fwd / _dgrad 1x1x1", "pointwise_mid", "pointwise_mid_staged_k",
     "g.sld == g.CK && g.dld == g.CN && (tile_staging & 1)", "pointwise_mid_k"),
    ("msk_loss_fwd(_ex)", "loss_fwd_stats", "loss_stats_tpv_k<CM, ST = 1>",
     "(tile_staging & 2) && logits.ld == C && C % 4 == 0 && logits.p & 15 == 0", "loss_stats_tpv_k<CM, 0>"),
    ("msk_loss_fwd(_ex)", "loss_fwd_stats", "loss_stats_tpv_k<4, 2>",
     "(tile_staging & 4) && 2 <= C <= 4 && logits.ld == C && logits.p & 15 == 0", "loss_stats_tpv_k<CM, 0>"),
    ("msk_loss_bwd(_ex)", "loss_bwd", "loss_bwd_tpv_k<CM, ST = 1 | 2>",
     "the same with dlogits.ld == C and (logits.p | dlogits.p) & 15 == 0", "loss_bwd_tpv_k<CM, 0>"),
    ("msk_bce_fwd / _bwd", "bce_fwd / bce_bwd", "the float4-quad branch inside bce_fwd_k / bce_bwd_k",
     "ld == C (&& lddz == C) && pointers & 15 == 0", "the per-element branch of the same kernel"),
    ("msk_bn_stats, msk_affine_act_fwd / _bwd_reduce / _bwd_apply, msk_channel_sum", "bn_stats_partial, affine_act_*, channel_sum_partial",
     "*_d12_k (C in 1, 2, 3, 6; voxels * C % 12 == 0)", "d12_ok: t.ld == t.c && t.p % 16 == 0", "the scalar kernels"),
]

# The kernel class a case is here for: a tag prefix that must be among the kernels of the aligned AND the dense run (they are
# equal), so that a dispatch change that moves a case elsewhere, or a profile that records nothing, does not pass silently.
EXPECT = {
    ("wino5_64_40", "fwd"): "conv_halo_wino4_k", ("wino5_64_40", "dgrad"): "conv_halo_wino4_k",
    ("wino3_16_24", "fwd"): "conv_halo_wino43_k", ("wino3_16_24", "dgrad"): "conv_halo_wino43_k",
    ("foldn_32_3", "fwd"): "conv_foldn_h2", ("foldn_32_3", "dgrad"): "conv_tk_h2", ("foldn_32_3", "wgrad"): "wgrad_cbs_h2",
    ("c1_1_16", "fwd"): "conv_c1_mfma",
    ("pw_thin_32_3", "fwd"): "pointwise_thin", ("pw_thin_32_3", "dgrad"): "pointwise_thin",
    ("pw_mid_20_20", "fwd"): "pointwise_mid", ("pw_mid_20_20", "dgrad"): "pointwise_mid",
}


@functools.lru_cache(maxsize=None)
def _conv_problem(name):
    """Inputs and float64 references of one case, computed once and shared by its flavours (never modified)."""
    tr, cin, cout, k, s, p, (N, D, H, W), _ = CONV_VIEW_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    f8 = lambda a: a.astype(np.float64)
    x = rng.standard_normal((N, cin, D, H, W)).astype(np.float32)
    wshape = ((cin, cout) if tr else (cout, cin)) + k
    w = (rng.standard_normal(wshape) / np.sqrt(cin * np.prod(k))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    if tr:
        y = O.conv_transpose3d(f8(x), f8(w), f8(b), s)
    else:
        y = O.conv3d(f8(x), f8(w), f8(b), s, p)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    dx0 = rng.standard_normal(x.shape).astype(np.float32)      # what an accumulating data gradient finds in its target
    if tr:
        dx = O.conv_transpose3d_dgrad(f8(dy), f8(w), s)
        dw, db = O.conv_transpose3d_wgrad(f8(dy), f8(x), k, s)
    else:
        dx = O.conv3d_dgrad(f8(dy), f8(w), x.shape, s, p)
        dw, db = O.conv3d_wgrad(f8(dy), f8(x), k, s, p)
    for a in (x, w, b, y, dy, dx0, dx, dw, db):
        a.setflags(write=False)
    return dict(x=x, w=w, b=b, y=y, dy=dy, dx0=dx0, dx=dx, dw=dw, db=db)


def _conv_run(name, flavour):
    """Forward, data gradient (fresh, then into a target that holds dx0), weight + bias gradient; returns results and kernel tags
    per op."""
    tr, cin, cout, k, s, p, _, impl = CONV_VIEW_CASES[name]
    q = _conv_problem(name)
    d = dev()
    pl = _Place(flavour)
    fn = ("msk_convT3d_%s" if tr else "msk_conv3d_%s")
    cd = _desc(k, s, p)
    xt, dyt = pl.inp(q["x"]), pl.inp(q["dy"])
    yt, dxt, dxa = pl.out(q["y"].shape), pl.out(q["x"].shape), pl.out(q["x"].shape, q["dx0"])
    wp, bp = vec(q["w"].ravel()), vec(q["b"])                  # fresh pointers: the packed-weight caches miss in every run
    dwp, dbp = vec(np.full(q["w"].size, 0.5, np.float32)), vec(np.full(cout, 0.25, np.float32))
    res, tags = {}, {}
    d.set_option("conv_impl", impl)
    try:
        _, tags["fwd"] = _profiled(d, lambda: d.call(fn % "fwd", cd, xt.msk(), vp(wp), vp(bp), yt.msk()))
        _, tags["dgrad"] = _profiled(d, lambda: d.call(fn % "dgrad", cd, dyt.msk(), vp(wp), dxt.msk(), 0))
        _, tags["dgrad_acc"] = _profiled(d, lambda: d.call(fn % "dgrad", cd, dyt.msk(), vp(wp), dxa.msk(), 1))
        _, tags["wgrad"] = _profiled(d, lambda: d.call(fn % "wgrad", cd, xt.msk(), dyt.msk(), vp(dwp), vp(dbp), 0))
    finally:
        d.set_option("conv_impl", 0)
    res = dict(y=yt.numpy(), dx=dxt.numpy(), dxa=dxa.numpy(), dw=vec_back(dwp, q["w"].size).reshape(q["w"].shape),
               db=vec_back(dbp, cout))
    pl.check()
    return res, tags


def _conv_check(name, res):
    tr, cin, cout, k, s, p, _, _ = CONV_VIEW_CASES[name]
    q = _conv_problem(name)
    taps = int(np.prod(k))
    M = q["y"].size // cout if not tr else q["x"].size // cin      # voxels the weight gradient sums over (dy's for conv, x's for convT)
    Mb = q["y"].size // cout                                      # ... and the bias gradient (always dy's)
    e = {"y": rel_err(res["y"], q["y"]), "dx": rel_err(res["dx"], q["dx"]),
         "dxa": rel_err(res["dxa"], q["dx"] + q["dx0"]), "dw": rel_err(res["dw"], q["dw"]), "db": rel_err(res["db"], q["db"])}
    print(name, {k_: "%.2e" % v for k_, v in e.items()})
    # reduction lengths: a transposed convolution's output voxel sums Cin * prod(ceil(k / s)) terms
    kf = cin * int(np.prod([-(-a // b) for a, b in zip(k, s)])) if tr else cin * taps
    assert e["y"] < _conv_tol(kf), e
    assert e["dx"] < _conv_tol(cout * taps) and e["dxa"] < _conv_tol(cout * taps), e
    assert e["dw"] < _conv_tol(M) * 2, e
    assert e["db"] < 1e-5 * np.sqrt(Mb / 1000 + 1), e


@pytest.mark.parametrize("name,flavour", _cross(list(CONV_VIEW_CASES), lambda n: CONV_VIEW_CASES[n][1:3]))
def test_conv_on_views(name, flavour):
    """msk_conv3d_{fwd,dgrad,wgrad} / msk_convT3d_{fwd,dgrad,wgrad}: x, y, dy and dx (fresh and accumulating) are views; dw and db sit
    in guarded vectors.  Aligned views run the kernels of the dense run; unaligned views give the oracle's answer (UNALIGNED)."""
    tr = CONV_VIEW_CASES[name][0]
    for op in ("fwd", "dgrad", "wgrad"):
        assert UNALIGNED[("msk_convT3d_%s" if tr else "msk_conv3d_%s") % op] == ANSWER
    res, tags = _conv_run(name, flavour)
    _conv_check(name, res)
    if flavour == "aligned":
        dres, dtags = _conv_run(name, None)
        _conv_check(name, dres)
        for op in tags:
            gone, come, _why = DECLINES.get((name, op), (set(), set(), ""))
            assert tags[op], op                                    # the profile recorded the launches
            assert tags[op] == (dtags[op] - gone) | come, (op, sorted(tags[op]), sorted(dtags[op]))
            want = EXPECT.get((name, "dgrad" if op == "dgrad_acc" else op))
            assert want is None or any(t.startswith(want) for t in tags[op]), (op, want, sorted(tags[op]))
        print(name, {op: sorted(t) for op, t in tags.items()})


# ---------------------------------------------------------------------------------------------------------------------------
# fused forms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,flavour", _cross([(32, 3, 5, (1, 9, 11, 21)),      # slope in conv_foldn's epilogue
                                                 (64, 48, 5, (1, 4, 8, 24)),      # ... in the Winograd epilogue
                                                 (16, 8, 3, (1, 6, 7, 9))],       # ... by the in-place pass behind the other kernels
                                                lambda c: c[:2]))
def test_conv_fwd_act_on_views(case, flavour):
    """msk_conv3d_fwd_act = PReLU(conv(x) + b) (test_conv_fold_bn_and_fused_prelu_epilogue's reference with the BatchNorm already
    folded into w, b), source and destination views."""
    cin, cout, K, (N, D, H, W) = case
    k, p = (K,) * 3, (K // 2,) * 3
    assert UNALIGNED["msk_conv3d_fwd_act"] == ANSWER
    d = dev()
    rng = np.random.default_rng(cin + cout)
    f8 = lambda a: a.astype(np.float64)
    x = rng.standard_normal((N, cin, D, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin) + k) / np.sqrt(cin * K ** 3)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    slope = rng.uniform(0.05, 0.5, cout).astype(np.float32)
    z = O.conv3d(f8(x), f8(w), f8(b), S1, p)
    ref = np.where(z > 0, z, z * f8(slope).reshape(1, cout, 1, 1, 1))
    pl = _Place(flavour)
    xt, yt = pl.inp(x), pl.out(z.shape)
    d.call("msk_conv3d_fwd_act", _desc(k, S1, p), xt.msk(), vp(vec(w.ravel())), vp(vec(b)), vp(vec(slope)), yt.msk())
    assert rel_err(yt.numpy(), ref) < _conv_tol(cin * K ** 3)
    pl.check()


@functools.lru_cache(maxsize=None)
def _bwd_bnact_problem(c, K, shape):
    N, D, H, W = shape
    k, p = (K,) * 3, (K // 2,) * 3
    rng = np.random.default_rng(10 * c + K)
    f8 = lambda a: a.astype(np.float64)
    x = rng.standard_normal((N, c, D, H, W)).astype(np.float32)
    w = (rng.standard_normal((c, c) + k) / np.sqrt(c * K ** 3)).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    dout = rng.standard_normal((N, c, D, H, W)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), (0.3 * rng.standard_normal(c)).astype(np.float32)
    alpha = rng.uniform(0.05, 0.5, c).astype(np.float32)
    y = O.conv3d(f8(x), f8(w), f8(b), S1, p).astype(np.float32)
    yc = np.moveaxis(f8(y), 1, -1).reshape(-1, c)
    M = yc.shape[0]
    mean, var = yc.mean(0), yc.var(0)
    invstd = 1.0 / np.sqrt(var + 1e-5)
    scale, shift = f8(gamma) * invstd, f8(beta) - mean * f8(gamma) * invstd
    u = yc * scale + shift
    du = np.moveaxis(f8(dout), 1, -1).reshape(-1, c) * np.where(u > 0, 1.0, f8(alpha))
    xhat = (yc - mean) * invstd
    sums = np.concatenate([du.sum(0), (du * xhat).sum(0)])
    dy = np.moveaxis((scale * (du - sums[:c] / M - xhat * sums[c:] / M)).reshape(N, D, H, W, c), -1, 1)
    dx = O.conv3d_dgrad(dy, f8(w), x.shape, S1, p)
    dw, _ = O.conv3d_wgrad(dy, f8(x), k, S1, p)
    coef = dict(scale=scale, shift=shift, alpha=alpha, mean=mean, invstd=invstd, gamma=gamma, sums=sums)
    return dict(x=x, w=w, b=b, y=y, dout=dout, coef=coef, M=M, dy=dy, dx=dx, dw=dw)


def _bwd_bnact_run(c, K, shape, flavour):
    """The forward pass that leaves the layer's transforms (msk_conv3d_fwd_ex), the reduce pass that leaves the maxima, then
    msk_conv3d_bwd_bnact -- as nn.ConvBNAct does; the caller-owned buffers are sized by the library for THESE tensors."""
    q = _bwd_bnact_problem(c, K, shape)
    k, p = (K,) * 3, (K // 2,) * 3
    d = dev()
    cd = _desc(k, S1, p)
    pl = _Place(flavour)
    xt, yt, dot = pl.inp(q["x"]), pl.inp(q["y"]), pl.inp(q["dout"])
    ytmp, dyt, dxt = pl.out(q["y"].shape), pl.out(q["y"].shape), pl.out(q["x"].shape)
    cv = {n_: vec(v.astype(np.float32)) for n_, v in q["coef"].items()}
    wp, bp = vec(q["w"].ravel()), vec(q["b"])
    nx = int(d.lib.msk_conv3d_xform_bytes(d.ctx, cd, xt.msk(), c))
    nb = int(d.lib.msk_conv3d_bwd_bnact_bytes(d.ctx, cd, xt.msk(), yt.msk()))
    xf, ybuf = dmalloc(nx) if nx else None, dmalloc(nb) if nb else None
    d.call("msk_conv3d_fwd_ex", cd, xt.msk(), vp(wp), vp(bp), ytmp.msk(), None, vp(xf))
    assert rel_err(ytmp.numpy(), q["y"]) < _conv_tol(c * K ** 3)
    maxes = None
    if flavour in (None, "aligned"):    # the maxima come from the float4 reduce kernel only (MSK_REQUIRE in msk_affine_act_bwd_reduce_pg)
        from medicalseg_amd._lib import NULL_TENSOR
        maxes, sums_dev = vec(np.zeros(128, np.float32)), vec(np.zeros(3 * c, np.float32))
        d.call("msk_affine_act_bwd_reduce_ex", yt.msk(), vp(cv["scale"]), vp(cv["shift"]), NULL_TENSOR, vp(cv["alpha"]),
               vp(cv["mean"]), vp(cv["invstd"]), dot.msk(), vp(sums_dev), vp(maxes))
    dw = vec(np.full(q["w"].size, 0.5, np.float32))
    _, tags = _profiled(d, lambda: d.call(
        "msk_conv3d_bwd_bnact", cd, xt.msk(), vp(wp), yt.msk(), vp(cv["scale"]), vp(cv["shift"]), vp(cv["alpha"]), vp(cv["mean"]),
        vp(cv["invstd"]), vp(cv["gamma"]), dot.msk(), vp(cv["sums"]), C.c_double(float(q["M"])), dyt.msk(), dxt.msk(), 0, vp(dw), 0,
        vp(xf), vp(ybuf), vp(maxes)))
    fused = any(t.startswith("wbf_tin_dual") or t.endswith("_bn_k") for t in tags)
    dy = dyt.numpy()
    if fused:
        assert np.isnan(dy).all()                                   # dy is never stored in the fused forms
    else:
        assert rel_err(dy, q["dy"]) < 1e-5
    assert rel_err(dxt.numpy(), q["dx"]) < _conv_tol(c * K ** 3)
    assert rel_err(vec_back(dw, q["w"].size).reshape(q["w"].shape), q["dw"]) < 2 * _conv_tol(q["M"])
    pl.check()
    return tags, fused


@pytest.mark.parametrize("case,flavour", _cross([(16, 5, (1, 6, 7, 9)),          # not eligible for the fused form: the three calls inside
                                                 (32, 3, (2, 16, 16, 16))],      # eligible: dy evaluated inside the transform kernels
                                                lambda c: c[:1]))
def test_conv_bwd_bnact_on_views(case, flavour):
    """msk_conv3d_bwd_bnact (backward of conv -> BatchNorm -> PReLU) with x, y, dout and the written dy, dx as views, against the float64
    oracle of the three operations (test_conv3d_bwd_bnact_fused_equals_three_call_form's reference).  An aligned view takes the form
    the dense tensors take (fused at 32 channels); an unaligned one the three-call form inside the same entry point."""
    assert UNALIGNED["msk_conv3d_bwd_bnact"] == ANSWER
    c, K, shape = case
    tags, fused = _bwd_bnact_run(c, K, shape, flavour)
    if flavour == "aligned":
        dtags, dfused = _bwd_bnact_run(c, K, shape, None)
        assert dfused == (c >= 32)
        assert tags == dtags, (sorted(tags), sorted(dtags))
    else:
        assert not fused


@pytest.mark.parametrize("case,flavour", _cross([(32, 8, (1, 5, 6, 7)), (32, 8, (2, 2, 3, 64))],      # the second: the LDS-staged form (W % 32 == 0)
                                                lambda c: c[:2]))
def test_convT_bwd_bnact_on_views(case, flavour):
    """msk_convT3d_bwd_bnact (backward of convT -> BatchNorm -> PReLU, dx accumulated) with x, y, dout, dy and dx as views, against
    the float64 oracle of the whole chain (test_convT_bwd_bnact_equals_the_three_call_form's)."""
    assert UNALIGNED["msk_convT3d_bwd_bnact"] == DECLINE
    cin, cout, src = case
    d = dev()
    N, D, H, W = src
    rng = np.random.default_rng(cin + cout)
    k = s_ = K2
    f8 = lambda a: a.astype(np.float64)
    x = rng.standard_normal((N, cin, D, H, W)).astype(np.float32)
    y = (rng.standard_normal((N, cout, 2 * D, 2 * H, 2 * W)) * 2 + 0.5).astype(np.float32)
    dout = rng.standard_normal(y.shape).astype(np.float32)
    w = (rng.standard_normal((cin, cout) + k) / np.sqrt(cin)).astype(np.float32)
    scale, shift = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    alpha = rng.uniform(0.05, 0.4, cout).astype(np.float32)
    mean, invstd = rng.standard_normal(cout).astype(np.float32), rng.uniform(0.5, 2.0, cout).astype(np.float32)
    M = N * 8 * D * H * W
    sums = (rng.standard_normal(2 * cout) * np.sqrt(M)).astype(np.float32)
    dx0 = rng.standard_normal(x.shape).astype(np.float32)
    sh = (1, cout, 1, 1, 1)
    u = f8(y) * f8(scale).reshape(sh) + f8(shift).reshape(sh)
    du = f8(dout) * np.where(u > 0, 1.0, f8(alpha).reshape(sh))
    xh = (f8(y) - f8(mean).reshape(sh)) * f8(invstd).reshape(sh)
    dy_ref = f8(scale).reshape(sh) * (du - f8(sums[:cout]).reshape(sh) / M - xh * f8(sums[cout:]).reshape(sh) / M)
    dx_ref = O.conv3d(dy_ref, f8(w), None, s_, 0) + f8(dx0)       # convT^T = a k == s convolution with w[ci][co]
    dw_ref, _ = O.conv_transpose3d_wgrad(dy_ref, f8(x), k, s_)
    pl = _Place(flavour)
    xt, yt, dt = pl.inp(x), pl.inp(y), pl.inp(dout)
    dyt, dxt = pl.out(y.shape), pl.out(x.shape, dx0)
    dw = vec(np.zeros(w.size, np.float32))
    wp, psc, psf, pal, pmu, pis, psm = (vec(v) for v in (w.ravel(), scale, shift, alpha, mean, invstd, sums))
    rc = d.lib.msk_convT3d_bwd_bnact(d.ctx, _desc(k, s_, P0), xt.msk(), vp(wp), yt.msk(), vp(psc), vp(psf), vp(pal), vp(pmu), vp(pis),
                                     dt.msk(), vp(psm), C.c_double(M), dyt.msk(), dxt.msk(), 1, vp(dw), 0)
    d.sync()
    if flavour != "aligned":
        from medicalseg_amd._lib import NULL_TENSOR
        assert rc == 1, rc
        assert np.isnan(dyt.numpy()).all() and np.array_equal(dxt.numpy(), dx0) and not vec_back(dw, w.size).any()   # nothing launched
        d.call("msk_affine_act_bwd_apply", yt.msk(), vp(psc), vp(psf), NULL_TENSOR, vp(pal), vp(pmu), vp(pis), None, dt.msk(),
               vp(psm), C.c_double(M), 1, dyt.msk(), NULL_TENSOR, 0)
        d.call("msk_convT3d_wgrad", _desc(k, s_, P0), xt.msk(), dyt.msk(), vp(dw), None, 0)
        d.call("msk_convT3d_dgrad", _desc(k, s_, P0), dyt.msk(), vp(wp), dxt.msk(), 1)
        d.sync()
    else:
        assert rc == 0, rc
    assert rel_err(dyt.numpy(), dy_ref) < 1e-5
    assert rel_err(dxt.numpy(), dx_ref) < _conv_tol(cout * 8)
    assert rel_err(vec_back(dw, w.size).reshape(w.shape), dw_ref) < 2 * _conv_tol(M // 8)
    pl.check()


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm, activations, elementwise
# ---------------------------------------------------------------------------------------------------------------------------
# C = 3 at 2 * 5 * 6 * 7 voxels: voxels * C % 12 == 0, the shape class of the dense12 kernels (which want ld == c: d12_ok, so a view
# must not reach them); 1 * 7 * 7 * 9: a size they decline anyway; C = 16: the float4 kernels.
EW_SHAPES = [(3, (2, 5, 6, 7)), (3, (1, 7, 7, 9)), (16, (2, 5, 6, 7))]


@pytest.mark.parametrize("case,flavour", _cross(EW_SHAPES, lambda c: c[:1]))
def test_bn_stats_and_affine_act_on_views(case, flavour):
    for op in ("msk_bn_stats", "msk_affine_act_fwd", "msk_affine_act_bwd_reduce", "msk_affine_act_bwd_apply"):
        assert UNALIGNED[op] == ANSWER
    d = dev()
    C_, shape = case
    N, D, H, W = shape
    M = N * D * H * W
    rng = np.random.default_rng(C_ + D)
    f8 = lambda a: a.astype(np.float64)
    x = (rng.standard_normal((N, C_, D, H, W)) * 1.5 + 0.5).astype(np.float32)
    res = rng.standard_normal(x.shape).astype(np.float32)
    dout = rng.standard_normal(x.shape).astype(np.float32)
    dres0 = rng.standard_normal(x.shape).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C_).astype(np.float32), rng.standard_normal(C_).astype(np.float32)
    alpha = rng.uniform(0.1, 0.4, C_).astype(np.float32)
    y_ref, xhat, mean, var, invstd = O.bn_train(f8(x), f8(gamma), f8(beta))
    out_ref = O.prelu(y_ref + f8(res), f8(alpha))
    du, dalpha = O.prelu_bwd(f8(dout), y_ref + f8(res), f8(alpha))
    dx_ref, dg_ref, db_ref = O.bn_train_bwd(du, xhat, f8(gamma), invstd)

    pl = _Place(flavour)
    xt, rt, dt = pl.inp(x), pl.inp(res), pl.inp(dout)
    ot, dxt, drt = pl.out(x.shape), pl.out(x.shape), pl.out(x.shape, dres0)
    stats = vec(np.zeros(2 * C_))
    d.call("msk_bn_stats", xt.msk(), vp(stats))
    st = vec_back(stats, 2 * C_)
    assert rel_err(st[:C_], mean) < 1e-5 and rel_err(st[C_:] / M, var) < 1e-5
    g, b_, rmp, rvp = vec(gamma), vec(beta), vec(np.zeros(C_)), vec(np.ones(C_))
    sm, si, sc, sh = vec(np.zeros(C_)), vec(np.zeros(C_)), vec(np.zeros(C_)), vec(np.zeros(C_))
    d.call("msk_bn_finalize", vp(stats), 1, C.c_double(M), C_, vp(g), vp(b_), C.c_float(1e-5), C.c_float(0.9),
           vp(rmp), vp(rvp), vp(sm), vp(si), vp(sc), vp(sh))
    al = vec(alpha)
    d.call("msk_affine_act_fwd", xt.msk(), vp(sc), vp(sh), rt.msk(), vp(al), ot.msk())
    assert rel_err(ot.numpy(), out_ref) < 1e-5
    sums = vec(np.zeros(3 * C_))
    d.call("msk_affine_act_bwd_reduce", xt.msk(), vp(sc), vp(sh), rt.msk(), vp(al), vp(sm), vp(si), dt.msk(), vp(sums))
    s_ = vec_back(sums, 3 * C_)
    assert rel_err(s_[:C_], db_ref) < 1e-5
    assert rel_err(s_[C_:2 * C_], dg_ref) < 1e-5
    assert rel_err(s_[2 * C_:], dalpha) < 1e-5
    d.call("msk_affine_act_bwd_apply", xt.msk(), vp(sc), vp(sh), rt.msk(), vp(al), vp(sm), vp(si), vp(g), dt.msk(),
           vp(sums), C.c_double(M), 1, dxt.msk(), drt.msk(), 1)
    assert rel_err(dxt.numpy(), dx_ref) < 1e-5
    assert rel_err(drt.numpy(), du + dres0) < 1e-5
    pl.check()


@pytest.mark.parametrize("case,flavour", _cross(EW_SHAPES, lambda c: c[:1]))
def test_join_fwd_bwd_on_views(case, flavour):
    """msk_affine_act_join_fwd (any view: the scalar kernel behind the float4 ones) and msk_add_act_join_bwd, which states its
    requirement -- C % 4 == 0 and float4-aligned tensors -- and returns an error otherwise, writing nothing."""
    assert UNALIGNED["msk_affine_act_join_fwd"] == ANSWER and UNALIGNED["msk_add_act_join_bwd"] == ERROR
    d = dev()
    C_, shape = case
    N, D, H, W = shape
    full = (N, C_, D, H, W)
    rng = np.random.default_rng(C_ + H)
    f8 = lambda a: a.astype(np.float64)
    y, res, dout = (rng.standard_normal(full).astype(np.float32) for _ in range(3))
    dres0 = rng.standard_normal(full).astype(np.float32)
    scale, shift = rng.uniform(0.5, 1.5, C_).astype(np.float32), rng.standard_normal(C_).astype(np.float32)
    ai, ao = rng.uniform(0.05, 0.5, C_).astype(np.float32), rng.uniform(-0.2, 0.5, C_).astype(np.float32)
    sh = (1, C_, 1, 1, 1)
    u = f8(y) * f8(scale).reshape(sh) + f8(shift).reshape(sh)
    a = np.where(u > 0, u, u * f8(ai).reshape(sh))
    s_ = a + f8(res)
    out_ref = np.where(s_ > 0, s_, s_ * f8(ao).reshape(sh))
    ds = f8(dout) * np.where(s_ > 0, 1.0, f8(ao).reshape(sh))
    dao_ref = (f8(dout) * s_ * (s_ <= 0)).sum(axis=(0, 2, 3, 4))
    pl = _Place(flavour)
    yt, rt, dt = pl.inp(y), pl.inp(res), pl.inp(dout)
    ot, da, dres = pl.out(full), pl.out(full), pl.out(full, dres0)
    sc, sf, pai, pao = vec(scale), vec(shift), vec(ai), vec(ao)
    d.call("msk_affine_act_join_fwd", yt.msk(), vp(sc), vp(sf), vp(pai), rt.msk(), vp(pao), ot.msk())
    assert rel_err(ot.numpy(), out_ref) < 1e-5
    dao = vec(np.full(C_, 0.25, np.float32))
    args = (yt.msk(), vp(sc), vp(sf), vp(pai), rt.msk(), vp(pao), dt.msk(), da.msk(), dres.msk(), 1, vp(dao))
    if flavour != "aligned" or C_ % 4:
        with pytest.raises(_msk_error()):
            d.call("msk_add_act_join_bwd", *args)
        d.sync()
        assert np.isnan(da.numpy()).all() and np.array_equal(dres.numpy(), dres0)          # nothing was written
        assert np.array_equal(vec_back(dao, C_), np.full(C_, 0.25, np.float32))
    else:
        d.call("msk_add_act_join_bwd", *args)
        assert rel_err(da.numpy(), ds) < 1e-5
        assert rel_err(dres.numpy(), ds + dres0) < 1e-5
        assert rel_err(vec_back(dao, C_), dao_ref + 0.25) < 1e-5
    pl.check()


@pytest.mark.parametrize("case,flavour", _cross(EW_SHAPES, lambda c: c[:1]))
def test_elementwise_on_views(case, flavour):
    """msk_elu_fwd / msk_elu_bwd, msk_copy_scale, msk_channel_sum, msk_argmax_c, msk_softmax_c."""
    for op in ("msk_elu_fwd", "msk_elu_bwd", "msk_copy_scale", "msk_channel_sum", "msk_argmax_c", "msk_softmax_c"):
        assert UNALIGNED[op] == ANSWER
    d = dev()
    C_, shape = case
    N, D, H, W = shape
    full = (N, C_, D, H, W)
    M = N * D * H * W
    rng = np.random.default_rng(C_ + W)
    f8 = lambda a: a.astype(np.float64)
    x = (rng.standard_normal(full) * 2).astype(np.float32)
    dout = rng.standard_normal(full).astype(np.float32)
    g0 = rng.standard_normal(full).astype(np.float32)
    pl = _Place(flavour)
    xt, dt = pl.inp(x), pl.inp(dout)
    # ELU, derivative taken from the output; fresh and accumulating
    alpha = 0.5
    ref = np.where(x > 0, f8(x), alpha * np.expm1(np.minimum(f8(x), 0)))
    dref = f8(dout) * np.where(x > 0, 1.0, alpha * np.exp(np.minimum(f8(x), 0)))
    ot, gt, ga = pl.out(full), pl.out(full), pl.out(full, g0)
    d.call("msk_elu_fwd", xt.msk(), C.c_float(alpha), ot.msk())
    assert rel_err(ot.numpy(), ref) < 1e-5
    d.call("msk_elu_bwd", ot.msk(), dt.msk(), C.c_float(alpha), gt.msk(), 0)
    d.call("msk_elu_bwd", ot.msk(), dt.msk(), C.c_float(alpha), ga.msk(), 1)
    assert rel_err(gt.numpy(), dref) < 1e-5 and rel_err(ga.numpy(), dref + g0) < 1e-5
    # copy_scale with a per-(sample, channel) mask, fresh and accumulating
    mask = ((rng.random((N, C_)) < 0.5) * 2).astype(np.float32)
    c0, c1 = pl.out(full), pl.out(full, g0)
    mp = vec(mask.ravel())
    d.call("msk_copy_scale", xt.msk(), vp(mp), c0.msk(), 0)
    d.call("msk_copy_scale", xt.msk(), vp(mp), c1.msk(), 1)
    want = f8(x) * mask[:, :, None, None, None]
    assert rel_err(c0.numpy(), want) < 1e-5 and rel_err(c1.numpy(), want + g0) < 1e-5
    # channel_sum into a guarded vector (accumulating), argmax into a guarded int buffer, softmax into a view
    cs = vec(np.ones(C_))
    d.call("msk_channel_sum", xt.msk(), vp(cs), 1)
    assert rel_err(vec_back(cs, C_), f8(x).sum(axis=(0, 2, 3, 4)) + 1.0) < 1e-5
    am = dmalloc(M * 4)
    d.call("msk_argmax_c", xt.msk(), vp(am))
    assert np.array_equal(d.d2h(am, (N, D, H, W), np.int32), x.argmax(axis=1))
    st = pl.out(full)
    d.call("msk_softmax_c", xt.msk(), st.msk())
    assert rel_err(st.numpy(), O.softmax(f8(x), axis=1)) < 1e-5
    pl.check()


# ---------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------
def _labels(rng, ncls, shape):
    y = rng.integers(0, ncls, shape).astype(np.int32)
    y[0, 0, 0, :2] = 255                                          # ignore_index voxels
    p = dmalloc(y.nbytes)
    dev().h2d(p, y)
    return y, p


@pytest.mark.parametrize("ncls,flavour", _cross([3, 4, 20], lambda n: (n,)))
def test_ce_dice_loss_on_views(ncls, flavour):
    """msk_loss_fwd / msk_loss_bwd and the _ex forms (softmax-normalised, class-weighted dice): logits and dlogits are views.
    Bounds: test_loss_fwd_bwd's and test_dice_options's."""
    for op in ("msk_loss_fwd", "msk_loss_bwd", "msk_loss_fwd_ex", "msk_loss_bwd_ex"):
        assert UNALIGNED[op] == ANSWER
    d = dev()
    N, D, H, W = 2, 5, 6, 7
    rng = np.random.default_rng(ncls)
    z = (rng.standard_normal((N, ncls, D, H, W)) * 2).astype(np.float32)
    z64 = z.astype(np.float64)
    y, yp = _labels(rng, ncls, (N, D, H, W))
    pl = _Place(flavour)
    zt = pl.inp(z)
    w_ref = O.class_weights(z64)
    wv = vec(w_ref)
    ce_ref, dce = O.cross_entropy(z64, y, w_ref, 255)
    # sigmoid dice with the ignored voxels masked out of the one-hot target (test_loss_fwd_bwd)
    s = 1 / (1 + np.exp(-z64))
    t = np.moveaxis(np.eye(ncls)[np.where(y == 255, 0, y)], -1, 1) * (y != 255)[:, None]
    inter, den = (s * t).sum((0, 2, 3, 4)), (s * s).sum((0, 2, 3, 4)) + (t * t).sum((0, 2, 3, 4))
    den = np.maximum(den, 1e-6)
    per = 2 * inter / den
    ddice = -(1.0 / ncls) * (2 * t / den.reshape(1, -1, 1, 1, 1) - (2 * inter / den ** 2).reshape(1, -1, 1, 1, 1) * 2 * s) * s * (1 - s)
    out, stats = vec(np.zeros(2 + ncls)), dmalloc((3 * ncls + 2) * 8)
    d.call("msk_loss_fwd", zt.msk(), vp(yp), vp(wv), 255, vp(out), vp(stats))
    o = vec_back(out, 2 + ncls)
    assert abs(o[0] - ce_ref) < 2e-5 * abs(ce_ref)
    assert abs(o[1] - (1 - per.mean())) < 2e-6 and rel_err(o[2:], per) < 2e-6
    dz = pl.out(z.shape)
    d.call("msk_loss_bwd", zt.msk(), vp(yp), vp(wv), 255, vp(stats), C.c_float(0.7), C.c_float(1.3), dz.msk())
    assert rel_err(dz.numpy(), 0.7 * dce + 1.3 * ddice) < 2e-5
    # _ex: DiceLoss(sigmoid_norm=False, weight=...); labels without ignored voxels as in test_dice_options
    y2 = np.where(y == 255, 1, y).astype(np.int32)
    yp2 = dmalloc(y2.nbytes)
    d.h2d(yp2, y2)
    dwt = rng.uniform(0.5, 2.0, ncls)
    dwp = vec(dwt)
    ce2, dce2 = O.cross_entropy(z64, y2, w_ref, 255)
    dl_ref, per_ref, ddl = O.dice(z64, y2, sigmoid_norm=False, weight=dwt)
    out2, stats2 = vec(np.zeros(2 + ncls)), dmalloc((3 * ncls + 2) * 8)
    d.call("msk_loss_fwd_ex", zt.msk(), vp(yp2), vp(wv), 255, 1, vp(dwp), vp(out2), vp(stats2))
    o = vec_back(out2, 2 + ncls)
    assert abs(o[0] - ce2) < 2e-5 * abs(ce2)
    assert abs(o[1] - dl_ref) < 2e-6 and rel_err(o[2:], per_ref) < 2e-6
    dz2 = pl.out(z.shape)
    d.call("msk_loss_bwd_ex", zt.msk(), vp(yp2), vp(wv), 255, 1, vp(dwp), vp(stats2), C.c_float(0.7), C.c_float(1.3), dz2.msk())
    assert rel_err(dz2.numpy(), 0.7 * dce2 + 1.3 * ddl) < 5e-6
    pl.check()


@pytest.mark.parametrize("ncls,flavour", _cross([3, 4, 20], lambda n: (n,)))
def test_bce_loss_on_views(ncls, flavour):
    """msk_bce_fwd / msk_bce_bwd (dynamic class and positive weights; fresh and accumulating dlogits); bounds of tests/test_gpu_bce.py:
    loss 1e-5 relative, gradient relative L2 <= 1e-6 and max-abs <= 1e-5 max|g|."""
    assert UNALIGNED["msk_bce_fwd"] == ANSWER and UNALIGNED["msk_bce_bwd"] == ANSWER
    d = dev()
    N, D, H, W = 2, 5, 6, 7
    rng = np.random.default_rng(ncls + 50)
    z = (rng.standard_normal((N, ncls, D, H, W)) * 2).astype(np.float32)
    y, yp = _labels(rng, ncls, (N, D, H, W))
    ref_loss, ref_g = R.bce(z, y, 255, 'dynamic', 'dynamic')
    g0 = (rng.standard_normal(z.shape) * np.abs(ref_g).max()).astype(np.float32)
    pl = _Place(flavour)
    zt, dz, dza = pl.inp(z), pl.out(z.shape), pl.out(z.shape, g0)
    out, stats = vec(np.zeros(4)), dmalloc(8 * 8)
    d.call("msk_bce_fwd", zt.msk(), vp(yp), 255, 1, 2, C.c_float(0.0), vp(out), vp(stats))
    loss = float(vec_back(out, 1)[0])
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss)
    d.call("msk_bce_bwd", zt.msk(), vp(yp), 255, vp(stats), C.c_float(0.75), 0, dz.msk())
    d.call("msk_bce_bwd", zt.msk(), vp(yp), 255, vp(stats), C.c_float(0.75), 1, dza.msk())
    for got, want in ((dz.numpy(), 0.75 * ref_g), (dza.numpy(), 0.75 * ref_g + g0.astype(np.float64))):
        got = got.astype(np.float64)
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-6
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    pl.check()


# ---------------------------------------------------------------------------------------------------------------------------
# trilinear resize
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,flavour", _cross([(20, (1, 8, 8, 6), (64, 64, 12)),      # INTERP_CASES: C % 4 == 0 (float4 kernels when aligned)
                                                 (5, (2, 5, 7, 3), (13, 9, 8))],         # ... and not: non-integer ratios, one axis shrinks
                                                lambda c: c[:1]))
def test_interp_trilinear_on_views(case, flavour):
    """msk_interp_trilinear_fwd / _bwd (fresh and accumulating), source, destination and both gradients views; 1e-5 of max|ref|."""
    assert UNALIGNED["msk_interp_trilinear_fwd"] == ANSWER and UNALIGNED["msk_interp_trilinear_bwd"] == ANSWER
    Cn, (N, sd, sh, sw), size = case
    d = dev()
    rng = np.random.default_rng(Cn * 1000 + sd * 7 + size[0])
    x = rng.standard_normal((N, Cn, sd, sh, sw)).astype(np.float32)
    y_ref = O.trilinear_resize(x.astype(np.float64), size)
    g = rng.standard_normal(y_ref.shape).astype(np.float32)
    dx_ref = O.trilinear_resize_bwd(g.astype(np.float64), (sd, sh, sw))
    dx0 = rng.standard_normal(x.shape).astype(np.float32)
    pl = _Place(flavour)
    xt, yt, gt = pl.inp(x), pl.out(y_ref.shape), pl.inp(g)
    dxt, dxa = pl.out(x.shape), pl.out(x.shape, dx0)
    d.call("msk_interp_trilinear_fwd", xt.msk(), yt.msk())
    assert rel_err(yt.numpy(), y_ref) < 1e-5
    need = C.c_size_t(0)
    d.call("msk_interp_scratch_bytes", dxt.msk(), gt.msk(), C.byref(need))
    scratch = dmalloc(max(need.value, 16))
    d.call("msk_interp_trilinear_bwd", gt.msk(), dxt.msk(), 0, vp(scratch), C.c_size_t(need.value))
    d.call("msk_interp_trilinear_bwd", gt.msk(), dxa.msk(), 1, vp(scratch), C.c_size_t(need.value))
    assert rel_err(dxt.numpy(), dx_ref) < 1e-5
    assert rel_err(dxa.numpy(), dx_ref + dx0) < 1e-5
    pl.check()

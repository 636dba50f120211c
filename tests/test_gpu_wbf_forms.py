"""The stage forms of wbf_gemm_k (msk_conv_wbf.hip, option "wbf_gemm_form") on the product path (fp16 x 2 pieces, 5^3, >= 64
output channels), through the C ABI against the float64 oracle:

  0  one 16-channel chunk per LDS stage, v_mfma_f32_32x32x16_f16 (every other class runs it; here forced)
  2  two chunks per stage, v_mfma_f32_16x16x32_f16 (one instruction's K = 32 spans the two chunks): the default of the class

(Form 1 -- two chunks per stage on 32x32x16, bitwise form 0 -- was measured slower than form 0 in every class and was not
shipped: profiles/r21_gemm_forms.txt.)  Scratch is NaN-poisoned ("poison_scratch" 0xFF): the second chunk's tile region is
LDS / V territory form 0 never read.
Bounds: those of tests/test_gpu_wbf.py (8e-6 * sqrt(K/1000 + 1) and 4e-6 of max|ref|)."""
import functools

import numpy as np
import pytest

from helpers import dev, redzone_check, rel_err, t_empty, t_from_ncdhw, t_to_ncdhw, vec, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

from oracle import vnet_numpy as O  # noqa: E402

K3, S3, P3 = (5, 5, 5), (1, 1, 1), (2, 2, 2)
TAG = "wbf_gemm_h2_k"

# (Cin, Cout, (N, D, H, W), "wbf_ks_blocks")
ODD_SLAB = (128, 256, (1, 8, 16, 24), 1)
CASES = [
    (128, 128, (1, 8, 16, 8), 2),     # 8 x 16 tile, split-K over chunk pairs
    (256, 128, (2, 8, 8, 8), 2),      # 8 x 8 tile with TH = 8 sub-fragments, 16 chunks
    (64, 256, (1, 15, 16, 4), 2),     # two column groups, ragged D, T = 1
    (128, 128, (1, 16, 8, 7), 2),     # permuted transform axis
    (256, 256, (1, 16, 16, 2), 2),    # ragged W tile
    ODD_SLAB,                         # the rule of run_pipeline before chunk pairs left 3 chunks per slab in both directions
]


def _conv_tol(K):
    return 8e-6 * np.sqrt(K / 1000.0 + 1.0)


def _desc():
    from medicalseg_amd._lib import MskConvDesc
    return MskConvDesc(*K3, *S3, *P3)


@functools.lru_cache(maxsize=None)
def _problem(case):
    """Inputs and float64 references of a case, computed once and shared by every arm."""
    cin, cout, (N, D, H, W), _ = case
    rng = np.random.default_rng(cin * 7 + cout + D * H)
    x = rng.standard_normal((N, cin, D, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin) + K3) / np.sqrt(cin * 125)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    f8 = lambda a: a.astype(np.float64)
    y_ref = O.conv3d(f8(x), f8(w), f8(b), S3, P3)
    dy = rng.standard_normal(y_ref.shape).astype(np.float32)
    dx_ref = O.conv3d_dgrad(f8(dy), f8(w), x.shape, S3, P3)
    for a in (x, w, b, dy, y_ref, dx_ref):
        a.setflags(write=False)
    return x, w, b, dy, y_ref, dx_ref


def _run(case, form):
    """forward, data gradient, accumulating data gradient with the form forced -> (y, dx, dx_acc, profile tags)"""
    cin, cout, (N, D, H, W), ks_blocks = case
    x, w, b, dy, _, _ = _problem(case)
    d = dev()
    xt, yt, dyt = t_from_ncdhw(x), t_empty(N, cout, D, H, W, fill=7.0), t_from_ncdhw(dy)
    dxt = t_empty(N, cin, D, H, W, fill=3.0)
    wp, bp = vec(w.ravel()), vec(b)
    d.set_option("prof_shapes", 1)
    d.set_option("prof_only_halo", 0)
    d.set_option("poison_scratch", 0xFF)
    d.set_option("wbf_gemm_form", form)
    d.set_option("wbf_ks_blocks", ks_blocks)
    try:
        d.prof_reset()
        d.prof_enable(True)
        d.call("msk_conv3d_fwd", _desc(), xt.msk(), vp(wp), vp(bp), yt.msk())
        d.call("msk_conv3d_dgrad", _desc(), dyt.msk(), vp(wp), dxt.msk(), 0)
        y, dx = t_to_ncdhw(yt), t_to_ncdhw(dxt)
        d.call("msk_conv3d_dgrad", _desc(), dyt.msk(), vp(wp), dxt.msk(), 1)
        dx_acc = t_to_ncdhw(dxt)
        d.prof_enable(False)
        tags = sorted(d.prof_report())
    finally:
        d.set_option("wbf_gemm_form", -1)
        d.set_option("wbf_ks_blocks", 2)
        d.set_option("poison_scratch", -1)
        d.set_option("prof_shapes", 0)
    return y, dx, dx_acc, tags


def _gemm_tags(tags):
    return [t for t in tags if t.startswith(TAG)]


def _check_form_ran(tags, form):
    g = _gemm_tags(tags)
    # forward, data gradient, accumulating data gradient: every matrix-stage launch of the case is in the class that has the
    # forms (>= 64 output channels, an even number of chunks) and ran the forced one
    assert len(g) >= 1, tags
    for t in g:
        assert "fused" not in t, t
        assert (",form=%d]" % form in t) if form else (",form=" not in t), (form, g)
    assert any("ck=%d," % c in t for t in g for c in (64, 128, 256)), g


def _check_oracle(case, y, dx, dx_acc, label):
    cin, cout = case[0], case[1]
    _, _, _, _, y_ref, dx_ref = _problem(case)
    e_f, e_d, e_acc = rel_err(y, y_ref), rel_err(dx, dx_ref), rel_err(dx_acc, 2 * dx_ref)
    print(f"\nwbf forms {case} {label}: fwd {e_f:.2e} dgrad {e_d:.2e} acc {e_acc:.2e}")
    assert e_f < _conv_tol(cin * 125) and e_d < _conv_tol(cout * 125) and e_acc < _conv_tol(cout * 125)
    assert e_f < 4e-6 and e_d < 4e-6


@pytest.mark.parametrize("form", (0, 2))
@pytest.mark.parametrize("case", CASES)
def test_gemm_form_matches_oracle(case, form):
    y, dx, dx_acc, tags = _run(case, form)
    _check_form_ran(tags, form)
    _check_oracle(case, y, dx, dx_acc, "form %d" % form)
    if form == 2:
        # a fixed order of accumulation: bitwise reproducible run to run
        y2, dx2, dxa2, _ = _run(case, form)
        assert np.array_equal(y, y2) and np.array_equal(dx, dx2) and np.array_equal(dx_acc, dxa2)


def test_form_2_is_the_default():
    _, _, _, tags = _run(CASES[0], -1)
    _check_form_ran(tags, 2)


def _slabs(KC, base_blocks, ks_blocks, num_cu, pairs):
    """run_pipeline's split-K rule -> (chunks per slab, slabs)"""
    ksplit, kc_per = 1, KC
    if base_blocks < 3 * num_cu:
        want = min(KC, (ks_blocks * num_cu + base_blocks - 1) // base_blocks)
        kc_per = (KC + want - 1) // want
        if pairs:
            kc_per = (kc_per + 1) & ~1
        ksplit = (KC + kc_per - 1) // kc_per
    return kc_per, ksplit


@pytest.mark.parametrize("form", (0, 2))
def test_odd_slab_is_rounded_to_chunk_pairs(form):
    """The split-K rule without the rounding leaves THREE chunks per slab in both directions of this case (forward: 8 chunks, 2
    column groups x 6 W tiles x 8 points = 96 workgroups; data gradient: 16 chunks, 48 workgroups; one workgroup per CU wanted):
    slabs are whole chunk pairs in this class, for every form, and the result is the oracle's."""
    case = ODD_SLAB
    cin, cout, (N, D, H, W), ks_blocks = case
    d = dev()
    num_cu = d.get_option("num_cu")
    T = W // 4                                   # transform along W; one 8 x 16 tile per (n, W tile)
    expect = {}
    for ck, cn in ((cin, cout), (cout, cin)):    # forward, data gradient
        base = 8 * (cn // 128) * T * N
        per_old, _ = _slabs(ck // 16, base, ks_blocks, num_cu, False)
        per_new, ks_new = _slabs(ck // 16, base, ks_blocks, num_cu, True)
        if num_cu == 256:
            assert per_old == 3, (ck, cn, per_old)   # what the case is about (MI355X: 256 CUs)
        assert per_new % 2 == 0
        expect[(ck, cn)] = ks_new
    y, dx, dx_acc, tags = _run(case, form)
    _check_form_ran(tags, form)
    g = _gemm_tags(tags)
    for (ck, cn), ks in expect.items():
        assert any("ck=%d,cn=%d," % (ck, cn) in t and (",ks=%d," % ks in t or ",ks=%d]" % ks in t) for t in g), (ck, cn, ks, g)
    _check_oracle(case, y, dx, dx_acc, "odd slab, form %d" % form)


# ---------------------------------------------------------------------------------------------------------
# one-kernel matrix stage, pipelined form, 32 output channels: option "wbf_fused_sh" (1 = 16x16x32 over tap pairs, the
# default; 0 = 32x32x16), forced below its size threshold by "wbf_fuse" 2
# ---------------------------------------------------------------------------------------------------------
FUSED_CASES = [
    (32, 32, (2, 16, 32, 16)),      # exact fit
    (32, 32, (1, 30, 60, 8)),       # ragged tiles
    (32, 32, (1, 32, 32, 9)),       # ragged W
]


@functools.lru_cache(maxsize=None)
def _fused_problem(case):
    cin, cout, (N, D, H, W) = case
    x, w, b, dy, y_ref, dx_ref = _problem(case + (2,))
    rng = np.random.default_rng(D * W + 1)
    c = cout
    f8 = lambda a: a.astype(np.float64)
    # a LUConv unit's backward (BatchNorm + PReLU behind the convolution), float64: dout -> dy -> dx
    y = y_ref.astype(np.float32)
    dout = (rng.standard_normal(y.shape) * 1e-6).astype(np.float32)   # real gradient magnitudes: below fp16's normal range
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), (0.3 * rng.standard_normal(c)).astype(np.float32)
    alpha = rng.uniform(0.05, 0.5, c).astype(np.float32)
    yc = np.moveaxis(f8(y), 1, -1).reshape(-1, c)
    M = yc.shape[0]
    mean, var = yc.mean(0), yc.var(0)
    invstd = 1.0 / np.sqrt(var + 1e-5)
    scale, shift = f8(gamma) * invstd, f8(beta) - mean * f8(gamma) * invstd
    du = np.moveaxis(f8(dout), 1, -1).reshape(-1, c) * np.where(yc * scale + shift > 0, 1.0, f8(alpha))
    xhat = (yc - mean) * invstd
    sums = np.concatenate([du.sum(0), (du * xhat).sum(0)])
    dyb = scale * (du - sums[:c] / M - xhat * sums[c:] / M)
    dyb = np.moveaxis(dyb.reshape(N, D, H, W, c), -1, 1)
    dxb_ref = O.conv3d_dgrad(dyb, f8(w), x.shape, S3, P3)
    coef = {k_: v.astype(np.float32) for k_, v in dict(scale=scale, shift=shift, alpha=alpha, mean=mean, invstd=invstd, gamma=gamma,
                                                       sums=sums).items()}
    return y, dout, coef, float(M), dxb_ref


@pytest.mark.parametrize("sh", (0, 1))
@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_matrix_stage_shape(case, sh):
    """plain forward, forward with statistics, accumulating data gradient and the split-store data gradient of the one-kernel
    form with either MFMA shape, against the float64 oracle"""
    import ctypes as C
    from helpers import dmalloc
    from medicalseg_amd._lib import NULL_TENSOR
    cin, cout, (N, D, H, W) = case
    x, w, b, dy, y_ref, dx_ref = _problem(case + (2,))
    y, dout, coef, M, dxb_ref = _fused_problem(case)
    d = dev()
    desc = _desc()
    tol = _conv_tol(cin * 125)
    xt, dyt = t_from_ncdhw(x), t_from_ncdhw(dy)
    wp, bp = vec(w.ravel()), vec(b)
    d.set_option("prof_shapes", 1)
    d.set_option("prof_only_halo", 0)
    d.set_option("poison_scratch", 0xFF)
    d.set_option("wbf_fuse", 2)
    d.set_option("wbf_fused_sh", sh)
    d.set_option("wgrad_async", 0)
    try:
        d.prof_reset()
        d.prof_enable(True)
        # plain forward
        yt = t_empty(N, cout, D, H, W, fill=7.0)
        d.call("msk_conv3d_fwd", desc, xt.msk(), vp(wp), vp(bp), yt.msk())
        e_f = rel_err(t_to_ncdhw(yt), y_ref)
        # forward with statistics
        ys = t_empty(N, cout, D, H, W, fill=7.0)
        stats = vec(np.zeros(2 * cout, np.float32))
        nx = int(d.lib.msk_conv3d_xform_bytes(d.ctx, desc, xt.msk(), cout))
        assert nx > 0
        xf = dmalloc(nx)
        d.call("msk_conv3d_fwd_ex", desc, xt.msk(), vp(wp), vp(bp), ys.msk(), vp(stats), vp(xf))
        got_s = t_to_ncdhw(ys)
        e_s = rel_err(got_s, y_ref)
        st = d.d2h(stats, (2 * cout,), np.float32)
        # accumulating data gradient
        dxt = t_empty(N, cin, D, H, W, fill=3.0)
        d.call("msk_conv3d_dgrad", desc, dyt.msk(), vp(wp), dxt.msk(), 0)
        e_d = rel_err(t_to_ncdhw(dxt), dx_ref)
        d.call("msk_conv3d_dgrad", desc, dyt.msk(), vp(wp), dxt.msk(), 1)
        e_acc = rel_err(t_to_ncdhw(dxt), 2 * dx_ref)
        # split-store data gradient of the LUConv backward: 16 + 16 dense channels, the interleaved buffer read only
        cv = {k_: vec(v) for k_, v in coef.items()}
        ytn, dot = t_from_ncdhw(y), t_from_ncdhw(dout)
        nb = int(d.lib.msk_conv3d_bwd_bnact_bytes(d.ctx, desc, xt.msk(), ytn.msk()))
        assert nb > 0
        ybuf = dmalloc(nb)
        maxes, sums_dev = vec(np.zeros(128, np.float32)), vec(np.zeros(3 * cout, np.float32))
        d.call("msk_affine_act_bwd_reduce_ex", ytn.msk(), vp(cv["scale"]), vp(cv["shift"]), NULL_TENSOR, vp(cv["alpha"]),
               vp(cv["mean"]), vp(cv["invstd"]), dot.msk(), vp(sums_dev), vp(maxes))
        old = (0.25 * dxb_ref).astype(np.float32)
        inter = t_from_ncdhw(old)
        dyn = t_empty(N, cout, D, H, W, fill=9.0)
        dw2 = vec(np.zeros(w.size, np.float32))
        lo, hi = t_empty(N, cin // 2, D, H, W, fill=7.0), t_empty(N, cin // 2, D, H, W, fill=7.0)
        done = C.c_int(-1)
        d.call("msk_conv3d_bwd_bnact_split", desc, xt.msk(), vp(wp), ytn.msk(), vp(cv["scale"]), vp(cv["shift"]), vp(cv["alpha"]),
               vp(cv["mean"]), vp(cv["invstd"]), vp(cv["gamma"]), dot.msk(), vp(cv["sums"]), C.c_double(M),
               dyn.msk(), inter.msk(), 1, vp(dw2), 0, vp(xf), vp(ybuf), vp(maxes), lo.msk(), hi.msk(), C.byref(done))
        d.sync()
        d.prof_enable(False)
        tags = sorted(d.prof_report())
        assert done.value == 1, done.value
        got_split = np.concatenate([t_to_ncdhw(lo), t_to_ncdhw(hi)], axis=1)
        e_split = rel_err(got_split, 1.25 * dxb_ref)
        assert np.array_equal(t_to_ncdhw(inter), old)          # read, never written (the red zones are checked after the test)
    finally:
        d.prof_enable(False)
        d.set_option("wbf_fused_sh", 1)
        d.set_option("wbf_fuse", 1)
        d.set_option("wgrad_async", 1)
        d.set_option("poison_scratch", -1)
        d.set_option("prof_shapes", 0)
    print(f"\nfused {case} sh {sh}: fwd {e_f:.2e} fwd+stats {e_s:.2e} dgrad {e_d:.2e} acc {e_acc:.2e} split {e_split:.2e}")
    g = [t for t in tags if t.startswith(TAG)]
    assert len(g) >= 1 and all(",fused" in t and (",sh16" in t) == (sh == 1) for t in g), tags   # the one-kernel form, this shape
    assert e_f < tol and e_s < tol and e_d < tol and e_acc < tol and e_split < tol
    assert e_f < 4e-6 and e_d < 4e-6
    # the statistics are those of the stored values (float64 mean / M2 of the oracle's y)
    yc = np.moveaxis(y_ref, 1, -1).reshape(-1, cout)
    mean_ref, m2_ref = yc.mean(0), ((yc - yc.mean(0)) ** 2).sum(0)
    assert np.abs(st[:cout] - mean_ref).max() < 1e-5 * (np.abs(mean_ref).max() + 1)
    assert np.abs(st[cout:] - m2_ref).max() < 1e-5 * m2_ref.max()

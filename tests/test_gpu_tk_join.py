"""The residual-join backward fused into out_tr.conv1's data gradient (msk_conv3d_bwd_bnact_join, conv_tk_h2_k<JOIN>) against the
separate calls it replaces (option "tk_join" 0: the entry point declines and the caller runs them).

The first-operand gradient and the two maxima must be bit-equal between the paths and between two fused runs; the four
per-channel sums (and the parameter gradients the merge adds them to) change their summation order only.  They are compared with
a float64 host sum of the per-element terms, evaluated from the same inputs and from the GPU's own join-output gradient (read back
from the separate calls).  Tolerance: the separate calls' own deviation from that sum is measured at run time on the same inputs;
the fused path gets 4x that per channel and quantity (another partial count and tree), with the floor eps_fp32 * sum |term| per
channel -- the rounding of one fp32 addition chain at unit weight."""
import ctypes as C

import numpy as np
import pytest

from helpers import dev, redzone_check, t_empty, t_from_ncdhw, t_to_ncdhw, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

K5, S1, P2 = (5, 5, 5), (1, 1, 1), (2, 2, 2)
CJ = 32
EPS = float(np.finfo(np.float32).eps)


def _desc():
    from medicalseg_amd._lib import MskConvDesc
    return MskConvDesc(*K5, *S1, *P2)


def _null():
    from medicalseg_amd._lib import NULL_TENSOR
    return NULL_TENSOR


def _inputs(ncls, N, D, H, W, seed, C=CJ):
    rng = np.random.default_rng(seed)
    f = np.float32
    shp = (N, C, D, H, W)
    i = {"x": rng.standard_normal(shp).astype(f),
         "w": (rng.standard_normal((ncls, C) + K5) / np.sqrt(125 * ncls)).astype(f),
         "y": rng.standard_normal((N, ncls, D, H, W)).astype(f),
         "dout": rng.standard_normal((N, ncls, D, H, W)).astype(f)}
    for k in ("scale", "gamma", "invstd"):
        i[k] = rng.uniform(0.5, 1.5, ncls).astype(f)
    for k in ("shift", "mean"):
        i[k] = rng.uniform(-0.3, 0.3, ncls).astype(f)
    i["alpha"] = rng.uniform(0.1, 0.4, ncls).astype(f)
    i["sums"] = (rng.standard_normal(3 * ncls) * 1e-2).astype(f)
    # the join: about 30 % of t = scale * jy + shift and about 30 % of u = prelu(t) + res are <= 0
    i["jy"] = rng.standard_normal(shp).astype(f)
    i["jscale"] = rng.uniform(0.5, 1.5, C).astype(f)
    i["jshift"] = (0.52 * i["jscale"]).astype(f)
    i["jai"] = rng.uniform(0.1, 0.4, C).astype(f)
    i["jal"] = rng.uniform(0.1, 0.4, C).astype(f)
    i["jmean"] = rng.uniform(-0.3, 0.3, C).astype(f)
    i["jinvstd"] = rng.uniform(0.5, 1.5, C).astype(f)
    bc = lambda v: v.reshape(1, C, 1, 1, 1)
    t = i["jy"] * bc(i["jscale"]) + bc(i["jshift"])
    a = np.where(t > 0, t, t * bc(i["jai"]))
    i["jres"] = (rng.standard_normal(shp).astype(f) + f(0.52) - a).astype(f)
    return i


def _run(i, fused, da_ld=None, res_ld=None, da_accumulate=0, db_ld=None):
    """One backward of the unit + join through the entry point (fused) or, when it declines, the separate calls.  Returns
    (rc, outputs).  db_ld: the second operand's gradient is written too (not shared), into a buffer of that leading dimension."""
    d = dev()
    N, C_, D, H, W = i["x"].shape
    ncls = i["y"].shape[1]
    d.set_option("tk_join", 1 if fused else 0)
    try:
        xt, yt, dt = t_from_ncdhw(i["x"]), t_from_ncdhw(i["y"]), t_from_ncdhw(i["dout"])
        jyt, jrt = t_from_ncdhw(i["jy"]), t_from_ncdhw(i["jres"], ld=res_ld)
        dy, da = t_empty(N, ncls, D, H, W), t_empty(N, C_, D, H, W, ld=da_ld, fill=-7.0)
        db = t_empty(N, C_, D, H, W, ld=db_ld, fill=-7.0) if db_ld else None
        dbm = db.msk() if db_ld else _null()
        w = vec(i["w"].ravel())
        p = {k: vec(i[k]) for k in ("scale", "shift", "alpha", "mean", "invstd", "gamma", "sums", "jscale", "jshift", "jai", "jal",
                                    "jmean", "jinvstd")}
        dw = vec(np.zeros(i["w"].size))
        pg = {k: vec(np.zeros(C_)) for k in ("dal", "dgamma", "dbeta", "dai")}
        usums = vec(np.zeros(4 * C_))       # the merge stores all four quantities
        maxes = vec(np.full(128, 3.0))       # stale values: the call clears them
        amax = d.amax_new()
        M = float(N * D * H * W)
        rc = d.lib.msk_conv3d_bwd_bnact_join(
            d.ctx, _desc(), xt.msk(), vp(w), yt.msk(), vp(p["scale"]), vp(p["shift"]), vp(p["alpha"]), vp(p["mean"]), vp(p["invstd"]),
            vp(p["gamma"]), dt.msk(), vp(p["sums"]), C.c_double(M), dy.msk(), vp(amax), vp(dw), 1, None, None,
            jyt.msk(), vp(p["jscale"]), vp(p["jshift"]), vp(p["jai"]), jrt.msk(), vp(p["jal"]), vp(p["jmean"]), vp(p["jinvstd"]),
            da.msk(), da_accumulate, dbm, 0, vp(pg["dal"]), vp(usums), vp(maxes), 1, vp(pg["dgamma"]), vp(pg["dbeta"]), vp(pg["dai"]))
        assert rc in (0, 1), rc
        out = {"rc": rc}
        if rc == 1:
            out["da_untouched"] = (bool(np.all(t_to_ncdhw(da) == -7.0)) and bool(np.all(vec_back(maxes, 128) == 3.0))
                                   and (db is None or bool(np.all(t_to_ncdhw(db) == -7.0))))
            dj = t_empty(N, C_, D, H, W)
            d.call("msk_affine_act_bwd_apply_amax", yt.msk(), vp(p["scale"]), vp(p["shift"]), _null(), vp(p["alpha"]), vp(p["mean"]),
                   vp(p["invstd"]), vp(p["gamma"]), dt.msk(), vp(p["sums"]), C.c_double(M), 1, dy.msk(), _null(), 0, vp(amax))
            d.call("msk_conv3d_wgrad_ex3", _desc(), xt.msk(), dy.msk(), vp(dw), None, 1, None, vp(amax), None)
            d.call("msk_conv3d_dgrad_ex", _desc(), dy.msk(), vp(w), dj.msk(), 0, vp(amax))
            d.call("msk_add_act_join_bwd_pg", jyt.msk(), vp(p["jscale"]), vp(p["jshift"]), vp(p["jai"]), jrt.msk(), vp(p["jal"]),
                   vp(p["jmean"]), vp(p["jinvstd"]), dj.msk(), da.msk(), dbm, 0, vp(pg["dal"]), vp(usums), vp(maxes), 1,
                   vp(pg["dgamma"]), vp(pg["dbeta"]), vp(pg["dai"]))
            out["dj"] = t_to_ncdhw(dj)
        d.sync()
        out["da"] = t_to_ncdhw(da)
        if db is not None:
            out["db"] = t_to_ncdhw(db)
        out["maxes"] = vec_back(maxes, 128).reshape(2, 64).max(axis=1)
        out["usums"] = vec_back(usums, 4 * C_).reshape(4, C_)
        for k in pg:
            out[k] = vec_back(pg[k], C_)
        out["dw"] = vec_back(dw, i["w"].size)
        return out
    finally:
        d.set_option("tk_join", 1)


def _host_sums(i, dj):
    """float64 sums of the per-element terms of the join backward; branches decided in fp32 as the kernels do.
    Returns (sums [4][C]: du, du * xhat, d alpha_in, d alpha; sum |term| [4][C])."""
    C_ = i["jy"].shape[1]
    bc = lambda v: v.reshape(1, C_, 1, 1, 1)
    t32 = i["jy"] * bc(i["jscale"]) + bc(i["jshift"])
    a32 = np.where(t32 > 0, t32, t32 * bc(i["jai"]))
    u32 = a32 + i["jres"]
    tneg, uneg = ~(t32 > 0), ~(u32 > 0)
    f8 = lambda v: v.astype(np.float64)
    x, dv = f8(i["jy"]), f8(dj)
    t = x * bc(f8(i["jscale"])) + bc(f8(i["jshift"]))
    u = np.where(tneg, t * bc(f8(i["jai"])), t) + f8(i["jres"])
    g = np.where(uneg, bc(f8(i["jal"])) * dv, dv)
    gu = np.where(tneg, g * bc(f8(i["jai"])), g)
    xh = (x - bc(f8(i["jmean"]))) * bc(f8(i["jinvstd"]))
    terms = [gu, gu * xh, np.where(tneg, g * t, 0.0), np.where(uneg, dv * u, 0.0)]
    ax = (0, 2, 3, 4)
    return np.stack([q.sum(axis=ax) for q in terms]), np.stack([np.abs(q).sum(axis=ax) for q in terms]), (tneg.mean(), uneg.mean())


def _got_sums(o):
    return np.stack([o["usums"][0], o["usums"][1], o["usums"][2], o["dal"]]).astype(np.float64)


CASES = [
    # ncls, (D, H, W), da ld, res ld, db ld
    (3, (4, 8, 12), None, None, None),     # a single partial tile, one D segment
    (3, (9, 18, 20), None, None, None),    # partial tiles on both axes, odd D
    (3, (17, 16, 33), None, None, None),   # two uneven D segments, three W tiles
    (2, (9, 18, 20), None, None, None),    # two classes
    (3, (9, 18, 20), 40, 64, None),        # da and b as channel slices of wider buffers
    (3, (9, 18, 20), 40, 64, 48),          # the second operand's gradient written as well (not shared), at a third ld
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_fused_join_backward_matches_the_separate_calls(case):
    ncls, (D, H, W), da_ld, res_ld, db_ld = case
    i = _inputs(ncls, 2, D, H, W, seed=ncls * 1000 + D * 37 + W)
    ref = _run(i, fused=False, da_ld=da_ld, res_ld=res_ld, db_ld=db_ld)
    assert ref["rc"] == 1 and ref["da_untouched"]
    f1 = _run(i, fused=True, da_ld=da_ld, res_ld=res_ld, db_ld=db_ld)
    f2 = _run(i, fused=True, da_ld=da_ld, res_ld=res_ld, db_ld=db_ld)
    assert f1["rc"] == 0 and f2["rc"] == 0
    assert np.abs(ref["dj"]).max() > 0
    assert np.array_equal(f1["da"], ref["da"])
    assert np.array_equal(f1["maxes"], ref["maxes"])
    assert np.array_equal(f1["dw"], ref["dw"])
    if db_ld:
        assert np.array_equal(f1["db"], ref["db"]) and np.array_equal(f1["db"], f1["da"]) and np.array_equal(f2["db"], f1["db"])
    for k in ("da", "maxes", "usums", "dal", "dgamma", "dbeta", "dai", "dw"):
        assert np.array_equal(f1[k], f2[k]), k
    sums, mags, frac = _host_sums(i, ref["dj"])
    assert 0.2 < frac[0] < 0.4 and 0.2 < frac[1] < 0.4, frac
    dev_ref, dev_fus = np.abs(_got_sums(ref) - sums), np.abs(_got_sums(f1) - sums)
    print("case", case, "deviation from the float64 sums, separate calls / fused, worst per quantity:",
          dev_ref.max(axis=1), dev_fus.max(axis=1), "floor", (EPS * mags).max(axis=1))
    tol = np.maximum(4 * dev_ref, EPS * mags)       # per channel and quantity
    assert np.all(dev_fus <= tol), (dev_fus.max(axis=1), tol.max(axis=1))
    # the parameter gradients the merge adds the sums to (zero before the call): d beta, d gamma, d alpha_in
    for k, q in (("dbeta", 0), ("dgamma", 1), ("dai", 2)):
        assert np.all(np.abs(f1[k].astype(np.float64) - sums[q]) <= tol[q]), k


@pytest.mark.gpu
def test_entry_point_declines_what_the_kernel_does_not_take():
    i = _inputs(3, 2, 9, 18, 20, seed=5)
    o = _run(i, fused=True, da_accumulate=1)
    assert o["rc"] == 1 and o["da_untouched"]
    ref = _run(i, fused=False)
    for k in ("da", "maxes", "usums", "dal", "dgamma", "dbeta", "dai", "dw"):
        assert np.array_equal(o[k], ref[k]), k
    i16 = _inputs(3, 2, 9, 18, 20, seed=6, C=16)
    o = _run(i16, fused=True)
    assert o["rc"] == 1 and o["da_untouched"]
    ref = _run(i16, fused=False)
    for k in ("da", "maxes", "usums", "dal", "dw"):
        assert np.array_equal(o[k], ref[k]), k


def _l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-30))


@pytest.mark.gpu
def test_vnet_step_takes_the_fused_path_and_keeps_its_gradients():
    """One training step of VNet at 2 x 16 x 32 x 32 with the option on and off, same seed: the forward is untouched (logits and loss
    bit-equal); every parameter gradient within the per-tensor bounds tests/test_gpu_model.py uses against the oracle (relative
    L2 2e-2, max-abs 1e-1 of the tensor's scale; the bulk far tighter: median 3e-3)."""
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation
    from oracle import vnet_numpy as O
    d = dev()
    ncls, N, shape = 3, 2, (16, 32, 32)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N, 1) + shape).astype(np.float32)
    y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
    res = []
    try:
        for on in (1, 0):
            d.set_option("tk_join", on)
            model = VNet(num_classes=ncls)
            model.set_state_dict(O.init_params(8, 1, ncls))
            model.train()
            model.set_dropout_masks({})
            losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
            logits = model(x)
            ll, _ = loss_computation(logits, to_tensor(y), losses)
            lg, lv = logits[0].numpy().copy(), float(sum(ll))
            model.clear_gradients()
            d.prof_reset()
            d.prof_enable(True)
            try:
                sum(ll).backward()
                d.sync()
            finally:
                d.prof_enable(False)
            tags = d.prof_report()
            res.append((lg, lv, {n_: p.grad_numpy().copy() for n_, p in model.named_parameters()}, tags))
    finally:
        d.set_option("tk_join", 1)
    (lg1, lv1, g1, t1), (lg0, lv0, g0, t0) = res
    count = lambda tags, name: sum(int(v[0]) for k, v in tags.items() if k.split("[")[0] == name)
    assert count(t1, "conv_tk_h2_join") == 1 and count(t1, "conv_tk_h2") == 0
    assert count(t0, "conv_tk_h2_join") == 0 and count(t0, "conv_tk_h2") == 1
    assert count(t1, "add_act_bwd_unit") == count(t0, "add_act_bwd_unit") - 1
    assert np.array_equal(lg1, lg0) and lv1 == lv0
    l2s = []
    for k in g0:
        scale = np.abs(g0[k]).max()
        if scale < 1e-9:
            assert np.abs(g1[k]).max() < 1e-4, k
            continue
        l2s.append(_l2(g1[k], g0[k]))
        assert l2s[-1] < 2e-2, (k, l2s[-1])
        assert np.abs(g1[k] - g0[k]).max() / scale < 1e-1, k
    assert float(np.median(l2s)) < 3e-3
    print("fused against separate: gradient L2 worst %.2e median %.2e" % (max(l2s), float(np.median(l2s))))

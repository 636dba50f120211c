"""The top-k select and the top-k cross entropy on the device (msk_topk_select / msk_topk_ce_fwd / msk_topk_ce_bwd,
medicalseg_amd/csrc/msk_loss_topk.hip) against the statement tests/topk_reference.py, and TopKLoss / DiceTopKLoss inside the
training stack.

Bounds.  The select is exact: every field of the record is compared with ==, S_gt bit for bit.  The per-voxel losses use the
device's expf / logf: they are held to the float64 statement within 4 x the largest deviation of the statement's own float32
evaluation from its float64 one on that input (computed here; the convention of tests/test_gpu_intensity.py).  The record of the
forward pass is the statement's select applied to the DOWNLOADED losses, with ==.  The loss is within 1e-5 relative of the float64
statement and the gradient max-abs <= 2e-5 max|g| with relative L2 <= 1e-5 (the bounds of tests/test_gpu_region_loss.py; the float32
statement stays within 3.3e-8 of the float64 loss at these shapes).  Against the gradient built from the downloaded losses and
record no voxel may flip; end to end against the float64 statement the voxels with |l64 - T64| <= 1e-5 max(1, T64) are left out,
at most 4 per case (1 with this data: the threshold voxel itself)."""
import ctypes as C
import os
import random
import re
import warnings

import numpy as np
import pytest

import region_reference as R
import topk_reference as T
from helpers import dev, dfree, dmalloc, redzone_check, t_from_ncdhw, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("T", "K", "n_gt", "n_eq", "S_gt", "r", "tie_w", "S")


def _ws_bytes(n):
    b = C.c_size_t(0)
    assert dev().lib.msk_topk_workspace(C.c_long(n), C.byref(b)) == 0
    return b.value


def _same_record(got, want, tag):
    for name, a, b in zip(FIELDS, got, want):
        assert a == b and np.signbit(a) == np.signbit(b), (tag, name, a, b)


# ---- 1. the select -------------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 257, 4095, 4097, 70001, 1052677]   # the last: more than 256 chunks, the finish pass takes a second row
KINDS = ["normal", "equal", "three", "sentinels", "denormals"]


def _select_data(kind, n):
    rng = np.random.default_rng(n + len(kind))
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.6931472, np.float32)
    if kind == "three":
        return rng.choice(np.array([-2.5, 0.25, 3.0], np.float32), n)
    if kind == "sentinels":
        x = np.abs(rng.standard_normal(n)).astype(np.float32)
        x[rng.permutation(n)[:n // 2]] = -1.0
        return x
    x = (rng.integers(-40, 40, n).astype(np.float32) * np.float32(1e-45)).astype(np.float32)   # denormals, -0.0 and +0.0
    x[::7] = -0.0
    x[3::7] = 0.0
    return x


def _ks(n):
    return sorted({0, 1, n // 10, n - 1, n})


def _select(xp, n, k, ws, rec):
    d = dev()
    d.call("msk_topk_select", vp(xp), C.c_long(n), C.c_long(k), vp(ws), vp(rec))
    return d.d2h(rec, (8,), np.float64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_select_matches_the_statement_exactly(n, kind):
    d = dev()
    x = _select_data(kind, n)
    xp, ws, rec = vec(x), dmalloc(_ws_bytes(n)), dmalloc(64)
    for k in _ks(n):
        _same_record(_select(xp, n, k, ws, rec), T.select(x, k), (kind, n, k))
    assert np.array_equal(d.d2h(xp, (n,), np.uint32), x.view(np.uint32))      # x is not modified
    for p in (xp, ws, rec):
        dfree(p)


@pytest.mark.parametrize("n", [257, 4097, 70001])
def test_select_takes_a_buffer_that_is_only_4_byte_aligned(n):
    x = _select_data("normal", n)
    host = np.zeros(n + 1, np.float32)
    host[1:] = x
    base, ws, rec = vec(host), dmalloc(_ws_bytes(n)), dmalloc(64)
    for k in _ks(n):
        _same_record(_select(base + 4, n, k, ws, rec), T.select(x, k), (n, k))
    for p in (base, ws, rec):
        dfree(p)


def test_select_gives_the_same_record_with_same_bin_aggregation():
    """option "topk_agg_hist": the first histogram pass through msk_count_slot counts the same"""
    d = dev()
    n = 70001
    try:
        for kind in ("equal", "sentinels"):
            x = _select_data(kind, n)
            xp, ws, rec = vec(x), dmalloc(_ws_bytes(n)), dmalloc(64)
            d.set_option("topk_agg_hist", 1)
            for k in (1, n // 10, n):
                _same_record(_select(xp, n, k, ws, rec), T.select(x, k), (kind, k))
            d.set_option("topk_agg_hist", 0)
    finally:
        d.set_option("topk_agg_hist", 0)


# ---- 2. and 3. the cross entropy --------------------------------------------------------------------------------------------------
CE_CASES = [((2, 5, 6, 7), 3), ((1, 8, 12, 20), 8), ((2, 9, 10, 33), 20), ((1, 3, 5, 130), 2), ((2, 5, 6, 7), 33)]
CE_IDS = ["%dx%dx%dx%d-C%d" % (s + (c,)) for s, c in CE_CASES]
SEEDS = dict(zip(CE_IDS, (11, 12, 13, 14, 15)))


def _data(rng, shape, Cn):
    N, D, H, W = shape
    z = (rng.standard_normal((N, Cn, D, H, W)) * 2).astype(np.float32)
    y = rng.integers(0, Cn, (N, D, H, W)).astype(np.int32)
    y[rng.random(y.shape) < 0.1] = 255
    y.flat[1] = Cn + 2                          # outside [0, C), not ignored: takes no part
    y[0, 0, 0, 2] = 1                           # a voxel where the softmax saturates at its label: l = 0 in float32
    z[0, :, 0, 0, 2] = -30.0
    z[0, 1, 0, 0, 2] = 30.0
    y[0, 0, 0, 3] = 0                           # and one that saturates at another class: l = 60, the largest
    z[0, :, 0, 0, 3] = -30.0
    z[0, 1, 0, 0, 3] = 30.0
    return z, y


def _device_labels(y):
    p = dmalloc(y.nbytes)
    dev().h2d(p, y)
    return p


def _tensor(z, sliced):
    """the logits dense or as a channel slice of a buffer 4 channels wider; -> (tensor to pass, the whole tensor, first channel)"""
    if not sliced:
        t = t_from_ncdhw(z)
        return t, t, 0
    N, Cn, D, H, W = z.shape
    wide = (np.random.default_rng(99).standard_normal((N, Cn + 4, D, H, W)) * 50).astype(np.float32)   # large: a wrong channel shows
    wide[:, 1:1 + Cn] = z
    tw = t_from_ncdhw(wide)
    return tw.channel_slice(1, 1 + Cn), tw, 1


def _ce_fwd(zt, yp, V, k, wp, ignore=255):
    d = dev()
    ws, rec, out = dmalloc(_ws_bytes(V)), dmalloc(64), vec(np.full(2 + zt.c, 7.0))
    d.call("msk_topk_ce_fwd", zt.msk(), vp(yp), ignore, vp(wp), C.c_float(k), vp(ws), vp(out), vp(rec))
    return ws, rec, vec_back(out, 2 + zt.c), d.d2h(rec, (8,), np.float64), d.d2h(ws, (V,), np.float32)


def _rel_ok(got, ref, tol=1e-5):
    return abs(float(got) - float(ref)) <= tol * abs(float(ref))


def _grad_ok(got, ref):
    """max-abs <= 2e-5 max|g| and relative L2 <= 1e-5"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    if scale == 0:
        return not got.any()
    return np.abs(got - ref).max() <= 2e-5 * scale and np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref)


@pytest.mark.parametrize("k,weighted", [(10.0, True), (37.5, False), (100.0, False)])
@pytest.mark.parametrize("case", CE_CASES, ids=CE_IDS)
def test_ce_forward_matches_statement(case, k, weighted):
    shape, Cn = case
    V = int(np.prod(shape))
    rng = np.random.default_rng(SEEDS[CE_IDS[CE_CASES.index(case)]])
    z, y = _data(rng, shape, Cn)
    w = rng.uniform(0.5, 2, Cn).astype(np.float32) if weighted else None
    yp, wp = _device_labels(y), (vec(w) if weighted else None)
    ref64, ref32 = T.topk_ce(z, y, k, weight=w, dtype=np.float64), T.topk_ce(z, y, k, weight=w, dtype=np.float32)
    got = {}
    for sliced in (False, True):
        zt, whole, _ = _tensor(z, sliced)
        ws, rec_p, out, rec, l = _ce_fwd(zt, yp, V, k, wp)
        got[sliced] = (out.view(np.uint32), rec.view(np.uint64), l.view(np.uint32))
        for p in (ws, rec_p, whole.ptr):
            dfree(p)
    for a, b in zip(got[False], got[True]):       # a channel slice (a lane's own loads) gives the bits of the dense tensor (LDS tiles)
        assert np.array_equal(a, b)
    out, rec, l = got[False][0].view(np.float32), got[False][1].view(np.float64), got[False][2].view(np.float32)
    valid = ref64["valid"]
    assert np.array_equal(l == -1.0, ~valid)                                   # the sentinels are exactly the invalid voxels
    tol = 4.0 * float(np.abs(ref32["l"].astype(np.float64) - ref64["l"]).max())
    err = float(np.abs(l.astype(np.float64) - ref64["l"]).max())
    print("l: device error %.3e, float32-numpy deviation x 4 = %.3e; loss %.3e (float32 statement %.3e)" % (
        err, tol, abs(out[0] - ref64["loss"]) / ref64["loss"], abs(ref32["loss"] - ref64["loss"]) / ref64["loss"]))
    assert np.isfinite(l).all() and err <= tol and l[valid].min() >= 0
    K = T.k_of(int(valid.sum()), k)
    assert K == ref64["K"] and K >= 1
    _same_record(rec, T.select(l, K), (case, k))
    assert _rel_ok(out[0], ref64["loss"]), (out[0], ref64["loss"])
    assert not out[1:].any()


@pytest.mark.parametrize("case", CE_CASES[:4], ids=CE_IDS[:4])
def test_k_100_is_the_region_loss_s_cross_entropy(case):
    d = dev()
    shape, Cn = case
    V = int(np.prod(shape))
    z, y = _data(np.random.default_rng(3), shape, Cn)
    yp, zt = _device_labels(y), t_from_ncdhw(z)
    _, _, out, rec, _ = _ce_fwd(zt, yp, V, 100.0, None)
    rout, rstats = vec(np.zeros(2 + Cn)), dmalloc((5 * Cn + 2) * 8)
    d.call("msk_region_loss_fwd", zt.msk(), vp(yp), 255, 0, 0, 1, 0, 0, C.c_float(1e-5), C.c_float(0), C.c_float(0), 1, C.c_float(0),
           None, vp(rout), vp(rstats))
    focal = vec_back(rout, 2 + Cn)[0]
    assert rec[1] == rec[2] + rec[3] == int(T.voxel_loss(z, y)[1].sum())        # K = n_valid: every valid voxel counts
    assert _rel_ok(out[0], focal), (out[0], focal)


@pytest.mark.parametrize("Cn", [3, 8])
def test_no_valid_voxel_gives_zero(Cn):
    d = dev()
    shape = (2, 5, 6, 7)
    V = int(np.prod(shape))
    z = np.random.default_rng(5).standard_normal((2, Cn) + shape[1:]).astype(np.float32)
    y = np.full(shape, 255, np.int32)
    y.flat[3] = Cn                               # out of range, not ignored: no part either
    yp, zt = _device_labels(y), t_from_ncdhw(z)
    ws, rec_p, out, rec, l = _ce_fwd(zt, yp, V, 10.0, None)
    assert out[0] == 0.0 and not out.any() and not rec.any() and np.all(l == -1.0)
    for acc in (0, 1):
        dz = t_from_ncdhw(np.full_like(z, 7.0))
        d.call("msk_topk_ce_bwd", zt.msk(), vp(yp), 255, None, vp(ws), vp(rec_p), C.c_float(1.0), acc, dz.msk())
        assert np.all(dz.numpy() == (7.0 if acc else 0.0))


@pytest.mark.parametrize("layout", ["dense", "dense_acc", "slice", "slice_acc"])
@pytest.mark.parametrize("case", CE_CASES, ids=CE_IDS)
def test_ce_backward_matches_statement(case, layout):
    d = dev()
    shape, Cn = case
    N = shape[0]
    V = int(np.prod(shape))
    rng = np.random.default_rng(SEEDS[CE_IDS[CE_CASES.index(case)]])
    z, y = _data(rng, shape, Cn)
    sliced, acc = layout.startswith("slice"), layout.endswith("acc")
    coef = 0.75
    for k, weighted in ((10.0, True), (50.0, False)):
        w = rng.uniform(0.5, 2, Cn).astype(np.float32) if weighted else None
        yp, wp = _device_labels(y), (vec(w) if weighted else None)
        zt, zwhole, _ = _tensor(z, sliced)
        ws, rec_p, out, rec, l = _ce_fwd(zt, yp, V, k, wp)
        valid = T.voxel_loss(z, y)[1]
        # the gradient built from the DOWNLOADED losses and record: membership is the forward's, no voxel may flip
        u = T.membership(l, rec[0], rec[6], valid)
        want = T.grad_from(z, y, u, rec[1], coef, weight=w)
        assert rec[1] >= 1 and abs(u.sum() - rec[1]) <= 1e-9 * rec[1]           # the weights of the members add up to K
        scale = np.abs(want).max()
        c0 = 1 if sliced else 0
        base = (rng.standard_normal((N, Cn + 4 if sliced else Cn) + shape[1:]) * scale).astype(np.float32)
        dwhole = t_from_ncdhw(base)
        dt = dwhole.channel_slice(c0, c0 + Cn) if sliced else dwhole
        under = base[:, c0:c0 + Cn]
        d.call("msk_topk_ce_bwd", zt.msk(), vp(yp), 255, vp(wp), vp(ws), vp(rec_p), C.c_float(coef), int(acc), dt.msk())
        full = dwhole.numpy()
        got = full[:, c0:c0 + Cn]
        if acc:
            assert _grad_ok(got, under.astype(np.float64) + want), (k, layout)
            assert np.abs(got - under.astype(np.float64) - want).max() <= 2e-5 * scale, (k, layout)
        else:
            assert _grad_ok(got, want), (k, layout)
            rows = np.moveaxis(got, 1, -1).reshape(V, Cn)
            assert not rows[~valid].any() and not rows[u == 0].any()            # exact zeros outside the selection
            assert np.all(np.abs(rows[u != 0]).max(axis=1) > 0)
        if sliced:        # the other channels of the wide buffer are untouched
            assert np.array_equal(full[:, :1], base[:, :1]) and np.array_equal(full[:, 1 + Cn:], base[:, 1 + Cn:])
        # end to end against the float64 statement, the voxels within float32 rounding of the threshold left out
        if not acc:
            ref = T.topk_ce(z, y, k, weight=w, coef=coef, dtype=np.float64)
            T64 = ref["record"][0]
            near = np.abs(ref["l"] - T64) <= 1e-5 * max(1.0, T64)
            print("k %g: %d voxel(s) near the threshold, K %d, tie_w %.3f" % (k, int(near.sum()), ref["K"], rec[6]))
            assert 1 <= near.sum() <= 4 and ref["K"] == rec[1]
            keep = np.repeat(~near[:, None], Cn, axis=1)
            g64 = np.moveaxis(ref["grad"], 1, -1).reshape(V, Cn)
            assert _grad_ok(rows[keep], g64[keep]), (k, layout)
        for p in (ws, rec_p, zwhole.ptr, dwhole.ptr, yp):
            dfree(p)


@pytest.mark.parametrize("Cn", [3, 8, 33])
def test_all_voxels_tied_share_the_weight(Cn):
    """all logits equal: every valid voxel has the same loss, T is that loss, and each carries tie_w = K / n_valid"""
    d = dev()
    shape = (2, 5, 6, 7)
    V = int(np.prod(shape))
    rng = np.random.default_rng(Cn)
    z = np.full((2, Cn) + shape[1:], 0.375, np.float32)
    y = rng.integers(0, Cn, shape).astype(np.int32)
    y[rng.random(shape) < 0.1] = 255
    yp, zt = _device_labels(y), t_from_ncdhw(z)
    ws, rec_p, out, rec, l = _ce_fwd(zt, yp, V, 10.0, None)
    valid = y.reshape(-1) != 255
    nv = int(valid.sum())
    K = T.k_of(nv, 10.0)
    assert np.unique(l[valid]).size == 1
    assert rec.tolist() == [float(l[valid][0]), K, 0, nv, 0.0, K, K / nv, K * float(l[valid][0])]
    assert _rel_ok(out[0], np.log(Cn))
    dz = t_from_ncdhw(np.full_like(z, 7.0))
    d.call("msk_topk_ce_bwd", zt.msk(), vp(yp), 255, None, vp(ws), vp(rec_p), C.c_float(2.0), 0, dz.msk())
    want = T.grad_from(z, y, np.where(valid, K / nv, 0.0), K, 2.0)
    got = dz.numpy()
    assert _grad_ok(got, want)
    rows = np.moveaxis(got, 1, -1).reshape(V, Cn)
    assert not rows[~valid].any() and np.unique(np.abs(rows[valid]).max(axis=1)).size == 1


@pytest.mark.parametrize("Cn", [3, 20])
def test_two_calls_give_the_same_bits(Cn):
    d = dev()
    shape = (2, 9, 10, 33)
    V = int(np.prod(shape))
    z, y = _data(np.random.default_rng(11), shape, Cn)
    yp, zt = _device_labels(y), t_from_ncdhw(z)
    runs = []
    for _ in range(2):
        ws, rec_p, out, rec, l = _ce_fwd(zt, yp, V, 10.0, None)
        dz = t_from_ncdhw(np.zeros_like(z))
        d.call("msk_topk_ce_bwd", zt.msk(), vp(yp), 255, None, vp(ws), vp(rec_p), C.c_float(1.0), 0, dz.msk())
        runs.append((out.view(np.uint32), rec.view(np.uint64), l.view(np.uint32), dz.numpy().view(np.uint32)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_argument_errors_launch_nothing():
    d = dev()
    from medicalseg_amd._lib import MskError
    rng = np.random.default_rng(3)
    n = 1000
    x = rng.standard_normal(n).astype(np.float32)
    xp, ws, rec = vec(x), dmalloc(_ws_bytes(n)), vec(np.full(16, 7.0))
    b = C.c_size_t(0)
    assert d.lib.msk_topk_workspace(C.c_long(0), C.byref(b)) != 0 and d.lib.msk_topk_workspace(C.c_long(1 << 31), C.byref(b)) != 0
    assert d.lib.msk_topk_workspace(C.c_long(5), None) != 0
    assert _ws_bytes(n) >= 4 * n + 3 * 2048 * 4 + 8 + 64
    bad = [((None, n, 1, ws, rec), "null"), ((xp, n, 1, None, rec), "null"), ((xp, n, 1, ws, None), "null"),
           ((xp, 0, 0, ws, rec), "n must be"), ((xp, 1 << 31, 1, ws, rec), "n must be"), ((xp, n, -1, ws, rec), "k must be"),
           ((xp, n, n + 1, ws, rec), "k must be"), ((xp + 2, n - 1, 1, ws, rec), "aligned"), ((xp, n, 1, ws + 4, rec), "aligned"),
           ((xp, n, 1, ws, rec + 4), "aligned"), ((xp, n, 1, xp, rec), "overlaps"), ((xp, n, 1, ws, ws + 4096), "overlaps")]
    for (a, nn, k, w, r), text in bad:
        with pytest.raises(MskError, match=text):
            d.call("msk_topk_select", vp(a), C.c_long(nn), C.c_long(k), vp(w), vp(r))
    assert np.all(vec_back(rec, 16) == 7.0)

    z3 = rng.standard_normal((1, 3, 4, 4, 4)).astype(np.float32)
    y = rng.integers(0, 3, (1, 4, 4, 4)).astype(np.int32)
    yp, t3 = _device_labels(y), t_from_ncdhw(z3)
    t1, t65 = t_from_ncdhw(z3[:, :1]), t_from_ncdhw(rng.standard_normal((1, 65, 4, 4, 4)).astype(np.float32))
    ws, out = dmalloc(_ws_bytes(64)), vec(np.full(5, 7.0))

    def fwd(zt=t3, labels=yp, k=10.0, w=ws, o=out, r=rec, wt=None):
        d.call("msk_topk_ce_fwd", zt.msk(), vp(labels), 255, vp(wt), C.c_float(k), vp(w), vp(o), vp(r))

    def bwd(zt=t3, labels=yp, w=ws, r=rec, dz=None, wt=None):
        d.call("msk_topk_ce_bwd", zt.msk(), vp(labels), 255, vp(wt), vp(w), vp(r), C.c_float(1.0), 0, dz.msk())

    dz3 = t_from_ncdhw(np.full_like(z3, 7.0))
    for kw, text in ((dict(zt=t1), r"\[2,64\]"), (dict(zt=t65), r"\[2,64\]"), (dict(k=0.0), "k_percent"), (dict(k=100.5), "k_percent"),
                     (dict(k=-3.0), "k_percent"), (dict(k=float("nan")), "k_percent"), (dict(labels=None), "null"), (dict(w=None), "null"),
                     (dict(o=None), "out"), (dict(r=None), "null"), (dict(w=ws + 8), "aligned"), (dict(w=t3.ptr), "overlaps"),
                     (dict(w=yp), "overlaps"), (dict(o=ws + 64), "overlaps"), (dict(r=ws + 64), "overlaps")):
        with pytest.raises(MskError, match=text):
            fwd(**kw)
    assert np.all(vec_back(out, 5) == 7.0) and np.all(vec_back(rec, 16) == 7.0)
    fwd()
    assert np.all(vec_back(out, 5) != 7.0)
    for shape in ((1, 2, 4, 4, 4), (1, 3, 4, 4, 5)):
        dz = t_from_ncdhw(np.full(shape, 7.0, np.float32))
        with pytest.raises(MskError, match="shape"):
            bwd(dz=dz)
        assert np.all(dz.numpy() == 7.0)
    for kw, text in ((dict(zt=t1, dz=t_from_ncdhw(z3[:, :1])), r"\[2,64\]"), (dict(w=None, dz=dz3), "null"), (dict(r=None, dz=dz3), "null"),
                     (dict(w=dz3.ptr, dz=dz3), "overlaps")):
        with pytest.raises(MskError, match=text):
            bwd(**kw)
    assert np.all(dz3.numpy() == 7.0)
    bwd(dz=dz3)
    assert np.all(dz3.numpy() != 7.0)


# ---- 4. the training stack --------------------------------------------------------------------------------------------------------
class _Capture:
    """Stands in as the producer of a logits tensor: records the gradient Scalar.backward hands over and passes it on."""
    num_outputs = 1

    def __init__(self, inner):
        self.inner, self.grads = inner, []

    def backward(self, g):
        self.grads.append(g.numpy())
        self.inner.backward(g)


def _labels(rng, shape, Cn):
    y = rng.integers(0, Cn, shape).astype(np.int32)
    y[rng.random(shape) < 0.1] = 255
    return y


def test_dicetopk_trains_vnet_and_hands_over_the_sum_of_both_gradients():
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import DiceTopKLoss, VNet
    from medicalseg_amd.utils import loss_computation
    d = dev()
    rng = np.random.default_rng(4)
    model = VNet(num_classes=3)
    model.train()
    opt = optim.Momentum(1e-2, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    losses = {"types": [DiceTopKLoss(lambda_dice=1.0, lambda_topk=0.5, k=10)], "coef": [2.0]}
    x = rng.standard_normal((1, 1, 16, 16, 16)).astype(np.float32)
    y = _labels(rng, (1, 16, 16, 16), 3)
    V = y.size
    values = []
    for step in range(2):
        logits = model(x)[0]
        cap = _Capture(logits.producer)
        logits.producer = cap
        yt = to_tensor(y)
        loss_list, dice = loss_computation([logits], yt, losses)
        assert len(loss_list) == 1 and np.asarray(dice).shape == (3,)
        loss = sum(loss_list)
        if step == 0:
            z = logits.numpy()
            sd, tk = R.region_loss(z, y, smooth=float(np.float32(1e-5))), T.topk_ce(z, y, 10)
            assert _rel_ok(float(loss), 2.0 * (sd["L_r"] + 0.5 * tk["loss"]))
        loss.backward()
        if step == 0:   # region backward (writes) plus top-k backward (adds), called by hand on the same logits
            settings = (255, 0, 0, 1, 0, 0, C.c_float(1e-5), C.c_float(0), C.c_float(0), 0, C.c_float(0))
            rout, rstats = vec(np.zeros(5)), dmalloc(17 * 8)
            d.call("msk_region_loss_fwd", logits.msk(), vp(yt.ptr), *settings, None, vp(rout), vp(rstats))
            ws, rec, out = dmalloc(_ws_bytes(V)), dmalloc(64), vec(np.zeros(5))
            d.call("msk_topk_ce_fwd", logits.msk(), vp(yt.ptr), 255, None, C.c_float(10.0), vp(ws), vp(out), vp(rec))
            dz = t_from_ncdhw(np.full_like(z, 7.0))
            d.call("msk_region_loss_bwd", logits.msk(), vp(yt.ptr), *settings, None, vp(rstats), C.c_float(0.0), C.c_float(2.0), 0,
                   dz.msk())
            d.call("msk_topk_ce_bwd", logits.msk(), vp(yt.ptr), 255, None, vp(ws), vp(rec), C.c_float(1.0), 1, dz.msk())
            assert len(cap.grads) == 1 and np.array_equal(cap.grads[0].view(np.uint32), dz.numpy().view(np.uint32))
            assert np.abs(cap.grads[0]).max() > 0
        opt.step()
        values.append(float(loss))
    assert np.all(np.isfinite(values)) and values[1] < values[0], values
    assert all(np.isfinite(p.numpy()).all() for p in model.parameters())


def test_three_iterations_from_the_dicetopk_yaml(tmp_path, capsys):
    """configs/synthetic/vnet_synthetic_ct_patch_dicetopk_96.yml shrunk to a 16^3 patch of 20 x 16 x 24 volumes"""
    from medicalseg_amd.core import train
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceTopKLoss
    src = open(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_dicetopk_96.yml")).read()
    for old, new in (("'../_base_/global_configs.yml'", "'%s'" % os.path.join(ROOT, "configs", "_base_", "global_configs.yml")),
                     ("iters: 100", "iters: 3"), ("num_samples: 16", "num_samples: 4"), ("size: [96, 96, 96]", "size: [16, 16, 16]")):
        assert old in src, old
        src = src.replace(old, new)
    assert src.count("shape: [144, 128, 160]") == 2
    src = src.replace("shape: [144, 128, 160]", "shape: [20, 16, 24]")
    p = tmp_path / "dicetopk_16.yml"
    p.write_text(src)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # data_root warning
        cfg = Config(str(p))
    losses = cfg.loss
    assert type(losses["types"][0]) is DiceTopKLoss and losses["types"][0].k == 10.0
    random.seed(0)
    train(cfg.model, cfg.train_dataset, optimizer=cfg.optimizer, save_dir=str(tmp_path / "o"), iters=cfg.iters,
          batch_size=cfg.batch_size, save_interval=10, log_iters=1, losses=losses)
    logged = [float(v) for v in re.findall(r"\[TRAIN\].*? loss: ([^,]+),", capsys.readouterr().out)]
    assert len(logged) == 3 and np.isfinite(logged).all() and all(v > 0 for v in logged), logged


def test_native_heads_score_each_head_against_its_own_pyramid_level():
    import pyramid_reference as P
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import DiceTopKLoss, VNetDeepSup
    from medicalseg_amd.models.losses.fused import TopKNode
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(8)
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    model.train()
    shape = (16, 16, 16)
    x = rng.standard_normal((1, 1) + shape).astype(np.float32)
    y = _labels(rng, (1,) + shape, 3)
    outs = model(x)
    heads = [(o.d, o.h, o.w) for o in outs]
    assert len(outs) == 4 and heads[0] == shape and len(set(heads)) > 1
    labels = [y] + P.label_pyramid(y, heads[1:])
    loss_list, dice = loss_computation(outs, to_tensor(y), {"types": [DiceTopKLoss() for _ in range(4)], "coef": [0.25] * 4})
    assert len(loss_list) == 4
    for o, lab, term in zip(outs, labels, loss_list):
        node = [t[1] for t in term.terms if type(t[1]) is TopKNode][0]
        assert tuple(node.labels.shape) == (1, o.d, o.h, o.w) and np.array_equal(node.labels.numpy(), lab)
        sd, tk = R.region_loss(o.numpy(), lab, smooth=float(np.float32(1e-5))), T.topk_ce(o.numpy(), lab, 10)
        assert _rel_ok(float(term), 0.25 * (sd["L_r"] + tk["loss"])), (o.shape, float(term))
    sum(loss_list).backward()
    assert all(np.isfinite(p.grad_numpy()).all() for p in model.parameters() if p.arena is not None and p.arena.grad_ptr is not None)

"""The loss kernels of all five families (CE + Dice: msk_loss_fwd / _bwd and their _ex forms; region: msk_region_loss_*; BCE:
msk_bce_*; top-k CE: msk_topk_ce_*; boundary: msk_boundary_loss_*) against their float64 statements, where the other parity tests
do not go:

  1. multi-round grids.  Every launcher caps its grid at a few workgroups per CU, so at training sizes a workgroup walks several
     tiles and, from its second tile on, reuses its LDS tile (and, in topk_bwd_k, the label and loss it prefetched).  The cases are
     sized from the device's CU count by the restated grid rules of tests/loss_forms_cases.py: some workgroups run one round more
     than the others and the last tile is ragged.  Each test asserts that premise first.
  2. every instantiation.  One small shape (a full and a ragged tile per group), every class count at a step of MSK_TPV_LADDER and
     at the boundaries between the forms (4|5, 32|33, 64), dense and as a channel slice, through all five families.
  3. CE + Dice at its numeric and degenerate edges: logits of +-100, every voxel ignored, an ignore_index inside [0, C).

Bounds: each family's own, unchanged, as stated at the top of tests/test_gpu_ops.py (test_loss_fwd_bwd, test_dice_options),
test_gpu_region_loss.py, test_gpu_bce.py, test_gpu_topk.py and test_gpu_boundary.py; tests/loss_forms_cases.py restates the shared
predicates.  Two bounds are this module's own.  (a) The target counts of the CE + Dice record are compared with ==: a thread adds
1.0f a handful of times, a workgroup's float32 sum stays below 2^24, the merge is float64.  (b) test_gpu_topk.py leaves the voxels
with |l64 - T64| <= 1e-5 max(1, T64) out of the end-to-end gradient comparison and allows 4 of them at its few thousand voxels; at a
million voxels the same window holds more (9 of K = 106 226 at most), so here their number is held to a thousandth of K (the
comparison then still covers 99.9 % of the selection), while the comparison against the gradient built from the downloaded losses and record excludes nothing.

No bound had to be widened.  Measured on an MI355X (256 CUs) at 1.18 M voxels (BCE: 2.36 M): CE within 1.5e-7 relative, per-class Dice
within 5e-8, the CE + Dice gradient within 9.2e-7 of max|g| (bound 5e-6 for the _ex forms), the region, top-k and boundary
gradients within 5.9e-7 of max|g| (bound 2e-5), the BCE gradient within 2.5e-7 of max|g| and 7.4e-8 relative L2 (bounds 1e-5, 1e-6)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import bce_reference as BR
import boundary_reference as B
import loss_forms_cases as L
import region_reference as R
import topk_reference as T
from helpers import dev, dfree, dmalloc, redzone_check, t_from_ncdhw, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

FIELDS = ("T", "K", "n_gt", "n_eq", "S_gt", "r", "tie_w", "S")


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def _seed(text):
    return zlib.crc32(text.encode())


def _device_labels(y):
    y = np.ascontiguousarray(y, np.int32)
    p = dmalloc(y.nbytes)
    dev().h2d(p, y)
    return p


def _logits(z, layout, extra=3):
    """the logits dense, or as channels 1 .. C of a buffer `extra` channels wider whose other channels hold large numbers (a
    wrong channel shows); -> (tensor to pass, the whole tensor)"""
    if layout == "dense":
        t = t_from_ncdhw(z)
        return t, t
    N, Cn, D, H, W = z.shape
    wide = np.random.default_rng(99).standard_normal((N, Cn + extra, D, H, W), dtype=np.float32) * np.float32(50)
    wide[:, 1:1 + Cn] = z
    tw = t_from_ncdhw(wide)
    return tw.channel_slice(1, 1 + Cn), tw


class _GradBuffer:
    """dlogits in the logits' layout, filled with random numbers of the gradient's size (what an adding pass adds to, and what
    a writing pass must overwrite everywhere)"""

    def __init__(self, shape5, layout, scale, extra=3, seed=5):
        N, Cn, D, H, W = shape5
        self.Cn, self.c0 = Cn, (1 if layout == "slice" else 0)
        wide = Cn + (extra if layout == "slice" else 0)
        self.base = np.random.default_rng(seed).standard_normal((N, wide, D, H, W), dtype=np.float32) * np.float32(scale)
        self.whole = t_from_ncdhw(self.base)
        self.t = self.whole.channel_slice(self.c0, self.c0 + Cn) if layout == "slice" else self.whole
        self.under = self.base[:, self.c0:self.c0 + Cn]

    def read(self):
        """the gradient channels; the other channels of a wide buffer must be untouched"""
        full = self.whole.numpy()
        c0, Cn = self.c0, self.Cn
        assert np.array_equal(full[:, :c0], self.base[:, :c0]) and np.array_equal(full[:, c0 + Cn:], self.base[:, c0 + Cn:])
        return full[:, c0:c0 + Cn]

    def free(self):
        dfree(self.whole.ptr)


def _free(*ptrs):
    for p in ptrs:
        if p:
            dfree(p)


# ---- one family each: forward and backward against the statement --------------------------------------------------------------------------
def _run_ce_dice(z, y, layout, ex, extra=3, ignore=255, coefs=(0.7, 1.3), tag=""):
    """msk_loss_fwd / msk_loss_bwd (ex: the _ex forms with dice_softmax = 1 and a dice_weight) -> out, record, gradient, statement"""
    d = dev()
    N, Cn, D, H, W = z.shape
    rng = np.random.default_rng(Cn + 7)
    w = rng.uniform(0.5, 2.0, Cn).astype(np.float32)
    dwt = rng.uniform(0.5, 2.0, Cn).astype(np.float32) if ex else None
    ref = L.ce_dice_reference(z, y, w, ignore, dice_softmax=ex, dice_weight=dwt)
    (zt, zwhole), yp, wv, dwp = _logits(z, layout, extra), _device_labels(y), vec(w), (vec(dwt) if ex else None)
    out, stats = vec(np.zeros(2 + Cn)), dmalloc((3 * Cn + 2) * 8)
    if ex:
        d.call("msk_loss_fwd_ex", zt.msk(), vp(yp), vp(wv), ignore, 1, vp(dwp), vp(out), vp(stats))
    else:
        d.call("msk_loss_fwd", zt.msk(), vp(yp), vp(wv), ignore, vp(out), vp(stats))
    o, st = vec_back(out, 2 + Cn).astype(np.float64), d.d2h(stats, (3 * Cn + 2,), np.float64)   # (float64: no float32 differences below)
    want = coefs[0] * ref["dce"] + coefs[1] * ref["ddice"]
    g = _GradBuffer(z.shape, layout, 1.0, extra)
    if ex:
        d.call("msk_loss_bwd_ex", zt.msk(), vp(yp), vp(wv), ignore, 1, vp(dwp), vp(stats), C.c_float(coefs[0]), C.c_float(coefs[1]),
               g.t.msk())
    else:
        d.call("msk_loss_bwd", zt.msk(), vp(yp), vp(wv), ignore, vp(stats), C.c_float(coefs[0]), C.c_float(coefs[1]), g.t.msk())
    got = g.read()
    ce_err = abs(o[0] - ref["ce"]) / max(abs(ref["ce"]), 1e-30)
    print("%s ce+dice%s C=%d %s: CE rel %.2e, Dice abs %.2e, per-class %.2e, gradient %.2e" % (
        tag, "_ex" if ex else "", Cn, layout, ce_err, abs(o[1] - ref["dice"]), L.rel_err(o[2:], ref["per"]), L.rel_err(got, want)))
    assert np.isfinite(o).all() and np.isfinite(st).all() and np.isfinite(got).all()
    assert abs(o[0] - ref["ce"]) < 2e-5 * abs(ref["ce"]) or (ref["ce"] == 0 and o[0] == 0)
    assert abs(o[1] - ref["dice"]) < 2e-6 and L.rel_err(o[2:], ref["per"]) < 2e-6
    assert np.array_equal(st[2 * Cn:3 * Cn], ref["T"])
    assert L.rel_err(got, want) < (5e-6 if ex else 2e-5)
    g.free()
    _free(zwhole.ptr, yp, wv, dwp, out, stats)
    return {"out": o, "stats": st, "grad": got, "ref": ref}


def _region_settings(activation, squared, batch, do_bg, tversky, focal_on, gamma):
    a, b = tversky if tversky else (0.0, 0.0)
    return (255, L.ACT[activation], int(squared), int(batch), int(do_bg), int(tversky is not None), C.c_float(L.SMOOTH), C.c_float(a),
            C.c_float(b), int(focal_on), C.c_float(gamma))


def _run_region(z, y, layout, combo, accs=(0, 1), extra=3, tag=""):
    d = dev()
    activation, sq, batch, bg, tv, focal_on, gamma, weighted = combo
    N, Cn, D, H, W = z.shape
    G = 1 if batch else N
    w = np.random.default_rng(Cn + 11).uniform(0.5, 2, Cn).astype(np.float32) if weighted else None
    settings = _region_settings(activation, sq, batch, bg, tv, focal_on, gamma)
    coef_f, coef_r = 0.75, 1.25
    ref = R.region_loss(z, y, activation, bool(sq), bool(batch), bool(bg), L.SMOOTH, tv, coef_r, coef_f * focal_on, gamma, w)
    (zt, zwhole), yp, wp = _logits(z, layout, extra), _device_labels(y), (vec(w) if weighted else None)
    out, stats = vec(np.zeros(2 + Cn)), dmalloc((5 * G * Cn + 2) * 8)
    d.call("msk_region_loss_fwd", zt.msk(), vp(yp), *settings, vp(wp), vp(out), vp(stats))
    o, st = vec_back(out, 2 + Cn), d.d2h(stats, (5 * G * Cn + 2,), np.float64)
    print("%s region C=%d %s %s batch=%d: L_f %.2e L_r %.2e" % (tag, Cn, layout, activation, batch,
          abs(float(o[0]) - ref["L_f"]) / max(abs(ref["L_f"]), 1e-30), abs(float(o[1]) - ref["L_r"]) / max(abs(ref["L_r"]), 1e-30)))
    assert L.rel_ok(o[0], ref["L_f"]), (o[0], ref["L_f"])
    assert L.rel_ok(o[1], ref["L_r"]), (o[1], ref["L_r"])
    assert L.rel_ok(o[2:], ref["dice"]), (o[2:], ref["dice"])
    TP, SP, ST, A, Bc = (st[k * G * Cn:(k + 1) * G * Cn].reshape(G, Cn) for k in range(5))
    assert L.rel_ok(TP, ref["TP"], 1e-6) and L.rel_ok(SP, ref["SP"], 1e-6)
    assert np.array_equal(ST, ref["ST"])
    assert L.rel_ok(A, ref["A"]) and L.rel_ok(Bc, ref["B"])
    if not bg and Cn > 1:
        assert not A[:, 0].any() and not Bc[:, 0].any()
    if focal_on:
        assert L.rel_ok(st[-2:], [ref["f_num"], ref["f_den"]], 1e-6)
    scale = np.abs(ref["grad"]).max()
    for acc in accs:
        g = _GradBuffer(z.shape, layout, scale, extra)
        d.call("msk_region_loss_bwd", zt.msk(), vp(yp), *settings, vp(wp), vp(stats), C.c_float(coef_f), C.c_float(coef_r), int(acc),
               g.t.msk())
        got = g.read()
        if acc:
            under = g.under.astype(np.float64)
            print("   added: max-abs / max|g| %.2e" % (np.abs(got - under - ref["grad"]).max() / scale))
            assert L.grad_ok(got, under + ref["grad"])
            assert np.abs(got - under - ref["grad"]).max() <= 2e-5 * scale
        else:
            print("   written: max-abs / max|g| %.2e" % (np.abs(got - ref["grad"]).max() / scale))
            assert L.grad_ok(got, ref["grad"])
            assert not np.moveaxis(got, 1, -1)[y == 255].any()                 # m = 0: exactly 0
        g.free()
    _free(zwhole.ptr, yp, wp, out, stats)


def _run_bce(z, y, layout, weight, pos_weight, accs=(0, 1), extra=3, tag=""):
    d = dev()
    N, Cn, D, H, W = z.shape
    pwm, pwv = (0, 0.0) if pos_weight is None else ((2, 0.0) if pos_weight == "dynamic" else (1, float(pos_weight)))
    ref_loss, ref_g = BR.bce(z, y, 255, weight, pos_weight)
    (zt, zwhole), yp = _logits(z, layout, extra), _device_labels(y)
    out, stats = vec(np.zeros(4)), dmalloc(8 * 8)
    d.call("msk_bce_fwd", zt.msk(), vp(yp), 255, 1 if weight == "dynamic" else 0, pwm, C.c_float(pwv), vp(out), vp(stats))
    loss, st = float(vec_back(out, 1)[0]), d.d2h(stats, (8,), np.float64)
    print("%s bce C=%d %s: loss rel %.2e" % (tag, Cn, layout, abs(loss - ref_loss) / max(abs(ref_loss), 1e-30)))
    assert L.bce_loss_ok(loss, ref_loss), (loss, ref_loss)
    assert st[5] == np.count_nonzero(y != 255)                                  # the counts are exact: mask, pos, neg
    if weight == "dynamic" or pos_weight == "dynamic":
        onehot = BR.targets(y, Cn)
        assert st[6] == np.count_nonzero(onehot == 1) and st[7] == np.count_nonzero(onehot == 0)
    coef = 0.75
    for acc in accs:
        g = _GradBuffer(z.shape, layout, np.abs(ref_g).max(), extra)
        d.call("msk_bce_bwd", zt.msk(), vp(yp), 255, vp(stats), C.c_float(coef), int(acc), g.t.msk())
        got = g.read()
        want = coef * ref_g + (g.under.astype(np.float64) if acc else 0.0)
        print("   acc %d: max-abs / max|g| %.2e, relative L2 %.2e" % (acc, np.abs(got - want).max() / np.abs(want).max(),
                                                                     np.linalg.norm(got - want) / np.linalg.norm(want)))
        assert L.bce_grad_ok(got, want)
        g.free()
    _free(zwhole.ptr, yp, out, stats)


def _ws_bytes(n):
    b = C.c_size_t(0)
    assert dev().lib.msk_topk_workspace(C.c_long(n), C.byref(b)) == 0
    return b.value


def _same_record(got, want, tag):
    for name, a, b in zip(FIELDS, got, want):
        assert a == b and np.signbit(a) == np.signbit(b), (tag, name, a, b)


def _topk_forward(zt, yp, wp, V, k):
    d = dev()
    ws, rec, out = dmalloc(_ws_bytes(V)), dmalloc(64), vec(np.full(2 + zt.c, 7.0))
    d.call("msk_topk_ce_fwd", zt.msk(), vp(yp), 255, vp(wp), C.c_float(k), vp(ws), vp(out), vp(rec))
    return ws, rec, out, vec_back(out, 2 + zt.c), d.d2h(rec, (8,), np.float64), d.d2h(ws, (V,), np.float32)


def _run_topk(z, y, layout, k=10.0, accs=(0, 1), extra=3, tag=""):
    d = dev()
    N, Cn, D, H, W = z.shape
    V = y.size
    w = np.random.default_rng(Cn + 13).uniform(0.5, 2, Cn).astype(np.float32)
    coef = 0.75
    ref = T.topk_ce(z, y, k, weight=w, coef=coef, dtype=np.float64)
    l32 = T.voxel_loss(z, y, weight=w, dtype=np.float32)[0]
    valid = ref["valid"]
    (zt, zwhole), yp, wp = _logits(z, layout, extra), _device_labels(y), vec(w)
    ws, rec_p, out_p, out, rec, l = _topk_forward(zt, yp, wp, V, k)
    assert np.array_equal(l == -1.0, ~valid)                                   # the sentinels are exactly the invalid voxels
    tol = 4.0 * float(np.abs(l32.astype(np.float64) - ref["l"]).max())
    err = float(np.abs(l.astype(np.float64) - ref["l"]).max())
    print("%s topk C=%d %s: l error %.3e (4 x float32 numpy %.3e), loss rel %.2e" % (
        tag, Cn, layout, err, tol, abs(float(out[0]) - ref["loss"]) / ref["loss"]))
    assert np.isfinite(l).all() and err <= tol and l[valid].min() >= 0
    K = T.k_of(int(valid.sum()), k)
    assert K == ref["K"] and K >= 1
    _same_record(rec, T.select(l, K), tag)
    assert abs(float(out[0]) - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and not out[1:].any()
    # the gradient built from the DOWNLOADED losses and record: membership is the forward's, no voxel may flip
    u = T.membership(l, rec[0], rec[6], valid)
    want = T.grad_from(z, y, u, rec[1], coef, weight=w)
    assert abs(u.sum() - rec[1]) <= 1e-9 * rec[1]
    scale = np.abs(want).max()
    for acc in accs:
        g = _GradBuffer(z.shape, layout, scale, extra)
        d.call("msk_topk_ce_bwd", zt.msk(), vp(yp), 255, vp(wp), vp(ws), vp(rec_p), C.c_float(coef), int(acc), g.t.msk())
        got = g.read()
        if acc:
            under = g.under.astype(np.float64)
            print("   added: max-abs / max|g| %.2e" % (np.abs(got - under - want).max() / scale))
            assert L.grad_ok(got, under + want)
            assert np.abs(got - under - want).max() <= 2e-5 * scale
        else:
            print("   written: max-abs / max|g| %.2e" % (np.abs(got - want).max() / scale))
            assert L.grad_ok(got, want)
            rows = np.moveaxis(got, 1, -1).reshape(V, Cn)
            assert not rows[~valid].any() and not rows[u == 0].any()            # exact zeros outside the selection
            assert np.all(np.abs(rows[u != 0]).max(axis=1) > 0)
            # end to end against the float64 statement, the voxels within float32 rounding of the threshold left out
            T64 = ref["record"][0]
            near = np.abs(ref["l"] - T64) <= 1e-5 * max(1.0, T64)
            print("   %d voxel(s) near the threshold, K %d" % (int(near.sum()), ref["K"]))
            assert 1 <= near.sum() <= max(4, ref["K"] // 1000)
            g64 = np.moveaxis(ref["grad"], 1, -1).reshape(V, Cn)
            assert L.grad_ok(rows[~near], g64[~near])
        g.free()
    _free(zwhole.ptr, yp, wp, ws, rec_p, out_p)


def _run_boundary(z, y, layout, accs=(0, 1), extra=3, tag=""):
    d = dev()
    N, Cn, D, H, W = z.shape
    S = L.class_set(Cn)
    mask = sum(1 << c for c in S)
    phi = np.random.default_rng(Cn + 17).standard_normal((N, len(S), D, H, W), dtype=np.float32) * np.float32(3)
    ref = B.boundary_loss(z, y, S, phi=phi)
    (zt, zwhole), yp, php = _logits(z, layout, extra), _device_labels(y), vec(phi)
    out_p, stats_p = vec(np.full(2 + Cn, 7.0)), dmalloc((3 + Cn) * 8)
    d.call("msk_boundary_loss_fwd", zt.msk(), vp(yp), 255, C.c_uint64(mask), vp(php), vp(out_p), vp(stats_p))
    out, stats = vec_back(out_p, 2 + Cn), d.d2h(stats_p, (3 + Cn,), np.float64)
    A = ref["abs"]
    print("%s boundary C=%d %s: |L diff| / A %.2e, A rel %.2e, per class %.2e" % (
        tag, Cn, layout, abs(float(out[0]) - ref["loss"]) / A, abs(float(out[1]) - A) / A,
        np.abs(out[2:].astype(np.float64) - ref["per_class"]).max() / A))
    assert stats[0] == ref["n_valid"]                                           # exact
    outside = [c for c in range(Cn) if c not in S]
    assert not out[2:][outside].any() and not stats[3:][outside].any()          # exact zeros outside the set
    assert abs(float(out[0]) - ref["loss"]) <= 1e-5 * A
    assert abs(float(out[1]) - A) <= 1e-5 * A
    assert np.abs(out[2:].astype(np.float64) - ref["per_class"]).max() <= 1e-5 * A
    assert np.abs(stats[1:] - ref["stats"][1:]).max() <= 1e-5 * ref["stats"][2]
    flat_y = y.reshape(-1)
    invalid = (flat_y == 255) | (flat_y < 0) | (flat_y >= Cn)
    coef = 1.5
    want = coef * ref["grad"]
    scale = np.abs(want).max()
    for acc in accs:
        g = _GradBuffer(z.shape, layout, scale, extra)
        d.call("msk_boundary_loss_bwd", zt.msk(), vp(yp), 255, C.c_uint64(mask), vp(php), vp(stats_p), C.c_float(coef), int(acc), g.t.msk())
        got = g.read()
        rows = np.moveaxis(got, 1, -1).reshape(-1, Cn)
        if acc:
            print("   added: max-abs / max|g| %.2e" % (np.abs(got - g.under.astype(np.float64) - want).max() / scale))
            assert L.grad_ok(got, g.under.astype(np.float64) + want)
            assert np.array_equal(rows[invalid], np.moveaxis(g.under, 1, -1).reshape(-1, Cn)[invalid])   # untouched at invalid voxels
        else:
            print("   written: max-abs / max|g| %.2e" % (np.abs(got - want).max() / scale))
            assert L.grad_ok(got, want)
            assert not rows[invalid].any()                                      # exactly 0
            assert np.abs(got[:, outside]).max() > 0                            # classes outside the set do get a gradient
        g.free()
    _free(zwhole.ptr, yp, php, out_p, stats_p)


# ---- 1. multi-round grids ---------------------------------------------------------------------------------------------------------------
def _multi(case):
    """shape and data of a multi-round case on this device, its premise asserted"""
    cu = dev().get_option("num_cu")
    shape = L.multi_round_shape(case, cu)
    p = L.check_premise(case, shape, cu)
    print("%s: %d CUs, shape %s, %s pass: %d workgroup(s) x %d group(s), %d tiles of %d, rounds %d..%d" % (
        case["id"], cu, shape, L.sized_pass(case), p["wg"], p["groups"], p["tiles"], p["tile"], p["min_rounds"], p["max_rounds"]))
    z, y = L.make_data(np.random.default_rng(_seed(case["id"])), shape, case["C"])
    return shape, z, y


def _of(family):
    return [c for c in L.MULTI if c["family"] == family]


CE_DICE_MULTI = [(c, ex) for c in _of("ce_dice") for ex in ((False,) if c["layout"] == "slice" else (False, True))]


@pytest.mark.parametrize("case,ex", CE_DICE_MULTI, ids=["%s%s" % (c["id"], "-ex" if ex else "") for c, ex in CE_DICE_MULTI])
def test_ce_dice_over_several_rounds(case, ex):
    shape, z, y = _multi(case)
    _run_ce_dice(z, y, case["layout"], ex, case["extra"], tag=case["id"])


@pytest.mark.parametrize("case", _of("region"), ids=lambda c: c["id"])
def test_region_over_several_rounds(case):
    shape, z, y = _multi(case)
    combo = list(L.REGION_MULTI[case["act"]])
    combo[2] = case["batch"]
    dense = case["layout"] == "dense"
    f = L.form("region", case["C"], dense, L.seg_aligned("region", shape, case["C"], bool(case["batch"])))
    if case["mod4"] is not None:
        assert f == ((4, 2) if case["mod4"] == 0 else (4, 0))                   # group offsets on a quad (flat tile) and off it
    _run_region(z, y, case["layout"], tuple(combo), case["acc"], case["extra"], tag=case["id"])


@pytest.mark.parametrize("case", _of("bce"), ids=lambda c: c["id"])
def test_bce_over_several_rounds(case):
    shape, z, y = _multi(case)
    if case["C"] == 3:
        assert (shape[3] % L.BCE_TILE) * 3 % 4 != 0                             # the ragged tile ends in the scalar tail behind the quads
    _run_bce(z, y, case["layout"], "dynamic", "dynamic" if case["C"] == 1 else 2.5, case["acc"], case["extra"], tag=case["id"])


@pytest.mark.parametrize("case", _of("topk"), ids=lambda c: c["id"])
def test_topk_over_several_rounds(case):
    shape, z, y = _multi(case)
    _run_topk(z, y, case["layout"], 10.0, case["acc"], case["extra"], tag=case["id"])


@pytest.mark.parametrize("case", _of("boundary"), ids=lambda c: c["id"])
def test_boundary_over_several_rounds(case):
    shape, z, y = _multi(case)
    _run_boundary(z, y, case["layout"], case["acc"], case["extra"], tag=case["id"])


def test_topk_backward_skips_empty_tiles_in_the_first_and_in_a_later_round():
    """Members in a few chosen tiles only: everywhere else topk_bwd_k takes its __syncthreads_or branch (no softmax, zeros stored
    or nothing at all), in tiles next to tiles that do have members, in the first round and in the second, and the label and loss
    a workgroup prefetched for its next tile cross from a tile of one kind to one of the other in both directions."""
    d = dev()
    case, Cn = L.CONCENTRATED, L.CONCENTRATED["C"]
    cu = d.get_option("num_cu")
    shape = L.multi_round_shape(case, cu)
    p = L.check_premise(case, shape, cu)
    G, ntile, V = p["wg"], p["tiles"], p["vox"]
    tiles = L.concentrated_tiles(G, ntile)
    z, y = L.concentrated_data(np.random.default_rng(_seed(case["id"])), shape, Cn, tiles)
    valid = T.voxel_loss(z, y)[1]
    in_tiles = np.zeros(V, bool)
    for t in tiles:
        in_tiles[t * L.TPV_TILE:(t + 1) * L.TPV_TILE] = True
    k = 100.0 * 0.5 * np.count_nonzero(valid & in_tiles) / np.count_nonzero(valid)
    coef = 0.75
    ref = T.topk_ce(z, y, k, coef=coef)
    starts = np.arange(0, V, L.TPV_TILE)
    has = np.add.reduceat((ref["u"] != 0).astype(np.int64), starts) > 0         # the reference's membership, tile by tile
    empty, first = ~has, np.arange(ntile) < G
    assert 1 <= ref["K"] < np.count_nonzero(valid & in_tiles) and np.array_equal(np.flatnonzero(has), tiles)
    beside = np.zeros(ntile, bool)                                              # empty tiles with a member tile as a neighbour
    beside[1:] |= has[:-1]
    beside[:-1] |= has[1:]
    beside &= empty
    assert (beside & first).any() and (beside & ~first).any() and (empty & first).sum() > 1 and (empty & ~first).sum() > 1
    second = np.arange(G, min(2 * G, ntile))                                    # tile b + G follows tile b in workgroup b
    kinds = {(bool(has[t - G]), bool(has[t])) for t in second}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    zt, yp = t_from_ncdhw(z), _device_labels(y)
    ws, rec_p, out_p, out, rec, l = _topk_forward(zt, yp, None, V, k)
    assert abs(float(out[0]) - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and rec[1] == ref["K"]
    u = T.membership(l, rec[0], rec[6], valid)
    assert np.array_equal(np.add.reduceat((u != 0).astype(np.int64), starts) > 0, has)   # the device's members sit in the same tiles
    want = T.grad_from(z, y, u, rec[1], coef)
    scale = np.abs(want).max()
    vox_empty = np.repeat(empty, L.TPV_TILE)[:V]
    for acc in (0, 1):
        g = _GradBuffer(z.shape, "dense", scale)
        d.call("msk_topk_ce_bwd", zt.msk(), vp(yp), 255, None, vp(ws), vp(rec_p), C.c_float(coef), acc, g.t.msk())
        got = g.read()
        rows = np.moveaxis(got, 1, -1).reshape(V, Cn)
        old = np.moveaxis(g.under, 1, -1).reshape(V, Cn)
        if acc:
            assert np.array_equal(rows[vox_empty].view(np.uint32), old[vox_empty].view(np.uint32))   # the old values, bit for bit
            assert L.grad_ok(got, g.under.astype(np.float64) + want)
            assert np.abs(got - g.under.astype(np.float64) - want).max() <= 2e-5 * scale
        else:
            assert not rows[vox_empty].view(np.uint32).any()                    # exact zeros (+0.0) in the empty tiles
            assert L.grad_ok(got, want) and not rows[u == 0].any()
            assert np.all(np.abs(rows[u != 0]).max(axis=1) > 0)
        g.free()
    _free(zt.ptr, yp, ws, rec_p, out_p)


# ---- 2. every instantiation ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_data(Cn, shape=L.SWEEP_SHAPE):
    z, y = L.make_data(np.random.default_rng(700 + Cn), shape, Cn)
    for a in (z, y):
        a.setflags(write=False)
    return z, y


SWEEP = [(f, c, lay) for f in L.FAMILIES for c in L.sweep_classes(f) for lay in L.SWEEP_LAYOUTS]


@pytest.mark.parametrize("family,Cn,layout", SWEEP, ids=["%s-C%d-%s" % s for s in SWEEP])
def test_every_class_count_dense_and_as_a_slice(family, Cn, layout):
    z, y = _sweep_data(Cn)
    dense = layout == "dense"
    tag = "form %s" % (L.form(family, Cn, dense, L.seg_aligned(family, L.SWEEP_SHAPE, Cn)),)
    if family == "ce_dice":
        for ex in (False, True):
            _run_ce_dice(z, y, layout, ex, tag=tag)
    elif family == "region":
        for combo in L.REGION_SWEEP:
            _run_region(z, y, layout, combo, tag="form %s" % (L.form(family, Cn, dense, L.seg_aligned(family, L.SWEEP_SHAPE, Cn, bool(combo[2]))),))
    elif family == "bce":
        _run_bce(z, y, layout, "dynamic", 2.5, tag=tag)
    elif family == "topk":
        _run_topk(z, y, layout, tag=tag)
    else:
        _run_boundary(z, y, layout, tag=tag)


@pytest.mark.parametrize("layout", L.SWEEP_LAYOUTS)
@pytest.mark.parametrize("Cn,shape", L.BCE_EDGE, ids=["C%d" % c for c, _ in L.BCE_EDGE])
def test_bce_element_index_up_to_65535(Cn, shape, layout):
    """1024 + 1 voxels: a full tile, whose elements an element finds its voxel for through the float reciprocal (at 64 classes
    the index runs to 65 535, the end of elem_voxel's exactness claim), and a tile of one voxel"""
    z, y = _sweep_data(Cn, shape)
    _run_bce(z, y, layout, "dynamic", "dynamic", tag="1025 voxels")


# ---- 3. CE + Dice at its edges -----------------------------------------------------------------------------------------------------------
EDGE_FORMS = [(3, "dense"), (8, "dense"), (5, "slice"), (40, "dense")]         # ST 2, ST 1, ST 0, lane per class
EDGE_IDS = ["C%d-%s" % f for f in EDGE_FORMS]


@pytest.mark.parametrize("Cn,layout", EDGE_FORMS, ids=EDGE_IDS)
def test_ce_dice_extreme_logits(Cn, layout):
    """+-100: saturated at the label, saturated at another class, all equal at +100; in the full tile and in the ragged one"""
    z0, y0 = _sweep_data(Cn)
    z, y = z0.copy(), y0.copy()
    for n, (d_, h, w0) in enumerate(((1, 2, 3), (4, 5, 1))):                    # sample 0: voxel 84 ..; sample 1: voxel 298 .. (ragged tile)
        z[n, :, d_, h, w0] = -100.0
        z[n, 1, d_, h, w0] = 100.0
        y[n, d_, h, w0] = 1
        z[n, :, d_, h, w0 + 1] = -100.0
        z[n, 0, d_, h, w0 + 1] = 100.0
        y[n, d_, h, w0 + 1] = Cn - 1
        z[n, :, d_, h, w0 + 2] = 100.0
        y[n, d_, h, w0 + 2] = 0
    for ex in (False, True):
        res = _run_ce_dice(z, y, layout, ex, tag="extreme")
        assert np.isfinite(res["out"]).all() and np.isfinite(res["stats"]).all() and np.isfinite(res["grad"]).all()


@pytest.mark.parametrize("Cn,layout", EDGE_FORMS, ids=EDGE_IDS)
def test_ce_dice_every_voxel_ignored(Cn, layout):
    """the CE term is 0 and its gradient exactly 0; the Dice term (all-zero targets, p^2 summed over every voxel: loss 1 and, the
    intersections being 0, a zero gradient) still matches"""
    z = _sweep_data(Cn)[0]
    y = np.full(L.SWEEP_SHAPE, 255, np.int32)
    for ex in (False, True):
        res = _run_ce_dice(z, y, layout, ex, tag="all ignored")
        assert res["out"][0] == 0.0 and not res["stats"][3 * Cn:].any()
        assert res["stats"][Cn:2 * Cn].min() > 0 and not res["stats"][2 * Cn:3 * Cn].any()   # sum p^2 is there, the targets are empty
        res = _run_ce_dice(z, y, layout, ex, coefs=(1.0, 0.0), tag="all ignored, CE alone")
        assert not res["grad"].any()


@pytest.mark.parametrize("Cn,layout", EDGE_FORMS, ids=EDGE_IDS)
def test_ce_dice_ignore_index_inside_the_class_range(Cn, layout):
    """ignore_index = 0: CE skips those voxels, Dice counts them (what the statistics kernels do today)"""
    z, y = _sweep_data(Cn)
    n0 = np.count_nonzero(y == 0)
    assert n0 > 0
    for ex in (False, True):
        res = _run_ce_dice(z, y, layout, ex, ignore=0, tag="ignore_index 0")
        assert res["stats"][2 * Cn] == n0                                        # the Dice target of class 0 counts them
        res = _run_ce_dice(z, y, layout, ex, ignore=0, coefs=(1.0, 0.0), tag="ignore_index 0, CE alone")
        rows = np.moveaxis(res["grad"], 1, -1)
        assert not rows[y == 0].any() and rows[y == 1].any()                     # CE skips them

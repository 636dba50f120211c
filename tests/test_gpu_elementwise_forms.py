"""The per-voxel kernels of msk_elementwise.hip, form by form, at sizes where their loops take a second trip and a ragged tail,
against the float64 statement of tests/elementwise_reference.py.

Every entry point picks one of several kernel forms from the channel count, the voxel stride and the alignment of its
tensors (FORMS below; the tests re-evaluate the dispatch predicates of the source in Python, so a case cannot drift onto
another form unnoticed), and sizes its grid from three options.  The sweep runs each form under

    a   the product geometry (ew_cap 4, reduce_cap 4, reduce_vpl 8)
    b   ew_cap 1, reduce_cap 1, reduce_vpl 1      many blocks, many partial records
    c   ew_cap 1, reduce_cap 1, reduce_vpl 999    one or a few blocks, long dependent loops
    d   reduce_vpl 1 alone                        more than 256 partial records: the 256-lane form of the merges

with voxel counts computed from the chip's CU count so that under (b) some thread runs its loop body twice and some thread
takes the single-voxel / ragged tail while another does not.  Tolerances are those of tests/test_gpu_ops.py
(test_bn_stats_and_affine_act, test_affine_act_join_fwd_bwd, test_copy_scale_channel_sum_argmax_layout, test_elu_fwd_bwd) and
tests/test_gpu_wbf.py for the same quantities; per-element outputs must in addition be bit-identical across the geometries
(which thread computes an element is no part of its arithmetic).

The amax side outputs (the maxima the fp16 two-piece convolutions scale their operands by) are tested with a PLANTED maximum:
one element 1000 times the bulk at each position a kernel could skip (thread-trip boundaries, the second voxel of a pair, the
tail, every lane of a quad, every slot of a float4 triple, the last channel of a slice), then producer -> consumer agreement,
the low end of the scale rule, and the ring the arrays come from."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import elementwise_reference as R
from helpers import dev, dfree, dmalloc, redzone_check, rel_err, t_empty, t_from_ncdhw, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

from oracle import vnet_numpy as O  # noqa: E402

F4 = np.float32
PAD = F4(1e30)          # finite: what a kernel wrongly reads from a neighbouring slice reaches fmaxf (NaN would be dropped)
GEOMS = {"a": {}, "b": {"ew_cap": 1, "reduce_cap": 1, "reduce_vpl": 1}, "c": {"ew_cap": 1, "reduce_cap": 1, "reduce_vpl": 999},
         "d": {"reduce_vpl": 1}}
GEOM_KEYS = ("ew_cap", "reduce_cap", "reduce_vpl", "dense12")


@contextlib.contextmanager
def geometry(name):
    """options of geometry `name`; the values found are put back"""
    d = dev()
    old = {k: d.get_option(k) for k in GEOM_KEYS}
    try:
        for k, v in GEOMS[name].items():
            d.set_option(k, v)
        yield {**old, **GEOMS[name]}
    finally:
        for k, v in old.items():
            d.set_option(k, v)


@pytest.fixture(autouse=True)
def _amax_requests_outside_a_step():
    """These tests take thousands of amax arrays straight from the ring.  device.ActivationArena.reset() counts the requests
    between two model forwards as one training step's and refuses more than a ring half, so the count starts afresh after
    each test: the next model test in the process measures its own steps only."""
    yield
    dev().arena.restart_ring_count()


def _null():
    from medicalseg_amd._lib import NULL_TENSOR
    return NULL_TENSOR


def _desc(K):
    from medicalseg_amd._lib import MskConvDesc
    return MskConvDesc(K, K, K, 1, 1, 1, K // 2, K // 2, K // 2)


def _conv_tol(K):
    return 8e-6 * np.sqrt(K / 1000.0 + 1.0)


# ---- channels-last buffers ------------------------------------------------------------------------------------------------------
class Buf:
    """[V, C] float32 on the device, dense or as channels c0 .. c0 + C of a [V, ld] parent whose other channels hold PAD"""

    def __init__(self, a, ld=None, c0=0, n=1):
        a = np.asarray(a, dtype=F4)
        self.V, self.C = a.shape
        self.ld, self.c0 = ld or self.C, c0
        wide = a
        if ld:
            wide = np.full((self.V, ld), PAD, F4)
            wide[:, c0:c0 + self.C] = a
        self.parent = t_from_ncdhw(np.ascontiguousarray(wide.reshape(n, self.V // n, self.ld).transpose(0, 2, 1)).reshape(n, self.ld, 1, 1, self.V // n))
        self.t = self.parent.channel_slice(c0, c0 + self.C) if ld else self.parent

    @staticmethod
    def empty(V, Cn, ld=None, c0=0, n=1):
        """an output: NaN where the kernel has to write"""
        return Buf(np.full((V, Cn), np.nan, F4), ld, c0, n)

    def msk(self):
        return self.t.msk()

    def wide(self):
        return dev().d2h(self.parent.ptr, (self.V, self.ld), F4)

    def host(self):
        w = self.wide()
        pads = np.delete(w, np.s_[self.c0:self.c0 + self.C], axis=1)
        assert np.all(pads.view(np.uint32) == PAD.view(np.uint32)), "a neighbouring channel of the wide buffer was written"
        return np.ascontiguousarray(w[:, self.c0:self.c0 + self.C])

    def free(self):
        dfree(self.parent.ptr)

    def poke(self, v, c, value):
        dev().h2d(self.t.ptr + 4 * (int(v) * self.ld + int(c)), np.array([value], F4))


def _take(buf):
    """host copy of an output that is not needed on the device any more"""
    h = buf.host()
    buf.free()
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=F4).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _amax(ptr, n=1):
    return dev().d2h(ptr, (n, 64), F4)


# ---- the dispatch predicates of msk_elementwise.hip, restated ----------------------------------------------------------------------
def _pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def _vec4_ok(t):
    return t is None or (t.c % 4 == 0 and t.ld % 4 == 0 and t.ptr % 16 == 0)


def _d12_ok(t):
    return t is None or (t.ld == t.c and t.ptr % 16 == 0)


def _d12_shape(x):
    return x.c in (1, 2, 3, 6) and (x.voxels * x.c) % 12 == 0


def _elementwise_form(x, others, res, d12_allowed=True):
    """msk_affine_act_fwd / _join_fwd (d12_allowed False: alpha_in or out2) and msk_affine_act_bwd_apply: x, the other
    full-size tensors (out | dout, dx, dres), the residual.  The mirror of ew_select in msk_elementwise.hip; the comment block
    "Which form of a pass runs" above it states the order of the forms and why it agrees with _reduce_form's."""
    v4 = all(_vec4_ok(t) for t in [x] + others) and (res is None or res.c != x.c or _vec4_ok(res))
    if (dev().get_option("dense12") and not v4 and d12_allowed and _d12_shape(x) and all(_d12_ok(t) for t in [x] + others)
            and (res is None or (res.c == x.c and _d12_ok(res)))):
        return "d12"
    cq = x.c // 4
    if v4 and cq >= 1 and cq & (cq - 1) == 0 and cq <= 256:
        return "cs"
    return "k4" if v4 else "k1"


def _reduce_form(x, dout, res):
    """msk_affine_act_bwd_reduce_ex; with dout None: msk_bn_stats.  The mirror of reduce_plan's form in msk_elementwise.hip
    (same comment block: "Which form of a pass runs")."""
    o = [t for t in (x, dout) if t is not None]
    if x.c % 4 == 0 and x.c // 4 <= 256 and all(_vec4_ok(t) for t in o) and (res is None or res.c != x.c or _vec4_ok(res)):
        return "v4"
    if dev().get_option("dense12") and _d12_shape(x) and all(_d12_ok(t) for t in o) and (res is None or (res.c == x.c and _d12_ok(res))):
        return "d12"
    return "scalar"


def _copy_form(src, dst):
    """msk_copy_scale: pass_v4 of the same block, the K4 / K1 half of ew_select"""
    return "k4" if _vec4_ok(src) and _vec4_ok(dst) else "k1"


def _ew_threads(total, cu, cap):
    """threads of a grid-stride kernel over `total` items (msk_ew_blocks)"""
    return 256 * max(1, min((total + 255) // 256, cu * cap))


def _reduce_blocks(voxels, vpb, cu, g):
    return max(1, min((voxels + vpb * g["reduce_vpl"] - 1) // (vpb * g["reduce_vpl"]), cu * g["reduce_cap"]))


# name: (C, ld, c0, form of the forward / backward-apply kernels, form of the backward reduction = of the statistics)
FORMS = {
    "cs16": (16, None, 0, "cs", "v4"),             # channel-stationary float4: C / 4 a power of two
    "cs32": (32, None, 0, "cs", "v4"),
    "cs256": (256, None, 0, "cs", "v4"),           # one quad column per lane: VL = 4 voxel lanes in the reductions
    "cs16_in32": (16, 32, 16, "cs", "v4"),         # the second half of a concat buffer: ld > c, aligned
    "k4_20": (20, None, 0, "k4", "v4"),            # 5 quads: element-indexed float4, 64-bit division; QCB = 8 with 3 idle quad lanes
    "k4_24": (24, None, 0, "k4", "v4"),
    "k1_5": (5, None, 0, "k1", "scalar"),
    "k1_16_in20": (16, 20, 2, "k1", "scalar"),     # channels 2 .. 18 of a 20-wide buffer: 8 bytes off the float4 alignment
    "d12_3": (3, None, 0, "d12", "d12"),           # dense, voxels * C % 12 == 0: float4 triples
    "d12_6": (6, None, 0, "d12", "d12"),
    "k1_3": (3, None, 0, "k1", "scalar"),          # dense 3 channels at a voxel count the triples decline
}


def _voxels(form, cu):
    """the smallest size at which, with one block per CU (geometry b), some thread runs its body twice and some thread takes the
    ragged / single-voxel tail while another does not"""
    Cn, _, _, ew, _ = FORMS[form]
    T = 256 * cu
    if ew == "cs":
        return 9 * (T // (Cn // 4)) // 2 + 17      # 4.5 voxel strides: two pair iterations for every thread, a single-voxel tail for half of them
    if ew == "k4":
        return 23 * T // (10 * (Cn // 4)) + 3      # 2.3 grid strides of quads
    if ew == "d12":
        return (23 * T // 10 + 5) * 12 // Cn       # 2.3 grid strides of triples
    V = 23 * T // (10 * Cn) + 3
    while form == "k1_3" and (V * Cn) % 12 == 0:
        V += 1
    return V


def _positions(form, V, cu, g, kind="ew", ew=None):
    """(voxel, channel) places a kernel form could skip: first and last element, the last element of the first thread trip and the
    first of the second, the second voxel of a pair, the end of the tail, every lane of a quad / slot of a triple, the last channel.
    kind "ew": the grid-stride kernels; "red": the block-partitioned reductions (float4 form)."""
    Cn = FORMS[form][0]
    ew = ew or FORMS[form][3]
    pos = [(0, 0), (V - 1, Cn - 1), (V // 2, Cn - 1)]
    if kind == "red":
        VL = 256 // _pow2ceil(Cn // 4)
        nb = _reduce_blocks(V, VL, cu, g)
        per = (V + nb - 1) // nb
        last0 = min(per, V) - 1
        for i, v in enumerate([VL - 1, VL, 2 * VL - 1, 2 * VL, last0, last0 + 1, (nb - 1) * per, V - 2]):
            if 0 <= v < V:
                pos.append((v, (5 * i + 3) % Cn))
        pos += [(min(VL + 1, V - 1), Cn - 4 + j) for j in range(4)]      # the lanes of a quad, in the second voxel of a pair
    elif ew == "cs":
        cq = Cn // 4
        vs = _ew_threads(V * cq // 2, cu, g["ew_cap"]) // cq
        for i, v in enumerate([vs - 1, vs, 2 * vs - 1, 2 * vs, 3 * vs, 4 * vs - 1, 4 * vs, V - 2]):     # pair 1, pair 2, tail
            if 0 <= v < V:
                pos.append((v, (7 * i + 3) % Cn))
        pos += [(min(vs + 1, V - 1), Cn - 4 + j) for j in range(4)]
    elif ew == "d12":
        groups = V * Cn // 12
        T = _ew_threads(groups, cu, g["ew_cap"])
        for i, gi in enumerate([T - 1, T, 2 * T - 1, 2 * T]):
            if 0 <= gi < groups:
                pos.append(divmod(12 * gi + (5 * i + 1) % 12, Cn))
        pos += [divmod(12 * min(T, groups - 1) + s, Cn) for s in range(12)]
        pos += [divmod(12 * (groups - 1) + s, Cn) for s in (0, 7, 11)]
    else:
        w = 4 if ew == "k4" else 1
        cv = Cn // w
        T = _ew_threads(V * cv, cu, g["ew_cap"])
        for i in [T - 1, T, 2 * T - 1, 2 * T, V * cv - 2]:
            if 0 <= i < V * cv:
                v, cg = divmod(i, cv)
                pos.append((v, cg * w + i % w))
        pos += [(V // 3, Cn - min(Cn, 4) + j) for j in range(min(Cn, 4))]
    return list(dict.fromkeys((int(v), int(c)) for v, c in pos))


def _res_array(rng, kind, V, Cn):
    if kind == "none":
        return None
    return rng.standard_normal((V, {"full": Cn, "one": 1, "div": max(Cn // 4, 1)}[kind])).astype(F4)


# ==== A. launch-geometry sweep ==========================================================================================================
CHAIN_CASES = [("cs16", "none"), ("cs16", "full"), ("cs16", "one"), ("cs16", "div"), ("cs32", "full"), ("cs256", "full"), ("cs256", "one"),
               ("cs16_in32", "full"), ("k4_20", "full"), ("k4_20", "one"), ("k4_20", "div"), ("k4_24", "none"), ("k1_5", "full"),
               ("k1_5", "one"), ("k1_16_in20", "full"), ("k1_16_in20", "div"), ("d12_3", "full"), ("d12_3", "none"), ("d12_6", "full"),
               ("k1_3", "full")]


@pytest.mark.parametrize("form,reskind", CHAIN_CASES)
def test_bn_affine_act_chain_under_every_geometry(form, reskind):
    """msk_bn_stats, msk_affine_act_fwd, msk_affine_act_bwd_reduce_ex (with maxes in the float4 form), msk_affine_act_bwd_apply_amax
    (bn_mode 1 with dres written, bn_mode 2 with dres accumulated) and msk_channel_sum of one form under the four geometries."""
    d = dev()
    cu = d.get_option("num_cu")
    Cn, ld, c0, ew, red = FORMS[form]
    V = _voxels(form, cu)
    rng = np.random.default_rng(sum(map(ord, form + reskind)))
    x = (rng.standard_normal((V, Cn)) * 3 + 50.0).astype(F4)      # large mean: cancellation in the statistics
    gamma, beta = rng.uniform(0.5, 1.5, Cn).astype(F4), rng.standard_normal(Cn).astype(F4)
    alpha = rng.uniform(0.1, 0.4, Cn).astype(F4)
    res, dout, dres_old = _res_array(rng, reskind, V, Cn), rng.standard_normal((V, Cn)).astype(F4), rng.standard_normal((V, Cn)).astype(F4)
    mean, m2 = R.bn_stats(x)
    invstd = 1.0 / np.sqrt(m2 / V + 1e-5)
    scale, shift = (gamma * invstd).astype(F4), (beta - mean * gamma * invstd).astype(F4)
    mean32, invstd32 = mean.astype(F4), invstd.astype(F4)
    out_ref = R.affine_act_fwd(x, scale, shift, res, alpha)
    bw = R.affine_act_bwd(x, scale, shift, res, alpha, mean32, invstd32, dout, 1)
    sums32 = bw["sums"].astype(F4)                                  # the apply passes of every geometry get the SAME sums
    dx1_ref = R.affine_act_bwd(x, scale, shift, res, alpha, mean32, invstd32, dout, 1, sums=sums32)["dx"]
    dx2_ref = R.f8(scale) * bw["du"]

    X, DOUT = Buf(x, ld, c0), Buf(dout, ld, c0)
    RES = Buf(res) if res is not None else None
    rt, rmsk = (RES.t, RES.msk()) if RES else (None, _null())
    sc, sh, al, mu, si, g_ = (vec(a) for a in (scale, shift, alpha, mean32, invstd32, gamma))
    sums_fixed = vec(sums32.ravel())
    per_element = {}
    for gname in GEOMS:
        with geometry(gname):
            OUT, DX1, DR1, DX2, DR2 = Buf.empty(V, Cn, ld, c0), Buf.empty(V, Cn, ld, c0), Buf.empty(V, Cn, ld, c0), Buf.empty(V, Cn, ld, c0), Buf(dres_old, ld, c0)
            assert _elementwise_form(X.t, [OUT.t], rt) == ew and _elementwise_form(X.t, [DOUT.t, DX1.t, DR1.t], rt) == ew, (form, gname)
            assert _reduce_form(X.t, DOUT.t, rt) == red and _reduce_form(X.t, None, None) == red, (form, gname)
            stats, sums, csum = vec(np.zeros(2 * Cn)), vec(np.zeros(3 * Cn)), vec(np.ones(Cn))
            maxes = vec(np.full(128, 5.0, F4)) if red == "v4" else None     # cleared by the call
            am1, am2 = d.amax_new(1), d.amax_new(1)
            d.call("msk_bn_stats", X.msk(), vp(stats))
            d.call("msk_affine_act_fwd", X.msk(), vp(sc), vp(sh), rmsk, vp(al), OUT.msk())
            d.call("msk_affine_act_bwd_reduce_ex", X.msk(), vp(sc), vp(sh), rmsk, vp(al), vp(mu), vp(si), DOUT.msk(), vp(sums), vp(maxes))
            d.call("msk_affine_act_bwd_apply_amax", X.msk(), vp(sc), vp(sh), rmsk, vp(al), vp(mu), vp(si), vp(g_), DOUT.msk(),
                   vp(sums_fixed), C.c_double(V), 1, DX1.msk(), DR1.msk(), 0, vp(am1))
            d.call("msk_affine_act_bwd_apply_amax", X.msk(), vp(sc), vp(sh), rmsk, vp(al), vp(mu), vp(si), vp(g_), DOUT.msk(),
                   vp(sums_fixed), C.c_double(V), 2, DX2.msk(), DR2.msk(), 1, vp(am2))
            d.call("msk_channel_sum", DOUT.msk(), vp(csum), 1)
            st, s_ = vec_back(stats, 2 * Cn), vec_back(sums, 3 * Cn).reshape(3, Cn)
            assert np.abs(st[:Cn] - mean).max() < 1e-5 * 50, (form, gname)
            assert rel_err(st[Cn:] / V, m2 / V) < 2e-5, (form, gname)
            for q in range(3):
                assert rel_err(s_[q], bw["sums"][q]) < 1e-4, (form, gname, q)
            assert rel_err(vec_back(csum, Cn), R.channel_sum(dout) + 1.0) < 1e-5
            got = {"out": OUT.host(), "dx1": DX1.host(), "dres1": DR1.host(), "dx2": DX2.host(), "dres2": DR2.host()}
            assert not any(np.isnan(a).any() for a in got.values()), (form, gname)       # an unwritten element reads back NaN
            assert np.abs(got["out"] - out_ref).max() < 2e-4
            assert rel_err(got["dx1"], dx1_ref) < 2e-4 and rel_err(got["dx2"], dx2_ref) < 2e-4
            assert rel_err(got["dres1"], bw["du"]) < 1e-5 and rel_err(got["dres2"], bw["du"] + R.f8(dres_old)) < 1e-5
            assert _amax(am1).max() == np.abs(got["dx1"]).max() and _amax(am2).max() == np.abs(got["dx2"]).max()
            if maxes:
                mx = _amax(maxes, 2).max(axis=1)
                assert abs(mx[0] - np.abs(bw["du"]).max()) <= 1e-6 * np.abs(bw["du"]).max()
                assert abs(mx[1] - np.abs(bw["xhat"]).max()) < 1e-4 * np.abs(bw["xhat"]).max()
            per_element[gname] = got
    for gname in "bcd":
        for k, a in per_element["a"].items():
            assert _same_bits(a, per_element[gname][k]), (form, k, gname)


JOIN_CASES = [("cs16", "null"), ("cs16", "acc"), ("cs32", "write"), ("cs16_in32", "write"), ("k4_20", "acc"), ("k4_20", "null"), ("k4_24", "write"),
              ("cs256", "acc")]


@pytest.mark.parametrize("form,dbmode", JOIN_CASES)
def test_join_fwd_bwd_under_every_geometry(form, dbmode):
    """msk_affine_act_join_fwd, msk_add_act_bwd (the v4 reduction kernel's mode 1) and msk_add_act_join_bwd_ex (mode 2) with the
    second operand's gradient skipped / written / accumulated."""
    d = dev()
    cu = d.get_option("num_cu")
    Cn, ld, c0, ew, red = FORMS[form]
    V = _voxels(form, cu)
    rng = np.random.default_rng(sum(map(ord, form + dbmode)) + 1)
    y, res, dout, old = (rng.standard_normal((V, Cn)).astype(F4) for _ in range(4))
    scale, shift = rng.uniform(0.5, 1.5, Cn).astype(F4), rng.standard_normal(Cn).astype(F4)
    ai, ao = rng.uniform(0.05, 0.5, Cn).astype(F4), rng.uniform(-0.2, 0.5, Cn).astype(F4)
    mean, invstd = rng.standard_normal(Cn).astype(F4), rng.uniform(0.5, 2.0, Cn).astype(F4)
    out_ref = R.affine_act_fwd(y, scale, shift, res, ao, alpha_in=ai)
    j1 = R.add_act_join_bwd(y, None, None, None, res, ao, dout)
    j2 = R.add_act_join_bwd(y, scale, shift, ai, res, ao, dout, mean, invstd)
    Y, RES, DOUT = Buf(y, ld, c0), Buf(res, ld, c0), Buf(dout, ld, c0)
    sc, sf, pai, pao, mu, si = (vec(a) for a in (scale, shift, ai, ao, mean, invstd))
    acc = 1 if dbmode == "acc" else 0
    per_element = {}
    for gname in GEOMS:
        with geometry(gname):
            OUT, DA1, DA2 = Buf.empty(V, Cn, ld, c0), Buf.empty(V, Cn, ld, c0), Buf.empty(V, Cn, ld, c0)
            DB1 = None if dbmode == "null" else (Buf(old, ld, c0) if acc else Buf.empty(V, Cn, ld, c0))
            DB2 = None if dbmode == "null" else (Buf(old, ld, c0) if acc else Buf.empty(V, Cn, ld, c0))
            assert _elementwise_form(Y.t, [OUT.t], RES.t, d12_allowed=False) == ew and red == "v4"
            assert Cn % 4 == 0 and all(_vec4_ok(b.t) for b in (Y, RES, DOUT, DA1) + ((DB1,) if DB1 else ()))
            dal1, dal2, sums4 = vec(np.full(Cn, 0.25, F4)), vec(np.full(Cn, 0.25, F4)), vec(np.zeros(4 * Cn, F4))
            maxes = vec(np.full(128, 5.0, F4))
            d.call("msk_affine_act_join_fwd", Y.msk(), vp(sc), vp(sf), vp(pai), RES.msk(), vp(pao), OUT.msk())
            d.call("msk_add_act_bwd", Y.msk(), RES.msk(), vp(pao), DOUT.msk(), DA1.msk(), DB1.msk() if DB1 else _null(), acc, vp(dal1))
            d.call("msk_add_act_join_bwd_ex", Y.msk(), vp(sc), vp(sf), vp(pai), RES.msk(), vp(pao), vp(mu), vp(si), DOUT.msk(),
                   DA2.msk(), DB2.msk() if DB2 else _null(), acc, vp(dal2), vp(sums4), vp(maxes))
            got = {"out": OUT.host(), "da1": DA1.host(), "da2": DA2.host()}
            if DB1:
                got.update(db1=DB1.host(), db2=DB2.host())
            assert not any(np.isnan(a).any() for a in got.values()), (form, gname)
            assert rel_err(got["out"], out_ref) < 1e-6
            assert rel_err(got["da1"], j1["da"]) < 1e-6 and rel_err(got["da2"], j2["da"]) < 1e-6
            if DB1:
                assert rel_err(got["db1"], j1["da"] + (R.f8(old) if acc else 0.0)) < 1e-6
                assert rel_err(got["db2"], j2["da"] + (R.f8(old) if acc else 0.0)) < 1e-6
            assert rel_err(vec_back(dal1, Cn), j1["dalpha"] + 0.25) < 2e-5 and rel_err(vec_back(dal2, Cn), j2["dalpha"] + 0.25) < 2e-5
            us = vec_back(sums4, 3 * Cn)
            assert np.abs(us - j2["unit_sums"].ravel()).max() < 2e-5 * np.abs(j2["unit_sums"]).max()
            mx = _amax(maxes, 2).max(axis=1)
            assert abs(mx[0] - np.abs(j2["du"]).max()) < 1e-6 * np.abs(j2["du"]).max()
            assert abs(mx[1] - np.abs(j2["xhat"]).max()) < 1e-5 * np.abs(j2["xhat"]).max()
            per_element[gname] = got
    for gname in "bcd":
        for k, a in per_element["a"].items():
            assert _same_bits(a, per_element[gname][k]), (form, k, gname)


@pytest.mark.parametrize("form", ["k1_5", "k1_16_in20"])
def test_join_fwd_scalar_form_under_every_geometry(form):
    """msk_affine_act_join_fwd needs no float4 (its backward does): 5 channels, and channels 2 .. 18 of a 20-wide buffer, take
    affine_act_fwd_k<1> with the unit's own PReLU (alpha_in) ahead of the join."""
    d = dev()
    cu = d.get_option("num_cu")
    Cn, ld, c0, ew, _ = FORMS[form]
    V = _voxels(form, cu)
    rng = np.random.default_rng(sum(map(ord, form)) + 2)
    y, res = rng.standard_normal((V, Cn)).astype(F4), rng.standard_normal((V, Cn)).astype(F4)
    scale, shift = rng.uniform(0.5, 1.5, Cn).astype(F4), rng.standard_normal(Cn).astype(F4)
    ai, ao = rng.uniform(0.05, 0.5, Cn).astype(F4), rng.uniform(-0.2, 0.5, Cn).astype(F4)
    ref = R.affine_act_fwd(y, scale, shift, res, ao, alpha_in=ai)
    Y, RES = Buf(y, ld, c0), Buf(res, ld, c0)
    sc, sf, pai, pao = (vec(a) for a in (scale, shift, ai, ao))
    outs = {}
    for gname in "abc":
        with geometry(gname):
            OUT, am = Buf.empty(V, Cn, ld, c0), d.amax_new(1)
            assert _elementwise_form(Y.t, [OUT.t], RES.t, d12_allowed=False) == ew == "k1"
            d.call("msk_affine_act_join_fwd", Y.msk(), vp(sc), vp(sf), vp(pai), RES.msk(), vp(pao), OUT.msk())
            outs[gname] = OUT.host()
            assert not np.isnan(outs[gname]).any() and rel_err(outs[gname], ref) < 1e-6
            OUT2 = Buf.empty(V, Cn, ld, c0)
            d.call("msk_affine_act_join_fwd_amax", Y.msk(), vp(sc), vp(sf), vp(pai), RES.msk(), vp(pao), OUT2.msk(), vp(am))
            assert _same_bits(OUT2.host(), outs[gname]) and _same_bits(_amax(am).max(), np.abs(outs[gname]).max())
    assert _same_bits(outs["a"], outs["b"]) and _same_bits(outs["a"], outs["c"])


@pytest.mark.parametrize("clear", [0, 1])
def test_pg_twins_fold_into_or_clear_the_maxes(clear):
    """msk_affine_act_bwd_reduce_pg / msk_add_act_join_bwd_pg: the _ex forms plus `clear_maxes` and the parameter-gradient
    pointers.  clear_maxes 0 folds into what the two arrays hold (a larger value in one way of the first stays, smaller
    values in the second are overtaken); clear_maxes 1 forgets it.  The parameter gradients are the sums, added."""
    d = dev()
    Cn, V = 16, 1500 + 3
    P = _planted_inputs(np.random.default_rng(40 + clear), V, Cn)
    X, RES, DOUT = Buf(P["x"]), Buf(P["res"]), Buf(P["dout"])
    dv = {k: vec(P[k]) for k in ("scale", "shift", "alpha", "ai", "mean", "invstd")}
    b = R.affine_act_bwd(P["x"], P["scale"], P["shift"], P["res"], P["alpha"], P["mean"], P["invstd"], P["dout"], 0)
    j = R.add_act_join_bwd(P["x"], P["scale"], P["shift"], P["ai"], P["res"], P["alpha"], P["dout"], P["mean"], P["invstd"])
    pre = np.full((2, 64), 1e-6, F4)
    pre[0, 5] = 1e6
    for name, du, xhat, sums_ref in (("reduce", b["du"], b["xhat"], b["sums"]), ("join", j["du"], j["xhat"], j["unit_sums"])):
        maxes, sums = vec(pre.ravel()), vec(np.zeros(4 * Cn, F4))
        dg, db, da = vec(np.full(Cn, 0.5, F4)), vec(np.full(Cn, 0.5, F4)), vec(np.full(Cn, 0.5, F4))
        if name == "reduce":
            d.call("msk_affine_act_bwd_reduce_pg", X.msk(), vp(dv["scale"]), vp(dv["shift"]), RES.msk(), vp(dv["alpha"]), vp(dv["mean"]),
                   vp(dv["invstd"]), DOUT.msk(), vp(sums), vp(maxes), clear, vp(dg), vp(db), vp(da))
        else:
            d.call("msk_add_act_join_bwd_pg", X.msk(), vp(dv["scale"]), vp(dv["shift"]), vp(dv["ai"]), RES.msk(), vp(dv["alpha"]), vp(dv["mean"]),
                   vp(dv["invstd"]), DOUT.msk(), Buf.empty(V, Cn).msk(), _null(), 0, vp(vec(np.zeros(Cn, F4))), vp(sums), vp(maxes), clear,
                   vp(dg), vp(db), vp(da))
        mx = _amax(maxes, 2)
        m_du, m_xh = np.abs(du).max(), np.abs(xhat).max()
        if clear:
            assert abs(mx[0].max() - m_du) <= 1e-6 * m_du, name
        else:
            assert mx[0].max() == F4(1e6) and np.all(mx[0] >= F4(1e-6)), name          # folded: nothing was lowered
            assert abs(np.delete(mx[0], 5).max() - m_du) <= 1e-6 * m_du, name          # ... and the other ways took the measured maximum
        assert abs(mx[1].max() - m_xh) < 1e-4 * m_xh, name
        for q, ptr in enumerate((db, dg, da)):                                          # d beta, d gamma, d alpha = quantities 0, 1, 2, added
            assert rel_err(vec_back(ptr, Cn), sums_ref[q] + 0.5) < 1e-4, (name, q)


@pytest.mark.parametrize("form", ["cs16", "k4_20", "k1_5", "k1_16_in20"])
@pytest.mark.parametrize("masked,acc", [(1, 0), (0, 1), (1, 1), (0, 0)])
def test_copy_scale_amax_under_every_geometry(form, masked, acc):
    """msk_copy_scale_amax (Dropout3D / concat copies): k<4> and k<1>, mask on and off, accumulate on and off, two samples."""
    d = dev()
    cu = d.get_option("num_cu")
    Cn, ld, c0, ew, _ = FORMS[form]
    V = _voxels(form, cu) // 2 * 2
    rng = np.random.default_rng(7 + Cn)
    src, old = rng.standard_normal((V, Cn)).astype(F4), rng.standard_normal((V, Cn)).astype(F4)
    mask = ((rng.random((2, Cn)) < 0.5) * 2.0).astype(F4) if masked else None
    ref = R.copy_scale(src, mask, old, V // 2, acc)
    SRC = Buf(src, ld, c0, n=2)
    mp = vec(mask.ravel()) if masked else None
    outs = {}
    for gname in "abc":
        with geometry(gname):
            DST = Buf(old, ld, c0, n=2) if acc else Buf.empty(V, Cn, ld, c0, n=2)
            assert _copy_form(SRC.t, DST.t) == ("k1" if ew == "k1" else "k4")
            am = d.amax_new(1)
            d.call("msk_copy_scale_amax", SRC.msk(), vp(mp), DST.msk(), acc, vp(am))
            outs[gname] = DST.host()
            assert not np.isnan(outs[gname]).any()
            assert rel_err(outs[gname], ref) < 1e-6
            assert _same_bits(_amax(am).max(), np.abs(outs[gname]).max())
    assert _same_bits(outs["a"], outs["b"]) and _same_bits(outs["a"], outs["c"])


@pytest.mark.parametrize("Cn", [3, 5])
def test_softmax_argmax_under_every_geometry(Cn):
    d = dev()
    cu = d.get_option("num_cu")
    V = 23 * 256 * cu // 10 + 3                        # one voxel per thread: 2.3 grid strides under ew_cap 1
    rng = np.random.default_rng(Cn)
    x = (rng.standard_normal((V, Cn)) * 4).astype(F4)
    x[::7, 1] = x[::7, 0]                              # ties: the first maximum wins
    X = Buf(x)
    outs = {}
    for gname in "abc":
        with geometry(gname):
            P, am = Buf.empty(V, Cn), dmalloc(V * 4)
            d.call("msk_softmax_c", X.msk(), P.msk())
            d.call("msk_argmax_c", X.msk(), vp(am))
            outs[gname] = P.host()
            assert rel_err(outs[gname], R.softmax_c(x)) < 1e-6
            assert np.array_equal(d.d2h(am, (V,), np.int32), R.argmax_c(x))
    assert _same_bits(outs["a"], outs["b"]) and _same_bits(outs["a"], outs["c"])


def test_elu_second_trip_and_layout_ragged_tiles():
    """msk_elu_fwd / msk_elu_bwd size their own grid (16 blocks per CU): 2.3 grid strides; the layout kernels on ragged 32 x 32 tiles
    of a channel slice."""
    d = dev()
    cu = d.get_option("num_cu")
    Cn, ld, c0 = 6, 8, 1
    V = 23 * 16 * 256 * cu // (10 * Cn) + 3
    rng = np.random.default_rng(3)
    x, dout, old = ((rng.standard_normal((V, Cn)) * 2).astype(F4) for _ in range(3))
    X, DOUT, OUT, DX = Buf(x, ld, c0), Buf(dout), Buf.empty(V, Cn), Buf(old, ld, c0)
    d.call("msk_elu_fwd", X.msk(), C.c_float(0.5), OUT.msk())
    o = OUT.host()
    assert rel_err(o, R.elu_fwd(x, 0.5)) < 1e-6
    d.call("msk_elu_bwd", OUT.msk(), DOUT.msk(), C.c_float(0.5), DX.msk(), 1)
    assert rel_err(DX.host(), R.elu_bwd(o, dout, 0.5) + R.f8(old)) < 2e-6
    n, Cl, S = 2, 37, 1003                              # two channel tiles, 32 voxel tiles per sample, both ragged
    a = rng.standard_normal((n, Cl, 1, 1, S)).astype(F4)
    W = Buf.empty(n * S, Cl, 40, 2, n=n)
    d.call("msk_ncdhw_to_ndhwc", vp(vec(a.ravel())), W.msk())
    assert _same_bits(W.host().reshape(n, S, Cl).transpose(0, 2, 1), a.reshape(n, Cl, S))
    back = dmalloc(a.nbytes)
    d.call("msk_ndhwc_to_ncdhw", W.msk(), vp(back))
    assert _same_bits(d.d2h(back, a.shape, F4), a)


@contextlib.contextmanager
def _blocks_allowed(nb):
    """geometry d (one voxel per lane) with "reduce_cap" raised, where the chip needs it, so that nb blocks fit under the cap"""
    d = dev()
    old = d.get_option("reduce_cap")
    try:
        d.set_option("reduce_cap", max(old, (nb + d.get_option("num_cu") - 1) // d.get_option("num_cu")))
        with geometry("d") as g:
            yield g
    finally:
        d.set_option("reduce_cap", old)


def test_merge_forms_with_many_partial_records():
    """The 256-lane form of sums_merge_k (more than 256 partial records) and the 1024-thread form of bn_stats_merge (more than 4096)
    against the product geometry: C = 256 at a little over 1024 voxels, and 5 channels (32 voxel lanes) at 4100 blocks."""
    d = dev()
    cu = d.get_option("num_cu")
    rng = np.random.default_rng(11)
    V, Cn = 1024 + 37, 256
    x, dout = (rng.standard_normal((V, Cn)) * 3 + 50.0).astype(F4), rng.standard_normal((V, Cn)).astype(F4)
    alpha, scale, shift = rng.uniform(0.1, 0.4, Cn).astype(F4), rng.uniform(0.2, 0.5, Cn).astype(F4), (-15 + rng.standard_normal(Cn)).astype(F4)
    mean, m2 = R.bn_stats(x)
    mean32, invstd32 = mean.astype(F4), (1.0 / np.sqrt(m2 / V + 1e-5)).astype(F4)
    bw = R.affine_act_bwd(x, scale, shift, None, alpha, mean32, invstd32, dout, 0)
    X, DOUT = Buf(x), Buf(dout)
    with _blocks_allowed(V // 4 + 1) as g:
        assert _reduce_blocks(V, 4, cu, g) > 256
        stats, sums = vec(np.zeros(2 * Cn)), vec(np.zeros(3 * Cn))
        d.call("msk_bn_stats", X.msk(), vp(stats))
        d.call("msk_affine_act_bwd_reduce_ex", X.msk(), vp(vec(scale)), vp(vec(shift)), _null(), vp(vec(alpha)), vp(vec(mean32)),
               vp(vec(invstd32)), DOUT.msk(), vp(sums), None)
        st, s_ = vec_back(stats, 2 * Cn), vec_back(sums, 3 * Cn).reshape(3, Cn)
    assert np.abs(st[:Cn] - mean).max() < 1e-5 * 50 and rel_err(st[Cn:] / V, m2 / V) < 2e-5
    for q in range(3):
        assert rel_err(s_[q], bw["sums"][q]) < 1e-4
    Cn = 5
    V = 32 * 4100 + 11                                  # scalar statistics kernel: CB = 8, 32 voxel lanes -> 4101 blocks of one voxel per lane
    x = (rng.standard_normal((V, Cn)) * 3 + 50.0).astype(F4)
    mean, m2 = R.bn_stats(x)
    X = Buf(x)
    with _blocks_allowed(4101) as g:
        assert _reduce_blocks(V, 32, cu, g) > 4096
        stats = vec(np.zeros(2 * Cn))
        d.call("msk_bn_stats", X.msk(), vp(stats))
        st = vec_back(stats, 2 * Cn)
    assert np.abs(st[:Cn] - mean).max() < 1e-5 * 50 and rel_err(st[Cn:] / V, m2 / V) < 2e-5


# ==== B. planted maximum ================================================================================================================
def _planted_inputs(rng, V, Cn):
    p = {k: rng.standard_normal((V, Cn)).astype(F4) for k in ("x", "res", "dout", "old")}
    p.update(scale=rng.uniform(0.5, 1.5, Cn).astype(F4), shift=(0.3 * rng.standard_normal(Cn)).astype(F4),
             alpha=rng.uniform(0.1, 0.4, Cn).astype(F4), ai=rng.uniform(0.1, 0.5, Cn).astype(F4),
             mean=(0.2 * rng.standard_normal(Cn)).astype(F4), invstd=rng.uniform(0.5, 1.5, Cn).astype(F4),
             sums=np.stack([30 * rng.standard_normal(Cn), 30 * rng.standard_normal(Cn)]).astype(F4))
    return p


PRODUCERS = {
    # name: (forms, kind of positions, planted tensors)
    "fwd_amax": (["cs16", "cs16_in32", "cs256", "k4_20", "k1_5", "k1_16_in20", "d12_3", "d12_6"], "ew", ("x",)),
    "fwd_amax2": (["cs16", "cs16_in32", "cs256"], "ew", ("x",)),          # the second output needs the channel-stationary kernel
    "join_fwd_amax": (["cs16", "cs16_in32", "k4_20", "k1_5", "k1_16_in20"], "ew", ("x",)),
    "copy_scale_amax": (["cs16", "k4_20", "k1_5", "k1_16_in20"], "ew", ("x",)),
    "bwd_apply_amax": (["cs16", "cs16_in32", "cs256", "k4_20", "k1_5", "k1_16_in20", "d12_3"], "ew", ("dout",)),
    "bwd_reduce_maxes": (["cs16", "cs16_in32", "cs256", "k4_20"], "red", ("dout", "x")),
    "join_bwd_maxes": (["cs16", "cs16_in32", "cs256", "k4_20"], "red", ("dout", "x")),
}


@pytest.mark.parametrize("producer,form", [(p, f) for p, (forms, _, _) in PRODUCERS.items() for f in forms])
def test_planted_maximum_reaches_the_amax_array(producer, form):
    """One element is made ~1000 times the bulk maximum at every place a form could skip, with both signs and on both PReLU
    branches; the array's maximum must be max |written tensor| of the GPU's own output bit for bit, the argmax of the written
    tensor the planted place, every other element what the unplanted run wrote, and the planted element the reference's."""
    d = dev()
    cu = d.get_option("num_cu")
    Cn, ld, c0, ew, red = FORMS[form]
    forms, kind, planted = PRODUCERS[producer]
    V = _voxels(form, cu)
    P = _planted_inputs(np.random.default_rng(sum(map(ord, producer + form))), V, Cn)
    X, RES, DOUT = Buf(P["x"], ld, c0), Buf(P["res"], ld, c0), Buf(P["dout"], ld, c0)
    dv = {k: vec(P[k]) for k in ("scale", "shift", "alpha", "ai", "mean", "invstd")}
    dv["sums"] = vec(P["sums"].ravel())
    dv["mask"] = vec(np.full(Cn, 0.5, F4))

    def rows(v):
        return {k: P[k][v:v + 1].copy() for k in ("x", "res", "dout", "old")}

    def reference(r):
        """written values (or the two maxima' terms) of the rows r"""
        if producer in ("fwd_amax", "fwd_amax2"):
            return R.affine_act_fwd(r["x"], P["scale"], P["shift"], r["res"], P["alpha"])
        if producer == "join_fwd_amax":
            return R.affine_act_fwd(r["x"], P["scale"], P["shift"], r["res"], P["alpha"], alpha_in=P["ai"])
        if producer == "copy_scale_amax":
            return R.copy_scale(r["x"], np.full((1, Cn), 0.5), r["old"], 1 << 60, 1)
        b = None
        if producer == "bwd_apply_amax":
            return R.affine_act_bwd(r["x"], P["scale"], P["shift"], r["res"], P["alpha"], P["mean"], P["invstd"], r["dout"], 1, M=V, sums=P["sums"])["dx"]
        if producer == "bwd_reduce_maxes":
            b = R.affine_act_bwd(r["x"], P["scale"], P["shift"], r["res"], P["alpha"], P["mean"], P["invstd"], r["dout"], 0)
            return b["du"], b["xhat"]
        b = R.add_act_join_bwd(r["x"], P["scale"], P["shift"], P["ai"], r["res"], P["alpha"], r["dout"], P["mean"], P["invstd"])
        return b["du"], b["xhat"], b["da"]

    def launch():
        """-> (amax arrays [n, 64], written tensor or None)"""
        if producer == "fwd_amax2":
            # out2 has a voxel stride of its own: dense beside a slice, the upper half of a 2C-wide buffer beside a dense out
            OUT, OUT2, am = Buf.empty(V, Cn, ld, c0), (Buf.empty(V, Cn) if ld else Buf.empty(V, Cn, 2 * Cn, Cn)), d.amax_new(1)
            assert _elementwise_form(X.t, [OUT.t], RES.t, d12_allowed=False) == "cs" and _vec4_ok(OUT2.t) and OUT2.ld != OUT.ld
            d.call("msk_affine_act_fwd_amax2", X.msk(), vp(dv["scale"]), vp(dv["shift"]), RES.msk(), vp(dv["alpha"]), OUT.msk(), vp(am), OUT2.msk())
            o, o2 = _take(OUT), _take(OUT2)
            assert not np.isnan(o2).any() and _same_bits(o, o2)      # the second copy: every element written, the same bits
            return _amax(am), o
        if producer in ("fwd_amax", "join_fwd_amax"):
            OUT, am = Buf.empty(V, Cn, ld, c0), d.amax_new(1)
            if producer == "fwd_amax":
                assert _elementwise_form(X.t, [OUT.t], RES.t) == ew
                d.call("msk_affine_act_fwd_amax", X.msk(), vp(dv["scale"]), vp(dv["shift"]), RES.msk(), vp(dv["alpha"]), OUT.msk(), vp(am))
            else:
                assert _elementwise_form(X.t, [OUT.t], RES.t, d12_allowed=False) == ew
                d.call("msk_affine_act_join_fwd_amax", X.msk(), vp(dv["scale"]), vp(dv["shift"]), vp(dv["ai"]), RES.msk(), vp(dv["alpha"]), OUT.msk(), vp(am))
            return _amax(am), _take(OUT)
        if producer == "copy_scale_amax":
            DST, am = Buf(P["old"], ld, c0), d.amax_new(1)
            assert _copy_form(X.t, DST.t) == ("k1" if ew == "k1" else "k4")
            d.call("msk_copy_scale_amax", X.msk(), vp(dv["mask"]), DST.msk(), 1, vp(am))
            return _amax(am), _take(DST)
        if producer == "bwd_apply_amax":
            DX, am = Buf.empty(V, Cn, ld, c0), d.amax_new(1)
            assert _elementwise_form(X.t, [DOUT.t, DX.t], RES.t) == ew
            d.call("msk_affine_act_bwd_apply_amax", X.msk(), vp(dv["scale"]), vp(dv["shift"]), RES.msk(), vp(dv["alpha"]), vp(dv["mean"]),
                   vp(dv["invstd"]), None, DOUT.msk(), vp(dv["sums"]), C.c_double(V), 1, DX.msk(), _null(), 0, vp(am))
            return _amax(am), _take(DX)
        maxes, sums = vec(np.full(128, 5.0, F4)), vec(np.zeros(4 * Cn, F4))
        assert _reduce_form(X.t, DOUT.t, RES.t) == "v4"
        if producer == "bwd_reduce_maxes":
            d.call("msk_affine_act_bwd_reduce_ex", X.msk(), vp(dv["scale"]), vp(dv["shift"]), RES.msk(), vp(dv["alpha"]), vp(dv["mean"]),
                   vp(dv["invstd"]), DOUT.msk(), vp(sums), vp(maxes))
            return _amax(maxes, 2), None
        DA = Buf.empty(V, Cn, ld, c0)
        d.call("msk_add_act_join_bwd_ex", X.msk(), vp(dv["scale"]), vp(dv["shift"]), vp(dv["ai"]), RES.msk(), vp(dv["alpha"]), vp(dv["mean"]),
               vp(dv["invstd"]), DOUT.msk(), DA.msk(), _null(), 0, vp(vec(np.zeros(Cn, F4))), vp(sums), vp(maxes))
        return _amax(maxes, 2), _take(DA)

    full = {k: P[k] for k in ("x", "res", "dout", "old")}
    tol = 2e-4 if producer == "bwd_apply_amax" else 1e-6      # test_bn_stats_and_affine_act's for dx; the join / slice tests' otherwise
    kernel = ("k1" if ew == "k1" else "k4") if producer == "copy_scale_amax" else ew
    branches = set()
    for gname in "ab":
        with geometry(gname) as g:
            am, base = launch()
            ref = reference(full)
            if kind == "ew":
                bulk = float(np.abs(ref).max())
                assert rel_err(base, ref) < tol and _same_bits(am.max(), np.abs(base).max())
            else:
                bulk, bulk_xh = float(np.abs(ref[0]).max()), float(np.abs(ref[1]).max())
                assert abs(am[0].max() - bulk) <= 1e-6 * bulk and abs(am[1].max() - bulk_xh) < 1e-4 * bulk_xh
                if base is not None:
                    assert rel_err(base, ref[2]) < tol
            for i, (v, c) in enumerate(_positions(form, V, cu, g, kind, kernel)):
                where = (producer, form, gname, v, c)
                r = rows(v)
                if kind == "red":                         # x planted as well -> max |xhat|; its sign picks the PReLU branch
                    r["x"][0, c] = F4((-1.0 if i % 4 < 2 else 1.0) * 1000.0 * bulk_xh)
                    r["x"][0, c] *= F4(1000.0 * bulk_xh / abs(float(reference(r)[1][0, c])))
                    branches.add(bool(r["x"][0, c] > 0))
                elif producer == "bwd_apply_amax" and i % 4 < 2:
                    r["x"][0, c] = F4(-9.0)               # dout planted on the negative branch (where the residual allows)
                k0 = planted[0]
                r[k0][0, c] = F4((-1.0 if i % 2 else 1.0) * 1000.0 * bulk)
                e = reference(r)                          # piecewise linear in the planted value: aim at 1000 x the bulk maximum
                r[k0][0, c] *= F4(1000.0 * bulk / abs(float((e if kind == "ew" else e[0])[0, c])))
                e = reference(r)
                pokes = [({"x": X, "dout": DOUT}[k], r[k][0, c], P[k][v, c]) for k in dict.fromkeys(planted + ("x",))]
                for b, new, _ in pokes:
                    b.poke(v, c, new)
                try:
                    am, got = launch()
                finally:
                    for b, _, orig in pokes:
                        b.poke(v, c, orig)
                if kind == "ew":
                    exp = float(e[0, c])
                    assert 500 * bulk < abs(exp) < 2000 * bulk, where
                    branches.add(exp > 0)
                    assert _same_bits(am.max(), np.abs(got).max()), where
                    assert int(np.abs(got).argmax()) == v * Cn + c, where
                    assert abs(float(got[v, c]) - exp) <= tol * abs(exp), where
                else:
                    du, xh = abs(float(e[0][0, c])), abs(float(e[1][0, c]))
                    assert 500 * bulk < du < 2000 * bulk and 500 * bulk_xh < xh < 2000 * bulk_xh, where
                    assert abs(float(am[0].max()) - du) <= 1e-6 * du, where
                    assert abs(float(am[1].max()) - xh) < 1e-4 * xh, where
                    if got is not None:
                        assert int(np.abs(got).argmax()) == v * Cn + c, where
                        assert abs(float(got[v, c]) - float(e[2][0, c])) <= tol * abs(float(e[2][0, c])), where
                if got is not None:
                    got[v, c] = base[v, c]
                    assert _same_bits(got, base), where    # every other element: what the unplanted run wrote
    assert branches == {True, False}, branches             # both signs (ew) / both PReLU branches (reductions) were planted


def test_amax_arrays_fold_zero_and_stay_apart():
    """Two calls folding into one array (the halves of a concat buffer) give the maximum over both; an all-zero tensor leaves the
    array zero; of three consecutive arrays only the one passed is written; msk_copy_scale_amax with accumulate holds
    max |dst + src * mask|, not max |src * mask|."""
    d = dev()
    rng = np.random.default_rng(5)
    V, Cn = 1500 + 3, 16
    a, b = rng.standard_normal((V, Cn)).astype(F4), (3 * rng.standard_normal((V, Cn))).astype(F4)
    ams = d.amax_new(3)
    mid = ams + 256
    cat = Buf.empty(V, 2 * Cn)                             # one concat buffer, its halves written by two calls
    lo, hi = cat.t.channel_slice(0, Cn), cat.t.channel_slice(Cn, 2 * Cn)
    alpha = vec(np.full(Cn, 0.25, F4))
    d.call("msk_affine_act_fwd_amax", Buf(a).msk(), None, None, _null(), vp(alpha), lo.msk(), vp(mid))
    first = _amax(mid).max()
    d.call("msk_affine_act_fwd_amax", Buf(b).msk(), None, None, _null(), vp(alpha), hi.msk(), vp(mid))
    got = _amax(ams, 3)
    wl, wh = cat.host()[:, :Cn], cat.host()[:, Cn:]
    assert not np.isnan(wl).any() and not np.isnan(wh).any()
    assert _same_bits(first, np.abs(wl).max()) and _same_bits(got[1].max(), max(np.abs(wl).max(), np.abs(wh).max()))
    assert np.abs(wh).max() > np.abs(wl).max()
    assert np.all(got[0] == 0) and np.all(got[2] == 0)
    z = d.amax_new(1)
    d.call("msk_affine_act_fwd_amax", Buf(np.zeros((V, Cn), F4)).msk(), None, None, _null(), vp(alpha), Buf.empty(V, Cn).msk(), vp(z))
    d.call("msk_copy_scale_amax", Buf(np.zeros((V, Cn), F4)).msk(), None, Buf(np.zeros((V, Cn), F4)).msk(), 1, vp(z))
    assert np.all(_bits(_amax(z)) == 0)
    # accumulate: the largest |src * mask| is cancelled by dst, the largest result sits elsewhere
    src, old = rng.standard_normal((V, Cn)).astype(F4), rng.standard_normal((V, Cn)).astype(F4)
    src[V - 1, Cn - 1], old[V - 1, Cn - 1] = 8000.0, -3999.5          # 8000 * 0.5 - 3999.5 = 0.5
    old[7, 2] = -2000.0
    mask = np.full((1, Cn), 0.5, F4)
    for ldc in ((None, 0), (20, 2)):                                   # k<4> and k<1>
        DST, am = Buf(old, *ldc), d.amax_new(1)
        d.call("msk_copy_scale_amax", Buf(src, *ldc).msk(), vp(vec(mask)), DST.msk(), 1, vp(am))
        w = DST.host()
        assert rel_err(w, R.copy_scale(src, mask, old, V, 1)) < 1e-6
        assert _same_bits(_amax(am).max(), np.abs(w).max()) and int(np.abs(w).argmax()) == 7 * Cn + 2 and _amax(am).max() < 2100.0


# ==== C. producer -> consumer ============================================================================================================
CONSUMER_CASES = [
    # name: (cin, cout, (N, D, H, W), ld of x, c0)
    ("dense32", 32, 32, (1, 16, 16, 16), None, 0),
    ("slice32_in64", 32, 32, (1, 16, 16, 16), 64, 32),
    ("in_tr", 1, 16, (1, 4, 8, 33), None, 0),
    ("in_tr_odd", 1, 16, (1, 5, 7, 33), None, 0),          # voxels % 4 != 0: the scalar form of the measuring pass
]


@pytest.mark.parametrize("gname", ["a", "b"])
@pytest.mark.parametrize("case", CONSUMER_CASES, ids=[c[0] for c in CONSUMER_CASES])
def test_planted_maximum_from_producer_to_convolution(case, gname):
    """msk_affine_act_fwd_amax writes x with an outlier at the last element; the convolution and the weight gradient given that
    array are bit-identical to the calls that measure x themselves (msk_absmax: dense float4 stream, strided quads, scalar), finite
    and inside the convolution tolerance."""
    _, cin, cout, (N, D, H, W), ld, c0 = case
    d = dev()
    assert d.get_option("conv_split") == 2
    K, V = 5, N * D * H * W
    rng = np.random.default_rng(cin + V)
    pre = rng.standard_normal((V, cin)).astype(F4)
    pre[V - 1, cin - 1] = -4000.0
    alpha = np.full(cin, 0.25, F4)
    w = (rng.standard_normal((cout, cin, K, K, K)) * np.sqrt(2.0 / (cin * K ** 3))).astype(F4)
    dy = rng.standard_normal((V, cout)).astype(F4)
    old_async = d.get_option("wgrad_async")
    d.set_option("wgrad_async", 0)
    try:
        with geometry(gname):
            XB, am = Buf.empty(V, cin, ld, c0), d.amax_new(1)
            d.call("msk_affine_act_fwd_amax", Buf(pre).msk(), None, None, _null(), vp(vec(alpha)), XB.msk(), vp(am))
            x = XB.host()
            assert _same_bits(_amax(am).max(), np.abs(x).max()) and np.abs(x).max() == 1000.0
            from medicalseg_amd.device import Tensor
            xt = Tensor(d, XB.t.ptr, N, D, H, W, cin, XB.ld)
            dyb = Buf(dy)
            dyt = Tensor(d, dyb.t.ptr, N, D, H, W, cout, cout)
            wp = vec(w.ravel())
            res = []
            for with_amax in (0, 1):
                yt = t_empty(N, cout, D, H, W)
                dw = vec(np.full(w.size, 9.0, F4))
                if with_amax:
                    d.call("msk_conv3d_fwd_ex2", _desc(K), xt.msk(), vp(wp), None, yt.msk(), None, None, vp(am))
                    d.call("msk_conv3d_wgrad_ex3", _desc(K), xt.msk(), dyt.msk(), vp(dw), None, 0, None, None, vp(am))
                else:
                    d.call("msk_conv3d_fwd", _desc(K), xt.msk(), vp(wp), None, yt.msk())
                    d.call("msk_conv3d_wgrad", _desc(K), xt.msk(), dyt.msk(), vp(dw), None, 0)
                res.append((d.d2h(yt.ptr, (V, cout), F4), vec_back(dw, w.size).reshape(w.shape)))
    finally:
        d.set_option("wgrad_async", old_async)
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])
    f8 = lambda a: a.astype(np.float64)
    x5 = np.moveaxis(f8(x).reshape(N, D, H, W, cin), -1, 1)
    dy5 = np.moveaxis(f8(dy).reshape(N, D, H, W, cout), -1, 1)
    y_ref = np.moveaxis(O.conv3d(x5, f8(w), None, 1, 2), 1, -1).reshape(V, cout)
    dw_ref, _ = O.conv3d_wgrad(dy5, x5, (K, K, K), 1, 2)
    assert np.isfinite(res[1][0]).all() and np.isfinite(res[1][1]).all()
    assert rel_err(res[1][0], y_ref) < _conv_tol(cin * K ** 3) and rel_err(res[1][1], dw_ref) < 2 * _conv_tol(V)


@pytest.mark.parametrize("form", ["dense", "strided", "scalar"])
def test_measuring_pass_unrolled_loops_see_a_planted_maximum(form):
    """absmax_k (the pass a convolution measures its input with when no array comes along) sizes its grid as 2 x "ew_cap" blocks per
    CU, so under ew_cap 1 a tensor of some MB reaches its 8-deep (dense) and 4-deep (strided quads) unrolled loops and their
    single-step tails, and the scalar form a second trip.  A maximum planted in a late load of the unrolled trip, in the last one
    and in the tail: the convolution that measures x itself must return the bits of the one that is given the producer's array
    (a missed maximum is a wrong power of two, and here an fp16 overflow)."""
    d = dev()
    cu = d.get_option("num_cu")
    assert d.get_option("conv_split") == 2
    with geometry("b") as g:
        cap = 256 * 2 * g["ew_cap"] * cu                    # threads of the measuring pass at most
        if form == "dense":
            cin, cout, ld, c0, depth = 32, 32, None, 0, 8
            N, D, H, W = 1, 48, 48, (73 * cap // 80 + 2303) // 2304      # 7.3 grid strides of quads
        elif form == "strided":
            cin, cout, ld, c0, depth = 32, 32, 64, 32, 4
            N, D, H, W = 1, 32, 40, (25 * cap // 64 + 1279) // 1280      # 3.125 grid strides
        else:
            cin, cout, ld, c0, depth = 1, 16, None, 0, 1
            N, D, H, W = 1, 53, 53, 53                                   # odd: neither float4 form
        V = N * D * H * W
        items = V * cin // 4 if depth > 1 else V * cin
        S = 256 * max(1, min((V * cin // 4 + 255) // 256, cap // 256))
        assert (V * cin) % 4 == (0 if depth > 1 else 1) and items > (depth - 1) * S + 16 and items > S
        if depth > 1:                                       # a late load and the last load of the unrolled trip; the tail of a thread that has no such trip
            places = [(depth - 3) * S + 3, (depth - 1) * S + 5, (S - 1) + (depth - 2) * S, items - 1]
            places = [divmod(4 * q + i % 4, cin) for i, q in enumerate(places)]
        else:
            places = [divmod(i, cin) for i in (S + 1, 3 * S + 5, V - 1)]
        rng = np.random.default_rng(V)
        pre = rng.standard_normal((V, cin)).astype(F4)
        w = (rng.standard_normal((cout, cin, 5, 5, 5)) * np.sqrt(2.0 / (cin * 125))).astype(F4)
        from medicalseg_amd.device import Tensor
        PRE, XB, wp, al = Buf(pre), Buf.empty(V, cin, ld, c0), vec(w.ravel()), vec(np.full(cin, 0.25, F4))
        xt = Tensor(d, XB.t.ptr, N, D, H, W, cin, XB.ld)
        for v, c in places:
            PRE.poke(v, c, -4000.0)
            try:
                am = d.amax_new(1)
                d.call("msk_affine_act_fwd_amax", PRE.msk(), None, None, _null(), vp(al), XB.msk(), vp(am))
                assert _amax(am).max() == 1000.0
                ys = []
                for given in (0, 1):
                    yt = t_empty(N, cout, D, H, W)
                    if given:
                        d.call("msk_conv3d_fwd_ex2", _desc(5), xt.msk(), vp(wp), None, yt.msk(), None, None, vp(am))
                    else:
                        d.call("msk_conv3d_fwd", _desc(5), xt.msk(), vp(wp), None, yt.msk())
                    ys.append(d.d2h(yt.ptr, (V, cout), F4))
                    dfree(yt.ptr)
            finally:
                PRE.poke(v, c, pre[v, c])
            assert np.isfinite(ys[1]).all() and np.abs(ys[1]).max() > 20.0, (form, v, c)
            assert _same_bits(ys[0], ys[1]), (form, v, c)


@pytest.mark.parametrize("case", [(32, 5, (2, 16, 32, 16)), (32, 3, (2, 16, 16, 16))])
def test_bn_bwd_bound_on_adversarial_channels(case):
    """msk_conv3d_bwd_bnact under "conv_split" 2, one-kernel and split fused forms: dy is never stored, the transforms scale it by
    the DERIVED bound  max|scale| * (max|du| + max|s1 / M| + max|xhat| * max|s2 / M|)  from the reduce pass's maxima.  Per-channel
    coefficients that pull the bound's factors apart: one channel with invstd = 300 and tiny du, one with large du and a small
    scale, one with a large s1 / M, and a planted du.  The bound must hold (asserted, on the float64 dy), its looseness is
    printed; results finite and inside test_conv3d_bwd_bnact_fused_equals_three_call_form's tolerances."""
    c, K, (N, D, H, W) = case
    d = dev()
    assert d.get_option("conv_split") == 2
    rng = np.random.default_rng(c + K + D)
    f8 = lambda a: a.astype(np.float64)
    M = N * D * H * W
    x = rng.standard_normal((N, c, D, H, W)).astype(F4)
    w = (rng.standard_normal((c, c, K, K, K)) / np.sqrt(c * K ** 3)).astype(F4)
    y = O.conv3d(f8(x), f8(w), None, 1, K // 2).astype(F4)
    yc = np.moveaxis(f8(y), 1, -1).reshape(M, c)
    dout = (rng.standard_normal((M, c)) * 1e-6).astype(F4)
    gamma, alpha = rng.uniform(0.5, 1.5, c), rng.uniform(0.05, 0.5, c).astype(F4)
    mean, invstd = yc.mean(0), 1.0 / np.sqrt(yc.var(0) + 1e-5)
    invstd[0] = 300.0
    dout[:, 0] *= 1e-3                      # channel 0: invstd 300 (max |xhat| and max |scale| come from here), tiny du
    dout[:, 1] *= 100.0
    gamma[1] = 1e-3 / invstd[1]             # channel 1: the largest bulk du, scale 1e-3
    dout[M - 1, 5] = 1e-3                   # planted du, 1000 x the bulk, in the last voxel
    scale, shift = (gamma * invstd).astype(F4), (0.3 * rng.standard_normal(c)).astype(F4)
    mean32, invstd32 = mean.astype(F4), invstd.astype(F4)
    b0 = R.affine_act_bwd(yc, scale, shift, None, alpha, mean32, invstd32, dout, 0)
    sums = b0["sums"][:2].copy()
    sums[0, 2] = 5e-5 * M                   # channel 2: s1 / M fifty times the bulk du
    sums32 = sums.astype(F4)
    dy_ref, bound_ref = R.bn_bwd_dy(b0["du"], b0["xhat"], scale, sums32, M)
    dy5 = np.moveaxis(dy_ref.reshape(N, D, H, W, c), -1, 1)
    dx_ref = O.conv3d_dgrad(dy5, f8(w), x.shape, 1, K // 2)
    dw_ref, _ = O.conv3d_wgrad(dy5, f8(x), (K, K, K), 1, K // 2)

    xt, yt = t_from_ncdhw(x), t_from_ncdhw(y)
    dot = t_from_ncdhw(np.moveaxis(dout.reshape(N, D, H, W, c), -1, 1))
    wp = vec(w.ravel())
    cv = {k: vec(np.asarray(v, F4)) for k, v in dict(scale=scale, shift=shift, alpha=alpha, mean=mean32, invstd=invstd32, gamma=gamma).items()}
    cv["sums"] = vec(sums32.ravel())
    desc = _desc(K)
    nx = int(d.lib.msk_conv3d_xform_bytes(d.ctx, desc, xt.msk(), c))
    nb = int(d.lib.msk_conv3d_bwd_bnact_bytes(d.ctx, desc, xt.msk(), yt.msk()))
    assert nx > 0 and nb > 0
    xf, ybuf = dmalloc(nx), dmalloc(nb)
    d.call("msk_conv3d_fwd_ex", desc, xt.msk(), vp(wp), None, t_empty(N, c, D, H, W).msk(), None, vp(xf))
    maxes, sums_dev = vec(np.zeros(128, F4)), vec(np.zeros(3 * c, F4))
    d.call("msk_affine_act_bwd_reduce_ex", yt.msk(), vp(cv["scale"]), vp(cv["shift"]), _null(), vp(cv["alpha"]), vp(cv["mean"]),
           vp(cv["invstd"]), dot.msk(), vp(sums_dev), vp(maxes))
    mx = _amax(maxes, 2).max(axis=1)
    assert abs(mx[0] - np.abs(b0["du"]).max()) <= 1e-6 * np.abs(b0["du"]).max() and abs(mx[1] - np.abs(b0["xhat"]).max()) < 1e-4 * np.abs(b0["xhat"]).max()
    # the bound as bn_bwd_bound_k and its in-kernel twin form it, from the maxima the device measured
    invM = F4(1.0 / M)
    bound = float(np.abs(scale).max() * (mx[0] + np.abs(sums32[0] * invM).max() + mx[1] * np.abs(sums32[1] * invM).max()))
    print("c=%d K=%d: max|dy| %.3e, bound %.3e (float64 %.3e): loose by %.1f x" % (c, K, np.abs(dy_ref).max(), bound, bound_ref, bound / np.abs(dy_ref).max()))
    assert bound >= np.abs(dy_ref).max() and abs(bound - bound_ref) < 1e-4 * bound_ref
    tol = _conv_tol(c * K ** 3)
    try:
        for fuse in (1, 2):
            d.set_option("bwd_fuse", fuse)
            dyt, dxt, dw = t_empty(N, c, D, H, W, fill=9.0), t_empty(N, c, D, H, W), vec(np.full(w.size, np.nan, F4))
            d.call("msk_conv3d_bwd_bnact", desc, xt.msk(), vp(wp), yt.msk(), vp(cv["scale"]), vp(cv["shift"]), vp(cv["alpha"]),
                   vp(cv["mean"]), vp(cv["invstd"]), vp(cv["gamma"]), dot.msk(), vp(cv["sums"]), C.c_double(float(M)),
                   dyt.msk(), dxt.msk(), 0, vp(dw), 0, vp(xf), vp(ybuf), vp(maxes))
            dx, dwh = dxt.numpy(), vec_back(dw, w.size).reshape(w.shape)
            assert np.all(dyt.numpy() == 9.0)                      # the fused forms ran: dy was not stored
            assert np.isfinite(dx).all() and np.isfinite(dwh).all()
            print("bwd_fuse %d: dx err %.2e (tol %.2e), dw err %.2e (tol %.2e)" % (fuse, rel_err(dx, dx_ref), tol, rel_err(dwh, dw_ref), 2 * _conv_tol(M)))
            assert rel_err(dx, dx_ref) < tol and rel_err(dwh, dw_ref) < 2 * _conv_tol(M)
    finally:
        d.set_option("bwd_fuse", -1)


# ==== D. low end of the scale rule ========================================================================================================
SCALE_CLASSES = [
    # (cin, cout, (N, D, H, W)): the 16-bit Winograd pipeline; conv_c1 (one input channel); conv_foldn forward with conv_tightk as
    # its data gradient (<= 4 output channels)
    (32, 32, (1, 16, 16, 16)), (1, 16, (1, 4, 8, 33)), (32, 3, (1, 6, 8, 33)), (32, 1, (1, 4, 8, 16)),
]
TINY = [2.0 ** -100, 2.0 ** -106, 1e-34, 1e-37, 1e-40]


@pytest.mark.parametrize("mag", TINY, ids=["2^-100", "2^-106", "1e-34", "1e-37", "1e-40"])
@pytest.mark.parametrize("which", ["x", "dy"])
@pytest.mark.parametrize("cls", SCALE_CLASSES, ids=["wbf32", "c1", "foldn3", "foldn1"])
def test_scale_rule_low_end(cls, which, mag):
    """He-initialised weights (no compensating magnitude) against activations, and separately gradients, whose maximum is `mag`:
    everything finite and |got - ref| <= tol * max |ref| + 2^-126 (the floor allows flush-to-zero of subnormal results, no more).
    The scales are 2^(10 - e) per operand; their product passes 2^128 below max |x| ~ 2^-105, so the output stages undo them one
    after the other (msk_wbf.h wbf_unscale), and the rule itself stops at 2^126."""
    cin, cout, (N, D, H, W) = cls
    K = 5
    d = dev()
    assert d.get_option("conv_split") == 2
    rng = np.random.default_rng(cin * 7 + cout)
    f8 = lambda a: a.astype(np.float64)

    def unit(shape):
        a = rng.standard_normal(shape)
        return a / np.abs(a).max()

    x = (unit((N, cin, D, H, W)) * (mag if which == "x" else 3.0)).astype(F4)
    dy = (unit((N, cout, D, H, W)) * (mag if which == "dy" else 3.0)).astype(F4)
    w = (rng.standard_normal((cout, cin, K, K, K)) * np.sqrt(2.0 / (cin * K ** 3))).astype(F4)
    assert np.abs(x if which == "x" else dy).max() == F4(mag)
    xt, dyt, wp = t_from_ncdhw(x), t_from_ncdhw(dy), vec(w.ravel())
    M = N * D * H * W
    floor = 2.0 ** -126
    checks = []
    if which == "x":
        yt = t_empty(N, cout, D, H, W)
        d.call("msk_conv3d_fwd", _desc(K), xt.msk(), vp(wp), None, yt.msk())
        checks.append(("fwd", yt.numpy(), O.conv3d(f8(x), f8(w), None, 1, 2), _conv_tol(cin * K ** 3)))
    else:
        dxt = t_empty(N, cin, D, H, W)
        d.call("msk_conv3d_dgrad", _desc(K), dyt.msk(), vp(wp), dxt.msk(), 0)
        checks.append(("dgrad", dxt.numpy(), O.conv3d_dgrad(f8(dy), f8(w), x.shape, 1, 2), _conv_tol(cout * K ** 3)))
    dw = vec(np.full(w.size, np.nan, F4))
    d.call("msk_conv3d_wgrad", _desc(K), xt.msk(), dyt.msk(), vp(dw), None, 0)
    checks.append(("wgrad", vec_back(dw, w.size).reshape(w.shape), O.conv3d_wgrad(f8(dy), f8(x), (K, K, K), 1, 2)[0], 2 * _conv_tol(M)))
    bad = []
    for name, got, ref, tol in checks:
        err, bound = np.abs(got - ref).max() if np.isfinite(got).all() else np.inf, tol * np.abs(ref).max() + floor
        print("%s max|ref| %.3e  err %.3e  bound %.3e  zeros %d/%d  nonfinite %d" % (name, np.abs(ref).max(), err, bound, int((got == 0).sum()),
                                                                                     got.size, int((~np.isfinite(got)).sum())))
        if not err <= bound:
            bad.append(name)
    assert not bad, bad


# ==== E. the amax ring ====================================================================================================================
def test_amax_ring_recycles_zeroed_and_counts():
    """msk_scalar_slots: 1024 arrays of 64 floats in two halves, each cleared when the cursor enters it."""
    from medicalseg_amd._lib import MskError
    d = dev()
    ARR, RING, HALF = 256, 1024, 512
    served0 = d.get_option("scalar_ring_served")
    count = [0]

    def take(n):
        count[0] += n
        return d.amax_new(n)

    # the ring's first array: the first pointer that is lower than the one before it (the cursor wraps to index 0)
    prev = take(1)
    for _ in range(RING + 1):
        p = take(1)
        if p < prev:
            break
        prev = p
    assert p < prev, "the ring did not come round in 1025 requests"
    base = p
    idx = lambda q: (q - base) // ARR
    # a written array is handed out again zeroed after 1024 further requests
    written = take(1)
    assert idx(written) == 1
    d.h2d(written, np.full(64, 7.0, F4))
    assert np.all(_amax(written) == 7.0)
    for _ in range(RING - 1):
        p = take(1)
    assert idx(p) == 0
    p = take(1)
    assert p == written and np.all(_bits(_amax(p)) == 0)
    # requests of 3 never straddle the halves: from index 2, 169 of them end at 509; the next one starts at 512, not 509 / 510 / 511
    for i in range(169):
        p = take(3)
        assert idx(p) == 2 + 3 * i
    p = take(1)
    assert idx(p) == 509
    p = take(3)
    assert idx(p) == HALF
    for i in range(1, 170):                                # 515 .. 1021
        p = take(3)
        assert idx(p) == HALF + 3 * i and idx(p) + 2 < RING
    p = take(3)                                           # 1022 + 3 > 1024: back to the start
    assert p == base
    assert (d.get_option("scalar_ring_served") - served0) & 0x3FFFFFFF == count[0]
    with pytest.raises(MskError):
        d.amax_new(HALF + 1)                              # more than half the ring
    ok = take(1)                                          # the context stays usable, and the refused request was not counted
    assert idx(ok) == 3 and np.all(_bits(_amax(ok)) == 0)
    assert (d.get_option("scalar_ring_served") - served0) & 0x3FFFFFFF == count[0]

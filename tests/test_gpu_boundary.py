"""msk_label_sdf / msk_boundary_loss_fwd / msk_boundary_loss_bwd (medicalseg_amd/csrc/msk_loss_boundary.hip) and the loss objects on
top of them against tests/boundary_reference.py, the numpy statement: the signed distance maps bit for bit, the loss record and the
gradient within the project's bounds for a float32 evaluation of float64 formulas.

Bounds.  The loss is a sum of signed terms that cancel, so its 1e-5 bound is taken against A, the mean of the absolute terms
(the float32 evaluation of the statement stays within 1.5e-7 A: tests/test_boundary_host.py).  The gradient takes the bounds of
tests/test_gpu_region_loss.py: max-abs <= 2e-5 max|g| and relative L2 <= 1e-5 (float32 statement: 5.5e-7 max|g|)."""
import ctypes as C
import functools
import os
import random
import re
import warnings

import numpy as np
import pytest

import boundary_reference as B
import region_reference as R
from helpers import dev, dfree, dmalloc, redzone_check, t_from_ncdhw, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACED = (2.5, 1.0, 0.7)


def _ws_bytes(d, h, w):
    b = C.c_size_t(0)
    assert dev().lib.msk_sdf_workspace(d, h, w, C.byref(b)) == 0
    return b.value


def _ilabels(y):
    """int32 labels -> guarded device buffer"""
    y = np.ascontiguousarray(y, np.int32)
    p = dmalloc(y.nbytes)
    dev().h2d(p, y)
    return p


def _spacing(sp):
    return None if sp is None else (C.c_double * 3)(*sp)


def _mask(S):
    return sum(1 << c for c in S)


# ---- 1. the maps --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sdf_labels(name):
    if name == "5x6x7":
        return B.example_volume((5, 6, 7), seed=7)[None]
    if name == "2x12x33x65":       # W = 65 crosses a 64-bit ballot word; the second sample is FILLED by class 1
        return np.stack([B.example_volume((12, 33, 65), seed=65), np.full((12, 33, 65), 1, np.int32)])
    if name == "9x17x130":         # W = 130: three ballot words and a tail
        return B.example_volume((9, 17, 130), seed=130)[None]
    rng = np.random.default_rng(20)
    y = rng.integers(0, 20, (1, 4, 16, 16)).astype(np.int32)
    y[:, :, 0, :] = 255
    return y


@functools.lru_cache(maxsize=None)
def _sdf_reference(name, S, spaced):
    return B.distance_maps(_sdf_labels(name), list(S), SPACED if spaced else None)


SDF_CASES = [("5x6x7", (1, 2, 3)), ("5x6x7", (0,)), ("2x12x33x65", (1, 2, 3)), ("2x12x33x65", (2,)), ("9x17x130", (0, 1, 2, 3)),
             ("9x17x130", (1, 63)), ("c20", tuple(range(1, 20)))]


@pytest.mark.parametrize("spaced", [False, True], ids=["unit", "spaced"])
@pytest.mark.parametrize("name,S", SDF_CASES, ids=["%s-%s" % (n, "all19" if len(s) == 19 else "_".join(map(str, s))) for n, s in SDF_CASES])
def test_label_sdf_is_the_statement_bit_for_bit(name, S, spaced):
    d = dev()
    y = _sdf_labels(name)
    N, D, H, W = y.shape
    V = D * H * W
    ref = _sdf_reference(name, S, spaced)
    if name != "c20":               # present, absent and (second sample) volume-filling classes, and the strip of 255
        assert (y == 1).any() and not (y == 3).any() and (y == 255).any()
    yp, ws, phi = _ilabels(y), dmalloc(_ws_bytes(D, H, W)), dmalloc(N * len(S) * V * 4)
    d.call("msk_label_sdf", vp(yp), N, D, H, W, C.c_uint64(_mask(S)), _spacing(SPACED if spaced else None), vp(ws),
           C.c_size_t(_ws_bytes(D, H, W)), vp(phi))
    got = d.d2h(phi, (N, len(S), D, H, W), np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.signbit(got[got == 0]).any()
    assert np.array_equal(d.d2h(yp, y.shape, np.int32), y)          # labels are not modified
    if name == "2x12x33x65" and 1 in S:
        assert not got[1].any() and got[0].any()                    # the filled sample: class 1 fills it, every other is absent
    for p in (yp, ws, phi):
        dfree(p)


@pytest.mark.parametrize("spaced", [False, True], ids=["unit", "spaced"])
def test_metric_signed_distance_on_a_device_volume(spaced):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import metric
    y = _sdf_labels("9x17x130")
    sp = SPACED if spaced else None
    yt = to_tensor(y)
    for c in (1, 2, 3):
        out = metric.signed_distance(yt, cls=c, spacing=sp)
        got = out.numpy()
        out.free()
        assert got.dtype == np.float32 and got.shape == y.shape[1:]
        assert np.array_equal(got.view(np.uint32), metric.signed_distance(y[0], cls=c, spacing=sp).view(np.uint32))
        assert np.array_equal(got.view(np.uint32), B.signed_distance(y[0], c, sp).view(np.uint32))
    with pytest.raises(ValueError):
        metric.signed_distance(yt, cls=64)


# ---- 2. the loss kernels ------------------------------------------------------------------------------------------------------------
# voxels: less than one tile of 256 / two samples of 210, the second starting inside a 16-byte quad when C = 3 (the dense
# 3-class tensor then takes the element form) / no multiple of 256, two samples
SHAPES = {"210": (1, 5, 6, 7), "2x210": (2, 5, 6, 7), "51480": (2, 12, 33, 65)}
CLASSES = [3, 4, 5, 8, 20, 40]                                   # flat tile; flat; ladder without quads; quads; quads; no tile


def _set_for(Cn):
    """every class but 0 for the small heads; a strict subset with a gap, an absent class and the last class for the wide ones"""
    return tuple(range(1, Cn)) if Cn <= 5 else (1, 2, 3, Cn - 1)


@functools.lru_cache(maxsize=None)
def _case(shape_id, Cn):
    """logits, labels and the float64 statement of one (shape, C), computed once and shared (never modified)"""
    N, D, H, W = SHAPES[shape_id]
    rng = np.random.default_rng(1000 * Cn + D)
    y = np.stack([B.example_volume((D, H, W), seed=Cn + s) for s in range(N)])
    y[rng.random(y.shape) < 0.03] = Cn - 1
    y.flat[1] = Cn + 2                               # outside [0, C), not ignored: takes no part
    z = (rng.standard_normal((N, Cn, D, H, W)) * 2).astype(np.float32)
    S = _set_for(Cn)
    ref = B.boundary_loss(z, y, S)
    for a in (z, y, ref["grad"], ref["phi"]):
        a.setflags(write=False)
    return z, y, S, ref


def _tensor(z, sliced):
    """the logits dense or as a channel slice of a buffer 4 channels wider; -> (tensor to pass, the whole tensor)"""
    if not sliced:
        t = t_from_ncdhw(z)
        return t, t
    N, Cn, D, H, W = z.shape
    wide = (np.random.default_rng(99).standard_normal((N, Cn + 4, D, H, W)) * 50).astype(np.float32)   # large: a wrong channel shows
    wide[:, 1:1 + Cn] = z
    tw = t_from_ncdhw(wide)
    return tw.channel_slice(1, 1 + Cn), tw


def _fwd(zt, yp, S, phi, ignore=255):
    d = dev()
    Cn = zt.c
    out, stats = vec(np.full(2 + Cn, 7.0)), dmalloc((3 + Cn) * 8)
    d.call("msk_boundary_loss_fwd", zt.msk(), vp(yp), ignore, C.c_uint64(_mask(S)), vp(phi), vp(out), vp(stats))
    return stats, vec_back(out, 2 + Cn), d.d2h(stats, (3 + Cn,), np.float64)


def _grad_ok(got, ref):
    """max-abs <= 2e-5 max|g| and relative L2 <= 1e-5"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    if scale == 0:
        return not got.any()
    return np.abs(got - ref).max() <= 2e-5 * scale and np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref)


def _check_record(out, stats, ref, Cn, S, tag):
    A = ref["abs"]
    print("%s: L %.6e (ref %.6e, |diff| / A %.2e), A rel %.2e, per class max |diff| / A %.2e" % (
        tag, out[0], ref["loss"], abs(float(out[0]) - ref["loss"]) / A, abs(float(out[1]) - A) / A,
        np.abs(out[2:].astype(np.float64) - ref["per_class"]).max() / A))
    assert stats[0] == ref["n_valid"]                                         # exact
    outside = [c for c in range(Cn) if c not in S]
    assert not out[2:][outside].any() and not stats[3:][outside].any()        # exact zeros outside the set
    assert abs(float(out[0]) - ref["loss"]) <= 1e-5 * A
    assert abs(float(out[1]) - A) <= 1e-5 * A
    assert np.abs(out[2:].astype(np.float64) - ref["per_class"]).max() <= 1e-5 * A      # the same bound per class
    assert np.abs(stats[1:] - ref["stats"][1:]).max() <= 1e-5 * ref["stats"][2]


@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("Cn", CLASSES)
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_forward_and_backward_match_the_statement_in_every_form(shape_id, Cn, layout):
    d = dev()
    z, y, S, ref = _case(shape_id, Cn)
    N, D, H, W = y.shape
    yp, phi = _ilabels(y), vec(ref["phi"])
    zt, whole = _tensor(z, layout == "slice")
    stats_p, out, stats = _fwd(zt, yp, S, phi)
    _check_record(out, stats, ref, Cn, S, "%s C=%d %s" % (shape_id, Cn, layout))
    flat_y = y.reshape(-1)
    invalid = (flat_y == 255) | (flat_y < 0) | (flat_y >= Cn)
    assert invalid.any()
    outside = [c for c in range(Cn) if c not in S]
    coef = 1.5
    want = coef * ref["grad"]
    base = (np.random.default_rng(5).standard_normal(z.shape) * np.abs(want).max()).astype(np.float32)
    for acc in (0, 1):
        if layout == "slice":       # the gradient as a channel slice too: the other channels of the buffer must stay as they are
            wide = np.full((N, Cn + 4, D, H, W), 3.0, np.float32)
            wide[:, 2:2 + Cn] = base if acc else 7.0
            dzw = t_from_ncdhw(wide)
            dz = dzw.channel_slice(2, 2 + Cn)
        else:
            dzw = dz = t_from_ncdhw(base if acc else np.full_like(z, 7.0))
        d.call("msk_boundary_loss_bwd", zt.msk(), vp(yp), 255, C.c_uint64(_mask(S)), vp(phi), vp(stats_p), C.c_float(coef), acc, dz.msk())
        got = dz.numpy()
        g = np.moveaxis(got, 1, -1).reshape(-1, Cn)
        if acc:
            assert _grad_ok(got, base.astype(np.float64) + want)              # base + ref, held to the gradient's bounds
            assert np.array_equal(g[invalid], np.moveaxis(base, 1, -1).reshape(-1, Cn)[invalid])   # untouched at invalid voxels
        else:
            assert _grad_ok(got, want)
            assert not g[invalid].any()                                       # exactly 0
            assert np.abs(got[:, outside]).max() > 0                          # classes outside the set do get a gradient
        if layout == "slice":
            rest = np.delete(dzw.numpy(), np.s_[2:2 + Cn], axis=1)
            assert np.all(rest == 3.0)
        dfree(dzw.ptr)
    for p in (yp, phi, stats_p, whole.ptr):
        dfree(p)


@pytest.mark.parametrize("Cn", [3, 5, 8])
def test_dense_and_slice_and_two_calls_give_the_same_bits(Cn):
    d = dev()
    z, y, S, ref = _case("51480", Cn)
    yp, phi = _ilabels(y), vec(ref["phi"])
    runs = []
    for sliced in (False, False, True):
        zt, whole = _tensor(z, sliced)
        stats_p, out, stats = _fwd(zt, yp, S, phi)
        dz = t_from_ncdhw(np.zeros_like(z))
        d.call("msk_boundary_loss_bwd", zt.msk(), vp(yp), 255, C.c_uint64(_mask(S)), vp(phi), vp(stats_p), C.c_float(1.0), 0, dz.msk())
        runs.append((out.view(np.uint32), stats.view(np.uint64), dz.numpy().view(np.uint32)))
        for p in (stats_p, dz.ptr, whole.ptr):
            dfree(p)
    for a, b in zip(runs[0], runs[1]):               # two calls: the same bits
        assert np.array_equal(a, b)
    assert np.array_equal(runs[0][1][:1], runs[2][1][:1])   # n_valid of a channel slice (a lane's own loads) is the dense tensor's


@pytest.mark.parametrize("Cn", [3, 8, 40])
def test_no_valid_voxel_gives_zero(Cn):
    d = dev()
    shape = (2, 5, 6, 7)
    z = np.random.default_rng(5).standard_normal((2, Cn) + shape[1:]).astype(np.float32)
    y = np.full(shape, 255, np.int32)
    y.flat[3] = Cn                                   # out of range, not ignored: no part either
    S = (1, 2)
    yp, zt, phi = _ilabels(y), t_from_ncdhw(z), vec(np.ones((2, 2) + shape[1:], np.float32))
    stats_p, out, stats = _fwd(zt, yp, S, phi)
    assert not out.any() and not stats.any()
    for acc in (0, 1):
        dz = t_from_ncdhw(np.full_like(z, 7.0))
        d.call("msk_boundary_loss_bwd", zt.msk(), vp(yp), 255, C.c_uint64(_mask(S)), vp(phi), vp(stats_p), C.c_float(1.0), acc, dz.msk())
        assert np.all(dz.numpy() == (7.0 if acc else 0.0))


def test_argument_errors_launch_nothing():
    from medicalseg_amd._lib import MskError
    from medicalseg_amd.device import Tensor
    d = dev()
    rng = np.random.default_rng(3)
    D, H, W = 4, 4, 5
    V = D * H * W
    y = rng.integers(0, 3, (1, D, H, W)).astype(np.int32)
    yp = _ilabels(y)
    need = _ws_bytes(D, H, W)
    assert need >= 16 * V
    b = C.c_size_t(0)
    for dims in ((0, 4, 4), (4, 2049, 4), (4, 4, -1)):
        assert d.lib.msk_sdf_workspace(*dims, C.byref(b)) != 0
    assert d.lib.msk_sdf_workspace(4, 4, 4, None) != 0
    ws, phi = dmalloc(need + 64), vec(np.full(2 * V + 16, 7.0))

    def sdf(labels=yp, n=1, d_=D, h=H, w=W, mask=0b110, sp=None, w_=ws, wb=need, p=phi):
        d.call("msk_label_sdf", vp(labels), n, d_, h, w, C.c_uint64(mask), _spacing(sp), vp(w_), C.c_size_t(wb), vp(p))

    for kw, text in ((dict(labels=None), "null"), (dict(w_=None), "null"), (dict(p=None), "null"), (dict(mask=0), "class_mask"),
                     (dict(d_=0), "extent"), (dict(h=2049), "extent"), (dict(n=0), "extent"), (dict(n=1 << 22, d_=8, h=8, w=8), "2\\^31"),
                     (dict(w_=ws + 8), "aligned"), (dict(p=phi + 4), "aligned"), (dict(wb=need - 1), "smaller"),
                     (dict(sp=(1.0, 0.0, 1.0)), "spacing"), (dict(sp=(1e200, 1.0, 1.0)), "spacing"), (dict(sp=(1.0, -2.0, 1.0)), "spacing"),
                     (dict(p=ws), "overlap")):
        with pytest.raises(MskError, match=text):
            sdf(**kw)
    assert np.all(vec_back(phi, 2 * V + 16) == 7.0)
    sdf()
    assert np.all(vec_back(phi, 2 * V) != 7.0) and np.all(vec_back(phi, 2 * V + 16)[2 * V:] == 7.0)

    z3 = rng.standard_normal((1, 3, D, H, W)).astype(np.float32)
    t3 = t_from_ncdhw(z3)
    t1, t65 = t_from_ncdhw(z3[:, :1]), t_from_ncdhw(rng.standard_normal((1, 65, D, H, W)).astype(np.float32))
    big = Tensor(d, t3.ptr, 2, 1024, 1024, 1024, 3)                  # N V = 2^31: refused before anything is read
    tall = Tensor(d, t3.ptr, 1, 2049, 1, 1, 3)
    out, stats = vec(np.full(5, 7.0)), vec(np.full(12, 7.0))

    def fwd(zt=t3, labels=yp, mask=0b110, p=phi, o=out, s=stats):
        d.call("msk_boundary_loss_fwd", zt.msk(), vp(labels), 255, C.c_uint64(mask), vp(p), vp(o), vp(s))

    def bwd(zt=t3, labels=yp, mask=0b110, p=phi, s=stats, dz=None):
        d.call("msk_boundary_loss_bwd", zt.msk(), vp(labels), 255, C.c_uint64(mask), vp(p), vp(s), C.c_float(1.0), 0, dz.msk())

    common = ((dict(zt=t1), r"\[2,64\]"), (dict(zt=t65), r"\[2,64\]"), (dict(mask=0), "class_mask"), (dict(mask=0b1000), "class_mask"),
              (dict(mask=1 << 63), "class_mask"), (dict(zt=big), "2\\^31"), (dict(zt=tall), "extent"), (dict(labels=None), "null"),
              (dict(p=None), "null"), (dict(p=phi + 4), "aligned"))
    for kw, text in common + ((dict(o=None), "null"), (dict(s=None), "null")):
        with pytest.raises(MskError, match=text):
            fwd(**kw)
    assert np.all(vec_back(out, 5) == 7.0) and np.all(vec_back(stats, 12) == 7.0)
    fwd()
    assert np.all(vec_back(out, 5) != 7.0)
    dz3 = t_from_ncdhw(np.full_like(z3, 7.0))
    for kw, text in common + ((dict(s=None), "null"),):
        with pytest.raises(MskError, match=text):
            bwd(dz=dz3, **kw)
    for shape in ((1, 2, D, H, W), (1, 3, D, H, W + 1)):             # mismatched shapes
        dz = t_from_ncdhw(np.full(shape, 7.0, np.float32))
        with pytest.raises(MskError, match="shape"):
            bwd(dz=dz)
        assert np.all(dz.numpy() == 7.0)
    phi_t = Tensor(d, phi, 1, D, H, W, 3)                            # a gradient tensor laid over the maps
    for dz in (t3, phi_t):
        with pytest.raises(MskError, match="overlap"):
            bwd(dz=dz)
    assert np.all(dz3.numpy() == 7.0) and np.array_equal(t3.numpy(), z3)
    bwd(dz=dz3)
    assert np.all(dz3.numpy() != 7.0)


# ---- 3. the training stack ----------------------------------------------------------------------------------------------------------
class _Capture:
    """Stands in as the producer of a logits tensor: records the gradient Scalar.backward hands over and passes it on."""
    num_outputs = 1

    def __init__(self, inner):
        self.inner, self.grads = inner, []

    def backward(self, g):
        self.grads.append(g.numpy())
        self.inner.backward(g)


def _labels(rng, shape):
    y = np.stack([B.example_volume(shape[1:], seed=11 + s) for s in range(shape[0])])
    y[rng.random(shape) < 0.05] = 255
    return y


@pytest.mark.parametrize("kind", ["boundary", "diceboundary", "mixed_ce_boundary"])
def test_losses_hand_the_vnet_the_sum_of_the_statements(kind):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import BoundaryLoss, CrossEntropyLoss, DiceBoundaryLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(4)
    model = VNet(num_classes=3)
    model.train()
    x = rng.standard_normal((1, 1, 16, 16, 16)).astype(np.float32)
    y = _labels(rng, (1, 16, 16, 16))
    losses = {"boundary": {"types": [BoundaryLoss(spacing=SPACED)], "coef": [2.0]},
              "diceboundary": {"types": [DiceBoundaryLoss(lambda_dice=1.0, lambda_boundary=0.05)], "coef": [2.0]},
              "mixed_ce_boundary": {"types": [MixedLoss([CrossEntropyLoss(weight=[1.0, 1.0, 1.0]), BoundaryLoss(classes=[2])], [1, 0.25])],
                                    "coef": [2.0]}}[kind]
    logits = model(x)[0]
    cap = _Capture(logits.producer)
    logits.producer = cap
    loss_list, dice = loss_computation([logits], to_tensor(y), losses)
    z = logits.numpy()
    if kind == "boundary":
        bd = B.boundary_loss(z, y, spacing=SPACED)
        value, grad, scale = 2.0 * bd["loss"], 2.0 * bd["grad"], 2.0 * bd["abs"]
    elif kind == "diceboundary":
        bd, sd = B.boundary_loss(z, y), R.region_loss(z, y, smooth=float(np.float32(1e-5)))
        value, grad, scale = 2.0 * (sd["L_r"] + 0.05 * bd["loss"]), 2.0 * (sd["grad"] + 0.05 * bd["grad"]), 2.0 * (sd["L_r"] + 0.05 * bd["abs"])
        assert np.asarray(dice).shape == (3,)
    else:
        bd, ce = B.boundary_loss(z, y, [2]), R.region_loss(z, y, lambda_r=0.0, lambda_f=1.0)
        value, grad, scale = 2.0 * (ce["loss"] + 0.25 * bd["loss"]), 2.0 * (ce["grad"] + 0.25 * bd["grad"]), 2.0 * (ce["loss"] + 0.25 * bd["abs"])
    loss = sum(loss_list)
    print("%s: loss %.6e, statement %.6e, scale %.3e" % (kind, float(loss), value, scale))
    assert abs(float(loss) - value) <= 1e-5 * scale
    loss.backward()
    assert len(cap.grads) == 1 and _grad_ok(cap.grads[0], grad)
    assert all(np.isfinite(p.grad_numpy()).all() for p in model.parameters() if p.arena is not None and p.arena.grad_ptr is not None)


def test_native_heads_build_one_map_per_head_from_its_own_label_level(monkeypatch):
    import pyramid_reference as P
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.device import Device, to_tensor
    from medicalseg_amd.models import DiceBoundaryLoss, VNetDeepSup
    from medicalseg_amd.models.losses.fused import BoundaryNode
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(8)
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=3, native_heads=True)
    model.train()
    opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    shape = (16, 32, 32)                             # 32 x 32 x 16 in x, y, z
    x = rng.standard_normal((1, 1) + shape).astype(np.float32)
    y = _labels(rng, (1,) + shape)
    losses = {"types": [DiceBoundaryLoss(lambda_boundary=0.05) for _ in range(4)], "coef": [0.25] * 4}
    names = []
    real = Device.call
    monkeypatch.setattr(Device, "call", lambda self, name, *a: (names.append(name), real(self, name, *a))[1])
    values = []
    for step in range(2):
        outs = model(x)
        heads = [(o.d, o.h, o.w) for o in outs]
        assert len(outs) == 4 and heads[0] == shape and len(set(heads)) > 1
        del names[:]
        loss_list, dice = loss_computation(outs, to_tensor(y), losses)
        assert len(loss_list) == 4
        if step == 0:
            labels = [y] + P.label_pyramid(y, heads[1:])
            for o, lab, term in zip(outs, labels, loss_list):
                node = [t[1] for t in term.terms if type(t[1]) is BoundaryNode][0]
                assert tuple(node.labels.shape) == (1, o.d, o.h, o.w) and np.array_equal(node.labels.numpy(), lab)
                sd, bd = R.region_loss(o.numpy(), lab, smooth=float(np.float32(1e-5))), B.boundary_loss(o.numpy(), lab)
                assert abs(float(term) - 0.25 * (sd["L_r"] + 0.05 * bd["loss"])) <= 1e-5 * 0.25 * (sd["L_r"] + 0.05 * bd["abs"]), o.shape
        loss = sum(loss_list)
        values.append(float(loss))
        loss.backward()
        assert names.count("msk_label_sdf") == 4 and names.count("msk_boundary_loss_fwd") == 4 and names.count("msk_boundary_loss_bwd") == 4
        opt.step()
    assert np.all(np.isfinite(values))
    assert all(np.isfinite(p.numpy()).all() for p in model.parameters())


def test_two_iterations_from_the_diceboundary_yaml_save_a_checkpoint(tmp_path, capsys):
    """configs/synthetic/vnet_synthetic_ct_patch_diceboundary_96.yml shrunk to a 16^3 patch of 20 x 16 x 24 volumes"""
    from medicalseg_amd.core import train
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.models import DiceBoundaryLoss
    src = open(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_diceboundary_96.yml")).read()
    for old, new in (("'../_base_/global_configs.yml'", "'%s'" % os.path.join(ROOT, "configs", "_base_", "global_configs.yml")),
                     ("iters: 100", "iters: 2"), ("num_samples: 16", "num_samples: 4"), ("size: [96, 96, 96]", "size: [16, 16, 16]")):
        assert old in src, old
        src = src.replace(old, new)
    assert src.count("shape: [144, 128, 160]") == 2
    src = src.replace("shape: [144, 128, 160]", "shape: [20, 16, 24]")
    p = tmp_path / "diceboundary_16.yml"
    p.write_text(src)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # data_root warning
        cfg = Config(str(p))
    losses = cfg.loss
    assert type(losses["types"][0]) is DiceBoundaryLoss and losses["types"][0].lambda_boundary == 0.01
    random.seed(0)
    train(cfg.model, cfg.train_dataset, optimizer=cfg.optimizer, save_dir=str(tmp_path / "o"), iters=cfg.iters,
          batch_size=cfg.batch_size, save_interval=2, log_iters=1, losses=losses)
    logged = [float(v) for v in re.findall(r"\[TRAIN\].*? loss: ([^,]+),", capsys.readouterr().out)]
    assert len(logged) == 2 and np.isfinite(logged).all(), logged
    saved = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path / "o")) for f in fs]
    assert any(f.endswith("model.pdparams") for f in saved), saved

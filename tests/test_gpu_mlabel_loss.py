"""The region-based training loss on the device (msk_mlabel_loss_fwd / msk_mlabel_loss_bwd,
medicalseg_amd/csrc/msk_loss_mlabel.hip) against the float64 statement tests/mlabel_reference.py.

Bounds: the region family's (tests/test_gpu_region_loss.py): the losses and the per-region Dice within 1e-5 relative, the
gradient max-abs <= 2e-5 max|g| and relative L2 <= 1e-5, the {TP, SP, ST} record within 1e-6 relative with ST exact.  A float32
numpy evaluation of the statement lies within 2.5e-7 (losses), 3.3e-7 of max|g| and 8.7e-8 (gradient) of the float64 one at
these shapes (tests/test_mlabel_host.py).  smooth enters the statement as the float32 value the kernels hold."""
import ctypes as C

import numpy as np
import pytest

import mlabel_cases as K
import mlabel_reference as M
from helpers import dev, dfree, dmalloc, redzone_check, t_from_ncdhw, vec, vec_back, vp  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu


def _upload(a):
    p = dmalloc(a.nbytes)
    dev().h2d(p, np.ascontiguousarray(a))
    return p


def _settings(tp, sq, batch, table_len=K.V, smooth=K.SMOOTH):
    return (255, vp(tp), int(table_len), int(sq), int(batch), C.c_float(smooth))


def _fwd(zt, yp, settings, groups):
    R = zt.c
    out, stats = vec(np.zeros(2 + R)), dmalloc((5 * groups * R + 2) * 8)
    dev().call("msk_mlabel_loss_fwd", zt.msk(), vp(yp), *settings, vp(out), vp(stats))
    return vec_back(out, 2 + R), stats


def _bwd(zt, yp, settings, stats, coef_bce, coef_dice, acc, dt):
    dev().call("msk_mlabel_loss_bwd", zt.msk(), vp(yp), *settings, vp(stats), C.c_float(coef_bce), C.c_float(coef_dice), int(acc),
               dt.msk())


def _check_forward(tag, out, st, ref, G, R):
    print(tag, "L_bce %.3e L_dice %.3e dice %.3e" % (K.rel_worst(out[0], ref["L_bce"]), K.rel_worst(out[1], ref["L_dice"]),
                                                     K.rel_worst(out[2:], ref["dice"])))
    assert K.rel_ok(out[0], ref["L_bce"]), (tag, out[0], ref["L_bce"])
    assert K.rel_ok(out[1], ref["L_dice"]), (tag, out[1], ref["L_dice"])
    assert K.rel_ok(out[2:], ref["dice"]), (tag, out[2:], ref["dice"])
    TP, SP, ST, A, B = (st[k * G * R:(k + 1) * G * R].reshape(G, R) for k in range(5))
    assert K.rel_ok(TP, ref["TP"], 1e-6) and K.rel_ok(SP, ref["SP"], 1e-6), tag
    assert np.array_equal(ST, ref["ST"]), tag
    assert K.rel_ok(A, ref["A"]) and K.rel_ok(B, ref["B"]), tag
    assert K.rel_ok(st[-2], ref["bce_sum"], 1e-6) and st[-1] == ref["valid"], tag


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("R", K.REGION_COUNTS)
def test_mlabel_kernels_match_statement(R, shape, layout):
    d = dev()
    N, D, H, W = shape
    rng = np.random.default_rng(R * 1000 + D * 10 + N)
    z, y = K.make_data(rng, shape, R)
    yp, tp = _upload(y), _upload(K.make_table(R))
    sliced, acc = layout.startswith("slice"), layout.endswith("acc")
    c0, wide = (1, R + 3) if sliced else (0, R)
    zw = np.zeros((N, wide, D, H, W), np.float32)
    zw[:, c0:c0 + R] = z
    zt = t_from_ncdhw(zw).channel_slice(c0, c0 + R) if sliced else t_from_ncdhw(z)
    coef_bce, coef_dice = 0.75, 1.25
    for sq, batch in K.OPTIONS:
        tag = (R, shape, layout, sq, batch)
        G = 1 if batch else N
        settings = _settings(tp, sq, batch)
        ref = K.reference(z, y, R, sq, batch, coef_bce, coef_dice)
        assert np.isfinite(ref["grad"]).all() and ref["valid"] > 0
        out, stats = _fwd(zt, yp, settings, G)
        st = d.d2h(stats, (5 * G * R + 2,), np.float64)
        _check_forward(tag, out, st, ref, G, R)
        base = (rng.standard_normal((N, wide, D, H, W)) * np.abs(ref["grad"]).max()).astype(np.float32)
        dw = t_from_ncdhw(base)
        dt = dw.channel_slice(c0, c0 + R) if sliced else dw
        _bwd(zt, yp, settings, stats, coef_bce, coef_dice, acc, dt)
        got = dw.numpy()
        mine = got[:, c0:c0 + R]
        if acc:    # as tests/test_gpu_region_loss.py: the stored sum against old + gradient, and the gradient's own max-abs bound
            under = base[:, c0:c0 + R].astype(np.float64)
            print(tag, "gradient added: max-abs %.3e of max|g|" % (np.abs(mine - under - ref["grad"]).max() / np.abs(ref["grad"]).max()))
            assert K.grad_ok(mine, under + ref["grad"]), tag
            assert np.abs(mine - under - ref["grad"]).max() <= 2e-5 * np.abs(ref["grad"]).max(), tag
        else:
            print(tag, "gradient: max-abs %.3e of max|g|, relative L2 %.3e" % K.grad_err(mine, ref["grad"]))
            assert K.grad_ok(mine, ref["grad"]), tag
            assert not np.moveaxis(mine, 1, -1)[y == 255].any(), tag        # m = 0: exactly 0
        if sliced:   # the other channels of the wide buffer are untouched
            assert np.array_equal(got[:, :c0], base[:, :c0]) and np.array_equal(got[:, c0 + R:], base[:, c0 + R:])
        dfree(dw.ptr)
        dfree(stats)


@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("R", [3, 8, 20])
def test_mlabel_kernels_give_the_same_bits_dense_and_as_a_view(R, batch):
    """A dense tensor travels through the LDS tiles (flat at 3 regions with batch_dice, quads at 8 and 20), a channel slice of a
    wider buffer through a lane's own loads and stores; the voxel of a thread, the plan and the arithmetic per voxel are the
    same, so the record, the statistics and both gradients are the same bits."""
    d = dev()
    shape = N, D, H, W = (2, 5, 7, 9)
    rng = np.random.default_rng(700 + R)
    z, y = K.make_data(rng, shape, R)
    yp, tp = _upload(y), _upload(K.make_table(R))
    G = 1 if batch else N
    settings = _settings(tp, 1, batch)
    c0, wide = 2, R + 4
    zw = rng.standard_normal((N, wide, D, H, W)).astype(np.float32)
    zw[:, c0:c0 + R] = z
    base = rng.standard_normal((N, wide, D, H, W)).astype(np.float32)
    got = {}
    for layout in ("dense", "view"):
        zt = t_from_ncdhw(zw).channel_slice(c0, c0 + R) if layout == "view" else t_from_ncdhw(z)
        out, stats = _fwd(zt, yp, settings, G)
        res = [out, d.d2h(stats, (5 * G * R + 2,), np.float64)]
        for acc in (0, 1):
            dw = t_from_ncdhw(base if layout == "view" else base[:, c0:c0 + R])
            dt = dw.channel_slice(c0, c0 + R) if layout == "view" else dw
            _bwd(zt, yp, settings, stats, 0.75, 1.25, acc, dt)
            g = dw.numpy()
            res.append(g[:, c0:c0 + R] if layout == "view" else g)
        got[layout] = res
    for what, a, b in zip(("out", "stats", "gradient", "gradient added"), got["dense"], got["view"]):
        assert np.array_equal(a, b), what
    assert np.abs(got["dense"][2]).max() > 0 and np.isfinite(got["dense"][0]).all()


@pytest.mark.parametrize("R,batch", [(3, 1), (3, 0), (20, 1), (5, 0)])
def test_two_calls_give_the_same_bits(R, batch):
    d = dev()
    shape = (2, 9, 16, 17)
    z, y = K.make_data(np.random.default_rng(11), shape, R)
    yp, tp, zt = _upload(y), _upload(K.make_table(R)), t_from_ncdhw(z)
    settings = _settings(tp, 0, batch)
    G = 1 if batch else 2
    runs = []
    for _ in range(2):
        out, stats = _fwd(zt, yp, settings, G)
        dz = t_from_ncdhw(np.zeros_like(z))
        _bwd(zt, yp, settings, stats, 1.0, 1.0, 0, dz)
        runs.append((out.view(np.uint32), d.d2h(stats, (5 * G * R + 2,), np.uint64), dz.numpy().view(np.uint32)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("R", [1, 3, 8])
def test_all_voxels_ignored(R):
    z = np.random.default_rng(5).standard_normal((2, R, 5, 7, 9)).astype(np.float32)
    y = np.full((2, 5, 7, 9), 255, np.int32)
    yp, tp, zt = _upload(y), _upload(K.make_table(R)), t_from_ncdhw(z)
    for batch in (0, 1):
        settings = _settings(tp, 0, batch)
        out, stats = _fwd(zt, yp, settings, 1 if batch else 2)
        assert np.isfinite(out).all() and out[0] == 0.0 and out[1] == 0.0 and np.all(out[2:] == 1.0)
        dz = t_from_ncdhw(np.full_like(z, 7.0))
        _bwd(zt, yp, settings, stats, 1.0, 1.0, 0, dz)
        assert not dz.numpy().any()


@pytest.mark.parametrize("name", sorted(K.MULTI))
def test_multi_round_grids(name):
    """Some workgroups run a second round (the LDS tile is reused) and the last tile is ragged; sized from the device's CU
    count."""
    d = dev()
    case = K.MULTI[name]
    R = case["R"]
    num_cu = d.get_option("num_cu")
    shape = K.multi_round_shape(case, num_cu)
    K.check_premise(case, shape, num_cu)
    rng = np.random.default_rng(900 + R)
    z, y = K.make_data(rng, shape, R)
    yp, tp, zt = _upload(y), _upload(K.make_table(R)), t_from_ncdhw(z)
    settings = _settings(tp, 1, 1)
    ref = K.reference(z, y, R, 1, 1)
    out, stats = _fwd(zt, yp, settings, 1)
    st = d.d2h(stats, (5 * R + 2,), np.float64)
    _check_forward(name, out, st, ref, 1, R)
    if case["pass"] == "bwd":
        base = (rng.standard_normal(z.shape) * np.abs(ref["grad"]).max()).astype(np.float32)
        dz = t_from_ncdhw(base)
        _bwd(zt, yp, settings, stats, 0.75, 1.25, case["acc"], dz)
        got = dz.numpy()
        want = base.astype(np.float64) + ref["grad"]
        print(name, "gradient added: max-abs %.3e of max|g|" % (np.abs(got - want).max() / np.abs(ref["grad"]).max()))
        assert K.grad_ok(got, want) and np.abs(got - want).max() <= 2e-5 * np.abs(ref["grad"]).max()


def test_argument_errors_launch_nothing():
    d = dev()
    from medicalseg_amd._lib import MskError
    rng = np.random.default_rng(3)
    y = rng.integers(0, 3, (1, 4, 4, 4)).astype(np.int32)
    yp, tp = _upload(y), _upload(K.make_table(3))
    t3 = t_from_ncdhw(rng.standard_normal((1, 3, 4, 4, 4)).astype(np.float32))
    t33 = t_from_ncdhw(rng.standard_normal((1, 33, 4, 4, 4)).astype(np.float32))
    good = _settings(tp, 0, 1)

    def refused(zt, settings, text, labels=yp):
        out, stats = vec(np.full(2 + zt.c, 7.0)), dmalloc((5 * zt.c + 2) * 8)
        dz = t_from_ncdhw(np.full((1, zt.c, 4, 4, 4), 7.0, np.float32))
        with pytest.raises(MskError, match=text):
            d.call("msk_mlabel_loss_fwd", zt.msk(), vp(labels), *settings, vp(out), vp(stats))
        with pytest.raises(MskError, match=text):
            _bwd(zt, labels, settings, stats, 1.0, 1.0, 0, dz)
        assert np.all(vec_back(out, 2 + zt.c) == 7.0) and np.all(dz.numpy() == 7.0)

    refused(t33, good, r"\[1,32\]")
    refused(t3, _settings(tp, 0, 1, table_len=0), r"\[1,256\]")
    refused(t3, _settings(tp, 0, 1, table_len=257), r"\[1,256\]")
    refused(t3, _settings(None, 0, 1), "null")
    refused(t3, good, "null", labels=None)
    refused(t3, (255, C.c_void_p(tp + 2), K.V, 0, 1, C.c_float(K.SMOOTH)), "aligned")
    refused(t3, _settings(tp, 0, 1, smooth=-1.0), "smooth")
    out, stats = vec(np.full(5, 7.0)), dmalloc(17 * 8)
    with pytest.raises(MskError, match="null"):
        d.call("msk_mlabel_loss_fwd", t3.msk(), vp(yp), *good, None, vp(stats))
    with pytest.raises(MskError, match="null"):
        d.call("msk_mlabel_loss_fwd", t3.msk(), vp(yp), *good, vp(out), None)
    with pytest.raises(MskError, match="aligned"):
        d.call("msk_mlabel_loss_fwd", t3.msk(), vp(yp), *good, vp(out), C.c_void_p(stats + 4))
    d.call("msk_mlabel_loss_fwd", t3.msk(), vp(yp), *good, vp(out), vp(stats))
    for shape in ((1, 2, 4, 4, 4), (1, 3, 4, 4, 5)):
        dz = t_from_ncdhw(np.full(shape, 7.0, np.float32))
        with pytest.raises(MskError, match="shape"):
            _bwd(t3, yp, good, stats, 1.0, 1.0, 0, dz)
        assert np.all(dz.numpy() == 7.0)
    # 2 x 1024^3 = 2^31 voxels: refused by the descriptor alone, whatever lies behind the pointer
    from medicalseg_amd._lib import MskTensor
    huge = MskTensor(t3.ptr, 2, 1024, 1024, 1024, 3, 3)
    with pytest.raises(MskError, match="voxel count"):
        d.call("msk_mlabel_loss_fwd", huge, vp(yp), *good, vp(out), vp(stats))
    with pytest.raises(MskError, match="voxel count"):
        d.call("msk_mlabel_loss_bwd", huge, vp(yp), *good, vp(stats), C.c_float(1.0), C.c_float(1.0), 0, huge)
    before = t3.numpy()
    with pytest.raises(MskError, match="overlaps"):
        _bwd(t3, yp, good, stats, 1.0, 1.0, 0, t3)
    assert np.array_equal(t3.numpy(), before)
    assert np.all(vec_back(out, 5) != 7.0)

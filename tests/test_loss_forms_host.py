"""tests/loss_forms_cases.py on a machine without a GPU: the restated grid and form rules against the launchers' text and against
hand-worked numbers, the premise of every multi-round case of tests/test_gpu_loss_forms.py at four CU counts, the coverage of the
class-count sweep, and the CE + Dice statement against oracle.vnet_numpy."""
import os
import re

import numpy as np
import pytest

import loss_forms_cases as L
from oracle import vnet_numpy as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "medicalseg_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_ladder_and_caps_are_the_launchers():
    """the numbers the restatement rests on, where the launchers write them"""
    dev_h = _src("msk_device.h")
    assert tuple(int(m) for m in re.findall(r"MSK_TPV_STEP\((\d+), QUAD_", dev_h)) == L.LADDER
    assert "constexpr int kTpvThreads = 256;" in dev_h and "long b = (total + 255) / 256;" in dev_h
    assert "static inline int msk_ew_blocks(long total, int num_cu, int per_cu = 16)" in dev_h
    optim = _src("msk_loss_optim.hip")
    assert "nb = (int)(tiles < 3L * ctx->num_cu ? tiles : 3L * ctx->num_cu);" in optim
    assert "const int blocks = msk_ew_blocks(voxels * CB, ctx->num_cu);" in optim and "const int tb = msk_ew_blocks(voxels, ctx->num_cu);" in optim
    assert "if ((C > 4 && C <= 32) || flat4)" in optim and "LOSS_STATS_TPV(4, 2);" in optim and "LOSS_BWD_TPV(4, 2);" in optim
    region = _src("msk_loss_region.hip")
    assert "long w = (long)num_cu * per_cu / p.nseg;" in region
    assert "msk_quad_dense(logits), batch_dice, ctx->num_cu, 3);" in region and "batch_dice, ctx->num_cu, 16);" in region
    assert "p.st = !dense ? 0 : (C <= 4 ? (seg_aligned ? 2 : 0) : ((C % 4 == 0 && C <= 32) ? 1 : 0));" in region
    boundary = _src("msk_loss_boundary.hip")
    assert "long w = (long)num_cu * per_cu / t.n;" in boundary
    assert "class_mask, ctx->num_cu, 3);" in boundary and "class_mask, ctx->num_cu, 16);" in boundary
    assert "p.st = !dense ? 0 : (C <= 4 ? (seg_aligned ? 2 : 0) : ((C % 4 == 0 && C <= 32) ? 1 : 0));" in boundary
    topk = _src("msk_loss_topk.hip")
    assert "const int nb = msk_ew_blocks(V, ctx->num_cu, 4);" in topk and "const int nb = msk_ew_blocks(V, ctx->num_cu, 16);" in topk
    assert "return !dense ? 0 : (C <= 4 ? 2 : ((C % 4 == 0 && C <= 32) ? 1 : 0));" in topk
    bce = _src("msk_loss_bce.hip")
    assert "constexpr int kTileV = 1024;" in bce and "const long cap = 8L * num_cu;" in bce
    for text in (region, boundary, topk):
        assert "if (C <= 4) { if (" in text and "else LAUNCH(64, 0);" in text and "MSK_TPV_LADDER(C, " in text


# (family, pass, C, dense, voxels before a second round at 256 CUs)
FIRST_ROUND = [("ce_dice", "stats", 8, True, 196608), ("region", "stats", 8, True, 196608), ("boundary", "stats", 8, True, 196608),
               ("topk", "stats", 8, True, 262144), ("bce", "stats", 3, True, 2097152), ("bce", "bwd", 3, True, 2097152),
               ("ce_dice", "bwd", 8, True, 1048576), ("region", "bwd", 8, True, 1048576), ("boundary", "bwd", 8, True, 1048576),
               ("topk", "bwd", 8, True, 1048576), ("ce_dice", "bwd", 40, True, 16384), ("ce_dice", "bwd", 3, False, 262144)]


@pytest.mark.parametrize("family,which,C,dense,first", FIRST_ROUND)
def test_voxels_before_a_second_round_at_256_cus(family, which, C, dense, first):
    for v, rounds in ((first, 1), (first + 1, 2)):
        p = L.plan(family, which, (1, 1, 1, v), C, 256, dense=dense)
        assert p["max_rounds"] == rounds, (v, p)
    assert L.plan(family, which, (1, 1, 1, 1000), C, 256, dense=dense)["wg"] == -(-1000 // L.plan(family, which, (1, 1, 1, 1000), C, 256, dense=dense)["tile"])


def test_grouped_plans_split_the_cap_between_the_groups():
    p = L.plan("region", "bwd", (3, 1, 1, 400000), 3, 256, batch_dice=False)
    assert (p["groups"], p["wg"], p["vox"]) == (3, 16 * 256 // 3, 400000) and p["max_rounds"] == 2
    assert L.plan("region", "bwd", (3, 1, 1, 400000), 3, 256, batch_dice=True)["groups"] == 1
    p = L.plan("boundary", "stats", (2, 5, 7, 9), 3, 256)
    assert (p["groups"], p["wg"], p["tiles"], p["ragged"]) == (2, 2, 2, True)
    assert L.plan("ce_dice", "stats", (1, 1, 1, 5000), 3, 256, dense=False) is None          # loss_stats_k: contiguous ranges


def test_form_rule():
    assert [L.ladder_cm(c) for c in (5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 32)] == [8, 8, 12, 12, 16, 16, 20, 20, 24, 24, 32, 32]
    for fam in ("region", "topk", "boundary"):
        assert L.form(fam, 3, True) == (4, 2) and L.form(fam, 3, False) == (4, 0)
        assert L.form(fam, 8, True) == (8, 1) and L.form(fam, 8, False) == (8, 0) and L.form(fam, 7, True) == (8, 0)
        assert L.form(fam, 28, True) == (32, 1) and L.form(fam, 33, True) == (64, 0) and L.form(fam, 64, False) == (64, 0)
    assert L.form("region", 3, True, seg_aligned=False) == (4, 0) and L.form("boundary", 2, True, seg_aligned=False) == (4, 0)
    assert L.form("topk", 3, True, seg_aligned=False) == (4, 2)                                   # one group: nothing to align
    assert L.form("ce_dice", 3, True) == (4, 2) and L.form("ce_dice", 3, False) is None and L.form("ce_dice", 1, True) is None
    assert L.form("ce_dice", 5, False) == (8, 0) and L.form("ce_dice", 32, True) == (32, 1) and L.form("ce_dice", 33, True) is None
    assert not L.seg_aligned("region", (3, 1, 1, 101), 3, batch_dice=False) and L.seg_aligned("region", (3, 1, 1, 101), 3, batch_dice=True)
    assert L.seg_aligned("boundary", (2, 1, 1, 100), 3) and not L.seg_aligned("boundary", (2, 5, 7, 9), 2)


@pytest.mark.parametrize("num_cu", L.NUM_CUS)
@pytest.mark.parametrize("case", L.MULTI + [L.CONCENTRATED], ids=lambda c: c["id"])
def test_every_multi_round_case_has_a_second_round_and_a_ragged_tile(case, num_cu):
    shape = L.multi_round_shape(case, num_cu)
    p = L.check_premise(case, shape, num_cu)
    assert shape[0] == case["N"] and p["vox"] * p["groups"] == int(np.prod(shape))
    dense = case["layout"] == "dense"
    f = L.form(case["family"], case["C"], dense, L.seg_aligned(case["family"], shape, case["C"], bool(case["batch"])))
    if case["mod4"] is not None and case["family"] in ("region", "boundary"):
        assert f == ((4, 2) if case["mod4"] == 0 else (4, 0)), (case["id"], f)       # group offsets, on and off a quad
    if case["id"].startswith("bce-C3"):
        assert (p["vox"] % L.BCE_TILE) * 3 % 4 != 0                                    # the last tile ends in a scalar tail
    if sized_for_bwd(case) and case["family"] != "bce" and case["size"] != "lanes":
        s = L.case_plan(case, "stats", shape, num_cu)
        assert s["tiles"] >= 3.3 * s["wg"]                                             # the statistics pass runs 4 rounds or more
    assert int(np.prod(shape)) * (case["C"] + (0 if dense else case["extra"])) * 4 <= 48 << 20, "logits above 48 MiB"
    if case is L.CONCENTRATED:
        tiles = L.concentrated_tiles(p["wg"], p["tiles"])
        assert tiles[0] < p["wg"] <= tiles[2] and all(t + 1 < p["tiles"] for t in tiles)


def sized_for_bwd(case):
    return L.sized_pass(case) == "bwd"


def test_the_multi_round_table_holds_what_it_should():
    ids = set(L.MULTI_BY_ID)
    assert len(ids) == len(L.MULTI)
    by_family = {f: [c for c in L.MULTI if c["family"] == f] for f in L.FAMILIES}
    assert {(c["C"], c["layout"], c["size"]) for c in by_family["ce_dice"]} >= {
        (3, "dense", "bwd"), (3, "slice", "lanes"), (5, "dense", "bwd"), (8, "dense", "bwd"), (20, "dense", "stats"), (40, "dense", "lanes")}
    assert {(c["C"], c["layout"]) for c in by_family["bce"]} == {(1, "dense"), (3, "dense"), (2, "slice")}
    assert all(c["acc"] == (0, 1) for c in by_family["bce"])
    for fam in ("topk", "boundary"):
        assert {(c["C"], c["layout"]) for c in by_family[fam] if c["size"] == "bwd"} == {(3, "dense"), (8, "dense"), (5, "slice")}
        assert any(1 in c["acc"] for c in by_family[fam])
    assert any(c["C"] == 8 and c["batch"] and c["acc"] == (0, 1) for c in by_family["region"])
    assert {c["mod4"] for c in by_family["region"] if c["N"] == 3 and not c["batch"]} == {0, 1}
    assert {c["act"] for c in by_family["region"]} == {"softmax", "sigmoid"}
    for fam in ("ce_dice", "region", "topk", "boundary"):           # each statistics pass: a two-round case and one of 3.3 rounds
        assert {"stats", "stats33"} <= {c["size"] for c in by_family[fam]} or fam == "topk"
    assert any(c["size"] == "stats" for c in by_family["topk"])


@pytest.mark.parametrize("family", [f for f in L.FAMILIES if f != "bce"])
def test_the_sweep_reaches_every_launchable_form(family):
    assert L.sweep_forms(family) == L.launchable(family)
    assert set(L.SWEEP_CLASSES) >= {4, 5, 32, 33, 64, 16, 24}
    p = L.plan(family, "stats", L.SWEEP_SHAPE, 8, 256)
    if p is not None:
        assert p["ragged"] and p["tiles"] >= 2 and p["wg"] == p["tiles"]


def test_bce_element_to_voxel_is_exact_where_the_sweep_goes():
    """elem_voxel of msk_loss_bce.hip in float32: (int)((i + 0.5f) * (1.f / C)) == i // C for every C <= 64 and i < 65 536"""
    i = np.arange(65536, dtype=np.int64)
    for C in range(1, 65):
        inv = np.float32(1.0) / np.float32(C)
        v = ((i.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)
        assert np.array_equal(v, i // C), C
    for C, shape in L.BCE_EDGE:
        assert int(np.prod(shape)) == L.BCE_TILE + 1
    assert L.BCE_EDGE[0][0] * L.BCE_TILE - 1 == 65535 and 1 in L.sweep_classes("bce") and 1 not in L.sweep_classes("topk")


def test_make_data_has_the_edges_the_kernels_treat_apart():
    for Cn in (1, 3, 8):
        z, y = L.make_data(np.random.default_rng(Cn), L.SWEEP_SHAPE, Cn)
        assert z.dtype == np.float32 and y.dtype == np.int32 and z.shape == (2, Cn, 5, 7, 9)
        assert 0.05 < (y == 255).mean() < 0.15
        if Cn > 1:
            assert y.flat[1] == Cn + 2 and z[0, 1, 0, 0, 2] == 30.0 and z[0, 0, 0, 0, 2] == -30.0 and y[0, 0, 0, 2] == 1


def test_concentrated_data_puts_every_member_in_its_tiles():
    import topk_reference as T
    G, ntile, Cn = 8, 20, 3
    tiles = L.concentrated_tiles(G, ntile)
    shape = (1, 1, 1, ntile * 256 - 100)
    z, y = L.concentrated_data(np.random.default_rng(0), shape, Cn, tiles)
    l, valid = T.voxel_loss(z, y)
    in_tiles = np.zeros(l.size, bool)
    for t in tiles:
        in_tiles[t * 256:(t + 1) * 256] = True
    assert l[valid & in_tiles].min() > 3.0 and l[valid & ~in_tiles].max() < 1e-2
    k = 100.0 * 0.5 * (valid & in_tiles).sum() / valid.sum()
    ref = T.topk_ce(z, y, k)
    assert 0 < ref["K"] < (valid & in_tiles).sum() and not ref["u"][~in_tiles].any()


@pytest.mark.parametrize("dice_softmax,weighted", [(False, False), (True, False), (False, True), (True, True)])
def test_ce_dice_statement_is_the_oracle_where_the_oracle_applies(dice_softmax, weighted):
    """labels inside [0, C), a few of them ignore_index = 255 for the CE term only: oracle.vnet_numpy says the same"""
    rng = np.random.default_rng(9)
    Cn, shape = 5, (2, 3, 4, 5)
    z = rng.standard_normal((2, Cn) + shape[1:]) * 2
    y = rng.integers(0, Cn, shape).astype(np.int32)
    w = rng.uniform(0.5, 2, Cn)
    dw = rng.uniform(0.5, 2, Cn) if weighted else None
    ref = L.ce_dice_reference(z, y, w, 255, dice_softmax, dw)
    dl, per, ddl = O.dice(z, y, sigmoid_norm=not dice_softmax, weight=dw)
    ce, dce = O.cross_entropy(z, y, w, 255)
    assert np.allclose(ref["dice"], dl, rtol=1e-13, atol=0) and np.allclose(ref["per"], per, rtol=1e-13, atol=0)
    assert np.allclose(ref["ddice"], ddl, rtol=1e-12, atol=1e-18) and ref["ce"] == ce and np.array_equal(ref["dce"], dce)
    # masking: ignored voxels leave the CE term, a label outside [0, C) leaves both targets, an ignore_index inside [0, C) stays
    # in the Dice target
    y2 = y.copy()
    y2[0, 0, 0, :3] = 255
    y2[1, 0, 0, 0] = Cn + 2
    ref2 = L.ce_dice_reference(z, y2, w, 255, dice_softmax, dw)
    keep = np.ones(shape, bool)
    keep[0, 0, 0, :3] = False
    keep[1, 0, 0, 0] = False
    assert not np.moveaxis(ref2["dce"], 1, -1)[~keep].any() and np.moveaxis(ref2["dce"], 1, -1)[keep].any()
    ref0 = L.ce_dice_reference(z, y, w, 0, dice_softmax, dw)
    assert np.array_equal(ref0["per"], ref["per"]) and ref0["ce"] != ref["ce"]
    assert not np.moveaxis(ref0["dce"], 1, -1)[y == 0].any()

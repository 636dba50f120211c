"""Grid rules, form rules, case tables, data and bounds of tests/test_gpu_loss_forms.py, restated in plain Python (no device code
is imported here: tests/test_loss_forms_host.py checks all of it on a machine without a GPU).

The five loss families (CE + Dice: msk_loss_optim.hip, region: msk_loss_region.hip, BCE: msk_loss_bce.hip, top-k CE:
msk_loss_topk.hip, boundary: msk_loss_boundary.hip) share one structure: a workgroup of 256 threads takes tiles of consecutive
voxels, the grid is capped at a few workgroups per CU, and from a workgroup's second tile (its second ROUND) on the LDS tile, and
in topk_bwd_k the prefetched label and loss, are reused.  `plan()` restates each launcher's grid, `form()` each family's choice of
kernel instantiation (CM, ST), and `multi_round_shape()` sizes a case from the device's CU count so that some workgroups run one
round more than the others and the last tile is ragged:

    voxels per group = (m G + k) T + r,   G the workgroups of a group, T the tile, 0 < k < G, 0 < r < T, m >= 1

so k + 1 workgroups run m + 1 rounds and the others m.  k = G // 8 + 1: an eighth of the grid takes the extra round (one
workgroup would do for the premise; an eighth spreads the later round over every CU at no measurable cost)."""
import numpy as np

from oracle import vnet_numpy as O

TPV_TILE = 256          # kTpvThreads: voxels per tile of the thread-per-voxel kernels
BCE_TILE = 1024         # kTileV of msk_loss_bce.hip
LADDER = (8, 12, 16, 20, 24, 32)
NUM_CUS = (64, 104, 256, 304)     # the CU counts the host test evaluates every case at
f32 = lambda v: float(np.float32(v))
SMOOTH, TVERSKY = f32(1e-5), (f32(0.3), f32(0.7))
ACT = {"softmax": 0, "sigmoid": 1}


def ceil_div(a, b):
    return -(-a // b)


def pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


# ---- grid rules --------------------------------------------------------------------------------------------------------------------
def ew_blocks(total, num_cu, per_cu=16):
    """msk_ew_blocks (msk_device.h): clamp(ceil(total / 256), 1, num_cu * per_cu)"""
    return max(1, min(ceil_div(total, 256), num_cu * per_cu))


def _plan(groups, vox_per_group, wg, tile):
    tiles = ceil_div(vox_per_group, tile)
    return {"groups": groups, "vox": vox_per_group, "wg": wg, "tile": tile, "tiles": tiles,
            "min_rounds": tiles // wg, "max_rounds": ceil_div(tiles, wg), "ragged": vox_per_group % tile != 0}


def _grouped(nseg, vox, num_cu, per_cu):
    """region_plan / boundary_plan: workgroups per group = clamp(num_cu * per_cu / nseg, 1, tiles of the group)"""
    seg_vox = vox // nseg
    tiles = ceil_div(seg_vox, TPV_TILE)
    return _plan(nseg, seg_vox, max(1, min(num_cu * per_cu // nseg, tiles)), TPV_TILE)


def plan(family, which, shape, C, num_cu, dense=True, batch_dice=True):
    """The grid of one pass: {"groups", "vox" (voxels of a group), "wg" (workgroups of a group), "tile" (voxels a workgroup
    takes per round), "tiles", "min_rounds", "max_rounds", "ragged"}.  which: "stats" (the forward pass over the logits) or
    "bwd".  None where the pass has no rounds (loss_stats_k gives each workgroup one contiguous range)."""
    N = shape[0]
    V = int(np.prod(shape))
    if family == "ce_dice":
        tpv = form("ce_dice", C, dense) is not None
        if which == "stats":
            return _plan(1, V, min(ceil_div(V, TPV_TILE), 3 * num_cu), TPV_TILE) if tpv else None
        if tpv:
            return _plan(1, V, ew_blocks(V, num_cu), TPV_TILE)
        CB = pow2ceil(C)                                     # loss_bwd_k: CB lanes per voxel, 256 / CB voxels per round
        return _plan(1, V, ew_blocks(V * CB, num_cu), 256 // CB)
    if family == "region":
        return _grouped(1 if batch_dice else N, V, num_cu, 3 if which == "stats" else 16)
    if family == "boundary":
        return _grouped(N, V, num_cu, 3 if which == "stats" else 16)
    if family == "topk":
        return _plan(1, V, ew_blocks(V, num_cu, 4 if which == "stats" else 16), TPV_TILE)
    if family == "bce":
        return _plan(1, V, min(ceil_div(V, BCE_TILE), 8 * num_cu), BCE_TILE)
    raise ValueError(family)


# ---- form rules --------------------------------------------------------------------------------------------------------------------
def ladder_cm(C):
    """MSK_TPV_LADDER: the register array of 4 < C <= 32 classes, in steps of a quad"""
    return next(cm for cm in LADDER if C <= cm)


def form(family, C, dense, seg_aligned=True):
    """(CM, ST) of the instantiation a call launches; None for CE + Dice's lane-per-class kernels (loss_stats_k / loss_bwd_k).
    dense: ld == C and 16-byte aligned (logits, and in a backward pass the gradient too).  seg_aligned (region without
    batch_dice, boundary): one group, or every group starts on a 16-byte quad (voxels of a group x C divisible by 4)."""
    if family == "bce":
        return None
    if 4 < C <= 32:
        return ladder_cm(C), 1 if dense and C % 4 == 0 else 0
    if family == "ce_dice":                                  # the st / flat4 predicates of msk_loss_fwd_ex / msk_loss_bwd_ex
        return (4, 2) if 2 <= C <= 4 and dense else None
    if C <= 4:                                               # region_plan / boundary_plan / topk_form
        return 4, 2 if dense and (seg_aligned or family == "topk") else 0
    return 64, 0


def launchable(family):
    """every (CM, ST) the family's dispatch can launch; None stands for the lane-per-class kernels"""
    ladder = {(cm, st) for cm in LADDER for st in (0, 1)}
    if family == "ce_dice":
        return ladder | {(4, 2), None}
    return ladder | {(4, 0), (4, 2), (64, 0)}


def seg_aligned(family, shape, C, batch_dice=True):
    groups = 1 if (family == "region" and batch_dice) or family not in ("region", "boundary") else shape[0]
    return groups == 1 or (int(np.prod(shape[1:])) * C) % 4 == 0


# ---- the multi-round cases ----------------------------------------------------------------------------------------------------------
# size: which pass the voxel count is made for.  "stats": the statistics pass (3 workgroups per CU; top-k: 4), two rounds for
# some; "stats33": the same pass with at least 3.3 rounds; "bwd": the gradient pass (16 per CU; BCE: 8 per CU, both passes);
# "lanes": loss_bwd_k, 256 / CB voxels per round, m = 2 at CB = 64 (2.3 x 16 num_cu x 4 voxels).  A slice is channels 1 .. C of a
# buffer with ld = C + extra.
def _c(id, family, C, layout, size, **kw):
    d = {"id": id, "family": family, "C": C, "layout": layout, "size": size, "N": 1, "batch": 1, "acc": (0,), "mod4": None, "extra": 3}
    d.update(kw)
    return d


MULTI = [
    _c("cedice-C3-dense-stats", "ce_dice", 3, "dense", "stats"),
    _c("cedice-C3-dense-stats33", "ce_dice", 3, "dense", "stats33"),
    _c("cedice-C3-dense-bwd", "ce_dice", 3, "dense", "bwd"),
    _c("cedice-C3-slice-lanes", "ce_dice", 3, "slice", "lanes"),
    _c("cedice-C5-dense-stats", "ce_dice", 5, "dense", "stats"),
    _c("cedice-C5-dense-bwd", "ce_dice", 5, "dense", "bwd"),
    _c("cedice-C8-dense-stats", "ce_dice", 8, "dense", "stats"),
    _c("cedice-C8-dense-bwd", "ce_dice", 8, "dense", "bwd"),
    _c("cedice-C20-dense-stats", "ce_dice", 20, "dense", "stats"),
    _c("cedice-C40-dense-lanes", "ce_dice", 40, "dense", "lanes"),
    # region: softmax with focal gamma = 2 and class weights, one sigmoid case with squared_pred
    _c("region-C8-dense-batch-bwd", "region", 8, "dense", "bwd", acc=(0, 1), act="softmax"),
    _c("region-C3-N3-unaligned-bwd", "region", 3, "dense", "bwd", N=3, batch=0, mod4=1, act="softmax"),      # ST 0, group offsets
    _c("region-C3-N3-aligned-bwd", "region", 3, "dense", "bwd", N=3, batch=0, mod4=0, act="sigmoid"),        # ST 2, group offsets
    _c("region-C3-dense-batch-stats", "region", 3, "dense", "stats", act="softmax"),
    _c("region-C3-dense-batch-stats33", "region", 3, "dense", "stats33", act="softmax"),
    # BCE: dynamic weight and pos_weight, writing and adding
    _c("bce-C1-dense", "bce", 1, "dense", "bwd", acc=(0, 1)),
    _c("bce-C3-dense", "bce", 3, "dense", "bwd", acc=(0, 1), mod4=1),            # 3 r floats in the last tile, r odd: a scalar tail
    _c("bce-C2-slice", "bce", 2, "slice", "bwd", acc=(0, 1), extra=2),   # ld = 4: 2.4 M voxels stay below 48 MiB
    # top-k CE at k = 10 per cent
    _c("topk-C3-dense-stats", "topk", 3, "dense", "stats"),
    _c("topk-C3-dense-bwd", "topk", 3, "dense", "bwd", acc=(0, 1)),
    _c("topk-C8-dense-bwd", "topk", 8, "dense", "bwd"),
    _c("topk-C5-slice-bwd", "topk", 5, "slice", "bwd", acc=(1,)),
    # boundary: two samples, synthetic phi
    _c("boundary-C3-dense-stats", "boundary", 3, "dense", "stats", N=2, mod4=0),
    _c("boundary-C3-dense-stats33", "boundary", 3, "dense", "stats33", N=2, mod4=0),
    _c("boundary-C3-dense-bwd", "boundary", 3, "dense", "bwd", N=2, mod4=0),
    _c("boundary-C8-dense-bwd", "boundary", 8, "dense", "bwd", N=2, acc=(1,)),
    _c("boundary-C5-slice-bwd", "boundary", 5, "slice", "bwd", N=2),
]
MULTI_BY_ID = {c["id"]: c for c in MULTI}
CONCENTRATED = _c("topk-C3-dense-concentrated", "topk", 3, "dense", "bwd", acc=(0, 1))


def sized_pass(case):
    """the pass whose rounds the case is sized for"""
    return "stats" if case["size"] in ("stats", "stats33") else "bwd"


def _cap(case, num_cu):
    """(G, T, m): the workgroup cap of a group, the voxels a workgroup takes per round, the rounds every workgroup runs"""
    fam, size, C = case["family"], case["size"], case["C"]
    nseg = case["N"] if (fam == "boundary" or (fam == "region" and not case["batch"])) else 1
    if fam == "bce":
        return 8 * num_cu, BCE_TILE, 1
    if size == "lanes":
        CB = pow2ceil(C)
        return 16 * num_cu, 256 // CB, (2 if CB == 64 else 1)
    per_cu = 16 if size == "bwd" else (4 if fam == "topk" else 3)
    return num_cu * per_cu // nseg, TPV_TILE, 1


def _factor3(v):
    """v = d h w with every extent <= 2048 (kMaxExtent of the boundary loss), or None"""
    for w in range(min(2048, v), 0, -1):
        if v % w:
            continue
        rest = v // w
        if rest > 2048 * 2048:
            return None
        for h in range(min(2048, rest), 0, -1):
            if rest % h == 0:
                return (rest // h, h, w) if rest // h <= 2048 else None
    return None


def multi_round_shape(case, num_cu):
    """(N, D, H, W) of a case on a device of num_cu CUs: per group (m G + k) T + r voxels, see the module docstring.  r is the
    first value from T / 3 upwards that meets the case's wish for the group's voxel count modulo 4 (mod4: 0 = every group starts
    on a quad, 1 = it does not) and, for the boundary loss, factors into three extents <= 2048."""
    G, T, m = _cap(case, num_cu)
    if case["size"] == "stats33":
        full = ceil_div(33 * G, 10)
    elif m == 2:
        full = 2 * G + (3 * G) // 10
    else:
        full = G + G // 8 + 1
    for r in list(range(T // 3 + 1, T)) + list(range(1, T // 3 + 1)):
        v = full * T + r
        if case["mod4"] is not None and (v % 4 == 0) != (case["mod4"] == 0):
            continue
        if case["family"] == "boundary":
            dhw = _factor3(v)
            if dhw is None:
                continue
            return (case["N"],) + dhw
        return (case["N"], 1, 1, v)
    raise ValueError("no ragged voxel count for %s at %d CUs" % (case["id"], num_cu))


def case_plan(case, which, shape, num_cu):
    return plan(case["family"], which, shape, case["C"], num_cu, dense=case["layout"] == "dense", batch_dice=bool(case["batch"]))


def check_premise(case, shape, num_cu):
    """What every multi-round test asserts first: in the pass it is sized for some workgroup runs a second round, not all run
    the same number, the last tile is ragged (stats33: at least 3.3 rounds on average); and the form is the one the id names."""
    p = case_plan(case, sized_pass(case), shape, num_cu)
    assert p is not None and p["max_rounds"] >= 2 and p["ragged"], (case["id"], p)
    assert p["min_rounds"] >= 1 and p["max_rounds"] == p["min_rounds"] + 1, (case["id"], p)
    assert p["wg"] * p["groups"] <= 16 * num_cu
    if case["size"] == "stats33":
        assert p["tiles"] >= 3.3 * p["wg"], (case["id"], p)
    if case["size"] == "lanes":
        assert form("ce_dice", case["C"], case["layout"] == "dense") is None
    if case["family"] == "boundary":
        assert max(shape[1:]) <= 2048
    return p


# ---- the class-count sweep -----------------------------------------------------------------------------------------------------------
SWEEP_SHAPE = (2, 5, 7, 9)                                   # 315 voxels per sample: a full tile and a ragged one per group
SWEEP_CLASSES = (2, 4, 5, 7, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 64)
SWEEP_LAYOUTS = ("dense", "slice")                           # slice: channels 1 .. C of a buffer with ld = C + 3
FAMILIES = ("ce_dice", "region", "bce", "topk", "boundary")
# region: (activation, squared_pred, batch_dice, do_bg, tversky, focal_on, gamma, weighted)
REGION_SWEEP = (("softmax", 0, 1, 0, None, 1, 2.0, True), ("sigmoid", 1, 0, 1, None, 0, 0.0, False))
REGION_MULTI = {"softmax": ("softmax", 0, None, 0, None, 1, 2.0, True), "sigmoid": ("sigmoid", 1, None, 1, None, 0, 0.0, False)}
BCE_EDGE = ((64, (1, 1, 25, 41)), (47, (1, 1, 25, 41)))      # 1024 + 1 voxels: a full tile, at 64 classes elements 0 .. 65 535


def sweep_classes(family):
    return ((1,) if family == "bce" else ()) + SWEEP_CLASSES


def sweep_forms(family):
    """every form the sweep table reaches in one family (forward and backward take the same form: the gradient buffer has the
    logits' layout)"""
    got = set()
    for C in sweep_classes(family):
        for layout in SWEEP_LAYOUTS:
            dense = layout == "dense"
            if family == "region":
                for combo in REGION_SWEEP:
                    if C == 1 and combo[0] == "softmax":
                        continue
                    got.add(form(family, C, dense, seg_aligned(family, SWEEP_SHAPE, C, bool(combo[2]))))
            else:
                got.add(form(family, C, dense, seg_aligned(family, SWEEP_SHAPE, C)))
    return got


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def make_data(rng, shape, Cn):
    """logits and labels as tests/test_gpu_region_loss.py builds them: about 10 % ignore_index, one label outside [0, C) that is
    not ignored, one voxel where the softmax saturates"""
    N, D, H, W = shape
    z = (rng.standard_normal((N, Cn, D, H, W), dtype=np.float32) * np.float32(2)).astype(np.float32)
    y = rng.integers(0, max(Cn, 2), (N, D, H, W)).astype(np.int32)
    y[rng.random(y.shape, dtype=np.float32) < 0.1] = 255
    if Cn > 1:
        y.flat[1] = Cn + 2                      # outside [0, C), not ignored: an all-zero target row
    k = min(1, Cn - 1)                          # one voxel where the softmax saturates: u = 1, 1 - u = 0
    y[0, 0, 0, 2] = k if Cn > 1 else 1
    z[0, :, 0, 0, 2] = -30.0
    z[0, k, 0, 0, 2] = 30.0
    return z, y


def class_set(Cn):
    """the boundary loss's class set: every class but 0 for the small heads; a strict subset with a gap and the last class else"""
    return tuple(range(1, Cn)) if Cn <= 5 else (1, 2, 3, Cn - 1)


def concentrated_data(rng, shape, Cn, member_tiles):
    """Top-k data whose members sit in a few tiles of 256 voxels: everywhere the label's logit leads by 8 to 12 (l below 1e-3),
    in `member_tiles` another class leads the label by 5 to 15 (l above 3, the noise of 0.5 on every logit counted).  With K about half the valid voxels of
    those tiles every member lies inside them, whatever the rounding of l does at the threshold."""
    N, D, H, W = shape
    V = N * D * H * W
    y = rng.integers(0, Cn, V).astype(np.int32)
    y[rng.random(V, dtype=np.float32) < 0.1] = 255
    y[1] = Cn + 2
    zv = (rng.standard_normal((V, Cn), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    yc = np.where((y >= 0) & (y < Cn), y, 0)
    rows = np.arange(V)
    zv[rows, yc] += rng.uniform(8, 12, V).astype(np.float32)
    for t in member_tiles:
        sl = slice(t * TPV_TILE, min((t + 1) * TPV_TILE, V))
        n = sl.stop - sl.start
        zv[sl] = (rng.standard_normal((n, Cn), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
        zv[rows[sl], (yc[sl] + 1) % Cn] += rng.uniform(5, 15, n).astype(np.float32)
    z = np.ascontiguousarray(np.moveaxis(zv.reshape(N, D, H, W, Cn), -1, 1))
    return z, y.reshape(N, D, H, W)


def concentrated_tiles(G, ntile):
    """member tiles for a backward grid of G workgroups: workgroup 1 goes member -> empty, 2 empty -> member, 3 member -> member,
    0 and 4 empty -> empty: every carry of the prefetched label and loss across a round, each beside tiles of the other kind"""
    tiles = [1, 3, G + 2, G + 3]
    assert G >= 5 and tiles[-1] < ntile
    return tiles


# ---- bounds (each family's own, from the test file named) ------------------------------------------------------------------------------
def rel_err(a, b):
    """tests/helpers.py"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rel_ok(got, ref, tol=1e-5):
    """tests/test_gpu_region_loss.py _rel_ok"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.all(np.where(ref == 0, got == 0, np.abs(got - ref) <= tol * np.abs(ref))))


def grad_ok(got, ref):
    """tests/test_gpu_region_loss.py, test_gpu_topk.py, test_gpu_boundary.py _grad_ok: max-abs <= 2e-5 max|g|, relative L2 <= 1e-5"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    if scale == 0:
        return not got.any()
    return bool(np.abs(got - ref).max() <= 2e-5 * scale and np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref))


def bce_grad_ok(got, ref):
    """tests/test_gpu_bce.py _grad_ok: relative L2 <= 1e-6, max-abs <= 1e-5 max|g|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    if scale == 0:
        return not got.any()
    return bool(np.linalg.norm(got - ref) / np.linalg.norm(ref) <= 1e-6 and np.abs(got - ref).max() <= 1e-5 * scale)


def bce_loss_ok(got, ref):
    """tests/test_gpu_bce.py _loss_ok"""
    return abs(got - ref) <= 1e-5 * abs(ref) if ref != 0 else got == 0


# ---- the CE + Dice statement with the kernels' masking ---------------------------------------------------------------------------------
def ce_dice_reference(z, y, w_ce, ignore_index=255, dice_softmax=False, dice_weight=None, epsilon=1e-6):
    """float64: oracle.vnet_numpy's cross_entropy and dice with the masking the statistics kernels apply.  CE skips a voxel whose
    label is ignore_index or outside [0, C).  The Dice target is one_hot(label) with an all-zero row for a label outside [0, C);
    ignore_index is not consulted there, so an ignore_index INSIDE [0, C) is counted by the Dice term and skipped by the CE
    term, and the Dice denominator sums p^2 over every voxel.  -> dict ce, dce, dice, per, ddice, T (the target counts)."""
    z64 = np.asarray(z, np.float64)
    y = np.asarray(y)
    C = z64.shape[1]
    inside = (y >= 0) & (y < C)
    ce, dce = O.cross_entropy(z64, np.where(inside, y, ignore_index), np.asarray(w_ce, np.float64), ignore_index)
    # O.dice / O._dice_general with t masked by hand (they one-hot every label, which must then lie inside [0, C))
    t = (y[:, None] == np.arange(C).reshape(1, C, 1, 1, 1)).astype(np.float64)
    p = O.softmax(z64, 1) if dice_softmax else 1.0 / (1.0 + np.exp(-z64))
    w = np.ones(C) if dice_weight is None else np.asarray(dice_weight, np.float64)
    ax = (0, 2, 3, 4)
    r = lambda v: v.reshape(1, -1, 1, 1, 1)
    inter = w * (p * t).sum(axis=ax)
    den = (p * p).sum(axis=ax) + t.sum(axis=ax)
    denc = np.maximum(den, epsilon)
    per = 2.0 * inter / denc
    g = -(1.0 / C) * (2.0 * r(w) * t / r(denc) - r(2.0 * inter / denc ** 2 * np.where(den > epsilon, 1.0, 0.0)) * 2.0 * p)
    ddice = p * (g - (g * p).sum(axis=1, keepdims=True)) if dice_softmax else g * p * (1.0 - p)
    return {"ce": float(ce), "dce": dce, "dice": float(1.0 - per.mean()), "per": per, "ddice": ddice, "T": t.sum(axis=ax)}

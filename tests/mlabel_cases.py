"""Grid rule, form rule, data and bounds of tests/test_gpu_mlabel_loss.py, restated in plain Python (no device code is imported
here: tests/test_mlabel_host.py checks all of it on a machine without a GPU).

mlabel_plan (medicalseg_amd/csrc/msk_loss_mlabel.hip) is region_plan's rule: a group is the batch (batch_dice) or a sample, a
workgroup of 256 threads takes tiles of 256 consecutive voxels inside one group, and a group gets
clamp(num_cu * per_cu / groups, 1, tiles of the group) workgroups, per_cu = 3 for the statistics pass and 16 for the gradient
pass.  multi_round_shape sizes a case by the rule of tests/loss_forms_cases.py:

    voxels per group = (m G + k) T + r,   G the workgroups of a group, T = 256, k = G // 8 + 1, 0 < r < T, m = 1

so k + 1 workgroups run two rounds, the others one, and the last tile is ragged."""
import numpy as np

import mlabel_reference as M

TILE = 256
LADDER = (8, 12, 16, 20, 24, 32)
NUM_CUS = (64, 104, 256, 304)
f32 = lambda v: float(np.float32(v))
SMOOTH = f32(1e-5)
SHAPES = [(1, 5, 7, 9), (3, 5, 7, 9), (2, 9, 16, 17), (2, 16, 16, 16)]
REGION_COUNTS = [1, 2, 3, 4, 5, 8, 12, 20, 32]
LAYOUTS = ["dense", "dense_acc", "slice", "slice_acc"]
OPTIONS = [(0, 1), (1, 0), (0, 0), (1, 1)]          # (squared_pred, batch_dice): both values of both
V = 7                                                # table length of the tests: label values 0 .. 6
# multi-round cases: one per pass
MULTI = {"stats-R3": {"R": 3, "pass": "stats", "acc": 0}, "bwd-R8-acc": {"R": 8, "pass": "bwd", "acc": 1}}


def ceil_div(a, b):
    return -(-a // b)


def plan(which, shape, num_cu, batch_dice=True):
    """{"groups", "vox", "wg", "tiles", "min_rounds", "max_rounds", "ragged"} of one pass; which: "stats" or "bwd" """
    groups = 1 if batch_dice else shape[0]
    vox = int(np.prod(shape)) // groups
    tiles = ceil_div(vox, TILE)
    wg = max(1, min(num_cu * (3 if which == "stats" else 16) // groups, tiles))
    return {"groups": groups, "vox": vox, "wg": wg, "tiles": tiles, "min_rounds": tiles // wg, "max_rounds": ceil_div(tiles, wg),
            "ragged": vox % TILE != 0}


def form(R, dense, shape, batch_dice=True):
    """(CM, ST) of the instantiation a call launches.  dense: ld == R and 16-byte aligned (logits, and in a backward pass the
    gradient too)"""
    groups = 1 if batch_dice else shape[0]
    seg_aligned = groups == 1 or (int(np.prod(shape[1:])) * R) % 4 == 0
    if R <= 4:
        return 4, 2 if dense and seg_aligned else 0
    return next(cm for cm in LADDER if R <= cm), 1 if dense and R % 4 == 0 else 0


def multi_round_shape(case, num_cu):
    G = num_cu * (3 if case["pass"] == "stats" else 16)
    full = G + G // 8 + 1
    return (1, 1, 1, full * TILE + TILE // 3 + 1)


def check_premise(case, shape, num_cu):
    p = plan(case["pass"], shape, num_cu)
    assert p["max_rounds"] == 2 and p["min_rounds"] == 1 and p["ragged"], p
    assert p["wg"] <= 16 * num_cu
    return p


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def make_table(R):
    """label values 0 .. 6: 0 belongs to no region, 1 to all, 2 .. 6 to the regions r with (r + v) % 3 == 0 and to region 0 when
    that leaves none"""
    t = np.zeros(V, dtype=np.uint32)
    t[1] = np.uint32((1 << R) - 1)
    for v in range(2, V):
        bits = sum(1 << r for r in range(R) if (r + v) % 3 == 0)
        t[v] = np.uint32(bits or 1)
    return t


def make_data(rng, shape, R):
    """logits and labels: about 10 % 255, one label at or above V and one of -1 (neither ignored: all-zero rows), value 0 (no
    region) and value 1 (all regions) present, one voxel with every logit at +100 under an all-zero target and one at -100
    under an all-one target (the naive -log(1 - p) is infinite there)"""
    N, D, H, W = shape
    z = (rng.standard_normal((N, R, D, H, W), dtype=np.float32) * np.float32(2)).astype(np.float32)
    y = rng.integers(0, V, (N, D, H, W)).astype(np.int32)
    y[rng.random(y.shape, dtype=np.float32) < 0.1] = 255
    y.flat[1] = V + 2
    y.flat[3] = -1
    y.flat[5], y.flat[6] = 0, 1
    y.flat[8] = 0
    z.reshape(N, R, -1)[0, :, 8] = 100.0
    y.flat[9] = 1
    z.reshape(N, R, -1)[0, :, 9] = -100.0
    return z, y


# ---- bounds: the region family's (tests/test_gpu_region_loss.py) ---------------------------------------------------------------------------
def rel_ok(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.all(np.where(ref == 0, got == 0, np.abs(got - ref) <= tol * np.abs(ref))))


def rel_worst(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nz = ref != 0
    return float(np.max(np.abs(got - ref)[nz] / np.abs(ref)[nz])) if nz.any() else 0.0


def grad_err(got, ref):
    """(max-abs / max|g|, relative L2)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max()), float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def grad_ok(got, ref):
    """max-abs <= 2e-5 max|g| and relative L2 <= 1e-5"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    if scale == 0:
        return not got.any()
    return bool(np.abs(got - ref).max() <= 2e-5 * scale and np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref))


def reference(z, y, R, sq, batch, coef_bce=0.75, coef_dice=1.25, dtype=np.float64):
    return M.mlabel_loss(z, y, make_table(R), bool(sq), bool(batch), SMOOTH, coef_bce, coef_dice, dtype=dtype)

"""Host side of sliding-window inference (core/infer.py SlidingPlan, evaluate's and val.py's arguments) against the numpy
statement of tests/sliding_reference.py, and the self-consistency of that statement.  No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest

import sliding_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRID = [(size, r, ov, mode) for size, r in [(5, 4), (7, 4), (9, 4), (8, 4), (2, 4), (3, 8), (4, 4), (16, 16), (24, 16), (300, 260),
                                             (13, 5), (1, 1), (10, 3)]
        for ov in (0.0, 0.25, 0.5, 0.75) for mode in ('constant', 'gaussian')]


def _plan(*a, **k):
    from medicalseg_amd.core.infer import SlidingPlan
    return SlidingPlan(*a, **k)


def test_window_starts_match_the_specification_literally():
    for (size, r, ov), want in R.LITERAL_STARTS:
        plan = _plan((size, size, size), (r, r, r), overlap=ov)
        assert plan.starts == [want, want, want], (size, r, ov)
        assert R.axis_plan(size, r, ov)[2] == want
    small = _plan((2, 5, 7), (4, 4, 4))
    assert small.padded == (4, 5, 7) and small.before == (1, 0, 0) and small.starts == [[0], [0, 1], [0, 2, 3]]
    assert _plan((1, 1, 3), (4, 4, 4)).before == (1, 1, 0)            # (r - size) // 2 in front, the rest behind


@pytest.mark.parametrize("size,r,ov,mode", GRID)
def test_plan_equals_the_reference(size, r, ov, mode):
    other = (7, 4)
    plan = _plan((size, other[0], size), (r, other[1], r), overlap=ov, mode=mode)
    ref = R.Plan((size, other[0], size), (r, other[1], r), ov, mode)
    assert plan.padded == ref.padded and plan.before == ref.before and plan.starts == ref.starts
    for got, want in zip(plan.tables, ref.tables):
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert plan.windows(2) == ref.windows(2)
    assert [plan.origin(w) for w in plan.windows(2)] == [ref.origin(w) for w in ref.windows(2)]
    # window order: batch item slowest, w fastest
    nd, nh, nw = (len(s) for s in plan.starts)
    assert plan.windows(2) == list(itertools.product(range(2), range(nd), range(nh), range(nw)))
    # every window lies inside the padded extent and the last one ends on it
    for a in range(3):
        assert plan.starts[a][0] == 0 and plan.starts[a][-1] + plan.roi_size[a] == plan.padded[a]
        assert sorted(set(plan.starts[a])) == plan.starts[a]


@pytest.mark.parametrize("size,r,ov,mode", GRID)
def test_tables_are_a_partition_of_unity(size, r, ov, mode):
    """per axis |sum_i T_i[p] - 1| <= 2^-24: every entry is rounded with relative error <= 2^-24 and the exact entries sum to 1"""
    plan = _plan((size, size, size), (r, r, r), overlap=ov, mode=mode)
    T, starts, P = plan.tables[0], plan.starts[0], plan.padded[0]
    total = np.zeros(P, np.float64)
    for row, s in zip(T, starts):
        total[s:s + r] += row.astype(np.float64)
    worst = np.abs(total - 1.0).max()
    assert worst <= 2.0 ** -24, worst
    assert (T > 0).all() and np.isfinite(T).all()


@pytest.mark.parametrize("size,r,ov", [(8, 4, .5), (12, 8, .5), (24, 16, .25), (9, 5, .5), (300, 260, .25), (2, 4, .5), (16, 4, .75)])
def test_gaussian_tables_are_symmetric_when_the_starts_are(size, r, ov):
    plan = _plan((size, size, size), (r, r, r), overlap=ov, mode='gaussian')
    starts, P, T = plan.starts[0], plan.padded[0], plan.tables[0]
    assert sorted(P - r - s for s in starts) == starts                    # the cases are chosen so
    for i, s in enumerate(starts):
        j = starts.index(P - r - s)
        assert np.array_equal(T[i], T[j][::-1]), (i, j)


@pytest.mark.parametrize("kwargs", [
    dict(overlap=1.0), dict(overlap=-0.1), dict(overlap=1.5), dict(overlap=float('nan')),
    dict(roi_size=(0, 4, 4)), dict(roi_size=(4, -1, 4)), dict(roi_size=(4, 4)), dict(roi_size=(4.0, 4, 4)),
    dict(mode='linear'), dict(mode=None),
    dict(sigma_scale=1e-3, roi_size=(64, 4, 4), shape=(64, 8, 8)),       # the profile underflows at the window border
    dict(sigma_scale=0.0), dict(sigma_scale=-1.0),
    dict(shape=(0, 8, 8)),
])
def test_plan_refuses(kwargs):
    args = dict(shape=(8, 8, 8), roi_size=(4, 4, 4))
    args.update(kwargs)
    with pytest.raises(ValueError):
        _plan(args.pop("shape"), args.pop("roi_size"), **args)


def test_constant_mode_blend_of_a_pointwise_model_is_exact():
    """overlap 0.5, volume (12, 8, 16), roi (8, 4, 8): every voxel is covered once or twice per axis, all weights are powers of
    two and the integer-valued data stay exact, so the blend IS the model of the whole volume"""
    plan = R.Plan((12, 8, 16), (8, 4, 8), 0.5, 'constant')
    for t in plan.tables:
        assert set(np.unique(t)) <= {np.float32(1.0), np.float32(0.5)}
    x = R.integer_volume(2, (12, 8, 16), 3)
    assert x.min() >= -8 and x.max() <= 8 and np.array_equal(x, np.round(x))
    got = R.blend(R.model_on_windows(R.pointwise_model, x, plan), plan, n=2)
    assert np.array_equal(got, R.pointwise_model(x))


def test_statement_pieces():
    plan = R.Plan((2, 6, 10), (4, 4, 8), 0.5, 'gaussian')
    x = R.volume(1, (2, 6, 10), 2, 0)
    ws = plan.windows(1)
    assert plan.before == (1, 0, 0) and [plan.origin(w) for w in ws][0] == (0, -1, 0, 0)
    p = R.crop(x, plan, ws[-1], cval=-3.5)
    assert p.shape == (2, 4, 4, 8)
    assert (p[:, 0] == -3.5).all() and (p[:, 3] == -3.5).all()                     # padded on d, in front and behind
    assert np.array_equal(p[:, 1:3], x[0, :, :, 2:6, 2:10])
    # overlap 0: the blend places the windows side by side
    flat = R.Plan((8, 8, 8), (4, 4, 4), 0.0, 'gaussian')
    assert all((t == 1.0).all() for t in flat.tables)
    lg = R.window_logits(flat, 1, 3, 5)
    out = R.blend(lg, flat)
    for w_, l_ in zip(flat.windows(1), lg):
        _, d0, h0, w0 = flat.origin(w_)
        assert np.array_equal(out[0, :, d0:d0 + 4, h0:h0 + 4, w0:w0 + 4], l_)
    # blend starts from a given accumulator and leaves it alone
    base = np.full((1, 3, 8, 8, 8), 2.0, np.float32)
    assert np.array_equal(R.blend(lg, flat, acc=base), (base + out).astype(np.float32)) and (base == 2.0).all()


def test_evaluate_refuses_sliding_window_with_aug_eval():
    from medicalseg_amd.core import evaluate
    with pytest.raises(ValueError, match="sliding_window"):
        evaluate(None, None, {"types": [None], "coef": [1]}, aug_eval=True, sliding_window=(16, 16, 16))


def test_val_flags():
    sys.path.insert(0, ROOT)
    try:
        import val
    finally:
        sys.path.remove(ROOT)
    a = val.parse_args(["--config", "x.yml"])
    assert a.sliding_window is None and a.sw_overlap == 0.5 and a.sw_mode == 'gaussian' and a.sw_batch_size == 1
    a = val.parse_args(["--config", "x.yml", "--sliding_window", "128", "128", "64", "--sw_overlap", "0.25", "--sw_mode",
                        "constant", "--sw_batch_size", "4"])
    assert a.sliding_window == [128, 128, 64] and a.sw_overlap == 0.25 and a.sw_mode == 'constant' and a.sw_batch_size == 4

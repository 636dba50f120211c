"""Host side of mirroring inside sliding-window inference: the self-consistency of the numpy statement
(tests/sliding_mirror_reference.py) and evaluate's / val.py's arguments.  No GPU."""
import os
import sys

import numpy as np
import pytest

import sliding_mirror_reference as M
import sliding_reference as R
import tta_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_mirrored_gather_is_about_the_window_not_the_volume():
    # volume (2, 1, 3) in a window (3, 1, 6): padding 0 / 1 on D and 1 / 2 on W, so both mirrors move the padding
    plan = R.Plan((2, 1, 3), (3, 1, 6), 0.5, 'constant')
    assert plan.before == (0, 0, 1) and plan.windows(1) == [(0, 0, 0, 0)]
    x = np.array([[1, 2, 3], [4, 5, 6]], np.float32).reshape(1, 1, 2, 1, 3)
    c = np.float32(-3.5)
    wd = plan.windows(1)[0]
    want = {0: [[c, 1, 2, 3, c, c], [c, 4, 5, 6, c, c], [c] * 6],
            1: [[c] * 6, [c, 4, 5, 6, c, c], [c, 1, 2, 3, c, c]],
            4: [[c, c, 3, 2, 1, c], [c, c, 6, 5, 4, c], [c] * 6],
            5: [[c] * 6, [c, c, 6, 5, 4, c], [c, c, 3, 2, 1, c]]}
    for mask, rows in want.items():
        got = M.gather(x, plan, wd, mask, cval=c)
        assert got.shape == (1, 3, 1, 6)
        assert np.array_equal(got[0, :, 0, :], np.array(rows, np.float32)), mask
    assert np.array_equal(M.gather(x, plan, wd, 2, cval=c), M.gather(x, plan, wd, 0, cval=c))       # extent 1: H mirrors onto itself


def test_work_list_and_masks():
    assert M.masks_of(()) == [0] and M.masks_of((2,)) == [0, 4] and M.masks_of((0, 1)) == [0, 1, 2, 3]
    assert M.masks_of((2, 0)) == [0, 1, 4, 5] and M.masks_of((0, 1, 2)) == list(range(8))
    from medicalseg_amd.core.infer import tta_passes
    for axes in [(), (1,), (2, 0), (0, 1, 2)]:
        assert [m for _, m in tta_passes(1.0, axes)] == M.masks_of(axes)
    plan = R.Plan((5, 7, 9), (4, 4, 4))
    w = M.work(plan, 2, [0, 4])
    assert len(w) == 2 * len(plan.windows(2)) and w[:3] == [((0, 0, 0, 0), 0), ((0, 0, 0, 0), 4), ((0, 0, 0, 1), 0)]


@pytest.mark.parametrize("shape,roi,overlap", [((5, 7, 9), (4, 4, 4), 0.5), ((3, 5, 6), (4, 8, 8), 0.5), ((2, 6, 10), (4, 4, 8), 0.5)])
def test_blend_pieces(shape, roi, overlap):
    plan = R.Plan(shape, roi, overlap, 'gaussian')
    n, c = 2, 3
    lg = R.window_logits(plan, n, c, 7)
    windows = plan.windows(n)
    plain = R.blend(lg, plan, n)
    # K = 1: the unmirrored blend, bit for bit (w * 1 == w)
    assert _same_bits(M.blend(lg, plan, [(wd, 0) for wd in windows], 1.0, n), plain)
    # one pass per window with mask m at scale 1: the unmirrored blend of the host-flipped logits
    for mask in range(1, 8):
        flipped = [T.flip(l_[None], mask)[0] for l_ in lg]
        assert _same_bits(M.blend(lg, plan, [(wd, mask) for wd in windows], 1.0, n), R.blend(flipped, plan, n)), mask
    # it starts from a given accumulator and leaves it alone
    base = np.full((n, c) + shape, 2.0, np.float32)
    got = M.blend(lg, plan, [(wd, 5) for wd in windows], 0.5, n, acc=base)
    assert (base == 2.0).all() and not np.array_equal(got, base)


def test_constant_mode_blend_of_a_pointwise_model_is_exact_with_mirrors():
    """coverage counts and K are powers of two and the data integer-valued: every product and sum is exact, and a
    flip-equivariant model's mirrored passes all say the same, so the statement's blend IS the model of the whole volume"""
    plan = R.Plan((12, 8, 16), (8, 4, 8), 0.5, 'constant')
    x = R.integer_volume(2, (12, 8, 16), 3)
    want = R.pointwise_model(x)
    for axes in [(2,), (0, 1), (0, 1, 2)]:
        assert np.array_equal(M.predict(R.pointwise_model, x, plan, axes), want), axes
    # a model that is NOT flip-equivariant: the mirrors change the blend (a mirror that silently does nothing would not)
    plain = R.blend(R.model_on_windows(R.ramp_model, x, plan), plan, n=2)
    assert _same_bits(M.predict(R.ramp_model, x, plan, ()), plain)
    for axes in [(2,), (0, 1), (0, 1, 2)]:
        assert not np.array_equal(M.predict(R.ramp_model, x, plan, axes), plain), axes


def test_val_flags():
    sys.path.insert(0, ROOT)
    try:
        import val
    finally:
        sys.path.remove(ROOT)
    a = val.parse_args(["--config", "x.yml"])
    assert a.sw_mirror_axes == []
    a = val.parse_args(["--config", "x.yml", "--sliding_window", "96", "96", "96", "--sw_mirror_axes", "0", "1", "2"])
    assert a.sliding_window == [96, 96, 96] and a.sw_mirror_axes == [0, 1, 2]
    assert val.parse_args(["--config", "x.yml", "--sw_mirror_axes"]).sw_mirror_axes == []


def test_evaluate_refusals_come_before_any_work():
    from medicalseg_amd.core import evaluate
    losses = {"types": [None], "coef": [1]}
    with pytest.raises(ValueError, match="sw_mirror_axes"):
        evaluate(None, None, losses, sw_mirror_axes=(0,))                        # without sliding_window
    with pytest.raises(ValueError, match="flip_axes are 0, 1 or 2"):
        evaluate(None, None, losses, sliding_window=(16, 16, 16), sw_mirror_axes=(3,))
    with pytest.raises(ValueError, match="duplicate"):
        evaluate(None, None, losses, sliding_window=(16, 16, 16), sw_mirror_axes=(1, 1))
    with pytest.raises(ValueError, match="sliding_window"):                      # the refusal of before stays
        evaluate(None, None, losses, sliding_window=(16, 16, 16), sw_mirror_axes=(0,), aug_eval=True)


def test_sliding_window_inference_validates_mirror_axes_first():
    from medicalseg_amd.core import infer
    for bad in [(3,), (-1,), (0, 0), (True,)]:
        with pytest.raises(ValueError, match="tta_passes"):
            infer.sliding_window_inference(None, None, (4, 4, 4), mirror_axes=bad)

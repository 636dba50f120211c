"""The statement tests/lovasz_reference.py WITHOUT a GPU: against a torch float64 autograd restatement of Berman's
lovasz_softmax (the flat / per_image / classes logic, written afresh here), and on its edge cases."""
import numpy as np
import pytest

import lovasz_reference as LV


# ---- Berman's lovasz_softmax, restated ----------------------------------------------------------------------------------------
def _berman_grad(gt_sorted):
    """the gradient of the Lovasz extension of the Jaccard loss along the sorted errors"""
    import torch
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1.0 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if gt_sorted.numel() > 1:
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
    return jaccard


def _berman_flat(probas, labels, classes):
    """probas [P, C], labels [P]"""
    import torch
    if probas.numel() == 0:
        return probas.sum() * 0.0
    C = probas.shape[1]
    losses = []
    for c in (range(C) if classes in ("all", "present") else classes):
        fg = (labels == c).to(probas.dtype)
        if classes != "all" and fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        losses.append(torch.dot(errors_sorted, _berman_grad(fg[perm])))
    return torch.stack(losses).mean() if losses else probas.sum() * 0.0


def _berman(z, y, classes="present", per_image=False, ignore=255):
    """loss and dL/dz [N, C, D, H, W] in float64; voxels with label `ignore` are removed first"""
    import torch
    zt = torch.from_numpy(np.asarray(z, np.float64)).requires_grad_(True)
    p = torch.softmax(zt, 1)
    yt = torch.from_numpy(np.asarray(y).astype(np.int64))
    N, C = z.shape[:2]

    def flat(pi, yi):
        pi = pi.movedim(0, -1).reshape(-1, C) if pi.dim() == 4 else pi.movedim(1, -1).reshape(-1, C)
        yi = yi.reshape(-1)
        keep = yi != ignore
        return pi[keep], yi[keep]

    if per_image:
        loss = torch.stack([_berman_flat(*flat(p[n], yt[n]), classes) for n in range(N)]).mean()
    else:
        loss = _berman_flat(*flat(p, yt), classes)
    loss.backward()
    return loss.item(), zt.grad.numpy()


def _data(seed, shape=(2, 4, 5, 6, 7), ignore_frac=0.1):
    rng = np.random.default_rng(seed)
    N, Cn = shape[:2]
    z = rng.standard_normal(shape) * 2
    y = rng.integers(0, Cn, (N,) + shape[2:]).astype(np.int32)
    y[rng.random(y.shape) < ignore_frac] = 255
    return z, y


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes", ["present", "all", [1, 3], [0]])
def test_statement_is_berman_s_lovasz_softmax(classes, per_image):
    pytest.importorskip("torch")
    z, y = _data(3)
    y[y == 3] = 2                                   # class 3 never occurs: absent under 'present', counted under 'all'
    y[1][y[1] == 1] = 0                             # and class 1 is absent in the second sample only
    ref = LV.lovasz_softmax(z, y, classes=classes, per_image=per_image, dtype=np.float64)
    want, grad = _berman(z, y, classes, per_image)
    e = ref["e"][ref["valid"]]
    assert all(np.unique(e[:, c]).size == e.shape[0] for c in range(4))      # no ties: the order is unique
    assert abs(ref["loss"] - want) <= 1e-12, (ref["loss"], want)
    assert np.abs(ref["grad"] - grad).max() <= 1e-12
    assert not np.moveaxis(ref["grad"], 1, -1).reshape(-1, 4)[~ref["valid"]].any()
    groups = 2 if per_image else 1
    assert ref["G"].shape == (groups, 4) and not ref["G"][:, 3].any()
    if classes == "all":
        assert ref["counted"].all() and ref["pairs"] == 4 * groups
    elif classes == "present":
        assert np.array_equal(ref["counted"], ref["G"] > 0) and not ref["counted"][:, 3].any()
        assert ref["pairs"] == (5 if per_image else 3)
    elif classes == [1, 3]:
        assert ref["pairs"] == 1 and ref["counted"][0, 1] and not ref["counted"][:, 3].any()
    assert float(ref["out"][0]) == np.float32(ref["loss"]) and ref["out"][1] == ref["pairs"]


def test_an_absent_class_under_all_takes_the_largest_error():
    """G = 0: J_i = 1 for every i, so g = (1, 0, 0, ...) and L is the largest error of the plane"""
    z, y = _data(5, shape=(1, 3, 3, 4, 5), ignore_frac=0.0)
    y[y == 2] = 1
    ref = LV.lovasz_softmax(z, y, classes="all")
    assert ref["G"][0, 2] == 0 and ref["counted"][0, 2]
    assert ref["L"][0, 2] == ref["e"][:, 2].max()
    assert np.count_nonzero(ref["ge"][0, 2]) == 1 and ref["ge"][0, 2].max() == 1.0 / 3.0
    present = LV.lovasz_softmax(z, y, classes="present")
    assert not present["counted"][0, 2] and not present["ge"][0, 2].any() and present["scale"][0, 2] == 0.0
    assert present["loss"] == (present["L"][0, 0] + present["L"][0, 1]) / 2.0


def test_ties_come_out_in_raster_order():
    """all logits equal: per class two tie runs (e = 1 - 1/C at the foreground, 1/C elsewhere), each in ascending voxel order"""
    rng = np.random.default_rng(7)
    shape = (2, 3, 4, 5, 6)
    y = rng.integers(0, 3, (2, 4, 5, 6)).astype(np.int32)
    y[rng.random(y.shape) < 0.1] = 255
    z = np.full(shape, 0.375)
    for dtype in (np.float32, np.float64):
        for per_image in (False, True):
            ref = LV.lovasz_softmax(z, y, per_image=per_image, dtype=dtype)
            for g, planes in enumerate(ref["perm"]):
                for c, perm in enumerate(planes):
                    fg = ref["fg_sorted"][g][c]
                    nfg = int(fg.sum())
                    assert fg[:nfg].all() and not fg[nfg:].any()              # the larger error first
                    assert np.all(np.diff(perm[:nfg]) > 0) and np.all(np.diff(perm[nfg:]) > 0)
                    assert perm.size == ref["n_valid"][g] and np.unique(perm).size == perm.size


def test_everything_ignored_gives_zero():
    z, _ = _data(9)
    y = np.full((2, 5, 6, 7), 255, np.int32)
    y.flat[3] = 4                                   # outside [0, C), not ignored: no part either
    for classes in ("present", "all", [0, 2]):
        for per_image in (False, True):
            ref = LV.lovasz_softmax(z, y, classes=classes, per_image=per_image)
            assert ref["loss"] == 0.0 and not ref["grad"].any() and not ref["ge"].any() and not ref["L"].any()
            assert not ref["n_valid"].any() and ref["out"][0] == 0.0
            assert ref["pairs"] == (4 * (2 if per_image else 1) if classes == "all" else 0)


def test_given_errors_reproduce_the_plain_call():
    z, y = _data(11)
    z = z.astype(np.float32)
    for per_image in (False, True):
        plain = LV.lovasz_softmax(z, y, per_image=per_image, dtype=np.float32)
        assert plain["e"].dtype == np.float32 and plain["ge"].dtype == np.float32
        given = LV.lovasz_softmax(z, y, per_image=per_image, errors=plain["e"].copy())
        for name in ("L", "G", "scale", "n_valid", "ge", "out", "grad"):
            assert np.array_equal(plain[name], given[name]), name
        assert plain["loss"] == given["loss"]
        assert np.array_equal(LV.stats_record(plain), LV.stats_record(given))
        assert all(np.array_equal(a, b) for pa, pb in zip(plain["perm"], given["perm"]) for a, b in zip(pa, pb))
        # float32 errors stay close to the float64 statement
        ref = LV.lovasz_softmax(z, y, per_image=per_image, dtype=np.float64)
        assert abs(plain["loss"] - ref["loss"]) <= 1e-6 * ref["loss"]


def test_jaccard_gradient_and_key_round_trip():
    g = LV.jaccard_grad([1, 0, 1, 0, 0])
    J = np.array([1 - 1 / 2, 1 - 1 / 3, 1 - 0 / 3, 1.0, 1.0])
    assert np.allclose(g, np.diff(np.concatenate([[0.0], J])), rtol=0, atol=1e-16) and abs(g.sum() - 1.0) <= 1e-15
    assert LV.jaccard_grad([0, 0, 0]).tolist() == [1.0, 0.0, 0.0] and LV.jaccard_grad([]).size == 0
    e = np.array([1.0, 0.75, 1e-30, 0.0], np.float32)
    keys = (np.uint32(LV.KEY_ONE) - e.view(np.uint32)) | np.array([LV.KEY_FG, 0, LV.KEY_FG, 0], np.uint32)
    keys = np.concatenate([keys, np.array([LV.KEY_MASK], np.uint32)])
    assert np.all(np.diff((keys & np.uint32(LV.KEY_MASK)).astype(np.int64)) > 0)   # ascending keys = descending errors, invalid last
    back, fg, valid = LV.unpack_keys(keys)
    assert np.array_equal(back[:4], e) and fg.tolist() == [True, False, True, False, False] and valid.tolist() == [True] * 4 + [False]

"""The elastic deformation of the patch crop without a GPU: the numpy statement of tests/elastic_reference.py against scipy and
against its own float64 evaluation, the host path of transforms.RandomElasticAffinePatchCrop3D against the statement (bit for
bit), the class's random stream, its arguments and its YAML."""
import functools
import os
import random

import numpy as np
import pytest
import scipy.ndimage

import affine_reference as A
import elastic_reference as E
import patch_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, LABEL_PAD = np.float32(-3.5), 255
TIE = 1e-3
SEED = 0x1234567887654321
# (roi, sigma, alpha, axes): the field alone
FIELDS = [((12, 16, 20), 9.0, 900.0, (0, 1, 2)), ((8, 8, 64), 13.0, 600.0, (1, 2)), ((4, 4, 4), 16.0, 4096.0, (0, 1, 2)),
          ((4, 5, 7), 0.5, 3.0, (0,)), ((2, 8, 300), 9.0, 900.0, (0, 1, 2)), ((140, 3, 5), 16.0, 2000.0, (0, 2))]


@functools.lru_cache(maxsize=None)
def _field(k):
    roi, sigma, alpha, axes = FIELDS[k]
    f32 = E.field(roi, SEED + k, sigma, alpha, axes)
    f64 = E.field(roi, SEED + k, sigma, alpha, axes, np.float64)
    f32.setflags(write=False)
    f64.setflags(write=False)
    return f32, f64


@functools.lru_cache(maxsize=None)
def _case(k):
    """affine_reference.CASES[k] sampled through a field of elastic_reference.FIELD_CASES[k] / ALPHAS[k], computed once"""
    shape, roi, origin, angles, scale = A.CASES[k]
    assert E.FIELD_CASES[k][0] == roi
    sigma, alpha = E.FIELD_CASES[k][1], E.ALPHAS[k]
    img, label = A.image_for(shape, 100 + k), A.label_for(shape, 200 + k)
    m = A.matrix(angles, scale)
    f32 = E.field(roi, SEED + k, sigma, alpha)
    f64 = E.field(roi, SEED + k, sigma, alpha, dtype=np.float64)
    p64 = E.coords(roi, origin, m, f64, np.float64)
    i32, l32 = E.elastic(img, label, roi, origin, m, f32, PAD, LABEL_PAD)
    i64, l64 = E.elastic(img, label, roi, origin, m, f64, PAD, LABEL_PAD, np.float64)
    for a in (img, label, m, f32, f64, p64, i32, l32, i64, l64):
        a.setflags(write=False)
    return dict(shape=shape, roi=roi, origin=origin, sigma=sigma, alpha=alpha, img=img, label=label, m=m, f32=f32, f64=f64,
                p64=p64, i32=i32, l32=l32, i64=i64, l64=l64)


# ---- the statement against scipy and against float64 -------------------------------------------------------------------------
def test_noise_is_exact_and_keeps_its_index_range():
    roi = (4, 5, 7)
    u = E.noise(roi, SEED)
    assert u.dtype == np.float32 and u.shape == (3,) + roi and u.min() >= -1.0 and u.max() < 1.0
    assert np.array_equal(u * np.float32(2.0 ** 23), np.round(u * np.float32(2.0 ** 23)))
    assert abs(float(E.noise((16, 16, 16), SEED).mean())) < 0.05
    part = E.noise(roi, SEED, (0, 2))
    assert np.array_equal(part[0], u[0]) and np.array_equal(part[2], u[2])
    assert not part[1].any() and not np.signbit(part[1]).any()
    # the documented convention, element by element
    key = int(E.splitmix64(np.uint64(SEED)))
    n = int(np.prod(roi))
    for a, v in ((0, 0), (1, 17), (2, n - 1)):
        h = int(E.splitmix64(np.uint64((key + a * n + v) & 0xFFFFFFFFFFFFFFFF)))
        assert u.reshape(3, -1)[a, v] == np.float32(h >> 40) * np.float32(2.0 ** -23) - np.float32(1.0)


@pytest.mark.parametrize("sigma", [0.5, 2.0, 9.0, 11.3, 13.0, 16.0])
def test_taps_equal_scipys_kernel(sigma):
    from scipy.ndimage._filters import _gaussian_kernel1d
    from medicalseg_amd.preprocess import ELASTIC_MAX_SIGMA, GAUSS_MAX_SIGMA, gauss_taps
    w = E.taps(sigma)
    r = int(4.0 * sigma + 0.5)
    assert w.dtype == np.float32 and len(w) == 2 * r + 1 and 2 <= r <= E.MAX_R
    want = _gaussian_kernel1d(sigma, 0, r)
    assert np.abs(w.astype(np.float64) - want).max() <= 2.0 ** -24 * want.max()      # one float32 rounding
    assert (w > 0).all() and np.array_equal(w, w[::-1])
    # the product's taps are these numbers; the existing callers keep their limit
    assert np.array_equal(gauss_taps(sigma, ELASTIC_MAX_SIGMA), w)
    if sigma <= GAUSS_MAX_SIGMA:
        assert np.array_equal(gauss_taps(sigma), w)
    else:
        with pytest.raises(ValueError):
            gauss_taps(sigma)
    with pytest.raises(ValueError):
        gauss_taps(16.5, ELASTIC_MAX_SIGMA)


@pytest.mark.parametrize("k", range(len(FIELDS)))
def test_float64_field_equals_scipy(k):
    roi, sigma, alpha, axes = FIELDS[k]
    f32, f64 = _field(k)
    assert f32.dtype == np.float32 and f64.dtype == np.float64 and f64.shape == (3,) + roi
    w = E.taps(sigma).astype(np.float64)
    x = E.noise(roi, SEED + k, axes).astype(np.float64)
    for axis in (3, 2, 1):
        x = scipy.ndimage.correlate1d(x, w, axis=axis, mode="constant", cval=0.0)
    err = float(np.abs(f64 - float(np.float32(alpha)) * x).max())
    print("field %d: float64 statement against correlate1d: %.3e (max |F| %.3f)" % (k, err, float(np.abs(f64).max())))
    assert err <= 1e-12
    for a in range(3):
        assert (a in axes) == bool(f32[a].any())
        if a not in axes:
            assert not np.signbit(f32[a]).any()


@pytest.mark.parametrize("k", range(len(FIELDS)))
def test_float32_field_within_the_rounding_bound(k):
    """3 * (2r + 2) * 2^-24 * alpha, to first order: a line is 2r+1 products and 2r sums of terms whose partial sums stay below
    max|u| <= 1 (the weights are positive and sum to 1), each rounded once, and one more rounding for the last operand; three
    passes, none of which amplifies an error (the weights sum to 1); times alpha."""
    roi, sigma, alpha, axes = FIELDS[k]
    f32, f64 = _field(k)
    r = int(4.0 * sigma + 0.5)
    bound = 3 * (2 * r + 2) * 2.0 ** -24 * alpha
    err = float(np.abs(f32.astype(np.float64) - f64).max())
    print("field %d: float32 against float64 %.3e, bound %.3e" % (k, err, bound))
    assert err <= bound


@pytest.mark.parametrize("k", range(len(A.CASES)))
def test_float64_image_equals_scipy(k):
    c = _case(k)
    assert c["i32"].dtype == np.float32 and c["i64"].dtype == np.float64 and c["l32"].dtype == np.int32
    want = scipy.ndimage.map_coordinates(c["img"].astype(np.float64), c["p64"], order=1, mode="grid-constant", cval=float(PAD))
    err = float(np.abs(c["i64"] - want).max())
    print("case %d: float64 statement against map_coordinates: %.3e" % (k, err))
    assert err <= 1e-12
    # batchgenerators' order: the displaced offsets go through the matrix
    o = np.stack(np.meshgrid(*[np.arange(r) - r // 2 for r in c["roi"]], indexing="ij")).astype(np.float64)
    centre = np.array([og + r // 2 for og, r in zip(c["origin"], c["roi"])], np.float64)
    p = np.einsum("ab,bzyx->azyx", c["m"].astype(np.float64), o + c["f64"]) + centre[:, None, None, None]
    assert np.abs(p - c["p64"]).max() <= 1e-9


def test_the_sampling_really_moves():
    moved = 0
    for k in range(len(A.CASES)):
        c = _case(k)
        plain = A.affine(c["img"], None, c["roi"], c["origin"], c["m"], PAD)[0]
        big = float(np.abs(c["f32"]).max())
        print("case %d: largest displacement %.2f voxels" % (k, big))
        if big > 1.0:
            moved += 1
            assert not np.array_equal(plain, c["i32"])
    assert moved >= 2


@pytest.mark.parametrize("k", range(len(A.CASES)))
def test_label_equals_scipy_order_0_away_from_ties(k):
    c = _case(k)
    tie = A.near_tie(c["p64"], TIE)
    share = float(tie.mean())
    want = scipy.ndimage.map_coordinates(c["label"].astype(np.float64), c["p64"], order=0, mode="grid-constant", cval=LABEL_PAD)
    print("case %d: %.2f %% of the voxels within %g of a rounding tie" % (k, 100 * share, TIE))
    assert share <= 0.02
    assert np.array_equal(c["l64"][~tie], want[~tie].astype(np.int32))
    assert np.array_equal(c["l32"][~tie], c["l64"][~tie])


# ---- the host path equals the statement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(FIELDS)))
def test_host_field_equals_the_statement(k):
    from medicalseg_amd.transforms.transform import _elastic_field_host
    roi, sigma, alpha, axes = FIELDS[k]
    got = _elastic_field_host(roi, sigma, alpha, SEED + k, axes)
    assert got.dtype == np.float32 and got.flags.c_contiguous
    assert np.array_equal(got.view(np.uint32), _field(k)[0].view(np.uint32))


@pytest.mark.parametrize("k", range(len(A.CASES)))
def test_host_path_equals_the_statement(k):
    from medicalseg_amd.transforms.transform import _affine_patch_host, _elastic_field_host
    c = _case(k)
    f = _elastic_field_host(c["roi"], c["sigma"], c["alpha"], SEED + k)
    assert np.array_equal(f.view(np.uint32), c["f32"].view(np.uint32))
    img, lab = _affine_patch_host(c["img"], c["label"], c["origin"], c["roi"], c["m"], PAD, LABEL_PAD, f)
    assert img.dtype == np.float32 and lab.dtype == np.int32
    assert np.array_equal(img.view(np.uint32), c["i32"].view(np.uint32)) and np.array_equal(lab, c["l32"])
    only, none = _affine_patch_host(c["img"], None, c["origin"], c["roi"], c["m"], PAD, LABEL_PAD, f)
    assert none is None and np.array_equal(only.view(np.uint32), c["i32"].view(np.uint32))


@pytest.mark.parametrize("k", range(len(A.CASES)))
def test_alpha_0_equals_the_affine_patch(k):
    from medicalseg_amd.transforms.transform import _affine_patch_host, _elastic_field_host
    c = _case(k)
    f = _elastic_field_host(c["roi"], c["sigma"], 0.0, SEED + k)
    assert np.signbit(f).any() and not np.signbit(f).all() and not f.any()                 # zeros of both signs
    want_i, want_l = _affine_patch_host(c["img"], c["label"], c["origin"], c["roi"], c["m"], PAD, LABEL_PAD)
    for got_i, got_l in (_affine_patch_host(c["img"], c["label"], c["origin"], c["roi"], c["m"], PAD, LABEL_PAD, f),
                         E.elastic(c["img"], c["label"], c["roi"], c["origin"], c["m"], E.field(c["roi"], SEED + k, c["sigma"], 0.0),
                                   PAD, LABEL_PAD)):
        assert np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32)) and np.array_equal(got_l, want_l)


# ---- the class: random stream ------------------------------------------------------------------------------------------------
def _sample(shape=(9, 70, 67)):
    return np.abs(A.image_for(shape, 22)) + np.float32(0.5), P.blobs(shape, 3, 21)


def _parent_draws():
    random.random()
    [random.getrandbits(32) for _ in range(5)]
    return [random.random() for _ in range(9)]


def _elastic_draws(seed):
    """(coin, u_alpha, u_sigma, seed) of the first call under this seed"""
    random.seed(seed)
    _parent_draws()
    return random.random(), random.random(), random.random(), random.getrandbits(64)


def test_draw_count_does_not_depend_on_the_coins_or_the_data():
    from medicalseg_amd import transforms as T
    img, label = _sample()
    random.seed(11)
    _parent_draws()
    [random.random() for _ in range(3)]
    random.getrandbits(64)
    want = random.getstate()
    for rp in (0.0, 1.0):
        for ep in (0.0, 1.0):
            for lab in (label, None):
                for axes in ((0, 1, 2), (1, 2)):
                    op = T.RandomElasticAffinePatchCrop3D((12, 16, 20), 3, fg_prob=0.5, rotate_prob=rp, scale_prob=rp, elastic_prob=ep,
                                                          elastic_axes=axes)
                    random.seed(11)
                    out_i, out_l = op(img, lab)
                    assert random.getstate() == want, (rp, ep, lab is None, axes)
                    assert out_i.shape == (12, 16, 20) and (out_l is None) == (lab is None)


def test_without_an_elastic_hit_it_is_the_parent():
    from medicalseg_amd import transforms as T
    img, label = _sample()
    kw = dict(fg_prob=0.5, pad_value=-3.5, label_pad=255, rotate_prob=0.5, scale_prob=0.5)
    parent = T.RandomAffinePatchCrop3D((12, 16, 20), 3, **kw)
    child = T.RandomElasticAffinePatchCrop3D((12, 16, 20), 3, elastic_prob=0.0, **kw)
    assert isinstance(child, T.RandomAffinePatchCrop3D)
    plain = 0
    for seed in range(8):
        random.seed(seed)
        want_i, want_l = parent(img, label)
        state = random.getstate()
        random.seed(seed)
        got_i, got_l = child(img, label)
        assert got_i.dtype == want_i.dtype and np.array_equal(got_i, want_i) and np.array_equal(got_l, want_l), seed
        # the parent's stream, then exactly the four elastic draws
        random.setstate(state)
        [random.random() for _ in range(3)]
        random.getrandbits(64)
        after = random.getstate()
        random.seed(seed)
        child(img, label)
        assert random.getstate() == after
        random.seed(seed)
        u = _parent_draws()
        plain += u[0] >= 0.5 and u[4] >= 0.5
    assert 0 < plain < 8                                  # both of the parent's paths were taken
    # the default probability: a seed whose elastic coin misses takes the same path
    child = T.RandomElasticAffinePatchCrop3D((12, 16, 20), 3, **kw)
    seed = next(s for s in range(100) if _elastic_draws(s)[0] >= 0.2)
    random.seed(seed)
    want_i, want_l = parent(img, label)
    random.seed(seed)
    got_i, got_l = child(img, label)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_l, want_l)


@pytest.mark.parametrize("axes", [(0, 1, 2), (1, 2)])
def test_class_equals_the_statement_with_the_parameters_it_drew(axes):
    """the order of the draws, the ranges, the identity matrix without an affine hit, replayed from the documented stream"""
    from medicalseg_amd import transforms as T
    shape, roi = (9, 70, 67), (12, 16, 20)
    img, label = _sample(shape)
    alpha_rng, sigma_rng = (100.0, 900.0), (9.0, 13.0)
    op = T.RandomElasticAffinePatchCrop3D(roi, 3, fg_prob=0.5, pad_value=-3.5, label_pad=255, rotate_prob=0.5, degrees=20,
                                          scale_prob=0.0, elastic_prob=1.0, elastic_alpha=alpha_rng, elastic_sigma=sigma_rng,
                                          elastic_axes=axes)
    with_matrix = set()
    for seed in range(4):
        random.seed(seed)
        words = P.draw_words(0.5)
        u = [random.random() for _ in range(9)]
        coin, ua, us, fseed = random.random(), random.random(), random.random(), random.getrandbits(64)
        rotate = u[0] < 0.5
        with_matrix.add(rotate)
        m = A.matrix([-20.0 + 40.0 * v for v in u[1:4]], 1.0) if rotate else np.eye(3, dtype=np.float32)
        alpha = np.float32(alpha_rng[0] + (alpha_rng[1] - alpha_rng[0]) * ua)
        sigma = float(np.float32(sigma_rng[0] + (sigma_rng[1] - sigma_rng[0]) * us))
        origin = P.select(label, roi, 3, [1, 2], words)[:3]
        f = E.field(roi, fseed, sigma, alpha, axes)
        want_i, want_l = E.elastic(img, label, roi, origin, m, f, PAD, LABEL_PAD)
        random.seed(seed)
        got_i, got_l = op(img, label)
        assert np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32)) and np.array_equal(got_l, want_l), seed
        if 0 not in axes:
            assert not f[0].any()
    assert with_matrix == {False, True}


# ---- the class: arguments and YAML -------------------------------------------------------------------------------------------
def test_constructor_validation():
    from medicalseg_amd import transforms as T
    ok = dict(size=(8, 8, 8), num_classes=3)
    for bad in (dict(elastic_prob=-0.1), dict(elastic_prob=1.5), dict(elastic_alpha=(-1.0, 10.0)), dict(elastic_alpha=(0.0, 5000.0)),
                dict(elastic_alpha=(10.0, 5.0)), dict(elastic_alpha=(1.0, 2.0, 3.0)), dict(elastic_sigma=(0.4, 9.0)),
                dict(elastic_sigma=(9.0, 16.5)), dict(elastic_sigma=(13.0, 9.0)), dict(elastic_sigma="x"),
                dict(elastic_axes=(0, 3)), dict(elastic_axes=(1, 1)), dict(elastic_axes=(-1,)), dict(elastic_axes=2),
                dict(rotate_prob=1.5), dict(scale=(0.2, 1.0)), dict(size=(8, 8)), dict(size=(1024, 1024, 1024))):
        with pytest.raises(ValueError):
            T.RandomElasticAffinePatchCrop3D(**{**ok, **bad})
    op = T.RandomElasticAffinePatchCrop3D(**ok)
    assert (op.elastic_prob, op.elastic_alpha, op.elastic_sigma, op.elastic_axes) == (0.2, (0.0, 900.0), (9.0, 13.0), (0, 1, 2))
    assert (op.rotate_prob, op.scale_prob, op.scale, op.per_axis_scale) == (0.2, 0.2, (0.7, 1.4), False)
    assert T.RandomElasticAffinePatchCrop3D(elastic_axes=[2, 1], **ok).elastic_axes == (1, 2)
    assert T.RandomElasticAffinePatchCrop3D(elastic_axes=(), **ok).elastic_axes == ()
    assert T.RandomElasticAffinePatchCrop3D(elastic_sigma=0.5, elastic_alpha=4096, **ok).elastic_sigma == (0.5, 0.5)


def test_registered_and_built_from_yaml(tmp_path):
    from medicalseg_amd import transforms as T
    from medicalseg_amd.cvlibs import Config, manager
    assert manager.TRANSFORMS["RandomElasticAffinePatchCrop3D"] is T.RandomElasticAffinePatchCrop3D
    cfg = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_elastic_96.yml"))
    ds = cfg.train_dataset
    ops = ds.transforms.transforms
    assert type(ops[0]) is T.RandomElasticAffinePatchCrop3D and ds.transforms.device and ops[0].size == (96, 96, 96)
    assert (ops[0].elastic_prob, ops[0].elastic_alpha, ops[0].elastic_sigma, ops[0].elastic_axes) == (0.2, (0.0, 900.0), (9.0, 13.0), (0, 1, 2))
    # the same file apart from the crop's class and its four elastic arguments: everything else is the affine recipe's
    base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_affine_96.yml"))
    bops = base.train_dataset.transforms.transforms
    assert [vars(o) for o in bops[1:]] == [vars(o) for o in ops[1:]]
    assert {k: v for k, v in vars(ops[0]).items() if not k.startswith("elastic_")} == vars(bops[0])
    assert cfg.batch_size == base.batch_size and cfg.iters == base.iters and ds.shape == base.train_dataset.shape
    # on host volumes, through a dataset
    p = tmp_path / "elastic.yml"
    p.write_text("data_root: d/\nbatch_size: 1\niters: 1\n"
                 "train_dataset:\n  type: SyntheticCT\n  num_samples: 2\n  shape: [10, 12, 14]\n  num_classes: 3\n  mode: train\n"
                 "  transforms:\n"
                 "    - type: RandomElasticAffinePatchCrop3D\n      size: [8, 8, 8]\n      num_classes: 3\n      rotate_prob: 1.0\n"
                 "      elastic_prob: 1.0\n      elastic_alpha: [50, 100]\n      elastic_sigma: [1.0, 2.0]\n      elastic_axes: [1, 2]\n")
    ds = Config(str(p)).train_dataset
    op = ds.transforms.transforms[0]
    assert op.elastic_axes == (1, 2) and op.elastic_sigma == (1.0, 2.0)
    random.seed(0)
    im, label, _ = ds[0]
    assert im.shape == (1, 8, 8, 8) and label.shape == (8, 8, 8) and np.isfinite(im).all()

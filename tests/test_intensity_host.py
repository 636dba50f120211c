"""Intensity augmentation without a GPU: the C ABI surface of msk_intensity_stats_workspace / msk_intensity_stats /
msk_intensity_apply / msk_gauss_blur3d, the registration of the five transform classes, their host paths against the numpy
statement of tests/intensity_reference.py (equal arrays), their fixed random streams, and the statement itself against scipy,
math.fsum and the moments of a normal sample."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import scipy.ndimage

import intensity_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"msk_intensity_stats_workspace": 2, "msk_intensity_stats": 5, "msk_intensity_apply": 9, "msk_gauss_blur3d": 13}
SHAPE = (9, 70, 67)


def _image(shape=SHAPE, seed=1):
    return (np.random.default_rng(seed).standard_normal(shape) * 0.5 + 0.25).astype(np.float32)


def _label(shape=SHAPE):
    return (np.arange(int(np.prod(shape))) % 3).astype(np.int32).reshape(shape)


def test_header_ctypes_table_and_library_carry_the_entry_points():
    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    for k, name in enumerate(("NOISE", "SCALE", "CONTRAST", "GAMMA", "RESTORE")):
        assert re.search(r"#define\s+MSK_INTENSITY_%s\s+%d\b" % (name, k), txt), name
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name + " is not declared in include/msegk.h"
        assert len(m.group(1).split(",")) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert hasattr(lib, name), "libmsegk.so does not export " + name
    assert _lib.SIGNATURES["msk_intensity_apply"][1][-1] is ctypes.c_uint64       # seed
    from medicalseg_amd import preprocess as pp
    assert (pp.INTENSITY_NOISE, pp.INTENSITY_SCALE, pp.INTENSITY_CONTRAST, pp.INTENSITY_GAMMA, pp.INTENSITY_RESTORE) == \
        (R.NOISE, R.SCALE, R.CONTRAST, R.GAMMA, R.RESTORE)


def test_workspace_answers_without_a_gpu():
    from medicalseg_amd import _lib
    lib = _lib.load()

    def ws(n):
        b = ctypes.c_size_t(0)
        assert lib.msk_intensity_stats_workspace(ctypes.c_long(n), ctypes.byref(b)) == 0
        return b.value

    assert ws(1) >= 24
    for n in (128 ** 3, 300 * 512 * 512, 2 ** 31 - 1):
        assert 24 * -(-n // 4096) <= ws(n) < 0.01 * 4 * n                          # under 1 % of the volume
    b = ctypes.c_size_t(0)
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert lib.msk_intensity_stats_workspace(ctypes.c_long(n), ctypes.byref(b)) != 0
        assert lib.msk_last_error(None)
    assert lib.msk_intensity_stats_workspace(ctypes.c_long(10), None) != 0


def test_transforms_are_registered_and_build_from_yaml(tmp_path):
    from medicalseg_amd import transforms as T
    from medicalseg_amd.cvlibs import Config, manager
    names = ["RandomGaussianNoise3D", "RandomGaussianBlur3D", "RandomBrightness3D", "RandomContrast3D", "RandomGamma3D"]
    for name in names:
        assert manager.TRANSFORMS[name] is getattr(T, name)
    p = tmp_path / "aug.yml"
    p.write_text("data_root: d/\nbatch_size: 1\niters: 1\n"
                 "train_dataset:\n  type: SyntheticCT\n  num_samples: 2\n  shape: [10, 12, 14]\n  num_classes: 3\n  mode: train\n"
                 "  transforms:\n"
                 "    - type: RandomGaussianNoise3D\n      prob: 1.0\n      std: [0.05, 0.1]\n"
                 "    - type: RandomGaussianBlur3D\n      prob: 1.0\n      sigma: [0.5, 1.5]\n      per_axis: True\n"
                 "    - type: RandomBrightness3D\n      prob: 1.0\n      factor: [0.5, 2.0]\n"
                 "    - type: RandomContrast3D\n      prob: 1.0\n      preserve_range: False\n"
                 "    - type: RandomGamma3D\n      prob: 1.0\n      invert: True\n      retain_stats: False\n")
    ds = Config(str(p)).train_dataset
    ops = ds.transforms.transforms
    assert [type(o).__name__ for o in ops] == names
    assert ops[0].std == (0.05, 0.1) and ops[1].sigma == (0.5, 1.5) and ops[1].per_axis and ops[2].factor == (0.5, 2.0)
    assert ops[3].factor == (0.75, 1.25) and not ops[3].preserve_range and ops[4].invert and not ops[4].retain_stats
    random.seed(0)
    im, label, _ = ds[0]
    assert im.shape == (1, 10, 12, 14) and label.shape == (10, 12, 14) and np.isfinite(im).all()
    # defaults
    assert (T.RandomGaussianNoise3D().prob, T.RandomGaussianNoise3D().std) == (0.1, (0.0, 0.1))
    assert (T.RandomGaussianBlur3D().prob, T.RandomGaussianBlur3D().sigma, T.RandomGaussianBlur3D().per_axis) == (0.2, (0.5, 1.0), False)
    assert (T.RandomBrightness3D().prob, T.RandomBrightness3D().factor) == (0.15, (0.75, 1.25))
    assert (T.RandomContrast3D().prob, T.RandomContrast3D().factor, T.RandomContrast3D().preserve_range) == (0.15, (0.75, 1.25), True)
    g = T.RandomGamma3D()
    assert (g.prob, g.gamma, g.invert, g.retain_stats) == (0.3, (0.7, 1.5), False, True)


def test_the_shipped_configuration_loads():
    from medicalseg_amd import transforms as T
    from medicalseg_amd.cvlibs import Config
    cfg = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_aug_96.yml"))
    ds = cfg.train_dataset
    ops = ds.transforms.transforms
    assert [type(o) for o in ops] == [T.RandomPatchCrop3D, T.RandomGaussianNoise3D, T.RandomGaussianBlur3D, T.RandomBrightness3D,
                                      T.RandomContrast3D, T.RandomGamma3D]
    assert ds.transforms.device and ops[0].size == (96, 96, 96) and ds.shape == (144, 128, 160)
    assert ops[5].retain_stats and not ops[5].invert and ops[4].preserve_range and ops[2].sigma == (0.5, 1.0)


def test_constructor_validation():
    from medicalseg_amd import transforms as T
    for cls in (T.RandomGaussianNoise3D, T.RandomGaussianBlur3D, T.RandomBrightness3D, T.RandomContrast3D, T.RandomGamma3D):
        for prob in (-0.1, 1.5):
            with pytest.raises(ValueError):
                cls(prob=prob)
        assert cls(prob=0).prob == 0 and cls(prob=1).prob == 1
    bad = [(T.RandomGaussianNoise3D, dict(std=(0.2, 0.1))), (T.RandomGaussianNoise3D, dict(std=(-0.1, 0.1))),
           (T.RandomGaussianNoise3D, dict(std=(0.1, 0.2, 0.3))),
           (T.RandomGaussianBlur3D, dict(sigma=(1.0, 0.5))), (T.RandomGaussianBlur3D, dict(sigma=(0.5, 2.5))),
           (T.RandomGaussianBlur3D, dict(sigma=(-0.5, 1.0))), (T.RandomGaussianBlur3D, dict(sigma=3.0)),
           (T.RandomBrightness3D, dict(factor=(1.25, 0.75))), (T.RandomContrast3D, dict(factor=(1.25, 0.75))),
           (T.RandomContrast3D, dict(factor="x")), (T.RandomGamma3D, dict(gamma=(1.5, 0.7))), (T.RandomGamma3D, dict(gamma=(0.0, 1.5)))]
    for cls, kw in bad:
        with pytest.raises(ValueError):
            cls(**kw)
    assert T.RandomGaussianBlur3D(sigma=(0.5, 2.0)).sigma == (0.5, 2.0)


# ---- the host paths equal the statement ----------------------------------------------------------------------------------------
def _draws(n_random, with_bits=False):
    out = [random.random() for _ in range(n_random)]
    if with_bits:
        out.append(random.getrandbits(64))
    return out


@pytest.mark.parametrize("seed", [0, 1, 4, 7])
def test_host_paths_equal_the_statement(seed):
    from medicalseg_amd import transforms as T
    img, label = _image(), _label()
    rec = R.stats(img)

    def run(op):
        random.seed(seed)
        out, lab = op(img.copy(), label)
        assert lab is label and out.dtype == np.float32 and out.shape == img.shape
        return out

    random.seed(seed)
    _, u, bits = _draws(2, True)
    want = R.noise(img, np.float32(R.value((0.02, 0.2), u)), bits, np.float32)
    assert np.array_equal(run(T.RandomGaussianNoise3D(1.0, (0.02, 0.2))), want)

    random.seed(seed)
    _, u0, u1, u2 = _draws(4)
    assert np.array_equal(run(T.RandomGaussianBlur3D(1.0, (0.3, 2.0))), R.blur(img, [R.value((0.3, 2.0), u0)] * 3))
    assert np.array_equal(run(T.RandomGaussianBlur3D(1.0, (0.3, 2.0), per_axis=True)),
                          R.blur(img, [R.value((0.3, 2.0), u) for u in (u0, u1, u2)]))

    random.seed(seed)
    _, u = _draws(2)
    assert np.array_equal(run(T.RandomBrightness3D(1.0, (0.5, 2.0))), R.scale(img, np.float32(R.value((0.5, 2.0), u))))

    random.seed(seed)
    _, branch, u = _draws(3)
    for rng in ((0.5, 2.0), (1.1, 1.3), (0.4, 0.9)):
        f = np.float32(R.value(R.branch_range(rng, branch), u))
        for keep in (True, False):
            assert np.array_equal(run(T.RandomContrast3D(1.0, rng, preserve_range=keep)), R.contrast(img, f, keep, rec)), (rng, keep)
        for invert in (False, True):
            g = R.gamma(img, f, invert, rec, np.float32)
            assert np.array_equal(run(T.RandomGamma3D(1.0, rng, invert=invert, retain_stats=False)), g), (rng, invert)
            assert np.array_equal(run(T.RandomGamma3D(1.0, rng, invert=invert, retain_stats=True)),
                                  R.restore(g, rec, R.stats(g), np.float32)), (rng, invert)


def test_branch_rule_and_clamp_are_exercised():
    """the data of the test above do reach both sides of the branch rule, and the clamp does bind"""
    assert R.branch_range((0.5, 2.0), 0.2) == (0.5, 1) and R.branch_range((0.5, 2.0), 0.7) == (1, 2.0)
    assert R.branch_range((1.1, 1.3), 0.2) == (1.1, 1.3) and R.branch_range((0.4, 0.9), 0.7) == (1, 0.9)
    sides = set()
    for seed in (0, 1, 4, 7):
        random.seed(seed)
        sides.add(_draws(3)[1] < 0.5)
    assert sides == {True, False}
    img = _image()
    rec = R.stats(img)
    assert not np.array_equal(R.contrast(img, 1.25, True, rec), R.contrast(img, 1.25, False, rec))
    out = R.contrast(img, 1.25, True, rec)
    assert out.min() == img.min() and out.max() == img.max()


CLASSES = [("RandomGaussianNoise3D", {}, (2, True)), ("RandomGaussianBlur3D", {}, (4, False)),
           ("RandomGaussianBlur3D", {"per_axis": True}, (4, False)), ("RandomBrightness3D", {}, (2, False)),
           ("RandomContrast3D", {}, (3, False)), ("RandomGamma3D", {}, (3, False)), ("RandomGamma3D", {"invert": True}, (3, False))]


@pytest.mark.parametrize("name,kw,draws", CLASSES, ids=["%s%s" % (c[0], "+" + ",".join(c[1]) if c[1] else "") for c in CLASSES])
def test_every_call_consumes_the_same_random_stream(name, kw, draws):
    from medicalseg_amd import transforms as T
    img, label = _image((5, 6, 7)), _label((5, 6, 7))
    for seed in (0, 1, 2):
        random.seed(seed)
        _draws(*draws)
        want = random.getstate()
        states = []
        for prob in (0.0, 1.0):
            random.seed(seed)
            out, lab = getattr(T, name)(prob=prob, **kw)(img.copy(), label)
            states.append(random.getstate())
            assert lab is label
            assert np.array_equal(out, img) == (prob == 0.0)
        assert states[0] == states[1] == want
    # without a label
    out, lab = getattr(T, name)(prob=1.0, **kw)(img.copy())
    assert lab is None and out.shape == img.shape


# ---- the statement itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (9, 70, 67), (16, 16, 16)])
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.0])
def test_blur_statement_against_scipy(shape, sigma):
    x = _image(shape, 3)
    x.reshape(-1)[0] += 1.0
    x.reshape(-1)[-1] += 1.0
    r = R.radius(sigma)
    assert r == {0.5: 2, 1.0: 4, 2.0: 8}[sigma] and len(R.taps(sigma)) == 2 * r + 1
    want = scipy.ndimage.gaussian_filter(x.astype(np.float64), sigma, mode="reflect", truncate=4)
    got = R.blur(x, [sigma] * 3)
    assert got.dtype == np.float32
    bound = 3 * (2 * r + 2) * 2.0 ** -24 * float(np.abs(x).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("blur %s sigma %g: error %.3e, bound %.3e" % (shape, sigma, err, bound))
    assert err <= bound


def test_reflect_map_and_taps():
    assert R.reflect(np.arange(-9, 9), 3).tolist() == [2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2]
    assert R.reflect(np.arange(-3, 4), 1).tolist() == [0] * 7
    pad = np.pad(np.arange(5), 8, mode="symmetric")
    assert R.reflect(np.arange(-8, 13), 5).tolist() == pad.tolist()
    assert len(R.taps(0.0)) == 0 and len(R.taps(0.1)) == 0 and R.radius(0.125) == 1
    from medicalseg_amd.preprocess import gauss_taps
    for sigma in (0.0, 0.1, 0.125, 0.5, 0.77, 1.0, 2.0):
        assert np.array_equal(gauss_taps(sigma), R.taps(sigma))
        if len(R.taps(sigma)):
            assert abs(float(R.taps(sigma).astype(np.float64).sum()) - 1.0) < 1e-6
    with pytest.raises(ValueError):
        gauss_taps(2.01)


@pytest.mark.parametrize("n", [1, 255, 4097, 256 * 4096 + 1, 37 * 190 * 187])
def test_statement_sums_against_fsum(n):
    rng = np.random.default_rng(n)
    for x in (rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) - 1000.0).astype(np.float32)):
        rec = R.stats(x)
        d = x.astype(np.float64)
        assert rec[0] == d.min() and rec[1] == d.max()
        for got, terms in ((rec[2], d), (rec[3], d * d)):
            exact = math.fsum(terms.tolist())
            assert abs(got - exact) <= n * 2.0 ** -53 * float(np.abs(terms).sum())


def test_chunk_order_is_the_stated_one():
    """a sum whose value depends on the order: the explicit loops against a direct transcription for one chunk and a half"""
    n = 4096 + 2048 + 3
    x = (np.random.default_rng(5).standard_normal(n) * 10.0 ** np.random.default_rng(6).integers(-6, 7, n)).astype(np.float64)
    chunks = []
    for c in range(2):
        v = [0.0] * 256
        for lane in range(256):
            for j in range(16):
                e = 4096 * c + lane + 256 * j
                v[lane] = v[lane] + (x[e] if e < n else 0.0)
        s = 128
        while s >= 1:
            for lane in range(s):
                v[lane] = v[lane] + v[lane + s]
            s //= 2
        chunks.append(v[0])
    assert np.array_equal(R.chunk_sums(x), np.array(chunks))
    assert R.reduce_chunks(chunks) == chunks[0] + chunks[1]
    assert R.reduce_chunks(np.arange(1.0, 601.0)) == float(sum(range(1, 601)))


def test_normal_sample_moments():
    n = 2 ** 22
    z = R.normals(1, n)
    mean, std = float(z.mean()), float(z.std())
    print("z over 2^22: mean * sqrt(n) = %.3f, std = %.6f, max |z| = %.3f" % (mean * math.sqrt(n), std, float(np.abs(z).max())))
    assert abs(mean) <= 5.0 / math.sqrt(n)
    assert abs(std - 1.0) <= 5.0 / math.sqrt(2 * n)
    z32 = R.normals(1, n, np.float32)
    assert z32.dtype == np.float32 and float(np.abs(z32 - z).max()) < 1e-5
    assert not np.array_equal(R.normals(2, 4096), z[:4096])                        # the seed matters
    u1, u2 = R.uniforms(1, 4096)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    # the first words of the generator, from its definition in Python integers
    def sm(v):
        v = (v + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        v = ((v ^ (v >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        v = ((v ^ (v >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return v ^ (v >> 31)
    k = sm(1)
    for i in (0, 1, 4095):
        h = sm((k + i) & (2 ** 64 - 1))
        assert float(u1[i]) == ((h >> 40) + 1) * 2.0 ** -24 and float(u2[i]) == ((h >> 8) & 0xFFFFFF) * 2.0 ** -24

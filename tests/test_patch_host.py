"""Random patch cropping without a GPU: the C ABI surface of msk_patch_workspace / msk_patch_select / msk_patch_crop, the
registration of transforms.RandomPatchCrop3D, its host path against the numpy statement of tests/patch_reference.py (equal
arrays, no tolerance), and its fixed random stream."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import patch_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"msk_patch_workspace": 3, "msk_patch_select": 16, "msk_patch_crop": 11}
PAIRS = [((9, 70, 67), (12, 16, 20)), ((20, 33, 130), (8, 8, 64)), ((5, 6, 7), (8, 8, 8))]


def test_header_ctypes_table_and_library_carry_the_entry_points():
    from medicalseg_amd import _lib
    txt = open(os.path.join(ROOT, "include", "msegk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name + " is not declared in include/msegk.h"
        assert len(m.group(1).split(",")) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert hasattr(lib, name), "libmsegk.so does not export " + name
    assert _lib.SIGNATURES["msk_patch_crop"][1][-1] is ctypes.c_uint32           # pad_bits


def test_workspace_answers_without_a_gpu():
    from medicalseg_amd import _lib
    lib = _lib.load()

    def ws(voxels, classes):
        b = ctypes.c_size_t(0)
        assert lib.msk_patch_workspace(ctypes.c_long(voxels), classes, ctypes.byref(b)) == 0
        return b.value

    assert ws(1, 1) >= 8                                                          # the totals and one chunk row
    for voxels in (128 ** 3, 300 * 512 * 512):
        for classes in (3, 20):
            b = ws(voxels, classes)
            assert b >= 4 * classes and b < 0.01 * 4 * voxels                      # under 1 % of the label
        assert ws(voxels, 20) > ws(voxels, 3)
    b = ctypes.c_size_t(0)
    for voxels, classes in ((0, 2), (2 ** 31, 2), (10, 0), (10, 257)):
        assert lib.msk_patch_workspace(ctypes.c_long(voxels), classes, ctypes.byref(b)) != 0
    assert lib.msk_patch_workspace(ctypes.c_long(10), 2, None) != 0
    assert ws(2 ** 31 - 1, 256) > 0


def test_transform_builds_from_a_yaml_transform_list(tmp_path):
    from medicalseg_amd import transforms as T
    from medicalseg_amd.cvlibs import Config, manager
    assert manager.TRANSFORMS["RandomPatchCrop3D"] is T.RandomPatchCrop3D
    p = tmp_path / "patch.yml"
    p.write_text("data_root: d/\nbatch_size: 1\niters: 1\n"
                 "train_dataset:\n  type: SyntheticCT\n  num_samples: 2\n  shape: [10, 12, 14]\n  num_classes: 3\n  mode: train\n"
                 "  transforms:\n    - type: RandomPatchCrop3D\n      size: [8, 8, 8]\n      num_classes: 3\n      fg_prob: 0.5\n"
                 "      classes: [2]\n      label_pad: 255\n")
    ds = Config(str(p)).train_dataset
    op = ds.transforms.transforms[0]
    assert isinstance(op, T.RandomPatchCrop3D)
    assert op.size == (8, 8, 8) and op.classes == [2] and op.fg_prob == 0.5 and op.label_pad == 255 and op.pad_value == 0
    random.seed(0)
    im, label, _ = ds[0]
    assert im.shape == (1, 8, 8, 8) and label.shape == (8, 8, 8)
    # the shipped configuration
    cfg = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_96.yml"))
    ds = cfg.train_dataset
    op = ds.transforms.transforms[0]
    assert isinstance(op, T.RandomPatchCrop3D) and op.size == (96, 96, 96) and op.classes == [1, 2]
    assert ds.transforms.device and ds.shape == (144, 128, 160)
    # defaults and argument checks
    assert T.RandomPatchCrop3D(16, 4).classes == [1, 2, 3] and T.RandomPatchCrop3D(16, 4).size == (16, 16, 16)
    assert abs(T.RandomPatchCrop3D(16, 4).fg_prob - 1 / 3) < 1e-15
    for bad in (dict(classes=[2, 1]), dict(classes=[4]), dict(classes=[-1]), dict(classes=[1, 1])):
        with pytest.raises(ValueError):
            T.RandomPatchCrop3D(16, 4, **bad)
    with pytest.raises(ValueError):
        T.RandomPatchCrop3D((8, 8), 4)
    with pytest.raises(ValueError):
        T.RandomPatchCrop3D(8, 0)


@pytest.mark.parametrize("shape,roi", PAIRS)
def test_host_path_equals_the_reference(shape, roi):
    from medicalseg_amd import transforms as T
    label = R.blobs(shape, 4, 7)
    img = R.image_for(shape, 8)
    op = T.RandomPatchCrop3D(roi, 4, fg_prob=0.5, classes=[1, 3], pad_value=-3.5, label_pad=255)
    forced = 0
    for seed in range(200):
        random.seed(seed)
        words = R.draw_words(0.5)
        want = R.select(label, roi, 4, [1, 3], words)
        forced += want[3] >= 0
        random.seed(seed)
        assert op.get_params() == words
        assert op.select(shape, label, words) == want, seed                          # origin, class and centre
        random.seed(seed)
        got_img, got_lab = op(img, label)
        assert got_img.dtype == np.float32 and got_lab.dtype == np.int32
        assert np.array_equal(got_img.view(np.uint32), R.crop(img, want[:3], roi, np.float32(-3.5)).view(np.uint32)), seed
        assert np.array_equal(got_lab, R.crop(label, want[:3], roi, 255)), seed
        for o, ro, dim in zip(want[:3], roi, shape):                                  # every origin is in range
            assert (o == -((ro - dim) // 2)) if dim <= ro else (0 <= o <= dim - ro)
    assert 60 <= forced <= 140
    for w in (0, R.WORD_MAX):                                                         # the extreme words
        for force in (0, 1):
            words = [force] + [w] * 5
            assert op.select(shape, label, words) == R.select(label, roi, 4, [1, 3], words)


CONSUMERS = [
    ("fg_prob 0", dict(fg_prob=0.0), "blobs"), ("fg_prob 1", dict(fg_prob=1.0), "blobs"), ("no label", dict(fg_prob=1.0), None),
    ("no foreground", dict(fg_prob=1.0), "empty")]


@pytest.mark.parametrize("name,kw,kind", CONSUMERS, ids=[c[0] for c in CONSUMERS])
def test_every_call_consumes_the_same_random_stream(name, kw, kind):
    from medicalseg_amd import transforms as T
    shape, roi = (9, 70, 67), (12, 16, 20)
    img = R.image_for(shape, 1)
    label = {"blobs": R.blobs(shape, 3, 2), "empty": np.zeros(shape, np.int32), None: None}[kind]
    op = T.RandomPatchCrop3D(roi, 3, **kw)
    for seed in (0, 1, 2):
        random.seed(seed)
        random.random()
        for _ in range(5):
            random.getrandbits(32)
        want = random.getstate()
        random.seed(seed)
        out = op(img, label)
        assert random.getstate() == want
        assert out[0].shape == roi and (out[1] is None) == (label is None)


@pytest.mark.parametrize("shape,roi", PAIRS)
def test_forced_foreground_patch_contains_its_centre(shape, roi):
    from medicalseg_amd import transforms as T
    label = R.blobs(shape, 4, 11)
    op = T.RandomPatchCrop3D(roi, 4, fg_prob=1.0, classes=[2, 3])
    seen = set()
    for seed in range(60):
        random.seed(seed)
        words = op.get_params()
        rec = op.select(shape, label, words)
        o, cls, centre = rec[:3], rec[3], rec[4:7]
        assert cls in (2, 3) and label[tuple(centre)] == cls
        seen.add(cls)
        random.seed(seed)
        _, patch = op(R.image_for(shape, 3), label)
        local = tuple(c - oo for c, oo in zip(centre, o))
        assert all(0 <= v < ro for v, ro in zip(local, roi)) and patch[local] == cls, seed
    assert seen == {2, 3}


def test_uniform_branch_ignores_the_label_values():
    from medicalseg_amd import transforms as T
    shape, roi = (20, 33, 130), (8, 8, 64)
    label = R.blobs(shape, 4, 5)
    perm = np.array([3, 0, 2, 1], np.int32)
    other = np.where((label >= 0) & (label < 4), perm[np.clip(label, 0, 3)], label).astype(np.int32)
    img = R.image_for(shape, 6)
    op = T.RandomPatchCrop3D(roi, 4, fg_prob=0.0)
    for seed in range(10):
        random.seed(seed)
        a_img, a_lab = op(img, label)
        random.seed(seed)
        b_img, b_lab = op(img, other)
        assert np.array_equal(a_img, b_img)
        sel = (a_lab >= 0) & (a_lab < 4)
        assert np.array_equal(np.where(sel, perm[np.clip(a_lab, 0, 3)], a_lab), b_lab)

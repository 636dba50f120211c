"""Random patch cropping on the device (medicalseg_amd/csrc/msk_patch.hip, preprocess.patch_select_device /
patch_crop_device, transforms.RandomPatchCrop3D) against the numpy statement of tests/patch_reference.py.  Everything is
compared with np.array_equal; the only tolerance is the max-normalisation's at the end of Compose."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import patch_reference as R

pytestmark = pytest.mark.gpu

CHUNK = 4096          # voxels per row of the chunk table (msk_patch.hip kChunk)
SELECT_LANES = 256    # threads of the select workgroup


class Owned:
    """device buffers outside the pools, freed on exit"""

    def __enter__(self):
        from medicalseg_amd.device import get_device
        self.dev, self.ptrs = get_device(), []
        return self

    def __exit__(self, *exc):
        self.dev.sync()
        for p in self.ptrs:
            self.dev.free(p)
        return False

    def malloc(self, nbytes):
        p = self.dev.malloc(nbytes)
        self.ptrs.append(p)
        return p

    def upload(self, arr, offset=0):
        """offset: bytes in front of the array (a pointer that is not 16-byte aligned)"""
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes + offset) + offset
        self.dev.h2d(p, arr)
        return p

    def filled(self, shape, dtype, byte=0xCD):
        n = int(np.prod(shape)) * 4
        p = self.malloc(n)
        self.dev.memset(p, byte, n)
        return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _workspace(o, voxels, num_classes):
    b = C.c_size_t(0)
    assert o.dev.lib.msk_patch_workspace(C.c_long(voxels), num_classes, C.byref(b)) == 0
    return o.malloc(b.value)


def _select(o, label_ptr, shape, roi, num_classes, classes, words, ws, sel, counts):
    cls = np.ascontiguousarray(np.array(classes, np.int32))
    words = np.ascontiguousarray(np.asarray(words, np.uint32).reshape(-1, 6))
    o.dev.call("msk_patch_select", C.c_void_p(label_ptr), *shape, num_classes, _ptr(cls) if len(cls) else None, len(cls), *roi,
               _ptr(words), len(words), C.c_void_p(ws), C.c_void_p(sel), C.c_void_p(counts) if counts else None)


# ---- msk_patch_select --------------------------------------------------------------------------------------------------------
# 37 x 190 x 187 = 321 chunks of 4096 voxels: more chunks than the select workgroup has lanes
SELECT_CASES = [((9, 70, 67), (12, 16, 20)), ((20, 33, 130), (8, 8, 64)), ((5, 6, 7), (8, 8, 8)), ((16, 16, 16), (16, 16, 16)),
                ((37, 190, 187), (16, 32, 48))]


def _label_variants(shape):
    """(name, label, num_classes, classes)"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(n)
    out = []
    lab = np.zeros(n, np.int32)                      # class 3 spans many chunks; 1 only at voxel 0; 2 only at the last voxel
    lab[n // 5: n // 5 + max(2, (3 * n) // 5)] = 3
    lab[::7][lab[::7] == 3] = 0                       # ... with holes
    lab[0], lab[-1] = 1, 2
    lab[n // 2], lab[n // 3] = 255, -1
    out.append(("corners", lab, 20, [1, 2, 3, 4, 7]))                              # 4 and 7 are absent candidates
    out.append(("one class fills the volume", np.full(n, 2, np.int32), 3, [1, 2]))
    out.append(("all candidates absent", np.where(rng.random(n) < 0.01, 255, 0).astype(np.int32), 3, [1, 2]))
    out.append(("subset", R.blobs(shape, 4, 3, fill=0.1).reshape(-1), 4, [2]))
    out.append(("blobs", R.blobs(shape, 3, 4).reshape(-1), 3, [1, 2]))
    out.append(("one class, a candidate", np.where(rng.random(n) < 0.3, -1, 0).astype(np.int32), 1, [0]))
    out.append(("one class, no candidates", np.zeros(n, np.int32), 1, []))
    out.append(("random labels", rng.integers(-1, 21, n).astype(np.int32), 20, list(range(1, 20))))
    return [(name, l_.reshape(shape), c, cl) for name, l_, c, cl in out]


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("shape,roi", SELECT_CASES)
def test_select_equals_the_reference(shape, roi, offset):
    n = int(np.prod(shape))
    if shape == SELECT_CASES[-1][0]:
        assert -(-n // CHUNK) > SELECT_LANES
    if offset and shape == SELECT_CASES[-1][0]:
        variants = _label_variants(shape)[:1]          # the scalar form of the large volume once
    else:
        variants = _label_variants(shape)
    words = R.mixed_words(16, n)
    with Owned() as o:
        sel = o.malloc(16 * 8 * 4)
        for name, label, num_classes, classes in variants:
            want_sel, want_counts = R.select_all(label, roi, num_classes, classes, words)
            lp = o.upload(label, offset)
            ws = _workspace(o, n, num_classes)
            counts = o.malloc(4 * num_classes)
            o.dev.memset(sel, 0xCD, 16 * 8 * 4)
            o.dev.memset(counts, 0xCD, 4 * num_classes)
            _select(o, lp, shape, roi, num_classes, classes, words, ws, sel, counts)
            got_sel = o.dev.d2h(sel, (16, 8), np.int32)
            got_counts = o.dev.d2h(counts, (num_classes,), np.int32)
            assert np.array_equal(got_counts, want_counts), name
            assert np.array_equal(got_sel, want_sel), (name, got_sel.tolist(), want_sel.tolist())
            # without the counts, and a single patch: the same records
            o.dev.memset(sel, 0xCD, 16 * 8 * 4)
            _select(o, lp, shape, roi, num_classes, classes, words, ws, sel, None)
            assert np.array_equal(o.dev.d2h(sel, (16, 8), np.int32), want_sel), name
            _select(o, lp, shape, roi, num_classes, classes, words[2:3], ws, sel, None)
            assert np.array_equal(o.dev.d2h(sel, (1, 8), np.int32), want_sel[2:3]), name
            if name == "corners":
                assert {1, 2, 3} >= set(want_sel[::2, 3].tolist()) and want_sel[0, 3] == 1 and want_sel[2, 3] == 3
                assert want_sel[1, 3] == -1
            if name == "all candidates absent":
                assert (want_sel[:, 3] == -1).all()


def test_select_without_a_forced_patch_does_not_read_the_label():
    """the uniform branch needs the geometry only (the transform passes the image when there is no label): the records of a
    call in which no patch forces foreground do not depend on the volume's contents, and the workspace is not written"""
    shape, roi = (9, 70, 67), (12, 16, 20)
    words = R.mixed_words(16, 5)
    words[:, 0] = 0
    want, _ = R.select_all(np.zeros(shape, np.int32), roi, 3, [1, 2], words)
    with Owned() as o:
        lp = o.upload(R.blobs(shape, 3, 1))
        ws = _workspace(o, int(np.prod(shape)), 3)
        o.dev.memset(ws, 0xCD, 64)
        sel = o.malloc(16 * 8 * 4)
        _select(o, lp, shape, roi, 3, [1, 2], words, ws, sel, None)
        assert np.array_equal(o.dev.d2h(sel, (16, 8), np.int32), want)
        assert (o.dev.d2h(ws, (16,), np.uint32) == 0xCDCDCDCD).all()
        words[:, 0] = 1
        _select(o, lp, shape, roi, 3, [], words, ws, sel, None)                    # no candidates: the same
        assert np.array_equal(o.dev.d2h(sel, (16, 8), np.int32), want)
        assert (o.dev.d2h(ws, (16,), np.uint32) == 0xCDCDCDCD).all()


# ---- msk_patch_crop ----------------------------------------------------------------------------------------------------------
CROP_CASES = [  # volume, roi
    ((6, 10, 24), (4, 4, 8)),      # W % 4 == 0, rw % 4 == 0: w0 = 0 .. 16, every residue; no padding
    ((6, 10, 23), (4, 4, 8)),      # W % 4 != 0
    ((6, 10, 24), (4, 5, 7)),      # rw % 4 != 0
    ((6, 10, 21), (4, 5, 7)),      # neither
    ((3, 9, 4), (5, 10, 12)),      # padding on both sides of d and w (w0 = -4: whole quads of padding), behind only on h
    ((5, 6, 5), (8, 8, 8)),        # w0 = -1
    ((7, 3, 40), (2, 4, 16))]      # padding on h only, long rows


@pytest.mark.parametrize("shape,roi", CROP_CASES)
def test_crop_equals_the_reference(shape, roi):
    n = int(np.prod(shape))
    label = R.blobs(shape, 3, n)
    img = R.image_for(shape, n + 1)
    words = R.mixed_words(16, n + 2)
    words[:, 0] = 0
    for k in range(16):                                                            # uniform patches at chosen origins
        for ax in range(3):
            span = shape[ax] - roi[ax] + 1
            if span > 1:
                words[k, 3 + ax] = R.word_for((k * (2, 3, 1)[ax]) % span, span)
    words[12:, 0] = 1                                                              # ... and four foreground ones
    want_sel, _ = R.select_all(label, roi, 3, [1, 2], words)
    if shape[2] > roi[2]:
        assert {0, 1, 3} <= set((want_sel[:12, 2] % 4).tolist())
    rv = int(np.prod(roi))
    with Owned() as o:
        lp, ip = o.upload(label), o.upload(img)
        ws = _workspace(o, n, 3)
        sel = o.malloc(16 * 8 * 4)
        out_i = [o.filled(roi, np.float32) for _ in range(16)]
        out_l = [o.filled(roi, np.int32) for _ in range(16)]
        pad_f = int(np.array([-3.5], np.float32).view(np.uint32)[0])
        # select and all crops are enqueued back to back: the origins never visit the host
        _select(o, lp, shape, roi, 3, [1, 2], words, ws, sel, None)
        for k in range(16):
            rec = C.c_void_p(sel + 32 * k)
            o.dev.call("msk_patch_crop", C.c_void_p(ip), *shape, rec, C.c_void_p(out_i[k]), *roi, C.c_uint32(pad_f))
            o.dev.call("msk_patch_crop", C.c_void_p(lp), *shape, rec, C.c_void_p(out_l[k]), *roi, C.c_uint32(255))
        assert np.array_equal(o.dev.d2h(sel, (16, 8), np.int32), want_sel)
        for k in range(16):
            origin = want_sel[k, :3].tolist()
            got = o.dev.d2h(out_i[k], roi, np.float32)
            assert np.array_equal(got.view(np.uint32), R.crop(img, origin, roi, np.float32(-3.5)).view(np.uint32)), (k, origin)
            assert np.array_equal(o.dev.d2h(out_l[k], roi, np.int32), R.crop(label, origin, roi, 255)), (k, origin)
        # a destination that is not 16-byte aligned takes the element form
        odd = o.malloc(rv * 4 + 16) + 4
        o.dev.call("msk_patch_crop", C.c_void_p(ip), *shape, C.c_void_p(sel + 32 * 5), C.c_void_p(odd), *roi, C.c_uint32(pad_f))
        assert np.array_equal(o.dev.d2h(odd, roi, np.float32), R.crop(img, want_sel[5, :3].tolist(), roi, np.float32(-3.5)))
        assert np.array_equal(o.dev.d2h(ip, shape, np.float32), img) and np.array_equal(o.dev.d2h(lp, shape, np.int32), label)


def test_preprocess_wrappers_use_the_pool_and_download_nothing():
    import inspect

    from medicalseg_amd import preprocess as pp
    for fn in (pp.patch_select_device, pp.patch_crop_device):
        assert not re.search(r"d2h|\.numpy\(|\.sync\(", inspect.getsource(fn)), fn.__name__
    shape, roi = (9, 70, 67), (12, 16, 20)
    label, img = R.blobs(shape, 3, 1), R.image_for(shape, 2)
    words = R.mixed_words(4, 3)
    want, _ = R.select_all(label, roi, 3, [1, 2], words)
    lv, iv = pp.upload_pooled(label), pp.upload_pooled(img)
    sel = pp.patch_select_device(lv, roi, 3, [1, 2], words)
    crops = [pp.patch_crop_device(iv, sel, roi, -3.5, index=k) for k in range(4)]
    lab0 = pp.patch_crop_device(lv, sel, roi, 255)
    assert sel.shape == (4, 8) and np.array_equal(sel.numpy(), want)
    for k, c_ in enumerate(crops):
        assert c_.pooled and c_.dtype == np.float32
        assert np.array_equal(c_.numpy(), R.crop(img, want[k, :3].tolist(), roi, np.float32(-3.5)))
    assert lab0.dtype == np.int32 and np.array_equal(lab0.numpy(), R.crop(label, want[0, :3].tolist(), roi, 255))
    one = pp.patch_select_device(lv, roi, 3, [1, 2], words[1])                     # six words = one patch
    assert np.array_equal(one.numpy(), want[1:2])
    ptr = sel.ptr
    for v in crops + [lab0, sel, one, iv]:
        v.free()
    again = pp.patch_select_device(lv, roi, 3, [1, 2], words)
    assert again.pooled and again.ptr == ptr                                       # the record buffer comes back from the pool
    again.free()
    lv.free()


# ---- the transform, the loader, training -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,roi", [((9, 70, 67), (12, 16, 20)), ((20, 33, 130), (8, 8, 64))])
def test_transform_device_path_equals_host_path(shape, roi):
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    label = R.blobs(shape, 3, 21)
    img = np.abs(R.image_for(shape, 22)) + 0.5
    op = T.RandomPatchCrop3D(roi, 3, fg_prob=0.5, pad_value=-3.5, label_pad=255)
    for seed in range(6):
        random.seed(seed)
        h_img, h_lab = op(img, label)
        state = random.getstate()
        random.seed(seed)
        d_img, d_lab = op(pp.upload_pooled(img), pp.upload_pooled(label))
        assert random.getstate() == state
        assert d_img.shape == roi and d_lab.shape == roi
        assert np.array_equal(d_img.numpy(), h_img) and np.array_equal(d_lab.numpy(), h_lab), seed
        d_img.free()
        d_lab.free()
        # without a label
        random.seed(seed)
        h_only, none = op(img, None)
        random.seed(seed)
        d_only, none_d = op(pp.upload_pooled(img), None)
        assert none is None and none_d is None and np.array_equal(d_only.numpy(), h_only)
        assert random.getstate() == state
        d_only.free()
        # inside Compose, behind the max normalisation
        ops = [T.RandomPatchCrop3D(roi, 3, fg_prob=0.5, label_pad=255)]
        random.seed(seed)
        c_img, c_lab = T.Compose(ops)(img.copy(), label.copy())
        random.seed(seed)
        g_img, g_lab = T.Compose(ops, device=True)(img.copy(), label.copy())
        gi = g_img.numpy()
        assert gi.shape == c_img.shape[1:] and np.array_equal(g_lab.numpy(), c_lab), seed
        assert np.abs(gi - c_img[0]).max() <= 2e-6, (seed, np.abs(gi - c_img[0]).max())
        g_img.free()
        g_lab.free()


def test_a_refused_crop_leaves_the_pool_balanced(monkeypatch):
    """the select's record goes back to the pool when a crop behind it is refused; the caller still owns the two inputs"""
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd import transforms as T
    from medicalseg_amd._lib import MskError
    shape, roi = (5, 6, 7), (4, 4, 4)
    iv, lv = pp.upload_pooled(R.image_for(shape, 5)), pp.upload_pooled(R.blobs(shape, 3, 6))
    balance, selected = [0], []
    alloc, release, select = pp._pool_alloc, pp._pool_release, pp.patch_select_device

    def counted_alloc(dev_, nbytes):
        balance[0] += 1
        return alloc(dev_, nbytes)

    def counted_release(dev_, ptr, nbytes):
        balance[0] -= 1
        return release(dev_, ptr, nbytes)

    def recorded_select(*args):
        selected.append(select(*args))
        return selected[-1]

    def refused(*args, **kwargs):
        assert len(selected) == 1                                                  # the select has run
        raise MskError("msk_patch_crop failed: refused")
    monkeypatch.setattr(pp, "_pool_alloc", counted_alloc)
    monkeypatch.setattr(pp, "_pool_release", counted_release)
    monkeypatch.setattr(pp, "patch_select_device", recorded_select)
    monkeypatch.setattr(pp, "patch_crop_device", refused)
    random.seed(0)
    with pytest.raises(MskError, match="refused"):
        T.RandomPatchCrop3D(roi, 3, fg_prob=0.5, label_pad=255)(iv, lv)
    assert balance[0] == 0
    assert selected[0].ptr is None and iv.ptr and lv.ptr
    iv.free()
    lv.free()
    assert balance[0] == -2


class _TwoSizes:
    """two samples of different extents, augmented on the device"""
    shapes = [(9, 30, 37), (14, 20, 25)]

    def __init__(self, ops, device):
        from medicalseg_amd import transforms as T
        self.transforms = T.Compose(ops, device=device)

    def __len__(self):
        return 2

    def __getitem__(self, i):
        im, lab = self.transforms(np.abs(R.image_for(self.shapes[i], 30 + i)) + 0.5, R.blobs(self.shapes[i], 3, 40 + i))
        return im, lab, "sample_%d" % i


def test_loader_stacks_patches_of_volumes_of_different_sizes():
    from medicalseg_amd import transforms as T
    from medicalseg_amd.datasets import DataLoader
    from medicalseg_amd.device import IntTensor, Tensor
    roi = (12, 16, 20)
    ops = [T.RandomPatchCrop3D(roi, 3, fg_prob=0.5, label_pad=255)]
    random.seed(3)
    batches = list(DataLoader(_TwoSizes(ops, True), batch_size=2))
    assert len(batches) == 1
    x, y, paths = batches[0]
    assert isinstance(x, Tensor) and isinstance(y, IntTensor) and paths == ["sample_0", "sample_1"]
    assert x.shape == (2, 1) + roi and tuple(y.shape) == (2,) + roi
    random.seed(3)
    hx, hy, _ = next(iter(DataLoader(_TwoSizes(ops, False), batch_size=2)))
    assert np.array_equal(y.numpy(), hy) and np.abs(x.numpy() - hx).max() <= 2e-6
    assert (hy == 255).any()                                                       # the first sample is padded on d


def test_patch_training_end_to_end(tmp_path, capsys):
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd import transforms as T
    from medicalseg_amd.core import evaluate, train
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    tf = [T.RandomPatchCrop3D(32, 3, fg_prob=0.5)]
    ds = SyntheticCT(num_samples=4, shape=(40, 44, 52), num_classes=3, transforms=tf, device_aug=True)
    val = SyntheticCT(num_samples=1, shape=(40, 44, 52), num_classes=3, mode="val", seed=99)
    random.seed(0)
    model = VNet(num_classes=3)
    opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    train(model, ds, optimizer=opt, save_dir=str(tmp_path / "o"), iters=2, batch_size=2, save_interval=10, log_iters=1, losses=losses)
    logged = [float(v) for v in re.findall(r"\[TRAIN\].*? loss: ([^,]+),", capsys.readouterr().out)]
    assert len(logged) == 2 and np.isfinite(logged).all() and all(v > 0 for v in logged), logged
    model.eval()
    got = evaluate(model, val, losses, print_detail=False, sliding_window=(32, 32, 32))
    assert np.isfinite(got["mdice"]) and 0.0 <= got["mdice"] <= 1.0


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from medicalseg_amd import _lib
    from medicalseg_amd._lib import MskError
    shape, roi = (5, 7, 9), (4, 4, 4)
    label = R.blobs(shape, 3, 1)
    words = R.mixed_words(2, 2)
    with Owned() as o:
        dev = o.dev
        lp = o.upload(label)
        ws = _workspace(o, int(np.prod(shape)), 3)
        sel, counts = o.filled((2, 8), np.int32), o.filled((3,), np.int32)
        dst = o.filled(roi, np.int32)
        V = C.c_void_p

        def ints(*v):
            return _ptr(np.ascontiguousarray(np.array(v, np.int32)))
        wp = _ptr(np.ascontiguousarray(words))

        def s(label=lp, d=5, h=7, w=9, nc=3, classes=ints(1, 2), ncls=2, rd=4, rh=4, rw=4, words=wp, npatch=2, ws=ws, sel=sel):
            return ("msk_patch_select", (V(label), d, h, w, nc, classes, ncls, rd, rh, rw, words, npatch, V(ws), V(sel), V(counts)))

        def c(src=lp, d=5, h=7, w=9, sel=sel, dst=dst, rd=4, rh=4, rw=4):
            return ("msk_patch_crop", (V(src), d, h, w, V(sel), V(dst), rd, rh, rw, C.c_uint32(255)))
        bad = [s(label=None), s(words=None), s(ws=None), s(sel=None), s(classes=None),                    # null pointers
               s(d=0), s(h=0), s(w=-1), s(rd=0), s(rh=-3), s(rw=0),                                          # extents < 1
               s(d=2048, h=1024, w=1024),                                                                    # 2^31 voxels
               s(nc=0), s(nc=257),
               s(ncls=-1), s(ncls=33, classes=ints(*range(33))),
               s(classes=ints(2, 1)), s(classes=ints(1, 1)), s(classes=ints(1, 3)), s(classes=ints(-1, 1)),  # order, range
               s(npatch=0), s(npatch=17),
               c(src=None), c(sel=None), c(dst=None),
               c(d=0), c(w=0), c(rd=0), c(rw=-2), c(d=2048, h=1024, w=1024), c(rd=2048, rh=1024, rw=1024),
               c(dst=lp), c(dst=lp + 16), c(src=dst)]                                                        # dst overlaps src
        for name, args in bad:
            rc = getattr(dev.lib, name)(dev.ctx, *args)
            assert rc != 0, (name, args)
            assert _lib.last_error(dev.ctx), name
            with pytest.raises(MskError, match=name):
                dev.call(name, *args)
        # nothing was launched
        assert (dev.d2h(sel, (16,), np.uint32) == 0xCDCDCDCD).all() and (dev.d2h(counts, (3,), np.uint32) == 0xCDCDCDCD).all()
        assert (dev.d2h(dst, roi, np.uint32) == 0xCDCDCDCD).all() and np.array_equal(dev.d2h(lp, shape, np.int32), label)
        # ... and the same calls with valid arguments run
        dev.call(*s()[:1], *s()[1])
        dev.call(*c()[:1], *c()[1])
        want, want_counts = R.select_all(label, roi, 3, [1, 2], words)
        assert np.array_equal(dev.d2h(sel, (2, 8), np.int32), want) and np.array_equal(dev.d2h(counts, (3,), np.int32), want_counts)
        assert np.array_equal(dev.d2h(dst, roi, np.int32), R.crop(label, want[0, :3].tolist(), roi, 255))

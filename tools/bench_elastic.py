"""Micro-benchmark of the elastic deformation of the patch crop (medicalseg_amd/csrc/msk_elastic.hip: msk_elastic_field;
msk_affine.hip: msk_affine_patch_elastic) beside existing kernels timed in the same run on same-sized buffers, and beside the
host round trip it replaces.
python tools/bench_elastic.py [--iters K] [--out FILE] [--no-step] [--no-host]

Workloads (patch from volume): 96^3 from 144 x 128 x 160, 128^3 from 300 x 512 x 512, 12 x 256 x 256 from 12 x 512 x 512, each
at sigma 9 (r = 36) and 13 (r = 52), alpha 900; the image is N(0,1), the label blobs of three classes.

device rows, HIP-event ms, median [min, max] of 5 means of --iters calls, a 1 GiB buffer written before every call so that
the operands come from HBM:
  field      msk_elastic_field, all three components.
             yardstick: three msk_gauss_blur3d calls at sigma 2 (r = 8: 17 taps per pass, three passes per call) on one
             patch-sized buffer, times (2r+1) / 17.  mark: that plus the yardstick's own max - min -- per tap the wide kernel is
             no slower than the narrow one.  Also its share of the unfused float32 vector rate, 78.5 Tflop/s (half of the 157
             Tflop/s that count a fused multiply-add as two), counting 2 (2r+1) - 1 operations per output and pass; no mark.
  sampling   msk_affine_patch_elastic at 30 degrees about all three axes and scale 1.4, image + label.
             mark: msk_affine_patch with the same matrix, plus msk_d2d of the field (reading the field may cost what copying
             it costs), plus the former's max - min.
without a mark:
  host       wall ms of the D2H copy of image and label, the numpy statement of tests/elastic_reference.py (field and
             sampling) and the H2D copy of the patch pair, once per patch at sigma 9; the device result is compared with it bit
             for bit.
  step       one VNet 96^3 batch-2 training step on resident data, and beside it the wall time of cutting the batch's two
             patches from resident 144 x 128 x 160 volumes with the crop of the affine and of the elastic config, every coin
             certain, between two device syncs."""
import argparse
import ctypes as C
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [((144, 128, 160), (96, 96, 96)), ((300, 512, 512), (128, 128, 128)), ((12, 512, 512), (12, 256, 256))]
SIGMAS = (9.0, 13.0)
ALPHA = 900.0
ANGLES, SCALE = (30, 30, 30), 1.4
FLUSH_BYTES = 1 << 30
REPEATS = 5
VECTOR_RATE = 78.5e12


def timed(dev, call, iters, flush):
    means = []
    for r in range(REPEATS):
        tot = 0.0
        for i in range(iters):
            dev.memset(flush, (r * iters + i) & 0xFF, FLUSH_BYTES)
            dev.timer_start()
            call()
            tot += dev.timer_stop()
        means.append(tot / iters)
    means.sort()
    return means[REPEATS // 2], means[0], means[-1]


def fmt(m):
    return f"{m[0]:.4f} [{m[1]:.4f}, {m[2]:.4f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true", help="skip the VNet step and the transform timings")
    ap.add_argument("--no-host", action="store_true", help="skip the host round trip (and the bit comparison with it)")
    args = ap.parse_args()
    import affine_reference as A
    import elastic_reference as E
    import patch_reference as P
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.device import get_device
    dev = get_device()
    lines, misses = [], []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# elastic deformation (msk_elastic_field, msk_affine_patch_elastic), {dev.name()}, host CPU: {os.cpu_count()} logical CPUs visible")
    emit(f"# device: HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call")
    flush = dev.malloc(FLUSH_BYTES)
    vp = C.c_void_p
    m = np.ascontiguousarray(A.matrix(ANGLES, SCALE).reshape(9))
    blur_taps = pp.gauss_taps(2.0)
    for shape, roi in CASES:
        vox, pv = int(np.prod(shape)), int(np.prod(roi))
        img = np.random.default_rng(vox).standard_normal(shape, dtype=np.float32)
        label = P.blobs(shape, 3, 7)
        origin = [(s - r) // 2 for s, r in zip(shape, roi)]
        ip, lp = dev.malloc(vox * 4), dev.malloc(vox * 4)
        dev.h2d(ip, img)
        dev.h2d(lp, label)
        sel = dev.malloc(32)
        dev.h2d(sel, np.array(origin + [-1, -1, -1, -1, 0], np.int32))
        out_i, out_l, blur_dst, blur_tmp = (dev.malloc(pv * 4) for _ in range(4))
        field, scratch, field_copy = (dev.malloc(pv * 12) for _ in range(3))
        emit(f"[{roi[0]}x{roi[1]}x{roi[2]} from {shape[0]}x{shape[1]}x{shape[2]}]  patch = {pv * 4 / 1e6:.2f} MB, field = {pv * 12 / 1e6:.2f} MB")
        # the yardsticks
        bt = blur_taps.ctypes.data_as(vp)

        def blur3():
            for _ in range(3):
                dev.call("msk_gauss_blur3d", vp(out_i), vp(blur_dst), *roi, bt, 8, bt, 8, bt, 8, vp(blur_tmp))

        def affine():
            dev.call("msk_affine_patch", vp(ip), vp(lp), *shape, vp(sel), m.ctypes.data_as(vp), vp(out_i), vp(out_l), *roi, C.c_float(0.0), 0)

        def sampling():
            dev.call("msk_affine_patch_elastic", vp(ip), vp(lp), *shape, vp(sel), m.ctypes.data_as(vp), vp(field), vp(out_i), vp(out_l),
                     *roi, C.c_float(0.0), 0)

        def copy_field():
            dev.d2d(field_copy, field, pv * 12)

        affine()                                              # out_i: finite data for the blur
        yard = {}
        for name, call in (("3 x msk_gauss_blur3d, sigma 2 (17 taps x 3 passes each)", blur3), ("msk_affine_patch, same matrix", affine),
                           ("msk_d2d of the field", copy_field)):
            for _ in range(3):
                call()
            yard[name] = timed(dev, call, args.iters, flush)
            emit(f"  yardstick  {name:58s} {fmt(yard[name])}")
        yb, ya, yc = (yard[k] for k in yard)
        for sigma in SIGMAS:
            w = pp.gauss_taps(sigma, pp.ELASTIC_MAX_SIGMA)
            r = (len(w) - 1) // 2

            def make_field(seed=7):
                dev.call("msk_elastic_field", C.c_uint64(seed), *roi, w.ctypes.data_as(vp), r, C.c_float(ALPHA), 7, vp(field), vp(scratch))
            for _ in range(3):
                make_field()
            t = timed(dev, make_field, args.iters, flush)
            mark = yb[0] * (2 * r + 1) / 17.0 + (yb[2] - yb[1])
            ops = 9.0 * pv * (2 * (2 * r + 1) - 1)
            ok = t[0] <= mark
            if not ok:
                misses.append(f"field {roi} sigma {sigma:g}: {t[0]:.4f} ms against the mark {mark:.4f} ms")
            emit(f"  field      sigma {sigma:4.1f} (r = {r}, {2 * r + 1} taps)  {fmt(t)}   mark {mark:.4f} ms = {yb[0]:.4f} x {2 * r + 1}/17 + {yb[2] - yb[1]:.4f}: "
                 f"{'met' if ok else 'MISSED'} ({t[0] / mark:.2f});  {ops / 1e9:.2f} Gop, {ops / (t[0] * 1e-3) / 1e12:.2f} Top/s = "
                 f"{100 * ops / (t[0] * 1e-3) / VECTOR_RATE:.1f} % of the unfused float32 vector rate")
            for _ in range(3):
                sampling()
            t = timed(dev, sampling, args.iters, flush)
            mark = ya[0] + yc[0] + (ya[2] - ya[1])
            ok = t[0] <= mark
            if not ok:
                misses.append(f"sampling {roi} sigma {sigma:g}: {t[0]:.4f} ms against the mark {mark:.4f} ms")
            emit(f"  sampling   sigma {sigma:4.1f} image + label              {fmt(t)}   mark {mark:.4f} ms = {ya[0]:.4f} + {yc[0]:.4f} + {ya[2] - ya[1]:.4f}: "
                 f"{'met' if ok else 'MISSED'} ({t[0] / mark:.2f})")
            if sigma == SIGMAS[0] and not args.no_host:
                make_field()
                sampling()
                got_f = dev.d2h(field, (3,) + roi, np.float32)
                got_i, got_l = dev.d2h(out_i, roi, np.float32), dev.d2h(out_l, roi, np.int32)
                t0 = time.perf_counter()
                hi, hl = dev.d2h(ip, shape, np.float32), dev.d2h(lp, shape, np.int32)
                t1 = time.perf_counter()
                want_f = E.field(roi, 7, sigma, ALPHA)
                want_i, want_l = E.elastic(hi, hl, roi, origin, m.reshape(3, 3), want_f, 0.0, 0)
                t2 = time.perf_counter()
                dev.h2d(out_i, want_i)
                dev.h2d(out_l, want_l)
                dev.sync()
                t3 = time.perf_counter()
                parts = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)
                same = bool(np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)) and
                            np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32)) and np.array_equal(got_l, want_l))
                emit(f"  host       sigma {sigma:4.1f}: d2h {parts[0]:.1f} ms + numpy {parts[1]:.1f} ms + h2d {parts[2]:.1f} ms = {sum(parts):.1f} ms "
                     f"(one run); largest displacement {float(np.abs(want_f).max()):.2f} voxels; device == statement (field, image, label): {same}")
                if not same:
                    misses.append(f"device != statement at {roi} sigma {sigma:g}")
                del hi, hl
        del img, label
        for ptr in (ip, lp, sel, out_i, out_l, blur_dst, blur_tmp, field, scratch, field_copy):
            dev.free(ptr)
    dev.free(flush)

    if not args.no_step:
        from medicalseg_amd import optimizer as optim
        from medicalseg_amd import transforms as T
        from medicalseg_amd.device import to_tensor
        from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
        from medicalseg_amd.utils import loss_computation
        rng = np.random.default_rng(1)
        model = VNet(num_classes=3)
        model.train()
        opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        x = to_tensor(rng.standard_normal((2, 1, 96, 96, 96)).astype(np.float32))
        yt = to_tensor(rng.integers(0, 3, (2, 96, 96, 96)).astype(np.int32))
        losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
        shape = (144, 128, 160)
        img = rng.standard_normal(shape).astype(np.float32)
        label = P.blobs(shape, 3, 7)
        kw = dict(size=(96, 96, 96), num_classes=3, rotate_prob=1.0, scale_prob=1.0)
        crops = {"RandomAffinePatchCrop3D (affine_96 config)": T.RandomAffinePatchCrop3D(**kw),
                 "RandomElasticAffinePatchCrop3D (elastic_96 config)": T.RandomElasticAffinePatchCrop3D(elastic_prob=1.0, **kw)}
        times = {k: [] for k in list(crops) + ["VNet step"]}
        random.seed(0)
        for rep in range(3 + REPEATS):
            dev.sync()
            t0 = time.perf_counter()
            loss_list, _ = loss_computation(model(x), yt, losses)
            sum(loss_list).backward()
            opt.step()
            dev.sync()
            if rep >= 3:
                times["VNet step"].append((time.perf_counter() - t0) * 1e3)
            for name, op in crops.items():
                vols = [(pp.upload_pooled(img), pp.upload_pooled(label)) for _ in range(2)]
                dev.sync()
                t0 = time.perf_counter()
                outs = [op(iv, lv) for iv, lv in vols]
                dev.sync()
                if rep >= 3:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                for oi, ol in outs:
                    oi.free()
                    ol.free()
        emit("[one VNet training step, 2x1x96^3, 3 classes, CE + Dice, and cutting its two patches from resident 144x128x160 volumes with "
             "every coin certain: wall clock between two device syncs, ms, 3 warm-up rounds]")
        for name, t in times.items():
            emit(f"  {name:52s} {np.median(t):.3f} [{min(t):.3f} .. {max(t):.3f}]")
    emit("misses: " + ("none" if not misses else "; ".join(misses)))
    emit("# not measured: hardware counters (LDS bank conflicts of the W pass, L2 hit rate of the column passes, VALU busy), the "
         "transform inside a training loop (reader_cost), fields with fewer than three components, alpha and seed (no influence "
         "on the instruction count)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

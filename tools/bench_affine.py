"""Micro-benchmark of the rotated and scaled patch crop (medicalseg_amd/csrc/msk_affine.hip: msk_affine_patch) beside the
kernels that could stand in for it today and beside the host path it replaces.
python tools/bench_affine.py [--iters K] [--out FILE]

Workloads (patch from volume): 96^3 from 144 x 128 x 160, 128^3 from 300 x 512 x 512, 12 x 256 x 256 from 12 x 512 x 512; the
patch sits in the middle of the volume, the image is N(0,1), the label blobs of three classes.

device rows, HIP-event ms, median [min, max] of 5 means of --iters calls, a 1 GiB buffer written before every call so that
the operands come from HBM:
  affine      msk_affine_patch with (a) the identity matrix, (b) 30 degrees about all three axes and scale 1.4, (c) 30 degrees
              about D only (in-plane), each with and without the label, and each under both thread -> voxel maps (context
              option "affine_map": 1 = a 2 x 2 x 16 box of the patch per wavefront, 0 = row-linear)
  crop        the yardstick msk_patch_crop of the same patch, image and label
  rotate3d    the yardstick msk_rotate3d (order 1, 30 degrees in the H-W plane) on a resident volume of the patch's extent:
              the existing 8-tap gather, one plane per call
  mark        fused image + label launch of (b) <= crop (image) + crop (label) + 2 x rotate3d, the cheapest chain of today's
              kernels (which rotates about two axes only, interpolates twice and rotates the label with order 1)
host row: wall ms of the D2H copy of image and label, the numpy statement of tests/affine_reference.py and the H2D copy of the
patch pair on this machine's CPU, best of 2; the device result of (b) is compared with it bit for bit."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [((144, 128, 160), (96, 96, 96)), ((300, 512, 512), (128, 128, 128)), ((12, 512, 512), (12, 256, 256))]
MATRICES = [("(a) identity", (0, 0, 0), 1.0), ("(b) 30/30/30 deg, scale 1.4", (30, 30, 30), 1.4), ("(c) 30 deg about D", (30, 0, 0), 1.0)]
MAPS = [(1, "box 2x2x16"), (0, "row-linear")]
FLUSH_BYTES = 1 << 30
REPEATS = 5


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
    args = ap.parse_args()
    import affine_reference as R
    import patch_reference as P
    from medicalseg_amd.device import get_device
    dev = get_device()
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# rotated and scaled patch crop (msk_affine_patch), {dev.name()}, host CPU: {os.cpu_count()} logical CPUs visible")
    emit(f"# device: HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call")
    emit("# host: wall ms of D2H (image + label) + affine_reference.affine on numpy + H2D (patch pair), best of 2")
    flush = dev.malloc(FLUSH_BYTES)
    vp = C.c_void_p
    default_map = 1                                  # msk_common.h: affine_map
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
        out_i, out_l, rot_src, rot_dst = (dev.malloc(pv * 4) for _ in range(4))
        emit(f"[{roi[0]}x{roi[1]}x{roi[2]} from {shape[0]}x{shape[1]}x{shape[2]}]  patch = {pv * 4 / 1e6:.2f} MB, "
             f"volume = {vox * 4 / 1e6:.1f} MB, origin {tuple(origin)}")

        def affine(m, with_label):
            dev.call("msk_affine_patch", vp(ip), vp(lp) if with_label else None, *shape, vp(sel), m.ctypes.data_as(vp), vp(out_i),
                     vp(out_l) if with_label else None, *roi, C.c_float(0.0), 0)

        res = {}
        for name, angles, scale in MATRICES:
            m = np.ascontiguousarray(R.matrix(angles, scale).reshape(9))
            for amap, map_name in MAPS:
                dev.set_option("affine_map", amap)
                for with_label in (True, False):
                    call = lambda: affine(m, with_label)
                    for _ in range(3):
                        call()
                    t = timed(dev, call, args.iters, flush)
                    res[(name, amap, with_label)] = t
                    what = "image + label" if with_label else "image only"
                    emit(f"  affine {name:28s} {map_name:11s} {what:14s} {fmt(t)}  {pv / (t[0] * 1e-3) / 1e9:6.2f} Gvoxel/s")
        dev.set_option("affine_map", default_map)
        # the yardsticks
        pad = int(np.array([0.0], np.float32).view(np.uint32)[0])
        crop_i = lambda: dev.call("msk_patch_crop", vp(ip), *shape, vp(sel), vp(out_i), *roi, C.c_uint32(pad))
        crop_l = lambda: dev.call("msk_patch_crop", vp(lp), *shape, vp(sel), vp(out_l), *roi, C.c_uint32(0))
        crop_i()
        dev.d2d(rot_src, out_i, pv * 4)
        rot = lambda: dev.call("msk_rotate3d", vp(rot_src), vp(rot_dst), *roi, 1, 2, C.c_double(30.0), 1, C.c_double(0.0), 0)
        yard = {}
        for name, call in (("crop (image)", crop_i), ("crop (label)", crop_l), ("rotate3d order 1, H-W plane", rot)):
            for _ in range(3):
                call()
            yard[name] = timed(dev, call, args.iters, flush)
            emit(f"  {name:62s} {fmt(yard[name])}")
        chain = yard["crop (image)"][0] + yard["crop (label)"][0] + 2.0 * yard["rotate3d order 1, H-W plane"][0]
        full = MATRICES[1][0]
        for amap, map_name in MAPS:
            fused = res[(full, amap, True)][0]
            emit(f"  mark, {map_name}: fused (b) image + label {fused:.4f} ms / (crop + crop + 2 x rotate3d = {chain:.4f} ms) = "
                 f"{fused / chain:.2f}  ({'met' if fused <= chain else 'MISSED'}: at most 1)")
        # the host round trip, and device == statement for (b)
        m = np.ascontiguousarray(R.matrix(MATRICES[1][1], MATRICES[1][2]).reshape(9))
        affine(m, True)
        got_i, got_l = dev.d2h(out_i, roi, np.float32), dev.d2h(out_l, roi, np.int32)
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            hi, hl = dev.d2h(ip, shape, np.float32), dev.d2h(lp, shape, np.int32)
            t1 = time.perf_counter()
            want_i, want_l = R.affine(hi, hl, roi, origin, m.reshape(3, 3), 0.0, 0)
            t2 = time.perf_counter()
            dev.h2d(out_i, want_i)
            dev.h2d(out_l, want_l)
            dev.sync()
            t3 = time.perf_counter()
            parts = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)
            if best is None or sum(parts) < sum(best):
                best = parts
        same = bool(np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32)) and np.array_equal(got_l, want_l))
        fused = res[(full, default_map, True)][0]
        emit(f"  host (b): d2h {best[0]:.1f} ms + numpy {best[1]:.1f} ms + h2d {best[2]:.1f} ms = {sum(best):.1f} ms   "
             f"({sum(best) / fused:.0f} x the fused launch), device == statement: {same}")
        del img, label, hi, hl
        for ptr in (ip, lp, sel, out_i, out_l, rot_src, rot_dst):
            dev.free(ptr)
    dev.free(flush)
    emit("# not measured: hardware counters (cache-line requests per wavefront, L2 hit rate) of the two maps, the transform inside a "
         "training loop (reader_cost), LDS staging of the source box, image pointers that are not 16-byte aligned")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

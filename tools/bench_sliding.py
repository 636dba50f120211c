"""Micro-benchmark of the sliding-window kernels (medicalseg_amd/csrc/msk_sliding.hip) and of core.infer.sliding_window_inference.
python tools/bench_sliding.py [--iters K] [--out FILE] [--part kernels|net|all]

--part all (default) touches no GPU itself: it runs the two parts as child processes, each under a time limit of its own, and
stops at the first that fails.

kernel rows (--part kernels), one window, operands resident in HBM, at roi 128^3 (C = 2) and 512 x 512 x 12 (C = 20), the
volume 8 voxels larger on every axis, the window at w origin 4 (row starts on 16-byte quads) and 3:
  copy        the yardstick, a plain streaming copy of a window-sized tensor: msk_copy_scale (2 tensors)
  accumulate  msk_sw_accumulate: reads the logits and the accumulator, writes the accumulator (3 tensors of roi x C floats)
  gather      msk_sw_gather at Cin = C and at Cin = 1: reads the volume, writes the patch (2 tensors; its own copy row each)
HIP-event ms, median [min, max] of 5 means of --iters calls, a 1 GiB buffer written before every call so that the operands
come from HBM.  GB/s = moved tensors * tensor bytes / median.  Target of accumulate: at most twice the time the same run's copy
needs for as many bytes, i.e. 3 x the copy's time.
call rows (--part net): wall ms (synchronised), best / median of --iters, of an eval-mode VNet (3 classes):
  sliding_window_inference of one 256^3 volume, roi 128^3, overlap 0.5 (27 windows), sw_batch_size 1
  27 plain inference() calls on a 128^3 input, each opening its own fused scope (BatchNorm is folded 27 times), and the same
  27 calls inside ONE nn.fused_inference scope (folded once, as the sliding call does): the forwards alone
  the down-sampled path: 256^3 -> 128^3 (trilinear), one forward, logits resized back to 256^3, argmax"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((128, 128, 128), 2), ((512, 512, 12), 20)]
MARGIN = 8
W_ORIGINS = (4, 3)
FLUSH_BYTES = 1 << 30
REPEATS = 5
PART_LIMIT_S = {"kernels": 360, "net": 420}


def spread(means):
    means = sorted(means)
    return means[len(means) // 2], means[0], means[-1]


def time_events(dev, call, iters, flush):
    means = []
    for r in range(REPEATS):
        tot = 0.0
        for i in range(iters):
            dev.memset(flush, (r * iters + i) & 0xFF, FLUSH_BYTES)
            dev.timer_start()
            call()
            tot += dev.timer_stop()
        means.append(tot / iters)
    return spread(means)


def fill(dev, ptr, nbytes, rng):
    chunk = rng.standard_normal(1 << 22).astype(np.float32)          # 16 MiB, repeated
    for off in range(0, nbytes, chunk.nbytes):
        dev.h2d(ptr + off, chunk[: min(chunk.nbytes, nbytes - off) // 4])


def part_kernels(args, emit):
    from medicalseg_amd.core.infer import SlidingPlan
    from medicalseg_amd.device import Tensor, get_device
    dev = get_device()
    emit(f"# sliding-window kernels (msk_sw_gather / msk_sw_accumulate), one window, {dev.name()}")
    emit(f"# HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call; "
         "GB/s = moved tensors * tensor bytes / median")
    flush = dev.malloc(FLUSH_BYTES)
    rng = np.random.default_rng(0)
    for roi, c in CASES:
        vol = tuple(v + MARGIN for v in roi)
        plan = SlidingPlan(vol, roi, overlap=0.5)
        tables = []
        for T in plan.tables:
            p = dev.malloc(T.nbytes)
            dev.h2d(p, T)
            tables.append(p)
        rows = [len(s) for s in plan.starts]
        for cc, what in ((c, "accumulate"), (c, "gather"), (1, "gather")):
            nbytes = roi[0] * roi[1] * roi[2] * cc * 4
            emit(f"[roi {roi[0]}x{roi[1]}x{roi[2]}, C = {cc}, volume {vol[0]}x{vol[1]}x{vol[2]}]  window tensor = {nbytes / 1e6:.1f} MB")
            win, win2 = (Tensor.empty(dev, 1, roi[0], roi[1], roi[2], cc, arena=False) for _ in range(2))
            big = Tensor.empty(dev, 1, vol[0], vol[1], vol[2], cc, arena=False)
            fill(dev, win.ptr, nbytes, rng)
            fill(dev, big.ptr, vol[0] * vol[1] * vol[2] * cc * 4, rng)

            def row(name, call, tensors):
                for _ in range(3):
                    call()
                m = time_events(dev, call, args.iters, flush)
                emit(f"  {name:34s} {m[0]:.4f} [{m[1]:.4f}, {m[2]:.4f}] ms  {tensors} tensors  "
                     f"{tensors * nbytes / (m[0] * 1e-3) / 1e9:6.0f} GB/s")
                return m[0]

            copy = row("copy (msk_copy_scale)", lambda: dev.call("msk_copy_scale", win.msk(), None, win2.msk(), 0), 2)
            for w0 in W_ORIGINS:
                quads = (w0 * cc) % 4 == 0 and (vol[2] * cc) % 4 == 0 and (roi[2] * cc) % 4 == 0
                if what == "accumulate":
                    o = np.array([[0, 4, 4, w0, 0, 0, 0]], np.int32)
                    t = row(f"msk_sw_accumulate, w origin {w0}",
                            lambda: dev.call("msk_sw_accumulate", win.msk(), o.ctypes.data_as(C.c_void_p), C.c_void_p(tables[0]), rows[0],
                                             C.c_void_p(tables[1]), rows[1], C.c_void_p(tables[2]), rows[2], big.msk()), 3)
                    emit(f"    {'16-byte' if quads else '4-byte'} path: {t / copy:.2f} x the copy's time for 1.5 x its bytes; target <= 3.00 x: "
                         + ("met" if t <= 3.0 * copy else "MISSED"))
                else:
                    o = np.array([[0, 4, 4, w0]], np.int32)
                    t = row(f"msk_sw_gather, w origin {w0}",
                            lambda: dev.call("msk_sw_gather", big.msk(), win2.msk(), o.ctypes.data_as(C.c_void_p), C.c_float(0.0)), 2)
                    emit(f"    {'16-byte loads' if quads else '4-byte loads, 16-byte stores' if (roi[2] * cc) % 4 == 0 else '4-byte path'}: "
                         f"{t / copy:.2f} x the copy's time for the same bytes")
            for t_ in (win, win2, big):
                dev.free(t_.ptr)
        for p in tables:
            dev.free(p)
    dev.free(flush)


def part_net(args, emit):
    from medicalseg_amd import nn
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import Tensor, get_device, to_tensor
    from medicalseg_amd.models import VNet
    dev = get_device()
    rng = np.random.default_rng(1)
    model = VNet(num_classes=3)
    model.eval()
    x128 = to_tensor(rng.standard_normal((1, 1, 128, 128, 128)).astype(np.float32))
    x256 = Tensor.empty(dev, 1, 256, 256, 256, 1, arena=False)
    fill(dev, x256.ptr, 256 ** 3 * 4, rng)
    small = Tensor.empty(dev, 1, 128, 128, 128, 1, arena=False)

    class Resize3D:
        size = (128, 128, 128)

    def wall(call):
        call()
        dev.sync()
        ts = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            call()
            dev.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[0], ts[len(ts) // 2]

    def downsampled():
        dev.call("msk_interp_trilinear_fwd", x256.msk(), small.msk())
        return infer.inference(model, small, ori_shape=(256, 256, 256), transforms=[Resize3D()])

    n = len(infer.SlidingPlan((256, 256, 256), (128, 128, 128), overlap=0.5).windows(1))
    emit(f"[VNet, 3 classes, eval mode, {dev.name()}]  wall ms, synchronised, best / median of {args.iters}")
    one = wall(lambda: infer.inference(model, x128))
    many = wall(lambda: [infer.inference(model, x128) for _ in range(n)])

    def one_scope():
        with nn.fused_inference():
            return [infer.inference(model, x128) for _ in range(n)]

    scoped = wall(one_scope)
    sw = wall(lambda: infer.sliding_window_inference(model, x256, (128, 128, 128), overlap=0.5))
    down = wall(downsampled)
    emit(f"  inference x 1 at 128^3                         {one[0]:.2f} / {one[1]:.2f}")
    emit(f"  inference x {n} at 128^3, a scope each          {many[0]:.2f} / {many[1]:.2f}")
    emit(f"  inference x {n} at 128^3, one fused scope       {scoped[0]:.2f} / {scoped[1]:.2f}")
    emit(f"  sliding_window_inference, 256^3, {n} windows    {sw[0]:.2f} / {sw[1]:.2f}   gather + blend + bookkeeping against the "
         f"forwards in one scope: {sw[1] - scoped[1]:+.2f} ms median, {100.0 * (sw[1] - scoped[1]) / sw[1]:+.1f} % of the call")
    emit(f"  resample to 128^3, one forward, resize back     {down[0]:.2f} / {down[1]:.2f}   (the sliding call takes {sw[1] / down[1]:.1f} x "
         "its time; here the net sees an eighth of the voxels)")
    infer.sliding_release(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("kernels", "net", "all"), default="all")
    args = ap.parse_args()
    if args.part == "all":
        if args.out and os.path.exists(args.out):
            os.remove(args.out)
        for part in ("kernels", "net"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--iters", str(args.iters if part == "kernels" else min(args.iters, 5))]
            if args.out:
                cmd += ["--out", args.out]
            rc = subprocess.run(cmd, timeout=PART_LIMIT_S[part]).returncode
            if rc != 0:
                sys.exit("bench_sliding: part %s ended with status %d; nothing more is started" % (part, rc))
        return
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    (part_kernels if args.part == "kernels" else part_net)(args, emit)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

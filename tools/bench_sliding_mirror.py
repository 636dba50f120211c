"""Micro-benchmark of mirroring inside the sliding window (msk_sw_gather_mirrored / msk_sw_accumulate_mirrored of
medicalseg_amd/csrc/msk_sliding.hip, core.infer.sliding_window_inference(mirror_axes=...)) beside the yardsticks of the same run.
python tools/bench_sliding_mirror.py [--iters K] [--out FILE] [--part kernels|net|all]

--part all (default) touches no GPU itself: it runs the two parts as child processes, each under a time limit of its own, and
stops at the first that fails.

kernel rows (--part kernels): one window, operands resident in HBM, at roi 128^3 (C = 2 and C = 3) and 512 x 512 x 12 (C = 20), the
volume 8 voxels larger on every axis, the window at w origin 4 (16 bytes per lane on the accumulator side).  HIP-event ms, median
[min .. max] of 5 means of --iters calls, a 1 GiB buffer written before every call.  For K = 2, 4, 8 passes of one window, with
and without a W mirror among the masks (K = 8 without W: the four D / H masks twice, which only the kernel interface can ask for):
  fused   ONE msk_sw_accumulate_mirrored call with the K rows: K logits read, the accumulator read and written: K + 2 tensors
  chain   what the kernels before it compose: per pass msk_flip_axes of the window logits (not for mask 0) + msk_sw_accumulate
          (two reads, one write): 5 K - 2 tensors, and no place for the factor 1 / K
The mark: fused median <= chain median + (chain max - chain min), the convention of bench_clip and bench_region_loss.  TB/s of the
fused row = (K + 2) window tensors / median, next to msk_d2d of one window tensor (2 tensors).
Report only: msk_sw_gather_mirrored of 8 patches (every mask) against msk_sw_gather + msk_flip_axes of the same patches, Cin = 1.
call rows (--part net): wall ms (synchronised), best / median of --iters, an eval-mode VNet (3 classes), one 256^3 volume, roi
128^3, overlap 0.5 (27 windows): the unmirrored call, and mirror_axes = (0, 1, 2) (216 forwards) against 8 x the unmirrored call."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((128, 128, 128), 2), ((128, 128, 128), 3), ((512, 512, 12), 20)]
MARGIN = 8
ORIGIN = (0, 4, 4, 4)
MASKS = {(2, True): [0, 4], (4, True): [0, 1, 4, 5], (8, True): list(range(8)),
         (2, False): [0, 1], (4, False): [0, 1, 2, 3], (8, False): [0, 1, 2, 3, 0, 1, 2, 3]}
FLUSH_BYTES = 1 << 30
REPEATS = 5
PART_LIMIT_S = {"kernels": 420, "net": 420}


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
    emit(f"# mirrored sliding-window kernels (msk_sw_accumulate_mirrored / msk_sw_gather_mirrored), one window, {dev.name()}")
    emit(f"# HIP-event ms, median [min .. max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call; "
         "TB/s = moved window tensors * tensor bytes / median")
    emit("# mark: fused median <= chain median + (chain max - chain min)")
    flush = dev.malloc(FLUSH_BYTES)
    rng = np.random.default_rng(0)
    misses = []
    vp = C.c_void_p

    def row(name, call, tensors, nbytes):
        for _ in range(3):
            call()
        m = time_events(dev, call, args.iters, flush)
        emit(f"  {name:46s} {m[0]:.4f} [{m[1]:.4f} .. {m[2]:.4f}] ms  {tensors:2d} tensors  {tensors * nbytes / (m[0] * 1e-3) / 1e12:5.2f} TB/s")
        return m

    for roi, c in CASES:
        vol = tuple(v + MARGIN for v in roi)
        plan = SlidingPlan(vol, roi, overlap=0.5)
        tables = []
        for T in plan.tables:
            p = dev.malloc(T.nbytes)
            dev.h2d(p, T)
            tables.append(p)
        tabs = tuple(v for p, s in zip(tables, plan.starts) for v in (vp(p), len(s)))
        nbytes = roi[0] * roi[1] * roi[2] * c * 4
        emit(f"[roi {roi[0]}x{roi[1]}x{roi[2]}, C = {c}, volume {vol[0]}x{vol[1]}x{vol[2]}]  window tensor = {nbytes / 1e6:.1f} MB")
        lg = Tensor.empty(dev, 8, roi[0], roi[1], roi[2], c, arena=False)
        fill(dev, lg.ptr, nbytes, rng)
        for p in range(1, 8):
            dev.d2d(lg.ptr + p * nbytes, lg.ptr, nbytes)
        tmp = Tensor.empty(dev, 1, roi[0], roi[1], roi[2], c, arena=False)
        acc = Tensor.empty(dev, 1, vol[0], vol[1], vol[2], c, arena=False)
        dev.memset(acc.ptr, 0, vol[0] * vol[1] * vol[2] * c * 4)
        one = [Tensor(dev, lg.ptr + p * nbytes, 1, roi[0], roi[1], roi[2], c) for p in range(8)]
        o7 = np.array([ORIGIN + (0, 0, 0)], np.int32)
        row("msk_d2d of one window tensor", lambda: dev.d2d(tmp.ptr, lg.ptr, nbytes), 2, nbytes)
        for K in (2, 4, 8):
            for with_w in (False, True):
                masks = MASKS[(K, with_w)]
                o8 = np.array([ORIGIN + (0, 0, 0, m) for m in masks], np.int32)
                run = Tensor(dev, lg.ptr, K, roi[0], roi[1], roi[2], c)
                tag = f"K = {K}, masks {masks}"

                def fused():
                    dev.call("msk_sw_accumulate_mirrored", run.msk(), o8.ctypes.data_as(vp), *tabs, C.c_float(1.0 / K), acc.msk())

                def chain():
                    for p, m in enumerate(masks):
                        src = one[p]
                        if m:
                            dev.call("msk_flip_axes", src.msk(), tmp.msk(), m)
                            src = tmp
                        dev.call("msk_sw_accumulate", src.msk(), o7.ctypes.data_as(vp), *tabs, acc.msk())

                chain_tensors = 5 * K - 2 * masks.count(0)
                y = row(f"chain, {tag}", chain, chain_tensors, nbytes)
                f = row(f"fused, {tag}", fused, K + 2, nbytes)
                limit = y[0] + (y[2] - y[1])
                ok = f[0] <= limit
                emit(f"    fused / chain = {f[0] / y[0]:.2f} (by traffic {(K + 2) / chain_tensors:.2f});  mark <= {limit:.4f} ms: "
                     + ("met" if ok else "MISSED"))
                if not ok:
                    misses.append(f"roi {roi} C = {c} {tag}: {f[0]:.4f} ms > {limit:.4f} ms")
                dev.memset(acc.ptr, 0, vol[0] * vol[1] * vol[2] * c * 4)
        for t_ in (lg, tmp, acc):
            dev.free(t_.ptr)
        # report only: the mirrored gather of 8 patches (every mask) at Cin = 1
        nb1 = roi[0] * roi[1] * roi[2] * 4
        big = Tensor.empty(dev, 1, vol[0], vol[1], vol[2], 1, arena=False)
        fill(dev, big.ptr, vol[0] * vol[1] * vol[2] * 4, rng)
        pat, pat2 = (Tensor.empty(dev, 8, roi[0], roi[1], roi[2], 1, arena=False) for _ in range(2))
        o5 = np.array([ORIGIN + (m,) for m in range(8)], np.int32)
        o4 = np.ascontiguousarray(o5[:, :4])
        pone = [(Tensor(dev, pat.ptr + p * nb1, 1, roi[0], roi[1], roi[2], 1), Tensor(dev, pat2.ptr + p * nb1, 1, roi[0], roi[1], roi[2], 1))
                for p in range(8)]

        def gather_chain():
            dev.call("msk_sw_gather", big.msk(), pat.msk(), o4.ctypes.data_as(vp), C.c_float(0.0))
            for m in range(1, 8):
                dev.call("msk_flip_axes", pone[m][0].msk(), pone[m][1].msk(), m)

        emit(f"  [gather, Cin = 1, 8 patches, every mask]  patch = {nb1 / 1e6:.1f} MB  (report only)")
        row("msk_sw_gather + 7 x msk_flip_axes", gather_chain, 16 + 14, nb1)
        row("msk_sw_gather_mirrored", lambda: dev.call("msk_sw_gather_mirrored", big.msk(), pat.msk(), o5.ctypes.data_as(vp), C.c_float(0.0)),
            16, nb1)
        for t_ in (big, pat, pat2):
            dev.free(t_.ptr)
        for p in tables:
            dev.free(p)
    dev.free(flush)
    emit("# marks missed: " + ("none" if not misses else "; ".join(misses)))


def part_net(args, emit):
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import Tensor, get_device
    from medicalseg_amd.models import VNet
    dev = get_device()
    rng = np.random.default_rng(1)
    model = VNet(num_classes=3)
    model.eval()
    x256 = Tensor.empty(dev, 1, 256, 256, 256, 1, arena=False)
    fill(dev, x256.ptr, 256 ** 3 * 4, rng)

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

    n = len(infer.SlidingPlan((256, 256, 256), (128, 128, 128), overlap=0.5).windows(1))
    emit(f"[VNet, 3 classes, eval mode, {dev.name()}]  256^3, roi 128^3, {n} windows, sw_batch_size 1; wall ms, synchronised, "
         f"best / median of {args.iters}")
    plain = wall(lambda: infer.sliding_window_inference(model, x256, (128, 128, 128), overlap=0.5))
    mirr = wall(lambda: infer.sliding_window_inference(model, x256, (128, 128, 128), overlap=0.5, mirror_axes=(0, 1, 2)))
    emit(f"  sliding_window_inference, no mirror ({n} forwards)           {plain[0]:.2f} / {plain[1]:.2f}")
    emit(f"  sliding_window_inference, mirror_axes (0, 1, 2) ({8 * n} forwards) {mirr[0]:.2f} / {mirr[1]:.2f}   against 8 x the unmirrored call: "
         f"{mirr[1] - 8 * plain[1]:+.2f} ms median, {100.0 * (mirr[1] - 8 * plain[1]) / (8 * plain[1]):+.1f} %")
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
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--iters", str(args.iters if part == "kernels" else min(args.iters, 3))]
            if args.out:
                cmd += ["--out", args.out]
            rc = subprocess.run(cmd, timeout=PART_LIMIT_S[part]).returncode
            if rc != 0:
                sys.exit("bench_sliding_mirror: part %s ended with status %d; nothing more is started" % (part, rc))
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

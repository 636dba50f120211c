"""Micro-benchmark of the confusion-count kernel (medicalseg_amd/csrc/msk_metrics.hip, msk_confusion3d) beside the host
path it replaces (device -> host copy of prediction and label, then utils.metric.confusion_counts on numpy arrays).
python tools/bench_metrics.py [--iters K] [--out FILE]

Sizes: 128^3 with C = 2, 512 x 512 x 12 with C = 20 (the MRI head), 300 x 512 x 512 with C = 2 and C = 20.
Distributions of (prediction, label): 'one bin' (all zeros), 'uniform' (independent uniformly random classes: C*C
equally likely bins) and 'blobs' (12 boxes, ~5 % foreground, the prediction shifted by one voxel).

device rows: HIP-event time of one msk_confusion3d call (accumulate = 0: the memset of the counts and the kernel),
after 3 warm-up calls.  Every figure is the mean of --iters calls, taken 5 times: the row gives the median and the
[min, max] of those 5 means, the spread one should read differences against.  'cold' writes a 1 GiB buffer before every
call so the inputs come from HBM (the 256 MB last-level cache holds the smaller sizes otherwise: 'warm').  GB/s = 8
bytes per voxel over the cold median.
host rows: wall time of the two D2H copies and of the numpy path on this machine's CPU, best of 2; the counts are
compared with the device's.
yardstick: msk_minmax_norm (a plain streaming kernel of this library: 4 bytes read + 4 written per voxel) over the
300 x 512 x 512 float volume, timed the same way in the same process."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [((128, 128, 128), 2), ((512, 512, 12), 20), ((300, 512, 512), 2), ((300, 512, 512), 20)]
FLUSH_BYTES = 1 << 30
REPEATS = 5


def inputs(shape, ncls, kind):
    import metrics_reference as R
    if kind == "one bin":
        z = np.zeros(shape, np.int32)
        return z, z.copy()
    if kind == "uniform":
        rng = np.random.default_rng(ncls)
        return (rng.integers(0, ncls, shape, dtype=np.int32), rng.integers(0, ncls, shape, dtype=np.int32))
    p, l = R.blobs(shape, ncls, 7)
    return np.ascontiguousarray(p[0, 0]), np.ascontiguousarray(l[0, 0])


def timed(dev, call, iters, flush):
    """median, min, max over REPEATS of the mean HIP-event ms of `iters` calls"""
    means = []
    for r in range(REPEATS):
        tot = 0.0
        for i in range(iters):
            if flush:
                dev.memset(flush, (r * iters + i) & 0xFF, FLUSH_BYTES)
            dev.timer_start()
            call()
            tot += dev.timer_stop()
        means.append(tot / iters)
    means.sort()
    return means[REPEATS // 2], means[0], means[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from medicalseg_amd.device import get_device
    from medicalseg_amd.utils import metric
    dev = get_device()
    lines = [f"# confusion counts (msk_confusion3d), {dev.name()}, host CPU: {os.cpu_count()} logical CPUs visible",
             f"# device: HIP-event ms per call, median [min, max] of {REPEATS} means of {args.iters} calls; warm = back to "
             "back, cold = 1 GiB written before every call; GB/s = 8 bytes per voxel / cold median",
             "# host: wall ms of the D2H copies of prediction and label + utils.metric.confusion_counts on numpy, best of 2"]
    flush = dev.malloc(FLUSH_BYTES)
    vp = C.c_void_p
    for shape, ncls in CASES:
        vox = int(np.prod(shape))
        B = (ncls + 1) ** 2 + 1
        pp_, lp = dev.malloc(vox * 4), dev.malloc(vox * 4)
        out = dev.malloc(B * 8)
        lines.append(f"[{shape[0]}x{shape[1]}x{shape[2]}, C = {ncls}]  {vox * 8 / 1e6:.1f} MB read, {B} bins")
        for kind in ("one bin", "uniform", "blobs"):
            p, l = inputs(shape, ncls, kind)
            dev.h2d(pp_, p)
            dev.h2d(lp, l)
            call = lambda: dev.call("msk_confusion3d", vp(pp_), vp(lp), 1, C.c_long(vox), ncls, 255, vp(out), 0)
            for _ in range(3):
                call()
            warm = timed(dev, call, args.iters, None)
            cold = timed(dev, call, args.iters, flush)
            got = dev.d2h(out, (1, B), np.uint64)
            d2h, host = [], []
            for _ in range(2):
                t0 = time.perf_counter()
                hp, hl = dev.d2h(pp_, (1,) + shape, np.int32), dev.d2h(lp, (1,) + shape, np.int32)
                t1 = time.perf_counter()
                want = metric.confusion_counts(hp, hl, ncls)
                t2 = time.perf_counter()
                d2h.append((t1 - t0) * 1e3)
                host.append((t2 - t1) * 1e3)
            same = bool(np.array_equal(got, want))
            fg = 100.0 * float(np.count_nonzero(l)) / vox
            lines.append(f"  {kind:8s} device  warm {warm[0]:.4f} [{warm[1]:.4f}, {warm[2]:.4f}] ms   cold {cold[0]:.4f} "
                         f"[{cold[1]:.4f}, {cold[2]:.4f}] ms  {vox * 8 / (cold[0] * 1e-3) / 1e9:6.0f} GB/s   "
                         f"non-zero bins {int(np.count_nonzero(got))}, foreground {fg:.1f} %, device == host: {same}")
            lines.append(f"  {kind:8s} host    d2h {min(d2h):.1f} ms + numpy {min(host):.1f} ms = {min(d2h) + min(host):.1f} ms"
                         f"   ({(min(d2h) + min(host)) / cold[0]:.0f} x the cold device call)")
            del p, l, hp, hl
        for ptr in (pp_, lp, out):
            dev.free(ptr)
    # the yardstick: a plain streaming kernel over 629 MB of traffic
    shape = CASES[-1][0]
    vox = int(np.prod(shape))
    src, dst = dev.malloc(vox * 4), dev.malloc(vox * 4)
    dev.h2d(src, np.random.default_rng(0).random(shape, dtype=np.float32))
    call = lambda: dev.call("msk_minmax_norm", vp(src), vp(dst), C.c_size_t(vox), 1, C.c_float(0.0), C.c_float(1.0))
    for _ in range(3):
        call()
    cold = timed(dev, call, args.iters, flush)
    lines.append(f"[yardstick: msk_minmax_norm {shape[0]}x{shape[1]}x{shape[2]} float32, given bounds]  {vox * 8 / 1e6:.1f} MB "
                 f"read + written   cold {cold[0]:.4f} [{cold[1]:.4f}, {cold[2]:.4f}] ms  "
                 f"{vox * 8 / (cold[0] * 1e-3) / 1e9:6.0f} GB/s")
    for ptr in (src, dst, flush):
        dev.free(ptr)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

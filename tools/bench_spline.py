"""Micro-benchmark of order-3 resampling (medicalseg_amd/csrc/msk_spline.hip: msk_spline_resample3d = three prefilter passes
over a float64 workspace + the 64-tap zoom) beside a streaming copy of that workspace, beside the order-1 msk_resample3d on
the same shapes, and beside the host round trip it replaces (device -> host copy, scipy.ndimage.zoom(order=3), host ->
device copy).
python tools/bench_spline.py [--iters K] [--out FILE]

Workloads (float32, standard normal values): 1008x1008x12 -> 512x512x12 (the MRI preprocessing shape), 300x512x512 -> 128^3
(the CT preprocessing shape), 48^3 -> 96^3 (the up-sample of RandomLowResolution3D at zoom 0.5).

device rows, HIP-event ms, median [min, max] of 5 means of --iters calls, a 1 GiB buffer written before every call so that
the operands come from HBM:
  copy        the yardstick of a prefilter pass: msk_d2d of the float64 workspace ((d+24)(h+24)(w+24) doubles)
  pass D/H/W  the three prefilter launches, from the per-launch profile of the whole call (event brackets around each launch).
              Every pass streams the workspace twice by construction (the forward sweep writes what the backward sweep
              reads), so its mark is 1.5 x 2 x copy; the D pass reads the float32 source instead of the workspace on its
              forward sweep and is held to the same mark
  zoom        the 64-tap launch, same profile; its yardstick is msk_resample3d order 1 on the same shapes (ratio reported,
              no mark)
  whole call  msk_spline_resample3d, profile off
host row: wall ms of the D2H copy, scipy.ndimage.zoom(order=3, mode='nearest') on this machine's CPU and the H2D copy, once."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [((1008, 1008, 12), (512, 512, 12)), ((300, 512, 512), (128, 128, 128)), ((48, 48, 48), (96, 96, 96))]
FLUSH_BYTES = 1 << 30
REPEATS = 5
PASS_MARK = 1.5 * 2      # the margin msk_gauss_blur3d was given per pass x the round trips a pass makes by construction
TAGS = ("spline_prefilter_d", "spline_prefilter_h", "spline_prefilter_w", "spline_zoom")


def median3(means):
    means = sorted(means)
    return means[len(means) // 2], means[0], means[-1]


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
    return median3(means)


def profiled(dev, call, iters, flush):
    """per-launch ms of one call, by tag: median [min, max] of REPEATS means"""
    means = {t: [] for t in TAGS}
    dev.prof_enable(True)
    for r in range(REPEATS):
        dev.prof_reset()
        for i in range(iters):
            dev.memset(flush, (r * iters + i) & 0xFF, FLUSH_BYTES)
            call()
        dev.sync()
        rep = dev.prof_report()
        for t in TAGS:
            calls, ms = rep[t]
            assert calls == iters, (t, calls)
            means[t].append(ms / iters)
    dev.prof_enable(False)
    return {t: median3(v) for t, v in means.items()}


def fmt(m):
    return f"{m[0]:.4f} [{m[1]:.4f}, {m[2]:.4f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import scipy.ndimage
    import spline_reference as R
    from medicalseg_amd.device import get_device
    dev = get_device()
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# order-3 resampling (msk_spline_resample3d), {dev.name()}, host CPU: {os.cpu_count()} logical CPUs visible")
    emit(f"# device: HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call")
    emit(f"# mark of a prefilter pass: {PASS_MARK:.1f} x copy (1.5 x the 2 round trips of the workspace a pass makes by construction)")
    emit("# host: wall ms of D2H + scipy.ndimage.zoom(order=3, mode='nearest') + H2D, once")
    flush = dev.malloc(FLUSH_BYTES)
    vp = C.c_void_p
    for src_shape, dst_shape in CASES:
        n_in, n_out = int(np.prod(src_shape)), int(np.prod(dst_shape))
        data = np.random.default_rng(n_in).standard_normal(src_shape).astype(np.float32)
        nbytes = C.c_size_t(0)
        assert dev.lib.msk_spline_workspace(*src_shape, C.byref(nbytes)) == 0
        wbytes = nbytes.value
        x, y, ws, ws2 = dev.malloc(n_in * 4), dev.malloc(n_out * 4), dev.malloc(wbytes), dev.malloc(wbytes)
        dev.h2d(x, data)
        dev.memset(ws2, 0, wbytes)
        emit("[%dx%dx%d -> %dx%dx%d]  source = %.1f MB, destination = %.1f MB, float64 workspace = %.1f MB" %
             (*src_shape, *dst_shape, n_in * 4 / 1e6, n_out * 4 / 1e6, wbytes / 1e6))

        def spline():
            dev.call("msk_spline_resample3d", vp(x), *src_shape, 0, 0, 0, *src_shape, vp(y), *dst_shape, vp(ws), C.c_size_t(wbytes))

        def linear():
            dev.call("msk_resample3d", vp(x), *src_shape, vp(y), *dst_shape, 1, 0)

        for call in (spline, linear):
            for _ in range(2):
                call()
        copy = timed(dev, lambda: dev.d2d(ws2, ws, wbytes), args.iters, flush)
        emit(f"  {'copy of the workspace (msk_d2d)':42s} {fmt(copy)}  {2 * wbytes / (copy[0] * 1e-3) / 1e9:6.0f} GB/s read + written")
        lin = timed(dev, linear, args.iters, flush)
        emit(f"  {'msk_resample3d order 1':42s} {fmt(lin)}")
        prof = profiled(dev, spline, args.iters, flush)
        for tag, name in zip(TAGS[:3], ("prefilter pass D (reads the source)", "prefilter pass H", "prefilter pass W (through LDS)")):
            m = prof[tag]
            ratio = m[0] / copy[0]
            emit(f"  {name:42s} {fmt(m)}  {ratio:6.2f} x copy   mark {PASS_MARK:.1f} x: {'met' if ratio <= PASS_MARK else 'MISSED'}")
        z = prof[TAGS[3]]
        emit(f"  {'zoom (64 taps)':42s} {fmt(z)}  {z[0] / lin[0]:6.2f} x msk_resample3d order 1")
        whole = timed(dev, spline, args.iters, flush)
        emit(f"  {'whole call (profile off)':42s} {fmt(whole)}  {whole[0] / lin[0]:6.2f} x msk_resample3d order 1")
        # the host round trip
        t0 = time.perf_counter()
        h = dev.d2h(x, src_shape, np.float32)
        t1 = time.perf_counter()
        out = scipy.ndimage.zoom(h, np.array(dst_shape) / np.array(src_shape), order=3, mode="nearest")
        t2 = time.perf_counter()
        dev.h2d(y, np.ascontiguousarray(out, np.float32))
        dev.sync()
        t3 = time.perf_counter()
        total = (t3 - t0) * 1e3
        emit(f"  host scipy.ndimage.zoom(order=3)           d2h {(t1 - t0) * 1e3:.1f} + cpu {(t2 - t1) * 1e3:.1f} + h2d {(t3 - t2) * 1e3:.1f} = "
             f"{total:.1f} ms   ({total / whole[0]:.0f} x the whole call)")
        spline()
        got = dev.d2h(y, dst_shape, np.float32)
        bound = 2.0 ** -23 * np.abs(out.astype(np.float64)) + 1e-12 * np.abs(data).max()
        emit(f"  device vs scipy: {int((got != out).sum())} of {n_out} voxels unequal, all within one float32 rounding: "
             f"{bool((np.abs(got.astype(np.float64) - out) <= bound).all())}")
        if n_in < 10 ** 6:
            emit(f"  device == statement: {bool(np.array_equal(got, R.spline_zoom(data, dst_shape)))}")
        del data
        for ptr in (x, y, ws, ws2):
            dev.free(ptr)
    dev.free(flush)
    emit("# not measured: crop boxes, the down-sample of RandomLowResolution3D (order 0), the transform inside a training loop "
         "(reader_cost), volumes whose padded box approaches 2^31 voxels, occupancy and LDS bank-conflict counters of the W pass")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

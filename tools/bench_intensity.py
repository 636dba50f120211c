"""Micro-benchmark of the intensity-augmentation kernels (medicalseg_amd/csrc/msk_intensity.hip: msk_intensity_stats,
msk_intensity_apply, msk_gauss_blur3d) beside a streaming copy and a streaming read of the same buffer, and beside the host
round trip they replace (device -> host copy, numpy / scipy, host -> device copy).
python tools/bench_intensity.py [--iters K] [--out FILE]

Workloads: float32 volumes of 96^3, 128^3 and 300 x 512 x 512 voxels (standard normal values).

device rows, HIP-event ms, median [min, max] of 5 means of --iters calls, a 1 GiB buffer written before every call so that
the operands come from HBM:
  copy      the yardstick of apply and blur: msk_d2d of the volume into a second buffer
  read      the yardstick of stats: a plain streaming read of the SAME buffer (msk_channel_sum over it as one channel)
  stats     msk_intensity_stats (chunk pass + finish pass)
  apply     msk_intensity_apply out of place, one row per mode (NOISE and GAMMA evaluate logf / cosf / powf per voxel)
  blur      msk_gauss_blur3d, sigma 0.5 (radius 2) and sigma 1 (radius 4) on all three axes: three passes
host rows: wall ms of the D2H copy, the numpy / scipy evaluation on this machine's CPU and the H2D copy, best of 2 (once for
the largest volume)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(96, 96, 96), (128, 128, 128), (300, 512, 512)]
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
    import intensity_reference as R
    import scipy.ndimage
    from medicalseg_amd._lib import MskTensor
    from medicalseg_amd.device import get_device
    dev = get_device()
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# intensity augmentation (msk_intensity_stats / msk_intensity_apply / msk_gauss_blur3d), {dev.name()}, "
         f"host CPU: {os.cpu_count()} logical CPUs visible")
    emit(f"# device: HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call")
    emit("# x = the ratio to the yardstick of the same run: copy (msk_d2d, same bytes as apply) or read (msk_channel_sum)")
    emit("# host: wall ms of D2H + numpy / scipy + H2D, best of 2 (once for 300x512x512)")
    flush = dev.malloc(FLUSH_BYTES)
    vp = C.c_void_p
    for shape in SHAPES:
        n = int(np.prod(shape))
        data = np.random.default_rng(n).standard_normal(shape).astype(np.float32)
        x, y, tmp = dev.malloc(n * 4), dev.malloc(n * 4), dev.malloc(n * 4)
        dev.h2d(x, data)
        nbytes = C.c_size_t(0)
        assert dev.lib.msk_intensity_stats_workspace(C.c_long(n), C.byref(nbytes)) == 0
        ws, rec_a, rec_b, sums = dev.malloc(nbytes.value), dev.malloc(32), dev.malloc(32), dev.malloc(64)
        emit(f"[{shape[0]}x{shape[1]}x{shape[2]}]  volume = {n * 4 / 1e6:.1f} MB, stats workspace = {nbytes.value / 1e3:.1f} KB "
             f"({100.0 * nbytes.value / (n * 4):.3f} % of the volume)")
        dev.call("msk_intensity_stats", vp(x), C.c_long(n), vp(ws), vp(rec_a))
        dev.call("msk_intensity_stats", vp(x), C.c_long(n), vp(ws), vp(rec_b))
        as_tensor = MskTensor(x, 1, shape[0], shape[1], shape[2], 1, 1)

        def apply(mode, *p):
            params = np.zeros(4, np.float32)
            params[:len(p)] = p
            return lambda: dev.call("msk_intensity_apply", vp(x), vp(y), C.c_long(n), mode, params.ctypes.data_as(vp), vp(rec_a),
                                    vp(rec_b), C.c_uint64(12345))

        def blur(sigma):
            t = R.taps(sigma)
            r = (len(t) - 1) // 2
            tp = t.ctypes.data_as(vp)
            return lambda: dev.call("msk_gauss_blur3d", vp(x), vp(y), *shape, tp, r, tp, r, tp, r, vp(tmp)), t

        b05, t05 = blur(0.5)
        b1, t1 = blur(1.0)
        rows = [("copy (msk_d2d)", lambda: dev.d2d(y, x, n * 4), None),
                ("read (msk_channel_sum)", lambda: dev.call("msk_channel_sum", as_tensor, vp(sums), 0), None),
                ("stats", lambda: dev.call("msk_intensity_stats", vp(x), C.c_long(n), vp(ws), vp(rec_b)), "read"),
                ("apply SCALE", apply(R.SCALE, 1.25), "copy"), ("apply CONTRAST", apply(R.CONTRAST, 1.25, 1.0), "copy"),
                ("apply RESTORE", apply(R.RESTORE), "copy"), ("apply GAMMA (powf)", apply(R.GAMMA, 0.7, 0.0), "copy"),
                ("apply NOISE (logf, cosf)", apply(R.NOISE, 0.1), "copy"),
                ("blur sigma 0.5 (r = 2), 3 passes", b05, "copy"), ("blur sigma 1 (r = 4), 3 passes", b1, "copy")]
        res = {}
        for name, call, yard in rows:
            for _ in range(3):
                call()
            res[name] = timed(dev, call, args.iters, flush)
            rate = f"  {n * 4 / (res[name][0] * 1e-3) / 1e9:6.0f} GB/s of volume"
            ratio = ""
            if yard:
                base = res[[k for k in res if k.startswith(yard)][0]][0]
                ratio = f"   {res[name][0] / base:.2f} x {yard}"
            emit(f"  {name:36s} {fmt(res[name])}{rate}{ratio}")
        # the host round trip
        reps = 1 if n > 10 ** 7 else 2
        rec = R.stats(data) if n < 10 ** 7 else None

        def host(fn):
            best = None
            for _ in range(reps):
                t0 = time.perf_counter()
                h = dev.d2h(x, shape, np.float32)
                t1_ = time.perf_counter()
                out = np.ascontiguousarray(fn(h), np.float32)
                t2 = time.perf_counter()
                dev.h2d(y, out)
                dev.sync()
                t3 = time.perf_counter()
                cur = ((t1_ - t0) * 1e3, (t2 - t1_) * 1e3, (t3 - t2) * 1e3)
                if best is None or sum(cur) < sum(best):
                    best = cur
            return best

        rng = np.random.default_rng(1)

        def np_contrast(h):
            m = h.mean(dtype=np.float64)
            return np.clip((h - np.float32(m)) * np.float32(1.25) + np.float32(m), h.min(), h.max())

        def np_gamma(h):
            mn, rg = h.min(), h.max() - h.min()
            return np.power((h - mn) / (rg + np.float32(1e-7)), np.float32(0.7)) * rg + mn

        host_rows = [("brightness (numpy multiply)", lambda h: h * np.float32(1.25), "apply SCALE"),
                     ("contrast (numpy mean, clip)", np_contrast, "apply CONTRAST"),
                     ("gamma (numpy power)", np_gamma, "apply GAMMA (powf)"),
                     ("noise (numpy Generator.normal)", lambda h: h + rng.normal(0.0, 0.1, h.shape).astype(np.float32),
                      "apply NOISE (logf, cosf)"),
                     ("blur sigma 1 (scipy gaussian_filter)",
                      lambda h: scipy.ndimage.gaussian_filter(h, 1.0, mode="reflect", truncate=4), "blur sigma 1 (r = 4), 3 passes")]
        for name, fn, device_row in host_rows:
            d2h, work, h2d = host(fn)
            total = d2h + work + h2d
            emit(f"  host {name:38s} d2h {d2h:.1f} + cpu {work:.1f} + h2d {h2d:.1f} = {total:.1f} ms   "
                 f"({total / res[device_row][0]:.0f} x the device row)")
        # the device results against the statement (the smaller volumes; the tests cover the rest)
        if rec is not None:
            got = dev.d2h(rec_b, (4,), np.float64)
            b1()
            ok = np.array_equal(dev.d2h(y, shape, np.float32), R.blur(data, (1.0, 1.0, 1.0)))
            emit(f"  device == statement: stats {bool(np.array_equal(got, rec))}, blur sigma 1 {bool(ok)}")
        del data
        for ptr in (x, y, tmp, ws, rec_a, rec_b, sums):
            dev.free(ptr)
    dev.free(flush)
    emit("# not measured: the transforms inside a training loop (reader_cost), pointers that are only 4-byte aligned (the scalar "
         "forms), sigma 2 (radius 8), per-axis sigmas, volumes of 2^31 - 1 voxels (the finish pass is one workgroup)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

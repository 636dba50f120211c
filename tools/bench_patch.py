"""Micro-benchmark of the patch-cropping kernels (medicalseg_amd/csrc/msk_patch.hip: msk_patch_select, msk_patch_crop) beside
the host path they replace (device -> host copy of the label, then the numpy statement of tests/patch_reference.py).
python tools/bench_patch.py [--iters K] [--out FILE]

Workloads: 128^3 with C = 3 on blobs (boxes, a few per cent foreground), 300 x 512 x 512 with C = 3 on blobs, and
12 x 512 x 512 with C = 20 on uniformly random labels (the worst case of the LDS histogram).

device rows, HIP-event ms, median [min, max] of 5 means of --iters calls, a 1 GiB buffer written before every call so that
the operands come from HBM:
  read        the yardstick: a plain streaming read of the SAME label buffer (msk_channel_sum over it as one float channel)
  select x1   one msk_patch_select call, one foreground patch: memset of the totals + histogram pass + select pass
  select x16  the same with 16 foreground patches (the histogram is shared)
  uniform     a call without a foreground patch: the select pass alone, the label is not read
  histogram / select pass   the two kernels of 'select x1' apart, from the library's per-launch profile (a run of its own:
              the profile's events sit between the launches)
  crop        msk_patch_crop of a float volume of the same extent at the origin select x1 chose; GB/s = patch read + written
host rows: wall ms of the D2H copy of the label and of patch_reference.select_all on this machine's CPU, best of 2; the
record is compared with the device's."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [((128, 128, 128), 3, "blobs", (96, 96, 96)), ((300, 512, 512), 3, "blobs", (96, 96, 96)),
         ((12, 512, 512), 20, "uniform", (12, 128, 128))]
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
    import patch_reference as R
    from medicalseg_amd._lib import MskTensor
    from medicalseg_amd.device import get_device
    dev = get_device()
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# patch cropping (msk_patch_select / msk_patch_crop), {dev.name()}, host CPU: {os.cpu_count()} logical CPUs visible")
    emit(f"# device: HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call")
    emit("# host: wall ms of the D2H copy of the label + patch_reference.select_all (one patch) on numpy, best of 2")
    flush = dev.malloc(FLUSH_BYTES)
    vp = C.c_void_p
    for shape, ncls, kind, roi in CASES:
        vox = int(np.prod(shape))
        classes = np.arange(1, ncls, dtype=np.int32)
        if kind == "blobs":
            label = R.blobs(shape, ncls, 7)
        else:
            label = np.random.default_rng(ncls).integers(0, ncls, shape, dtype=np.int32)
        fg = 100.0 * float(np.count_nonzero(label)) / vox
        lp, ip = dev.malloc(vox * 4), dev.malloc(vox * 4)
        dev.h2d(lp, label)
        dev.memset(ip, 0x3C, vox * 4)
        nbytes = C.c_size_t(0)
        assert dev.lib.msk_patch_workspace(C.c_long(vox), ncls, C.byref(nbytes)) == 0
        ws, sel, out = dev.malloc(nbytes.value), dev.malloc(16 * 32), dev.malloc(int(np.prod(roi)) * 4)
        sums = dev.malloc(64)
        emit(f"[{shape[0]}x{shape[1]}x{shape[2]}, C = {ncls}, {kind}, foreground {fg:.1f} %]  label = {vox * 4 / 1e6:.1f} MB, "
             f"workspace = {nbytes.value / 1e3:.1f} KB ({100.0 * nbytes.value / (vox * 4):.3f} % of the label), "
             f"{-(-vox // 4096)} chunks")
        words = np.ascontiguousarray(R.mixed_words(16, 11))
        words[:, 0] = 1
        words[0, 1:] = [0x9E3779B9, 0x7F4A7C15, 1, 2, 3]
        uni = words.copy()
        uni[:, 0] = 0

        def select(w, n):
            dev.call("msk_patch_select", vp(lp), *shape, ncls, classes.ctypes.data_as(vp), len(classes), *roi, w.ctypes.data_as(vp), n,
                     vp(ws), vp(sel), None)

        as_floats = MskTensor(lp, 1, shape[0], shape[1], shape[2], 1, 1)
        rows = [("read (msk_channel_sum, the label buffer)", lambda: dev.call("msk_channel_sum", as_floats, vp(sums), 0)),
                ("select x1", lambda: select(words, 1)), ("select x16", lambda: select(words, 16)),
                ("uniform x16 (no histogram)", lambda: select(uni, 16))]
        res = {}
        for name, call in rows:
            for _ in range(3):
                call()
            res[name] = timed(dev, call, args.iters, flush)
            rate = f"  {vox * 4 / (res[name][0] * 1e-3) / 1e9:6.0f} GB/s of label" if "uniform" not in name else ""
            emit(f"  {name:42s} {fmt(res[name])}{rate}")
        read = res[rows[0][0]][0]
        # the two kernels apart
        dev.sync()
        dev.prof_enable(True)
        dev.prof_reset()
        for i in range(args.iters):
            dev.memset(flush, i & 0xFF, FLUSH_BYTES)
            select(words, 1)
        dev.sync()
        prof = dev.prof_report()
        dev.prof_enable(False)
        hist = prof["patch_hist"][1] / prof["patch_hist"][0]
        selp = prof["patch_select"][1] / prof["patch_select"][0]
        emit(f"  {'histogram pass (profile, mean)':42s} {hist:.4f} ms  {vox * 4 / (hist * 1e-3) / 1e9:6.0f} GB/s of label   "
             f"{hist / read:.2f} x the streaming read of the same buffer (a cause is owed above 2 x)")
        emit(f"  {'select pass (profile, mean)':42s} {selp:.4f} ms")
        select(words, 1)
        got = dev.d2h(sel, (1, 8), np.int32)
        pad = int(np.array([0.0], np.float32).view(np.uint32)[0])
        crop = lambda: dev.call("msk_patch_crop", vp(ip), *shape, vp(sel), vp(out), *roi, C.c_uint32(pad))
        for _ in range(3):
            crop()
        m = timed(dev, crop, args.iters, flush)
        emit(f"  {'crop %dx%dx%d at w0 = %d' % (roi + (int(got[0, 2]),)):42s} {fmt(m)}  "
             f"{2 * int(np.prod(roi)) * 4 / (m[0] * 1e-3) / 1e9:6.0f} GB/s read + written")
        d2h, host = [], []
        for _ in range(2):
            t0 = time.perf_counter()
            hl = dev.d2h(lp, shape, np.int32)
            t1 = time.perf_counter()
            want, _ = R.select_all(hl, roi, ncls, classes.tolist(), words[:1])
            t2 = time.perf_counter()
            d2h.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
        total = min(d2h) + min(host)
        emit(f"  {'host':42s} d2h {min(d2h):.1f} ms + numpy {min(host):.1f} ms = {total:.1f} ms   "
             f"({total / res['select x1'][0]:.0f} x select x1), device == host: {bool(np.array_equal(got, want))}")
        del label, hl
        for ptr in (lp, ip, ws, sel, out, sums):
            dev.free(ptr)
    dev.free(flush)
    emit("# not measured: the transform inside a training loop (reader_cost), labels that are not 16-byte aligned, C = 256")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

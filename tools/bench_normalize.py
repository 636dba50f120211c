"""Micro-benchmark of msk_nonzero_bbox, msk_clip_zscore and msk_fg_stats (medicalseg_amd/csrc/msk_normalize.hip) beside the
yardsticks of the same run on the same buffers: msk_channel_sum, msk_d2d, and the chain 2 x msk_topk_select + msk_intensity_stats.
python tools/bench_normalize.py [--iters K] [--out FILE] [--no-host]

Every timed call is bracketed by a HIP event pair and preceded by a write of a 1 GiB buffer (four times the last-level cache),
so its operands come from HBM.  A row is repeated five times; a repeat is the mean of --iters calls; the table gives the median,
the minimum and the maximum of the five.

Marks, each against existing kernels of the same run:
  msk_nonzero_bbox   median <= 2 x msk_channel_sum of the same buffer (the project's mark for a one-pass reduction); a volume
                     with a zero border and zero blobs, and one that is non-zero everywhere (every workgroup issues its atomics).
  msk_clip_zscore    without a mask: median <= 1.5 x msk_d2d of the volume (the mark of msk_intensity_apply's non-transcendental
                     modes); with an int32 mask that is read: that mark x 12 / 8 for the 4 more bytes per voxel.
  msk_fg_stats       median <= the chain that yields the unmasked numbers today, 2 x msk_topk_select + 1 x msk_intensity_stats,
                     timed as one unit, plus that chain's max - min.  The chain has no mask and no interpolation neighbour.
Without a mark: the host round trips these replace (D2H + np.percentile + numpy clip / z-score + H2D; D2H + np.nonzero), wall
clock, once per shape."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(96, 96, 96), (128, 128, 128), (300, 512, 512)]
FLUSH_BYTES = 1 << 30
REPEATS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host round trips")
    args = ap.parse_args()
    from medicalseg_amd.device import Tensor, get_device
    dev = get_device()
    vp = lambda p: C.c_void_p(p) if p else None
    flush, it_byte = dev.malloc(FLUSH_BYTES), [1]

    def timed(fn):
        """median, min, max over REPEATS of the mean HIP-event time of args.iters calls, each behind a 1 GiB write"""
        for _ in range(3):
            fn()
        reps = []
        for _ in range(REPEATS):
            tot = 0.0
            for _ in range(args.iters):
                dev.memset(flush, it_byte[0] & 0xFF, FLUSH_BYTES)
                it_byte[0] += 1
                dev.timer_start()
                fn()
                tot += dev.timer_stop()
            reps.append(tot / args.iters)
        return float(np.median(reps)), min(reps), max(reps)

    lines = [f"# normalisation kernels, {dev.name()}: HIP-event time per call in ms, operands from HBM (1 GiB written before every call);",
             f"# median [min .. max] of {REPEATS} repeats, a repeat = the mean of {args.iters} calls.  GB/s = algorithmic bytes / median.",
             "# launches: msk_nonzero_bbox 1 memset + 2, msk_clip_zscore 1, msk_fg_stats 1 memset + 5; the chain 2 memsets + 12."]
    misses = []
    for d, h, w in SHAPES:
        n = d * h * w
        vb = n * 4
        rng = np.random.default_rng(0)
        full = np.round(rng.standard_normal(n, dtype=np.float32) * 300.0 - 200.0).astype(np.float32) + np.float32(0.5)   # CT-like, never zero
        blobs = full.reshape(d, h, w).copy()
        bd, bh, bw = max(d // 8, 1), max(h // 8, 1), max(w // 8, 1)
        blobs[:bd], blobs[-bd:], blobs[:, :bh], blobs[:, -bh:], blobs[:, :, :bw], blobs[:, :, -bw:] = 0, 0, 0, 0, 0, 0
        blobs[d // 3:d // 2, h // 3:h // 2, w // 3:w // 2] = 0
        label = ((blobs > 0) & (rng.random((d, h, w), dtype=np.float32) < 0.5)).astype(np.int32)
        xf, xb, y, mk = dev.malloc(vb), dev.malloc(vb), dev.malloc(vb), dev.malloc(vb)
        dev.h2d(xf, full)
        dev.h2d(xb, blobs)
        dev.h2d(mk, label)
        nbytes = C.c_size_t(0)
        assert dev.lib.msk_fg_stats_workspace(C.c_long(n), C.byref(nbytes)) == 0
        ws = dev.malloc(nbytes.value)
        assert dev.lib.msk_topk_workspace(C.c_long(n), C.byref(nbytes)) == 0
        tws = dev.malloc(nbytes.value)
        assert dev.lib.msk_intensity_stats_workspace(C.c_long(n), C.byref(nbytes)) == 0
        iws = dev.malloc(nbytes.value)
        rec, trec, irec, box, csum = dev.small(32), dev.small(32), dev.small(8), dev.small(8), dev.small(4)
        lines.append(f"[{d}x{h}x{w}]  volume {vb / 1e6:.1f} MB")

        def row(name, fn, nbytes, limit=None):
            med, lo, hi = timed(fn)
            text = f"  {name:64s} {med:.4f} [{lo:.4f} .. {hi:.4f}]  {nbytes / (med * 1e-3) / 1e9:5.0f} GB/s"
            if limit is not None:
                ok = med <= limit
                text += f"   mark <= {limit:.4f}: {'met' if ok else 'MISSED'}"
                if not ok:
                    misses.append(f"{d}x{h}x{w} {name.strip()}: {med:.4f} ms > {limit:.4f} ms")
            lines.append(text)
            return med, lo, hi

        # ---- bounding box ----
        for tag, xp in (("zero border and blobs", xb), ("non-zero everywhere", xf)):
            t = Tensor(dev, xp, 1, d, h, w, 1, 1, None)
            ys = row(f"msk_channel_sum, {tag}  [yardstick]", lambda: dev.call("msk_channel_sum", t.msk(), vp(csum), 0), vb)
            row(f"msk_nonzero_bbox, {tag}", lambda: dev.call("msk_nonzero_bbox", vp(xp), d, h, w, 0, vp(box)), vb, 2 * ys[0])
        # ---- statistics ----
        i_lo, i_hi = int(np.floor((n - 1) * 0.005)), int(np.floor((n - 1) * 0.995))

        def chain():
            dev.call("msk_topk_select", vp(xb), C.c_long(n), C.c_long(n - i_lo), vp(tws), vp(trec))
            dev.call("msk_topk_select", vp(xb), C.c_long(n), C.c_long(n - i_hi), vp(tws), vp(trec))
            dev.call("msk_intensity_stats", vp(xb), C.c_long(n), vp(iws), vp(irec))

        yc = row("2 x msk_topk_select + msk_intensity_stats  [yardstick]", chain, 9 * vb)
        limit = yc[0] + (yc[2] - yc[1])
        for tag, mode, mp, per in (("all voxels", 0, None, 4), ("x != 0", 1, None, 4), ("int32 mask", 2, mk, 8)):
            row(f"msk_fg_stats, {tag}, (0.5, 99.5)",
                lambda: dev.call("msk_fg_stats", vp(xb), vp(mp), C.c_long(n), mode, C.c_double(0.5), C.c_double(99.5), vp(ws), vp(rec)),
                4 * per * n, limit)
        # ---- apply ----
        yd = row("msk_d2d of the volume  [yardstick]", lambda: dev.d2d(y, xb, vb), 2 * vb)
        app = lambda mode, mp, flags: dev.call("msk_clip_zscore", vp(xb), vp(mp), C.c_long(n), mode, vp(rec), None, flags, C.c_float(0.0), vp(y))
        row("msk_clip_zscore, clip + z-score, no mask", lambda: app(0, None, 3), 2 * vb, 1.5 * yd[0])
        row("msk_clip_zscore, clip + z-score, x != 0 masked out", lambda: app(1, None, 7), 2 * vb, 1.5 * yd[0])
        row("msk_clip_zscore, clip + z-score, int32 mask masked out", lambda: app(2, mk, 7), 3 * vb, 1.5 * yd[0] * 12 / 8)
        row("msk_clip_zscore, in place, no mask (no mark)",
            lambda: dev.call("msk_clip_zscore", vp(y), None, C.c_long(n), 0, vp(rec), None, 1, C.c_float(0.0), vp(y)), 2 * vb)
        # ---- the host round trips these replace ----
        if not args.no_host:
            dev.sync()
            t0 = time.perf_counter()
            a = dev.d2h(xb, (d, h, w), np.float32)
            fg = a[a != 0].astype(np.float64)
            lo, hi = np.percentile(fg, [0.5, 99.5])
            out = ((np.clip(a, lo, hi) - fg.mean()) / max(fg.std(), 1e-8)).astype(np.float32)
            dev.h2d(y, out)
            dev.sync()
            t1 = time.perf_counter()
            nz = np.nonzero(dev.d2h(xb, (d, h, w), np.float32))
            _ = [(int(c.min()), int(c.max()) + 1) for c in nz]
            t2 = time.perf_counter()
            lines.append(f"  host: D2H + np.percentile + clip / z-score + H2D, wall clock, once {(t1 - t0) * 1e3:40.1f} ms")
            lines.append(f"  host: D2H + np.nonzero extremes, wall clock, once {(t2 - t1) * 1e3:59.1f} ms")
        for p in (xf, xb, y, mk, ws, tws, iws):
            dev.free(p)
    dev.free(flush)
    lines.append("misses: " + ("none" if not misses else "; ".join(misses)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

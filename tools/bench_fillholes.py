"""Micro-benchmark of the hole filling (medicalseg_amd/csrc/msk_ccl.hip, msk_fill_holes3d) beside three yardsticks of the same
run on the same buffers.   python tools/bench_fillholes.py [--iters K] [--out FILE] [--no-host]

Method: HIP-event time of one call (all of its launches, no host synchronisation) with 1 GiB written before every call, so
the operands come from HBM.  A row is repeated five times; a repeat is the mean of --iters calls; the table gives the median
[min .. max] of the repeats.

Inputs at 96^3, 128^3 and 300 x 512 x 512:
  body    float32, a smooth body with a zero margin, interior zero pockets and channels to the outside (the preprocessing
          case), mask form;
  noise   int32, 50 % random zeros, mask form;
  blobs   int32, a C = 3 blob prediction with 4 % zeros sprinkled in (the post-processing case), label form.

Yardsticks:
  msk_connected_components3d on the int32 complement mask (x == 0): the same union-find plus the compaction, radix sort,
          ranking and relabel that hole filling does not need.  MARK: msk_fill_holes3d median <= that median + the spread
          (max - min) of msk_fill_holes3d's own repeats.
  msk_d2d of the volume: the ratio is reported, no mark (the searches are data-dependent).
  the host round trip it replaces, wall clock, once: D2H + scipy.ndimage.binary_fill_holes (blobs: preprocess.fill_holes_host)
          + H2D.
Also: the wall time of DevicePipeline's chain zscore((0.5, 99.5), 'nonzero') at 128^3 with and without fill_holes=True (the
former downloads a status word, so both are timed on the host around a synchronisation)."""
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


def _coarse(rng, shape, cell, values):
    """a random field of `values` on cells of `cell` voxels, cut to shape"""
    g = rng.choice(np.asarray(values), [(s + cell - 1) // cell for s in shape])
    for ax in range(3):
        g = np.repeat(g, cell, axis=ax)
    return g[:shape[0], :shape[1], :shape[2]]


def inputs(shape):
    rng = np.random.default_rng(sum(shape))
    d, h, w = shape
    z, y, x = np.ogrid[:d, :h, :w]
    inside = ((z - d / 2) / (0.42 * d)) ** 2 + ((y - h / 2) / (0.42 * h)) ** 2 + ((x - w / 2) / (0.42 * w)) ** 2 < 1
    body = (rng.standard_normal(shape, dtype=np.float32) * 40 + 300).astype(np.float32)
    body[~inside] = 0
    body[_coarse(rng, shape, 6, [0] * 9 + [1]) == 1] = 0          # pockets; those that meet the margin are channels
    noise = (rng.random(shape, dtype=np.float32) < 0.5).astype(np.int32)
    blobs = _coarse(rng, shape, 12, [0, 0, 1, 2, 3]).astype(np.int32)
    blobs[rng.random(shape, dtype=np.float32) < 0.04] = 0
    return [("body  float32 mask ", body, 0, 0), ("noise int32   mask ", noise, 1, 0), ("blobs int32   label", blobs, 1, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the host round trips")
    args = ap.parse_args()
    import scipy.ndimage
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.device import get_device
    dev = get_device()
    flush, it_byte = dev.malloc(FLUSH_BYTES), [1]

    def timed(fn):
        for _ in range(2):
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

    lines = [f"# hole filling, {dev.name()}: HIP-event time per call in ms, operands from HBM (1 GiB written before every call);",
             f"# median [min .. max] of {REPEATS} repeats, a repeat = the mean of {args.iters} calls.",
             "# mark: msk_fill_holes3d median <= msk_connected_components3d median (complement mask) + fill's own max - min"]
    misses = []
    st, cnt = dev.small(4), dev.small(4)
    for shape in SHAPES:
        n = int(np.prod(shape))
        vb = n * 4
        src, dst, comp = dev.malloc(vb), dev.malloc(vb), dev.malloc(vb)
        lines.append(f"[{shape[0]}x{shape[1]}x{shape[2]}]  volume {vb / 1e6:.1f} MB")
        for name, arr, dtype, mode in inputs(shape):
            dev.h2d(src, arr)
            dev.h2d(comp, (arr == 0).astype(np.int32))
            fill = lambda: dev.call("msk_fill_holes3d", C.c_void_p(src), C.c_void_p(dst), 1, *shape, dtype, mode, None, 0,
                                    C.c_void_p(st), C.c_void_p(cnt))
            ccl = lambda: dev.call("msk_connected_components3d", C.c_void_p(comp), C.c_void_p(dst), 1, *shape, 1, 0, 0,
                                   C.c_void_p(st), None)
            f_med, f_lo, f_hi = timed(fill)
            fill()
            filled, status = int(dev.d2h(cnt, (1,), np.int32)[0]), int(dev.d2h(st, (1,), np.int32)[0])
            got = dev.d2h(dst, shape, np.int32)
            c_med, c_lo, c_hi = timed(ccl)
            d_med, d_lo, d_hi = timed(lambda: dev.d2d(dst, src, vb))
            limit = c_med + (f_hi - f_lo)
            ok = f_med <= limit
            if not ok:
                misses.append(f"{shape[0]}x{shape[1]}x{shape[2]} {name.strip()}: {f_med:.4f} ms > {limit:.4f} ms")
            zeros = int(np.count_nonzero(arr == 0))
            lines.append(f"  {name}  {zeros / n * 100:4.1f} % zeros, {filled} filled, status {status}")
            lines.append(f"    msk_fill_holes3d                        {f_med:9.4f} [{f_lo:.4f} .. {f_hi:.4f}]   "
                         f"mark <= {limit:.4f}: {'met' if ok else 'MISSED'}   {f_med / d_med:.1f} x msk_d2d")
            lines.append(f"    msk_connected_components3d (x == 0)     {c_med:9.4f} [{c_lo:.4f} .. {c_hi:.4f}]   [yardstick]")
            lines.append(f"    msk_d2d of the volume                   {d_med:9.4f} [{d_lo:.4f} .. {d_hi:.4f}]   [yardstick]")
            if not args.no_host:
                t0 = time.perf_counter()
                a = dev.d2h(src, shape, arr.dtype)
                t1 = time.perf_counter()
                ref = pp.fill_holes_host(a) if mode else scipy.ndimage.binary_fill_holes(a != 0).astype(np.int32)
                t2 = time.perf_counter()
                dev.h2d(dst, ref)
                dev.sync()
                t3 = time.perf_counter()
                lines.append(f"    host round trip, once: d2h {(t1 - t0) * 1e3:.1f} + scipy {(t2 - t1) * 1e3:.1f} + h2d {(t3 - t2) * 1e3:.1f} = "
                             f"{(t3 - t0) * 1e3:.1f} ms wall;  device == host: {bool(np.array_equal(got, ref))}")
        for p in (src, dst, comp):
            dev.free(p)
    # the chain at 128^3
    body = inputs((128, 128, 128))[0][1]
    pipe = pp.DevicePipeline(pooled=True)
    rows = {}
    for fill_flag in (False, True):
        reps = []
        for r in range(REPEATS + 1):
            tot = 0.0
            for _ in range(args.iters):
                chain = pipe.image(body)
                dev.sync()
                t0 = time.perf_counter()
                chain.zscore((0.5, 99.5), "nonzero", fill_holes=fill_flag)
                dev.sync()
                tot += time.perf_counter() - t0
                chain.vol.free()
            if r:                                                   # the first repeat warms the pool up
                reps.append(tot / args.iters * 1e3)
        rows[fill_flag] = (float(np.median(reps)), min(reps), max(reps))
    lines.append("[chain at 128x128x128]  wall ms of _Chain.zscore((0.5, 99.5), 'nonzero') between two synchronisations")
    for flag, (med, lo, hi) in rows.items():
        lines.append(f"    fill_holes={str(flag):5s}                        {med:9.4f} [{lo:.4f} .. {hi:.4f}]")
    lines.append("marks missed: " + ("none" if not misses else "; ".join(misses)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

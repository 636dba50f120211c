"""Micro-benchmark of the Lovasz-Softmax kernels (medicalseg_amd/csrc/msk_loss_lovasz.hip) beside the yardsticks of the same run.
python tools/bench_lovasz.py [--iters K] [--out FILE] [--no-step]

Every timed call is bracketed by a HIP event pair and preceded by a write of a 1 GiB buffer (four times the last-level cache),
so its operands come from HBM as they do inside a training step.  A row is repeated five times; a repeat is the mean of --iters
calls; the table gives the median, the minimum and the maximum of the five.

Marks.  Forward: the yardstick is msk_auc_pack + msk_auc_counts on the same voxels and classes (the softmax of the same logits):
a key-only radix sort with the same four digit passes.  A key-only digit pass moves 12 bytes per key (4 read by the histogram, 4
read and 4 written by the scatter), a key-index pass 20 (4, then 8 read and 8 written), so the mark is yardstick median x 20 / 12
+ (its max - min).  The Lovasz forward makes the same number of passes; its first reads no index plane (16 bytes), which the
factor does not claim.  Backward: the yardstick is msk_region_loss_bwd with the DiceCELoss defaults on the same buffers; the
Lovasz pass reads one more float per class (dL/de), so the mark is yardstick median x (12C + 4) / (8C + 4) + (its max - min).
Without a mark: the backward pass adding into dz; the stages of the forward from the library's per-launch profile (a run of its
own); the sum stage, which also delivers dL/de from rank to voxel (a scattered 4-byte write), beside msk_d2d of the bytes it
moves (12 per key); and one VNet 96^3 batch-2 training step with DiceCELoss and with DiceLovaszLoss, alternating on one model."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((2, 96, 96, 96), 3), ((2, 128, 128, 128), 3), ((1, 512, 512, 12), 20)]   # (N, D, H, W), C
FLUSH_BYTES = 1 << 30
REPEATS = 5
STAGES = ("lovasz_pack", "lovasz_hist", "lovasz_scan", "lovasz_scatter", "lovasz_scan_fg", "lovasz_sum", "lovasz_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true", help="skip the VNet training step")
    args = ap.parse_args()
    from medicalseg_amd.device import Tensor, get_device
    dev = get_device()
    vp = lambda p: C.c_void_p(p) if p else None
    f = C.c_float
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

    lines = [f"# Lovasz-Softmax kernels, {dev.name()}: HIP-event time per call in ms, operands from HBM (1 GiB written before every call);",
             f"# median [min .. max] of {REPEATS} repeats, a repeat = the mean of {args.iters} calls.  GB/s = algorithmic bytes / median.",
             "# forward mark: (msk_auc_pack + msk_auc_counts) median x 20/12 + (its max - min); both make four digit passes of 8, 8, 8 and",
             "# 7 / 6 bits.  backward mark: region bwd median x (12C+4)/(8C+4) + (its max - min).  10 per cent of the labels 255."]
    misses = []
    for (n, d, h, w), c in SHAPES:
        vox = n * d * h * w
        rng = np.random.default_rng(0)
        z = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        probs = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dz = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dev.h2d(z.ptr, (rng.standard_normal(vox * c) * 2).astype(np.float32))
        dev.memset(dz.ptr, 0, vox * c * 4)
        dev.call("msk_softmax_c", z.msk(), probs.msk())
        y = rng.integers(0, c, vox).astype(np.int32)
        y[rng.random(vox) < 0.1] = 255
        yp = dev.malloc(y.nbytes)
        dev.h2d(yp, y)
        ya = np.where(y == 255, 0, y).astype(np.int32)                        # msk_auc_pack takes labels in [0, C) only
        yap = dev.malloc(ya.nbytes)
        dev.h2d(yap, ya)
        out, stats = dev.small(2 + c), dev.small(2 * (5 * n * c + 2))          # dev.small counts floats
        l_out, l_stats = dev.small(2 + c), dev.small(2 * (4 * c + 2))
        nbytes = C.c_size_t(0)
        assert dev.lib.msk_lovasz_workspace(C.c_long(vox), c, 1, C.byref(nbytes)) == 0
        ws, ws_bytes = dev.malloc(nbytes.value), nbytes.value
        assert dev.lib.msk_auc_workspace(C.c_long(vox), c, C.byref(nbytes)) == 0
        a_ws, a_bytes = dev.malloc(nbytes.value), nbytes.value
        a_keys, a_status, a_out = dev.malloc(vox * c * 4), dev.small(4), dev.small(6 * c)
        lg, lb, keys = vox * c * 4, vox * 4, vox * c

        def y_fwd():
            dev.call("msk_auc_pack", probs.msk(), vp(yap), vp(a_keys), C.c_long(vox), C.c_long(0), vp(a_status))
            dev.call("msk_auc_counts", vp(a_keys), C.c_long(vox), C.c_long(vox), c, vp(a_ws), C.c_size_t(a_bytes), vp(a_out))

        s = (255, 0, 0, 1, 0, 0, f(1e-5), f(0.0), f(0.0), 1, f(0.0))
        r_fwd = lambda: dev.call("msk_region_loss_fwd", z.msk(), vp(yp), *s, None, vp(out), vp(stats))
        r_bwd = lambda: dev.call("msk_region_loss_bwd", z.msk(), vp(yp), *s, None, vp(stats), f(1.0), f(1.0), 0, dz.msk())
        l_fwd = lambda: dev.call("msk_lovasz_fwd", z.msk(), vp(yp), 255, 0, C.c_uint64(0), 0, vp(ws), C.c_size_t(ws_bytes), vp(l_out),
                                 vp(l_stats))
        l_bwd = lambda acc=0: dev.call("msk_lovasz_bwd", z.msk(), vp(yp), 255, 0, vp(ws), C.c_size_t(ws_bytes), vp(l_stats), f(1.0), acc,
                                       dz.msk())
        lines.append(f"[{n}x{d}x{h}x{w}, C = {c}]  logits {lg / 1e6:.1f} MB, labels {lb / 1e6:.1f} MB, {keys / 1e6:.1f} M keys")

        def row(name, fn, nbytes, limit=None):
            med, lo, hi = timed(fn)
            text = f"  {name:58s} {med:.4f} [{lo:.4f} .. {hi:.4f}]  {nbytes / (med * 1e-3) / 1e9:5.0f} GB/s"
            if limit is not None:
                ok = med <= limit
                text += f"   mark <= {limit:.4f}: {'met' if ok else 'MISSED'}"
                if not ok:
                    misses.append(f"{n}x{d}x{h}x{w} C={c} {name.strip()}: {med:.4f} ms > {limit:.4f} ms")
            lines.append(text)
            return med, lo, hi

        sort_key_only, sort_key_index = 4 * 12 * keys, (16 + 3 * 20) * keys
        yf = row("msk_auc_pack + msk_auc_counts  [yardstick]", y_fwd, lg + lb + 4 * keys + sort_key_only + 8 * keys)
        row("Lovasz fwd (22 launches)", l_fwd, lg + lb + 4 * keys + sort_key_index + 4 * keys + 12 * keys, yf[0] * 20 / 12 + (yf[2] - yf[1]))
        r_fwd()
        yb = row("region bwd, DiceCELoss defaults  [yardstick]", r_bwd, 2 * lg + lb)
        l_fwd()
        row("Lovasz bwd, writes dz", l_bwd, 3 * lg + lb, yb[0] * (12 * c + 4) / (8 * c + 4) + (yb[2] - yb[1]))
        row("Lovasz bwd, adds into dz (no mark)", lambda: l_bwd(1), 4 * lg + lb)
        row("msk_d2d of 6 bytes per key: 12 moved (no mark)", lambda: dev.d2d(ws, ws + 8 * keys, 6 * keys), 12 * keys)
        # the stages of the forward from the per-launch profile, in a run of its own
        dev.prof_reset()
        dev.prof_enable(True)
        for _ in range(args.iters):
            dev.memset(flush, it_byte[0] & 0xFF, FLUSH_BYTES)
            it_byte[0] += 1
            l_fwd()
        dev.sync()
        prof = dev.prof_report()
        dev.prof_enable(False)
        stage_bytes = {"lovasz_pack": lg + lb + 4 * keys, "lovasz_hist": 4 * 4 * keys, "lovasz_scatter": (12 + 3 * 16) * keys,
                       "lovasz_scan_fg": 4 * keys, "lovasz_sum": 12 * keys}
        for tag in STAGES:
            if tag in prof:
                ms = prof[tag][1] / args.iters
                note = "  (rank -> voxel delivery of dL/de inside)" if tag == "lovasz_sum" else ""
                rate = f"{stage_bytes[tag] / (ms * 1e-3) / 1e9:5.0f} GB/s" if tag in stage_bytes else " " * 10
                lines.append(f"  {'  stage ' + tag + ' (profile, no mark)':58s} {ms:.4f} per call, {prof[tag][0] // args.iters} launches  {rate}{note}")
        for p in (z.ptr, probs.ptr, dz.ptr, yp, yap, ws, a_ws, a_keys):
            dev.free(p)
    dev.free(flush)

    if not args.no_step:
        from medicalseg_amd import optimizer as optim
        from medicalseg_amd.device import to_tensor
        from medicalseg_amd.models import DiceCELoss, DiceLovaszLoss, VNet
        from medicalseg_amd.utils import loss_computation
        rng = np.random.default_rng(1)
        model = VNet(num_classes=3)
        model.train()
        opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        x = to_tensor(rng.standard_normal((2, 1, 96, 96, 96)).astype(np.float32))
        yt = to_tensor(rng.integers(0, 3, (2, 96, 96, 96)).astype(np.int32))
        recipes = {"DiceCELoss": {"types": [DiceCELoss()], "coef": [1]}, "DiceLovaszLoss": {"types": [DiceLovaszLoss()], "coef": [1]}}
        times = {k: [] for k in recipes}
        for rep in range(3 + REPEATS):
            for name, losses in recipes.items():
                dev.sync()
                t0 = time.perf_counter()
                loss_list, _ = loss_computation(model(x), yt, losses)
                sum(loss_list).backward()
                opt.step()
                dev.sync()
                if rep >= 3:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        lines.append("[one VNet training step, 2x1x96^3, 3 classes: wall clock between two device syncs, ms; the two losses alternate "
                     "on one model, 3 warm-up rounds]")
        for name, t in times.items():
            lines.append(f"  {name:58s} {np.median(t):.3f} [{min(t):.3f} .. {max(t):.3f}]")
    lines.append("misses: " + ("none" if not misses else "; ".join(misses)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

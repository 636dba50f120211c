"""Micro-benchmark of the top-k kernels (medicalseg_amd/csrc/msk_loss_topk.hip) beside the yardsticks of the same run:
msk_region_loss_fwd / msk_region_loss_bwd with the DiceCELoss defaults on the same buffers.
python tools/bench_topk.py [--iters K] [--out FILE] [--no-step]

Every timed call is bracketed by a HIP event pair and preceded by a write of a 1 GiB buffer (four times the last-level cache),
so its operands come from HBM as they do inside a training step.  A row is repeated five times; a repeat is the mean of --iters
calls; the table gives the median, the minimum and the maximum of the five.

Marks.  Forward: median <= region fwd median x (4C + 20) / (4C + 4) + extra launches x 2.2 us + (region fwd max - min).  The
factor is the ratio of algorithmic bytes per voxel (one pass over logits, label and the 4-byte workspace, then four 4-byte passes:
the histogram passes and the ordered sum; with digits of 11, 11 and 10 bits there are two histogram passes, one fewer than the
factor pays for); the top-k forward makes 5 launches and a 24 KiB memset where the region forward makes 2, and 2.2 us is the
dependent-launch cost measured in the training step: the memset is counted as a launch, 4 extra.
Backward: median <= region bwd median x (8C + 8) / (8C + 4) + (region bwd max - min).
Without a mark: msk_topk_select alone on the workspace against msk_channel_sum of the same buffer, the forward and the select with
msk_count_slot's same-bin aggregation in the first histogram pass (option "topk_agg_hist") instead of one LDS atomic per lane, and one VNet 128^3 batch-2 training
step with DiceCELoss and with DiceTopKLoss, alternating on one model."""
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
LAUNCH_MS = 2.2e-3
EXTRA_LAUNCHES = 4


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

    lines = [f"# top-k kernels, {dev.name()}: HIP-event time per call in ms, operands from HBM (1 GiB written before every call);",
             f"# median [min .. max] of {REPEATS} repeats, a repeat = the mean of {args.iters} calls.  GB/s = algorithmic bytes / median.",
             "# forward mark: region fwd median x (4C+20)/(4C+4) + 4 x 0.0022 + (its max - min); the top-k forward is 5 launches + 1 memset.",
             "# backward mark: region bwd median x (8C+8)/(8C+4) + (its max - min).  k = 10 per cent, 10 per cent of the labels 255."]
    misses = []
    for (n, d, h, w), c in SHAPES:
        vox = n * d * h * w
        rng = np.random.default_rng(0)
        z = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dz = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dev.h2d(z.ptr, (rng.standard_normal(vox * c) * 2).astype(np.float32))
        dev.memset(dz.ptr, 0, vox * c * 4)
        y = rng.integers(0, c, vox).astype(np.int32)
        y[rng.random(vox) < 0.1] = 255
        yp = dev.malloc(y.nbytes)
        dev.h2d(yp, y)
        out, stats = dev.small(2 + c), dev.small(2 * (5 * n * c + 2))          # dev.small counts floats
        t_out, rec, rec2, csum = dev.small(2 + c), dev.small(16), dev.small(16), dev.small(4)
        nbytes = C.c_size_t(0)
        assert dev.lib.msk_topk_workspace(C.c_long(vox), C.byref(nbytes)) == 0
        ws, ws2 = dev.malloc(nbytes.value), dev.malloc(nbytes.value)
        lvol = Tensor(dev, ws, 1, 1, 1, vox, 1, 1, None)                       # the per-voxel losses as a one-channel tensor
        lg, lb = vox * c * 4, vox * 4

        s = (255, 0, 0, 1, 0, 0, f(1e-5), f(0.0), f(0.0), 1, f(0.0))
        r_fwd = lambda: dev.call("msk_region_loss_fwd", z.msk(), vp(yp), *s, None, vp(out), vp(stats))
        r_bwd = lambda: dev.call("msk_region_loss_bwd", z.msk(), vp(yp), *s, None, vp(stats), f(1.0), f(1.0), 0, dz.msk())
        t_fwd = lambda: dev.call("msk_topk_ce_fwd", z.msk(), vp(yp), 255, None, f(10.0), vp(ws), vp(t_out), vp(rec))
        t_bwd = lambda acc=0: dev.call("msk_topk_ce_bwd", z.msk(), vp(yp), 255, None, vp(ws), vp(rec), f(1.0), acc, dz.msk())
        sel = lambda: dev.call("msk_topk_select", vp(ws), C.c_long(vox), C.c_long(vox // 10), vp(ws2), vp(rec2))
        lines.append(f"[{n}x{d}x{h}x{w}, C = {c}]  logits {lg / 1e6:.1f} MB, labels {lb / 1e6:.1f} MB")

        def row(name, fn, nbytes, limit=None):
            med, lo, hi = timed(fn)
            text = f"  {name:52s} {med:.4f} [{lo:.4f} .. {hi:.4f}]  {nbytes / (med * 1e-3) / 1e9:5.0f} GB/s"
            if limit is not None:
                ok = med <= limit
                text += f"   mark <= {limit:.4f}: {'met' if ok else 'MISSED'}"
                if not ok:
                    misses.append(f"{n}x{d}x{h}x{w} C={c} {name.strip()}: {med:.4f} ms > {limit:.4f} ms")
            lines.append(text)
            return med, lo, hi

        y_fwd = row("region fwd, DiceCELoss defaults  [yardstick]", r_fwd, lg + lb)
        r_fwd()
        y_bwd = row("region bwd, DiceCELoss defaults  [yardstick]", r_bwd, 2 * lg + lb)
        fwd_bytes, bwd_bytes = lg + 2 * lb + 3 * lb, 2 * lg + 2 * lb
        row("top-k fwd, k = 10 (5 launches + memset)", t_fwd, fwd_bytes,
            y_fwd[0] * (4 * c + 20) / (4 * c + 4) + EXTRA_LAUNCHES * LAUNCH_MS + (y_fwd[2] - y_fwd[1]))
        t_fwd()
        row("top-k bwd, k = 10, writes dz", t_bwd, bwd_bytes, y_bwd[0] * (8 * c + 8) / (8 * c + 4) + (y_bwd[2] - y_bwd[1]))
        row("top-k bwd, k = 10, adds into dz (no mark)", lambda: t_bwd(1), bwd_bytes)
        row("msk_channel_sum of the workspace (no mark)", lambda: dev.call("msk_channel_sum", lvol.msk(), vp(csum), 0), lb)
        row("msk_topk_select of the workspace, K = V / 10 (no mark)", sel, 4 * lb)
        dev.set_option("topk_agg_hist", 1)
        row("  ... same-bin aggregation in pass 1 (no mark)", sel, 4 * lb)
        row("top-k fwd, same-bin aggregation in pass 1 (no mark)", t_fwd, fwd_bytes)
        dev.set_option("topk_agg_hist", 0)
        for p in (z.ptr, dz.ptr, yp, ws, ws2):
            dev.free(p)
    dev.free(flush)

    if not args.no_step:
        from medicalseg_amd import optimizer as optim
        from medicalseg_amd.device import to_tensor
        from medicalseg_amd.models import DiceCELoss, DiceTopKLoss, VNet
        from medicalseg_amd.utils import loss_computation
        rng = np.random.default_rng(1)
        model = VNet(num_classes=3)
        model.train()
        opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        x = to_tensor(rng.standard_normal((2, 1, 128, 128, 128)).astype(np.float32))
        yt = to_tensor(rng.integers(0, 3, (2, 128, 128, 128)).astype(np.int32))
        recipes = {"DiceCELoss": {"types": [DiceCELoss()], "coef": [1]}, "DiceTopKLoss": {"types": [DiceTopKLoss()], "coef": [1]}}
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
        lines.append("[one VNet training step, 2x1x128^3, 3 classes: wall clock between two device syncs, ms; the two losses alternate "
                     "on one model, 3 warm-up rounds]")
        for name, t in times.items():
            lines.append(f"  {name:52s} {np.median(t):.3f} [{min(t):.3f} .. {max(t):.3f}]")
    lines.append("misses: " + ("none" if not misses else "; ".join(misses)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

"""Micro-benchmark of the region-loss kernels (medicalseg_amd/csrc/msk_loss_region.hip) beside the yardsticks of the same run:
the fused CE + Dice kernels (msk_loss_fwd_ex / msk_loss_bwd_ex with dice_softmax = 1) on the same buffers -- the same reads and
writes, one masked multiply less -- and msk_d2d of the logits.  python tools/bench_region_loss.py [--iters K] [--out FILE]

Every timed call is bracketed by a HIP event pair and preceded by a write of a 1 GiB buffer (four times the last-level cache),
so its operands come from HBM as they do inside a training step.  A row is repeated five times; a repeat is the mean of --iters
calls; the table gives the median, the minimum and the maximum of the five.

The mark (the convention of profiles/r17_bench_clip.txt): the new forward and backward with the DiceCELoss defaults each take no
longer than the matching CE + Dice call's median plus that call's own max - min.  gamma = 2 and batch_dice = False are reported
apart and carry no mark.  Last, one VNet 128^3 batch-2 training step with MixedLoss[CrossEntropyLoss, DiceLoss] and with
DiceCELoss, alternating on one model."""
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

    lines = [f"# region-loss kernels, {dev.name()}: HIP-event time per call in ms, operands from HBM (1 GiB written before every call);",
             f"# median [min .. max] of {REPEATS} repeats, a repeat = the mean of {args.iters} calls.  GB/s = algorithmic bytes / median.",
             "# mark: new <= yardstick median + (yardstick max - yardstick min), DiceCELoss defaults only."]
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
        ce_out, ce_stats = dev.small(2 + c), dev.small(2 * (3 * c + 2))
        wts = dev.small(c)
        dev.h2d(wts, np.ones(c, np.float32))
        lg, lb = vox * c * 4, vox * 4

        def region(gamma=0.0, batch=1):
            s = (255, 0, 0, batch, 0, 0, f(1e-5), f(0.0), f(0.0), 1, f(gamma))
            fwd = lambda: dev.call("msk_region_loss_fwd", z.msk(), vp(yp), *s, None, vp(out), vp(stats))
            bwd = lambda: dev.call("msk_region_loss_bwd", z.msk(), vp(yp), *s, None, vp(stats), f(1.0), f(1.0), 0, dz.msk())
            return fwd, bwd

        ce_fwd = lambda: dev.call("msk_loss_fwd_ex", z.msk(), vp(yp), vp(wts), 255, 1, None, vp(ce_out), vp(ce_stats))
        ce_bwd = lambda: dev.call("msk_loss_bwd_ex", z.msk(), vp(yp), vp(wts), 255, 1, None, vp(ce_stats), f(1.0), f(1.0), dz.msk())
        lines.append(f"[{n}x{d}x{h}x{w}, C = {c}]  logits {lg / 1e6:.1f} MB, labels {lb / 1e6:.1f} MB")

        def row(name, fn, nbytes, yard=None):
            med, lo, hi = timed(fn)
            text = f"  {name:44s} {med:.4f} [{lo:.4f} .. {hi:.4f}]  {nbytes / (med * 1e-3) / 1e9:5.0f} GB/s"
            if yard is not None:
                limit = yard[0] + (yard[2] - yard[1])
                ok = med <= limit
                text += f"   mark <= {limit:.4f}: {'met' if ok else 'MISSED'}"
                if not ok:
                    misses.append(f"{n}x{d}x{h}x{w} C={c} {name.strip()}: {med:.4f} ms > {limit:.4f} ms")
            lines.append(text)
            return med, lo, hi

        row("d2d of the logits", lambda: dev.d2d(dz.ptr, z.ptr, lg), 2 * lg)
        y_fwd = row("ce+dice fwd (dice_softmax=1)  [yardstick]", ce_fwd, lg + lb)
        ce_fwd()
        y_bwd = row("ce+dice bwd (dice_softmax=1)  [yardstick]", ce_bwd, 2 * lg + lb)
        fwd, bwd = region()
        row("region fwd, DiceCELoss defaults", fwd, lg + lb, y_fwd)
        fwd()
        row("region bwd, DiceCELoss defaults", bwd, 2 * lg + lb, y_bwd)
        fwd, bwd = region(gamma=2.0)
        row("region fwd, gamma = 2 (no mark)", fwd, lg + lb)
        fwd()
        row("region bwd, gamma = 2 (no mark)", bwd, 2 * lg + lb)
        if n == 2:
            fwd, bwd = region(batch=0)
            row("region fwd, batch_dice=False (no mark)", fwd, lg + lb)
            fwd()
            row("region bwd, batch_dice=False (no mark)", bwd, 2 * lg + lb)
        for p in (z.ptr, dz.ptr, yp):
            dev.free(p)
    dev.free(flush)

    if not args.no_step:
        from medicalseg_amd import optimizer as optim
        from medicalseg_amd.device import to_tensor
        from medicalseg_amd.models import CrossEntropyLoss, DiceCELoss, DiceLoss, MixedLoss, VNet
        from medicalseg_amd.utils import loss_computation
        rng = np.random.default_rng(1)
        model = VNet(num_classes=3)
        model.train()
        opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        x = to_tensor(rng.standard_normal((2, 1, 128, 128, 128)).astype(np.float32))
        yt = to_tensor(rng.integers(0, 3, (2, 128, 128, 128)).astype(np.int32))
        recipes = {"MixedLoss[CrossEntropyLoss, DiceLoss]": {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]},
                   "DiceCELoss": {"types": [DiceCELoss()], "coef": [1]}}
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
            lines.append(f"  {name:44s} {np.median(t):.3f} [{min(t):.3f} .. {max(t):.3f}]")
    lines.append("misses: " + ("none" if not misses else "; ".join(misses)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

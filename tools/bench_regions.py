"""Micro-benchmark of the region-based training kernels (medicalseg_amd/csrc/msk_loss_mlabel.hip) beside the yardsticks of the
same run on the same buffers: msk_region_loss_fwd / msk_region_loss_bwd with activation = sigmoid, do_bg = 1 and no focal term
(the same bytes; the new kernels add a table lookup and one logf per element), and msk_argmax_c for msk_regions_to_label.
python tools/bench_regions.py [--iters K] [--out FILE] [--no-step]

The method is that of tools/bench_region_loss.py: every timed call is bracketed by a HIP event pair and preceded by a write of a
1 GiB buffer (four times the last-level cache), so its operands come from HBM as they do inside a training step.  A row is
repeated five times; a repeat is the mean of --iters calls; the table gives the median, the minimum and the maximum of the five.

The mark: a new call takes no longer than its yardstick's median plus that yardstick's own max - min.  Last, one VNet 96^3
batch-2 training step with DiceCELoss and with DiceBCERegionLoss, alternating on one model."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((2, 96, 96, 96), 3), ((2, 128, 128, 128), 3), ((1, 512, 512, 12), 20)]   # (N, D, H, W), R
FLUSH_BYTES = 1 << 30
REPEATS = 5
LABEL_VALUES = 7


def make_table(R):
    """label value 0 in no region, 1 in all, the others in every third region (tests/mlabel_cases.py)"""
    t = np.zeros(256, dtype=np.uint32)
    t[1] = np.uint32((1 << R) - 1)
    for v in range(2, LABEL_VALUES):
        t[v] = np.uint32(sum(1 << r for r in range(R) if (r + v) % 3 == 0) or 1)
    return t


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

    lines = [f"# region-based training kernels, {dev.name()}: HIP-event time per call in ms, operands from HBM (1 GiB written before every call);",
             f"# median [min .. max] of {REPEATS} repeats, a repeat = the mean of {args.iters} calls.  GB/s = algorithmic bytes / median.",
             "# mark: new <= yardstick median + (yardstick max - yardstick min)."]
    misses = []
    for (n, d, h, w), c in SHAPES:
        vox = n * d * h * w
        rng = np.random.default_rng(0)
        z = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dz = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dev.h2d(z.ptr, (rng.standard_normal(vox * c) * 2).astype(np.float32))
        dev.memset(dz.ptr, 0, vox * c * 4)
        y = rng.integers(0, LABEL_VALUES, vox).astype(np.int32)
        y[rng.random(vox) < 0.1] = 255
        yp, pred = dev.malloc(y.nbytes), dev.malloc(y.nbytes)
        dev.h2d(yp, y)
        tp = dev.malloc(1024)
        dev.h2d(tp, make_table(c))
        out, stats = dev.small(2 + c), dev.small(2 * (5 * n * c + 2))          # dev.small counts floats
        r_out, r_stats = dev.small(2 + c), dev.small(2 * (5 * n * c + 2))
        order = (C.c_int32 * c)(*range(1, c + 1))
        lg, lb = vox * c * 4, vox * 4

        def yardstick(sq=0, batch=1):
            s = (255, 1, sq, batch, 1, 0, f(1e-5), f(0.0), f(0.0), 0, f(0.0))
            fwd = lambda: dev.call("msk_region_loss_fwd", z.msk(), vp(yp), *s, None, vp(r_out), vp(r_stats))
            bwd = lambda: dev.call("msk_region_loss_bwd", z.msk(), vp(yp), *s, None, vp(r_stats), f(0.0), f(1.0), 0, dz.msk())
            return fwd, bwd

        def mlabel(sq=0, batch=1):
            s = (255, vp(tp), 256, sq, batch, f(1e-5))
            fwd = lambda: dev.call("msk_mlabel_loss_fwd", z.msk(), vp(yp), *s, vp(out), vp(stats))
            bwd = lambda: dev.call("msk_mlabel_loss_bwd", z.msk(), vp(yp), *s, vp(stats), f(1.0), f(1.0), 0, dz.msk())
            return fwd, bwd

        lines.append(f"[{n}x{d}x{h}x{w}, R = {c}]  logits {lg / 1e6:.1f} MB, labels {lb / 1e6:.1f} MB")

        def row(name, fn, nbytes, yard=None):
            med, lo, hi = timed(fn)
            text = f"  {name:48s} {med:.4f} [{lo:.4f} .. {hi:.4f}]  {nbytes / (med * 1e-3) / 1e9:5.0f} GB/s"
            if yard is not None:
                limit = yard[0] + (yard[2] - yard[1])
                ok = med <= limit
                text += f"   mark <= {limit:.4f}: {'met' if ok else 'MISSED'}"
                if not ok:
                    misses.append(f"{n}x{d}x{h}x{w} R={c} {name.strip()}: {med:.4f} ms > {limit:.4f} ms")
            lines.append(text)
            return med, lo, hi

        row("d2d of the logits", lambda: dev.d2d(dz.ptr, z.ptr, lg), 2 * lg)
        yf, yb = yardstick()
        y_fwd = row("region fwd, sigmoid, do_bg  [yardstick]", yf, lg + lb)
        yf()
        y_bwd = row("region bwd, sigmoid, do_bg  [yardstick]", yb, 2 * lg + lb)
        fwd, bwd = mlabel()
        row("mlabel fwd (Dice + BCE)", fwd, lg + lb, y_fwd)
        fwd()
        row("mlabel bwd (Dice + BCE)", bwd, 2 * lg + lb, y_bwd)
        if n == 2:
            fwd, bwd = mlabel(sq=1, batch=0)
            row("mlabel fwd, squared_pred, per sample (no mark)", fwd, lg + lb)
            fwd()
            row("mlabel bwd, squared_pred, per sample (no mark)", bwd, 2 * lg + lb)
        y_arg = row("argmax_c  [yardstick]", lambda: dev.call("msk_argmax_c", z.msk(), vp(pred)), lg + lb)
        row("regions_to_label", lambda: dev.call("msk_regions_to_label", z.msk(), order, vp(pred)), lg + lb, y_arg)
        for p in (z.ptr, dz.ptr, yp, pred, tp):
            dev.free(p)
    dev.free(flush)

    if not args.no_step:
        from medicalseg_amd import optimizer as optim
        from medicalseg_amd.device import to_tensor
        from medicalseg_amd.models import DiceBCERegionLoss, DiceCELoss, VNet
        from medicalseg_amd.utils import loss_computation
        rng = np.random.default_rng(1)
        model = VNet(num_classes=3)
        model.train()
        opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        x = to_tensor(rng.standard_normal((2, 1, 96, 96, 96)).astype(np.float32))
        yt = to_tensor(rng.integers(0, 3, (2, 96, 96, 96)).astype(np.int32))
        recipes = {"DiceCELoss": {"types": [DiceCELoss()], "coef": [1]},
                   "DiceBCERegionLoss": {"types": [DiceBCERegionLoss([[1, 2, 3], [2, 3], [3]], [1, 2, 3])], "coef": [1]}}
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
        lines.append("[one VNet training step, 2x1x96^3, 3 channels: wall clock between two device syncs, ms; the two losses alternate "
                     "on one model, 3 warm-up rounds]")
        for name, t in times.items():
            lines.append(f"  {name:48s} {np.median(t):.3f} [{min(t):.3f} .. {max(t):.3f}]")
    lines.append("misses: " + ("none" if not misses else "; ".join(misses)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

"""What nnU-Net's form of deep supervision costs beside the reference's: VNetDeepSup(native_heads=True) scores its three heads
at their own extents against the label pyramid (msk_label_pyramid), VNetDeepSup resizes them to the input extent and scores
four full-size logit tensors.  python tools/bench_deepsup_native.py [--steps K] [--out FILE]

1. The pyramid launch at 2x96^3, 2x128^3 and 1x512x512x12 (the extents of the three heads of that input) next to msk_d2d of as
   many bytes as it writes: HIP-event time per call, back to back without a cache flush (the labels stay cache-resident: warm
   launch times).  Both are launch-bound; report only.
2. The training step of three models on one input in one run, alternating: plain VNet, VNetDeepSup (the yardstick) and
   VNetDeepSup(native_heads=True) at 1x512x512x12, 20 classes, the MRI kernels and strides, MixedLoss[CrossEntropyLoss, DiceLoss]
   per output; then at 2x96^3, 3 classes with DiceCELoss per output (report only).  A repeat is the mean of --steps consecutive
   steps of one model between two device synchronisations; the table gives the median, minimum and maximum of the repeats.
   Condition (MRI shape): median(VNetDeepSup) - median(native) > the larger of the two models' max - min.
3. The per-launch HIP-event profile of the two VNetDeepSup forms (one stream, serialised): every tag whose time per step differs
   between them."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PYRAMID_SHAPES = [((2, 96, 96, 96), [(12, 12, 12), (24, 24, 24), (48, 48, 48)]),
                  ((2, 128, 128, 128), [(16, 16, 16), (32, 32, 32), (64, 64, 64)]),
                  ((1, 512, 512, 12), [(64, 64, 4), (128, 128, 8), (256, 256, 9)])]
MRI_K, MRI_S = [[2, 2, 4], [2, 2, 2], [2, 2, 2], [2, 2, 2]], [[2, 2, 1], [2, 2, 1], [2, 2, 2], [2, 2, 2]]
ISO = [[2, 2, 2]] * 4
REPEATS = 7
WARMUP_ROUNDS = 3


def pyramid_rows(dev, iters, lines):
    def timed(fn):
        for _ in range(5):
            fn()
        reps = []
        for _ in range(REPEATS):
            tot = 0.0
            for _ in range(iters):
                dev.timer_start()
                fn()
                tot += dev.timer_stop()
            reps.append(tot / iters)
        return float(np.median(reps)), min(reps), max(reps)

    lines.append(f"[msk_label_pyramid, three levels in one launch, next to msk_d2d of the bytes it writes: HIP-event ms per call, median "
                 f"[min .. max] of {REPEATS} repeats of the mean of {iters} calls, warm (no cache flush between calls); both launch-bound, report only]")
    for (n, d, h, w), extents in PYRAMID_SHAPES:
        rng = np.random.default_rng(0)
        y = rng.integers(0, 20, (n, d, h, w)).astype(np.int32)
        src = dev.malloc(y.nbytes)
        dev.h2d(src, y)
        counts = [n * a * b * c for a, b, c in extents]
        out_bytes = 4 * sum(counts)
        dst = [dev.malloc(4 * c) for c in counts]
        copy = dev.malloc(out_bytes)
        ext = (C.c_int32 * (3 * len(extents)))(*[v for e in extents for v in e])
        ptrs = (C.c_void_p * len(dst))(*dst)
        a = timed(lambda: dev.call("msk_label_pyramid", C.c_void_p(src), n, d, h, w, len(extents), ext, ptrs))
        b = timed(lambda: dev.d2d(copy, src, out_bytes))
        lines.append(f"  {n}x{d}x{h}x{w} -> {' '.join('x'.join(map(str, e)) for e in extents)} ({out_bytes / 1e6:.2f} MB written)")
        lines.append(f"    msk_label_pyramid   {a[0]:.4f} [{a[1]:.4f} .. {a[2]:.4f}]")
        lines.append(f"    msk_d2d, same bytes {b[0]:.4f} [{b[1]:.4f} .. {b[2]:.4f}]")
        for p in [src, copy] + dst:
            dev.free(p)


def step_rows(dev, title, shape, batch, ncls, K, S, make_loss, steps, lines, profile):
    """-> True / False for the condition (DeepSup - native > the larger spread)"""
    from medicalseg_amd import models, optimizer as optim
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(0)
    x = to_tensor(rng.random((batch, 1) + shape, dtype=np.float32))
    y = to_tensor(rng.integers(0, ncls, (batch,) + shape).astype(np.int32))
    variants = {}
    for name, cls, kw in (("VNet", models.VNet, {}), ("VNetDeepSup", models.VNetDeepSup, {}),
                          ("VNetDeepSup(native_heads=True)", models.VNetDeepSup, {"native_heads": True})):
        model = cls(num_classes=ncls, kernel_size=K, stride_size=S, **kw)
        model.train()
        n_out = getattr(model, "num_outputs", 1)
        losses = {"types": [make_loss() for _ in range(n_out)], "coef": [1.0 / n_out] * n_out}
        opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        opt.enable_eager(model)                # as core.train() at one rank
        variants[name] = (model, losses, opt)

    def step(name):
        model, losses, opt = variants[name]
        ll, _ = loss_computation(model(x), y, losses)
        sum(ll).backward()
        opt.step()
        model.clear_gradients()

    times = {k: [] for k in variants}
    for rep in range(WARMUP_ROUNDS + REPEATS):
        for name in variants:
            dev.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(name)
            dev.sync()
            if rep >= WARMUP_ROUNDS:
                times[name].append((time.perf_counter() - t0) * 1e3 / steps)
    lines.append(f"[{title}: wall clock between two device syncs, ms per step; median [min .. max] of {REPEATS} repeats of {steps} "
                 f"steps, the three models alternate, {WARMUP_ROUNDS} warm-up rounds]")
    med = {}
    for name, t in times.items():
        med[name] = float(np.median(t))
        lines.append(f"  {name:34s} {med[name]:.3f} [{min(t):.3f} .. {max(t):.3f}]")
    up, nat, plain = "VNetDeepSup", "VNetDeepSup(native_heads=True)", "VNet"
    spread = max(max(times[up]) - min(times[up]), max(times[nat]) - min(times[nat]))
    gain = med[up] - med[nat]
    ok = gain > spread
    extra = med[up] - med[plain]
    lines.append(f"  deep supervision costs {extra:.3f} ms up-sampled and {med[nat] - med[plain]:.3f} ms native: native recovers "
                 f"{gain:.3f} ms = {100 * gain / extra if extra > 0 else float('nan'):.0f} % of it; the larger min-max spread is "
                 f"{spread:.3f} ms -> native faster by more than the spread: {'yes' if ok else 'NO'}")
    if profile:
        side = dev.get_option("wgrad_async")
        dev.set_option("wgrad_async", 0)       # one stream: a launch's HIP-event time is its own
        dev.prof_enable(True)
        prof = {}
        for name in (up, nat):
            step(name)
            dev.sync()
            dev.prof_reset()
            for _ in range(steps):
                step(name)
            dev.sync()
            prof[name] = dev.prof_report()
        dev.prof_enable(False)
        dev.set_option("wgrad_async", side)
        lines.append(f"  [per-launch HIP-event profile, one stream, ms per step: tags that differ by more than 0.005 ms between the two forms]")
        lines.append(f"    {'tag':44s} {'up-sampled':>18s} {'native':>18s}")
        tot = {up: 0.0, nat: 0.0}
        for tag in sorted(set(prof[up]) | set(prof[nat]), key=lambda t: -(prof[up].get(t, (0, 0))[1] - prof[nat].get(t, (0, 0))[1])):
            (ca, ma), (cb, mb) = prof[up].get(tag, (0, 0.0)), prof[nat].get(tag, (0, 0.0))
            tot[up] += ma / steps
            tot[nat] += mb / steps
            if abs(ma - mb) / steps > 0.005:
                lines.append(f"    {tag:44s} {ma / steps:9.3f} ({ca // steps:3d} calls) {mb / steps:9.3f} ({cb // steps:3d} calls)")
        lines.append(f"    {'all launches':44s} {tot[up]:9.3f}             {tot[nat]:9.3f}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="steps per repeat")
    ap.add_argument("--iters", type=int, default=50, help="pyramid calls per repeat")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="32x32x12 and 16^3 instead of the full shapes (a rehearsal of the tool itself)")
    args = ap.parse_args()
    from medicalseg_amd import models
    from medicalseg_amd.device import get_device
    dev = get_device()
    lines = [f"# deep supervision at the heads' own extents, {dev.name()}"]
    pyramid_rows(dev, args.iters, lines)
    mixed = lambda: models.MixedLoss([models.CrossEntropyLoss(), models.DiceLoss()], [1, 1])
    mri, patch = ((32, 32, 12), (16, 16, 16)) if args.small else ((512, 512, 12), (96, 96, 96))
    ok = step_rows(dev, "training step, 1x%dx%dx%d, 20 classes, MRI kernels and strides, MixedLoss[CrossEntropyLoss, DiceLoss] x outputs" % mri,
                   mri, 1, 20, MRI_K, MRI_S, mixed, args.steps, lines, profile=True)
    step_rows(dev, "training step, 2x%dx%dx%d, 3 classes, DiceCELoss x outputs (report only)" % patch,
              patch, 2, 3, ISO, ISO, models.DiceCELoss, args.steps, lines, profile=False)
    lines.append("condition (MRI shape): " + ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

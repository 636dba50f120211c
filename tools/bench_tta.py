"""Micro-benchmark of the test-time-augmentation kernels (medicalseg_amd/csrc/msk_tta.hip) and of core.infer.aug_inference.
python tools/bench_tta.py [--iters K] [--out FILE] [--no-net]

kernel rows, inputs resident in HBM, at 2 x 128^3 (C = 3) and 512 x 512 x 12 (C = 20), masks 0, 4 (W) and 7 (D, H, W):
  fused    one msk_tta_accumulate(first = 0): reads the logits and the accumulator, writes the accumulator (3 tensors)
  unfused  what it replaces: msk_softmax_c, msk_flip_axes (left out at mask 0), msk_copy_scale(accumulate) (up to 7 tensors)
  copy     the yardstick, a plain streaming copy of the same tensor: msk_copy_scale (2 tensors)
HIP-event ms, median [min, max] of 5 means of --iters calls, a 1 GiB buffer written before every call so that the operands
come from HBM.  GB/s = the tensors a row moves * the tensor's bytes / median.
call rows: wall ms (synchronised) of aug_inference(flip_axes = (0, 1, 2)), 8 passes, of an eval-mode VNet (3 classes) at
1 x 128^3 beside 8 plain inference() calls and one, best / median of --iters.  Every inference() call opens a
nn.fused_inference scope of its own (BatchNorm is folded into the weights 8 times); aug_inference opens one."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((2, 128, 128, 128), 3), ((1, 512, 512, 12), 20)]
MASKS = (0, 4, 7)
FLUSH_BYTES = 1 << 30
REPEATS = 5


def spread(means):
    means = sorted(means)
    return means[len(means) // 2], means[0], means[-1]


def time_events(dev, call, iters, flush):
    means = []
    for r in range(REPEATS):
        tot = 0.0
        for i in range(iters):
            dev.memset(flush, (r * iters + i) & 0xFF, FLUSH_BYTES)
            dev.timer_start()
            call()
            tot += dev.timer_stop()
        means.append(tot / iters)
    return spread(means)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-net", action="store_true", help="kernel rows only")
    args = ap.parse_args()
    from medicalseg_amd.device import Tensor, get_device, to_tensor
    dev = get_device()
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# test-time augmentation (msk_tta_accumulate / msk_flip_axes / msk_tta_finish), {dev.name()}")
    emit(f"# kernel rows: HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every "
         "call; GB/s = moved tensors * tensor bytes / median")
    flush = dev.malloc(FLUSH_BYTES)
    rng = np.random.default_rng(0)
    for (n, d, h, w), c in CASES:
        nbytes = n * d * h * w * c * 4
        emit(f"[{n}x{d}x{h}x{w}, C = {c}]  tensor = {nbytes / 1e6:.1f} MB")
        logits, acc, probs, mirrored = (Tensor.empty(dev, n, d, h, w, c, arena=False) for _ in range(4))
        chunk = (4.0 * rng.standard_normal(1 << 22)).astype(np.float32)          # 16 MiB of N(0, 4^2), repeated
        for off in range(0, nbytes, chunk.nbytes):
            dev.h2d(logits.ptr + off, chunk[: min(chunk.nbytes, nbytes - off) // 4])
        dev.memset(acc.ptr, 0, nbytes)

        def row(name, call, tensors, base=None):
            for _ in range(3):
                call()
            m = time_events(dev, call, args.iters, flush)
            rate = tensors * nbytes / (m[0] * 1e-3) / 1e9
            emit(f"  {name:24s} {m[0]:.4f} [{m[1]:.4f}, {m[2]:.4f}] ms  {tensors} tensors  {rate:6.0f} GB/s"
                 + (f"  ({base / m[0]:.2f} x faster than unfused)" if base else ""))
            return m[0]

        copy = row("copy (msk_copy_scale)", lambda: dev.call("msk_copy_scale", logits.msk(), None, probs.msk(), 0), 2)
        for mask in MASKS:
            def unfused(mask=mask):
                dev.call("msk_softmax_c", logits.msk(), probs.msk())
                src = probs
                if mask:
                    dev.call("msk_flip_axes", probs.msk(), mirrored.msk(), mask)
                    src = mirrored
                dev.call("msk_copy_scale", src.msk(), None, acc.msk(), 1)
            u = row(f"mask {mask} unfused", unfused, 7 if mask else 5)
            f = row(f"mask {mask} fused", lambda mask=mask: dev.call("msk_tta_accumulate", logits.msk(), mask, acc.msk(), 0), 3, u)
            emit(f"  mask {mask}: the fused pass takes {f / copy:.2f} x the copy's time for 1.5 x its bytes")
        pred = dev.malloc(n * d * h * w * 4)
        row("msk_tta_finish", lambda: dev.call("msk_tta_finish", acc.msk(), 8, probs.msk(), C.c_void_p(pred)), 2)
        row("msk_flip_axes mask 4", lambda: dev.call("msk_flip_axes", logits.msk(), mirrored.msk(), 4), 2)
        for p in (pred, logits.ptr, acc.ptr, probs.ptr, mirrored.ptr):
            dev.free(p)
    dev.free(flush)

    if not args.no_net:
        from medicalseg_amd.core import infer
        from medicalseg_amd.models import VNet
        model = VNet(num_classes=3)
        model.eval()
        x = to_tensor(rng.standard_normal((1, 1, 128, 128, 128)).astype(np.float32))

        def wall(call):
            call()
            dev.sync()
            ts = []
            for _ in range(args.iters):
                t0 = time.perf_counter()
                call()
                dev.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return ts[0], ts[len(ts) // 2]

        emit("[VNet, 3 classes, eval mode, 1x128x128x128]  wall ms, synchronised, best / median of %d" % args.iters)
        one = wall(lambda: infer.inference(model, x))
        eight = wall(lambda: [infer.inference(model, x) for _ in range(8)])
        aug = wall(lambda: infer.aug_inference(model, x, flip_axes=(0, 1, 2)))
        emit(f"  inference x 1                      {one[0]:.2f} / {one[1]:.2f}")
        emit(f"  inference x 8                      {eight[0]:.2f} / {eight[1]:.2f}")
        emit(f"  aug_inference, 8 flips             {aug[0]:.2f} / {aug[1]:.2f}   ({aug[1] - eight[1]:+.2f} ms median against 8 "
             "inference() calls, each of which opens its own fused scope and folds BatchNorm anew; aug_inference folds once)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

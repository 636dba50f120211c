"""Micro-benchmark of the gradient-clipping kernels (medicalseg_amd/csrc/msk_clip.hip: msk_grad_clip_coef,
msk_sgd_momentum_clip) beside their yardsticks, and of one VNet training step with the nnU-Net optimizer beside the plain one.
python tools/bench_clip.py [--iters K] [--steps S] [--size 128] [--out FILE]

kernel rows, for arenas of 45,607,944 floats (VNet's) and 1,048,576: HIP-event ms, median [min, max] of 5 means of --iters
calls, a 1 GiB buffer written before every call so that the operands come from HBM:
  read      the yardstick of the norm: a plain streaming read of the SAME buffer (msk_channel_sum over it as one channel)
  coef      msk_grad_clip_coef (chunk pass + finish pass); mark: at most 2 x read (msk_intensity_stats' own mark)
  sgd       the yardstick of the update: msk_sgd_momentum on the same three buffers
  sgd clip  msk_sgd_momentum_clip with a biting record and Nesterov; mark: no slower than sgd's median plus sgd's own
            max - min over its repeats
step rows: one VNet --size^3 batch-2 training step (bench.py's step), HIP-event ms per step over --steps steps, three rounds
alternating between plain Momentum with eager mode off, plain Momentum with eager mode on, and Momentum(momentum=0.99,
use_nesterov=True, grad_clip=ClipGradByGlobalNorm(12)), all three on one model."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [45607944, 1048576]
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


def kernels(dev, emit, iters):
    from medicalseg_amd._lib import MskTensor
    vp, sz, F = C.c_void_p, C.c_size_t, C.c_float
    flush = dev.malloc(FLUSH_BYTES)
    for n in SIZES:
        rng = np.random.default_rng(n)
        bufs = [dev.malloc(n * 4) for _ in range(3)]
        for b in bufs:
            dev.h2d(b, (rng.standard_normal(n) * 1e-2).astype(np.float32))
        p, g, v = bufs
        nbytes = sz(0)
        assert dev.lib.msk_grad_clip_workspace(sz(n), C.byref(nbytes)) == 0
        ws, rec, sums = dev.malloc(nbytes.value), dev.malloc(32), dev.malloc(64)
        emit(f"[{n} floats]  arena = {n * 4 / 1e6:.1f} MB, workspace = {nbytes.value / 1e3:.1f} KB")
        dev.call("msk_grad_clip_coef", vp(g), sz(n), F(1.0), F(1e9), vp(ws), vp(rec))
        norm = float(dev.d2h(rec, (4,), np.float64)[1])
        clip = norm / 3

        def coef():
            dev.call("msk_grad_clip_coef", vp(g), sz(n), F(1.0), F(clip), vp(ws), vp(rec))

        as_tensor = MskTensor(g, 1, 1, 1, n, 1, 1)
        rows = [("read (msk_channel_sum)", lambda: dev.call("msk_channel_sum", as_tensor, vp(sums), 0), 4),
                ("coef (msk_grad_clip_coef, 2 launches)", coef, 4),
                ("sgd (msk_sgd_momentum)", lambda: dev.call("msk_sgd_momentum", vp(p), vp(g), vp(v), sz(n), F(1e-3), F(0.9), F(1e-4),
                                                            F(1.0)), 20),
                ("sgd clip (biting record + Nesterov)", lambda: dev.call("msk_sgd_momentum_clip", vp(p), vp(g), vp(v), sz(n), F(1e-3),
                                                                         F(0.9), F(1e-4), F(1.0), 1, vp(rec), F(-np.inf), F(np.inf)), 20)]
        res = {}
        for name, call, bytes_per in rows:
            for _ in range(3):
                call()
            res[name] = timed(dev, call, iters, flush)
            emit(f"  {name:40s} {fmt(res[name])}  {n * bytes_per / (res[name][0] * 1e-3) / 1e9:6.0f} GB/s moved")
        rd, cf, sg, sc = (res[r[0]] for r in rows)
        emit(f"  coef / read = {cf[0] / rd[0]:.2f} (mark: <= 2): {'met' if cf[0] <= 2 * rd[0] else 'MISSED'}")
        bound = sg[0] + (sg[2] - sg[1])
        emit(f"  sgd clip {sc[0]:.4f} ms against sgd {sg[0]:.4f} + its spread {sg[2] - sg[1]:.4f} = {bound:.4f} ms: "
             f"{'met' if sc[0] <= bound else 'MISSED'}")
        emit(f"  record: coef = {float(dev.d2h(rec, (4,), np.float64)[2]):.6f} (clip_norm = norm / 3)")
        for ptr in bufs + [ws, rec, sums]:
            dev.free(ptr)
    dev.free(flush)


def steps(dev, emit, size, nsteps, warmup):
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation
    B, ncls = 2, 3
    ds = SyntheticCT(num_samples=B, shape=(size,) * 3, num_classes=ncls, seed=1234)
    items = [ds[i] for i in range(B)]
    images = to_tensor(np.stack([it[0] for it in items]), dev)
    labels = to_tensor(np.stack([it[1] for it in items]), dev)
    nn.seed(0)
    model = VNet(elu=False, in_channels=1, num_classes=ncls)
    model.train()
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    params = model.parameters()
    opts = [("plain Momentum, eager off", optim.Momentum(1e-3, parameters=params, momentum=0.9, weight_decay=1e-4), False),
            ("plain Momentum, eager on", optim.Momentum(1e-3, parameters=params, momentum=0.9, weight_decay=1e-4), True),
            ("nnU-Net: Nesterov 0.99 + global-norm clip 12", optim.Momentum(1e-3, parameters=params, momentum=0.99, weight_decay=3e-5,
                                                                           use_nesterov=True, grad_clip=optim.ClipGradByGlobalNorm(12)), False)]

    def run(opt, k):
        for _ in range(k):
            logits = model(images)
            loss_list, _ = loss_computation(logits, labels, losses)
            sum(loss_list).backward()
            opt.step()
            model.clear_gradients()

    emit(f"[VNet {size}^3, batch {B}]  HIP-event ms per step over {nsteps} steps, {warmup} untimed steps before each block")
    ms = {name: [] for name, _, _ in opts}
    for _ in range(3):
        for name, opt, eager in opts:
            for _, other, _ in opts:
                other.enable_eager(model, on=False)
            assert opt.enable_eager(model, on=eager) is eager
            run(opt, warmup)
            dev.sync()
            dev.timer_start()
            run(opt, nsteps)
            ms[name].append(dev.timer_stop() / nsteps)
    for name, _, _ in opts:
        emit(f"  {name:48s} " + " / ".join(f"{t:.3f}" for t in ms[name]) + f"   median {sorted(ms[name])[1]:.3f} ms")
    med = [sorted(ms[name])[1] for name, _, _ in opts]
    emit(f"  nnU-Net - plain (eager off) = {med[2] - med[0]:+.3f} ms;  plain eager off - eager on = {med[0] - med[1]:+.3f} ms;  "
         f"last norm {opts[2][1].grad_norm():.4g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--no-step", action="store_true", help="kernel rows only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from medicalseg_amd.device import get_device
    dev = get_device()
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit(f"# gradient clipping (msk_grad_clip_coef / msk_sgd_momentum_clip), {dev.name()}")
    emit(f"# kernels: HIP-event ms, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB written before every call")
    kernels(dev, emit, args.iters)
    if not args.no_step:
        steps(dev, emit, args.size, args.steps, args.warmup)
    emit("# not measured: msk_adam_clip, the value clamp, more than one rank")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Micro-benchmark of the boundary-loss kernels (medicalseg_amd/csrc/msk_loss_boundary.hip) beside the yardsticks of the same run:
msk_region_loss_fwd / msk_region_loss_bwd with the DiceCELoss defaults on the same buffers, and for msk_label_sdf the sum of its
2 N |S| msk_edt3d calls on the same masks plus msk_d2d of one float64 volume.
python tools/bench_boundary.py [--iters K] [--out FILE] [--no-step]

Every timed call is bracketed by a HIP event pair and preceded by a write of a 1 GiB buffer (four times the last-level cache),
so its operands come from HBM as they do inside a training step.  A row is repeated five times; a repeat is the mean of --iters
calls; the table gives the median, the minimum and the maximum of the five.

Marks.  Forward: median <= region fwd median x (4C + 4 + 4|S|) / (4C + 4) + (region fwd max - min): the ratio of algorithmic bytes
per voxel (logits, label and |S| map values) plus the yardstick's spread.  Backward: median <= region bwd median x
(8C + 4 + 4|S|) / (8C + 4) + (region bwd max - min).  msk_label_sdf: median <= the msk_edt3d sum's median + its max - min +
N |S| x 2 x 1.5 x the msk_d2d median: the mask and compose passes budgeted as 32 bytes per voxel, two copies of one float64
volume, with the project's factor 1.5 for a streaming pass.
Without a mark: the two transforms apart (features {== c} and {!= c}), and one VNet 96^3 batch-2 training step with DiceCELoss and
with DiceBoundaryLoss, alternating on one model.

Labels: ellipsoids of the classes on background 0 and a slab of 255 along one face (a padded patch); the time of the transforms
depends on them, the searches run as far as the nearest feature along a line."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, D, H, W), C, the class set
SHAPES = [((2, 96, 96, 96), 3, (1, 2)), ((2, 128, 128, 128), 3, (1, 2)), ((1, 512, 512, 12), 20, (1, 2, 3)),
          ((1, 512, 512, 12), 20, tuple(range(1, 20)))]
FLUSH_BYTES = 1 << 30
REPEATS = 5


def blobs(shape, classes, seed):
    """[D, H, W] int32: one ellipsoid per class on background 0, a slab of 255 along the low-y face"""
    D, H, W = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    lab = np.zeros(shape, np.int32)
    for c in classes:
        cz, cy, cx = rng.uniform(0.2, 0.8, 3) * (D, H, W)
        rz, ry, rx = rng.uniform(0.08, 0.25, 3) * (D, H, W) + 1.0
        lab[((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1.0] = c
    lab[:, :max(H // 16, 1), :] = 255
    return lab


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

    def timed(fn, iters=None):
        """median, min, max over REPEATS of the mean HIP-event time of `iters` calls, each behind a 1 GiB write"""
        iters = iters or args.iters
        for _ in range(2):
            fn()
        reps = []
        for _ in range(REPEATS):
            tot = 0.0
            for _ in range(iters):
                dev.memset(flush, it_byte[0] & 0xFF, FLUSH_BYTES)
                it_byte[0] += 1
                dev.timer_start()
                fn()
                tot += dev.timer_stop()
            reps.append(tot / iters)
        return float(np.median(reps)), min(reps), max(reps)

    lines = [f"# boundary-loss kernels, {dev.name()}: HIP-event time per call in ms, operands from HBM (1 GiB written before every call);",
             f"# median [min .. max] of {REPEATS} repeats, a repeat = the mean of {args.iters} calls (the transforms: of {max(args.iters // 3, 1)}).",
             "# forward mark: region fwd median x (4C+4+4|S|)/(4C+4) + (its max - min).",
             "# backward mark: region bwd median x (8C+4+4|S|)/(8C+4) + (its max - min).",
             "# msk_label_sdf mark: the sum of its 2 N |S| msk_edt3d calls (median + max - min) + N |S| x 2 x 1.5 x msk_d2d of one float64 volume."]
    misses = []
    for (n, d, h, w), c, S in SHAPES:
        V = d * h * w
        vox = n * V
        ns = len(S)
        mask = sum(1 << k for k in S)
        rng = np.random.default_rng(0)
        z = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dz = Tensor(dev, dev.malloc(vox * c * 4), n, d, h, w, c, c, None)
        dev.h2d(z.ptr, (rng.standard_normal(vox * c) * 2).astype(np.float32))
        dev.memset(dz.ptr, 0, vox * c * 4)
        y = np.stack([blobs((d, h, w), range(1, c), 7 + s) for s in range(n)])
        yp = dev.malloc(y.nbytes)
        dev.h2d(yp, y)
        # the complements as 0 / 1 volumes of their own: the yardstick's msk_edt3d calls run on the same masks
        neg = {}
        for s in range(n):
            for k in S:
                p = dev.malloc(V * 4)
                dev.h2d(p, (y[s] != k).astype(np.int32))
                neg[s, k] = p
        out, stats = dev.small(2 + c), dev.small(2 * (5 * n * c + 2))          # dev.small counts floats
        b_out, b_stats = dev.small(2 + c), dev.small(2 * (3 + c))
        nbytes = C.c_size_t(0)
        assert dev.lib.msk_sdf_workspace(d, h, w, C.byref(nbytes)) == 0
        ws, phi = dev.malloc(nbytes.value), dev.malloc(n * ns * V * 4)
        f64a, f64b = dev.malloc(V * 8), dev.malloc(V * 8)
        lg, lb = vox * c * 4, vox * 4

        rs = (255, 0, 0, 1, 0, 0, f(1e-5), f(0.0), f(0.0), 1, f(0.0))
        r_fwd = lambda: dev.call("msk_region_loss_fwd", z.msk(), vp(yp), *rs, None, vp(out), vp(stats))
        r_bwd = lambda: dev.call("msk_region_loss_bwd", z.msk(), vp(yp), *rs, None, vp(stats), f(1.0), f(1.0), 0, dz.msk())
        sdf = lambda: dev.call("msk_label_sdf", vp(yp), n, d, h, w, C.c_uint64(mask), None, vp(ws), C.c_size_t(nbytes.value), vp(phi))
        b_fwd = lambda: dev.call("msk_boundary_loss_fwd", z.msk(), vp(yp), 255, C.c_uint64(mask), vp(phi), vp(b_out), vp(b_stats))
        b_bwd = lambda acc=0: dev.call("msk_boundary_loss_bwd", z.msk(), vp(yp), 255, C.c_uint64(mask), vp(phi), vp(b_stats), f(1.0), acc,
                                       dz.msk())

        def edt_pos():
            for s in range(n):
                for k in S:
                    dev.call("msk_edt3d", vp(yp + s * V * 4), d, h, w, k, 0, None, vp(f64a))

        def edt_neg():
            for s in range(n):
                for k in S:
                    dev.call("msk_edt3d", vp(neg[s, k]), d, h, w, 1, 0, None, vp(f64b))

        def edt_both():
            edt_pos()
            edt_neg()

        lines.append(f"[{n}x{d}x{h}x{w}, C = {c}, |S| = {ns}]  logits {lg / 1e6:.1f} MB, labels {lb / 1e6:.1f} MB, maps {ns * lb / 1e6:.1f} MB")

        def row(name, fn, nb, limit=None, iters=None):
            med, lo, hi = timed(fn, iters)
            text = f"  {name:58s} {med:.4f} [{lo:.4f} .. {hi:.4f}]  {nb / (med * 1e-3) / 1e9:5.0f} GB/s"
            if limit is not None:
                ok = med <= limit
                text += f"   mark <= {limit:.4f}: {'met' if ok else 'MISSED'}"
                if not ok:
                    misses.append(f"{n}x{d}x{h}x{w} C={c} |S|={ns} {name.strip()}: {med:.4f} ms > {limit:.4f} ms")
            lines.append(text)
            return med, lo, hi

        slow = max(args.iters // 3, 1)
        y_fwd = row("region fwd, DiceCELoss defaults  [yardstick]", r_fwd, lg + lb)
        r_fwd()
        y_bwd = row("region bwd, DiceCELoss defaults  [yardstick]", r_bwd, 2 * lg + lb)
        sdf()
        row("boundary fwd", b_fwd, lg + lb + ns * lb, y_fwd[0] * (4 * c + 4 + 4 * ns) / (4 * c + 4) + (y_fwd[2] - y_fwd[1]))
        b_fwd()
        row("boundary bwd, writes dz", b_bwd, 2 * lg + lb + ns * lb, y_bwd[0] * (8 * c + 4 + 4 * ns) / (8 * c + 4) + (y_bwd[2] - y_bwd[1]))
        row("boundary bwd, adds into dz (no mark)", lambda: b_bwd(1), 3 * lg + lb + ns * lb)
        cp = row("msk_d2d of one float64 volume", lambda: dev.d2d(f64b, f64a, V * 8), 16 * V)
        row(f"  {n * ns} x msk_edt3d, features == c (no mark)", edt_pos, n * ns * 12 * V, iters=slow)
        row(f"  {n * ns} x msk_edt3d, features != c (no mark)", edt_neg, n * ns * 12 * V, iters=slow)
        y_edt = row(f"{2 * n * ns} x msk_edt3d on the same masks  [yardstick]", edt_both, 2 * n * ns * 12 * V, iters=slow)
        row(f"msk_label_sdf ({7 * n * ns} launches)", sdf, n * ns * (2 * 12 + 24) * V,
            y_edt[0] + (y_edt[2] - y_edt[1]) + n * ns * 2 * 1.5 * cp[0], iters=slow)
        for p in [z.ptr, dz.ptr, yp, ws, phi, f64a, f64b] + list(neg.values()):
            dev.free(p)
    dev.free(flush)

    if not args.no_step:
        from medicalseg_amd import optimizer as optim
        from medicalseg_amd.device import to_tensor
        from medicalseg_amd.models import DiceBoundaryLoss, DiceCELoss, VNet
        from medicalseg_amd.utils import loss_computation
        rng = np.random.default_rng(1)
        model = VNet(num_classes=3)
        model.train()
        opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        x = to_tensor(rng.standard_normal((2, 1, 96, 96, 96)).astype(np.float32))
        yt = to_tensor(np.stack([blobs((96, 96, 96), (1, 2), 3 + s) for s in range(2)]))
        recipes = {"DiceCELoss": {"types": [DiceCELoss()], "coef": [1]}, "DiceBoundaryLoss": {"types": [DiceBoundaryLoss()], "coef": [1]}}
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

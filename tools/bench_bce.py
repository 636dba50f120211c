"""Micro-benchmark of the BCELoss kernels (medicalseg_amd/csrc/msk_loss_bce.hip): HIP-event time per kernel after a warm-up
and GB/s on the algorithmic bytes, beside the CE + Dice kernels on the same logits, and the round-6 CE + Dice times of the
bench step.  python tools/bench_bce.py [--iters K] [--out FILE]

Each kernel is timed twice.  'warm' runs the launches back to back: inputs up to the 256 MB last-level cache (MALL) stay
resident from one launch to the next (the 2 x 128^3 logits are 50 MB).  'cold' writes a 1 GiB buffer before every launch,
so the inputs come from HBM as they do inside a training step.  Compare rows of the same kind with each other."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((2, 128, 128, 128), 3), ((1, 512, 512, 12), 20)]   # (N, D, H, W), C: the bench shape, the 20-class MRI head
FLUSH_BYTES = 1 << 30   # written before every 'cold' launch: four times the last-level cache
R06 = os.path.join(ROOT, "profiles", "r06_bench_hip_events_serial_shapes.tsv")


def r06_loss_rows():
    rows = []
    if os.path.exists(R06):
        for line in open(R06):
            if line.split("\t")[0] in ("loss_fwd_stats", "loss_fwd_final", "loss_bwd"):
                tag, calls, total, avg = line.split("\t")[:4]
                rows.append(f"  r06 {tag:16s} {float(avg):.4f} ms  (bench step, 2x128^3, C = 3; {calls} calls)")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from medicalseg_amd.device import Tensor, get_device
    dev = get_device()
    vp = lambda p: C.c_void_p(p) if p else None
    lines = [f"# BCELoss kernels, {dev.name()}: HIP-event time per launch (mean of {args.iters} after 5 warm-up rounds), "
             "GB/s = algorithmic bytes / time",
             "# warm = launches back to back (inputs <= 256 MB stay in the last-level cache between launches: the 2x128^3 logits "
             "are 50 MB); cold = a 1 GiB buffer written before every launch (inputs from HBM, as in a training step).",
             "# The r06 rows are in-step times (cold-like); compare them with the cold rows, and warm rows with warm rows."]
    flush, it_byte = dev.malloc(FLUSH_BYTES), [1]
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
        # separate, exactly sized outputs per entry point: msk_bce_fwd writes 1 float + 8 doubles, msk_loss_fwd_ex 2 + C floats
        # + 3 C + 2 doubles (include/msegk.h); dev.small counts floats
        out, stats = dev.small(2 + c), dev.small(2 * 8)
        ce_out, ce_stats = dev.small(2 + c), dev.small(2 * (3 * c + 2))
        wts = dev.small(c)
        dev.h2d(wts, np.ones(c, np.float32))
        lg, lb = vox * c * 4, vox * 4                       # bytes of the logits, of the labels
        cases = [
            ("bce fwd (dynamic weight + pos_weight)", {"bce_fwd": lg + lb},
             lambda: dev.call("msk_bce_fwd", z.msk(), vp(yp), 255, 1, 2, C.c_float(0.0), vp(out), vp(stats))),
            ("bce fwd (no weights)", {"bce_fwd": lg + lb},
             lambda: dev.call("msk_bce_fwd", z.msk(), vp(yp), 255, 0, 0, C.c_float(0.0), vp(out), vp(stats))),
            ("bce bwd (write)", {"bce_bwd": 2 * lg + lb},
             lambda: dev.call("msk_bce_bwd", z.msk(), vp(yp), 255, vp(stats), C.c_float(1.0), 0, dz.msk())),
            ("bce bwd (accumulate)", {"bce_bwd": 3 * lg + lb},
             lambda: dev.call("msk_bce_bwd", z.msk(), vp(yp), 255, vp(stats), C.c_float(1.0), 1, dz.msk())),
            ("ce+dice fwd", {"loss_fwd_stats": lg + lb},
             lambda: dev.call("msk_loss_fwd_ex", z.msk(), vp(yp), vp(wts), 255, 0, None, vp(ce_out), vp(ce_stats))),
            ("ce+dice bwd", {"loss_bwd": 2 * lg + lb},
             lambda: dev.call("msk_loss_bwd_ex", z.msk(), vp(yp), vp(wts), 255, 0, None, vp(ce_stats), C.c_float(1.0),
                              C.c_float(1.0), dz.msk())),
        ]
        lines.append(f"[{n}x{d}x{h}x{w}, C = {c}]  logits {lg / 1e6:.1f} MB, labels {lb / 1e6:.1f} MB")
        for name, traffic, fn in cases:
            if name.startswith("ce+dice bwd"):   # its stats come from its own forward
                dev.call("msk_loss_fwd_ex", z.msk(), vp(yp), vp(wts), 255, 0, None, vp(ce_out), vp(ce_stats))
            if name.startswith("bce bwd"):
                dev.call("msk_bce_fwd", z.msk(), vp(yp), 255, 1, 2, C.c_float(0.0), vp(out), vp(stats))
            for _ in range(5):
                fn()
            res = {}
            for mode in ("warm", "cold"):
                dev.sync()
                dev.prof_reset()
                dev.prof_enable(True)
                for _ in range(args.iters):
                    if mode == "cold":
                        dev.memset(flush, it_byte[0] & 0xFF, FLUSH_BYTES)   # (not a timed launch: no profile tag)
                        it_byte[0] += 1
                    fn()
                dev.sync()
                res[mode] = dev.prof_report()
                dev.prof_enable(False)
            totals = {"warm": 0.0, "cold": 0.0}
            for tag in sorted(res["warm"]):
                row = f"  {name:38s} {tag:16s}"
                for mode in ("warm", "cold"):
                    calls, ms = res[mode][tag]
                    avg = ms / max(calls, 1)
                    totals[mode] += avg
                    gbs = f"{traffic[tag] / (avg * 1e-3) / 1e9:5.0f} GB/s" if tag in traffic else " " * 10
                    row += f"  {mode} {avg:.4f} ms {gbs}"
                lines.append(row.rstrip())
            lines.append(f"  {name:38s} {'(all kernels)':16s}  warm {totals['warm']:.4f} ms            "
                         f"cold {totals['cold']:.4f} ms")
        if c == 3:
            lines.extend(r06_loss_rows())
        for p in (z.ptr, dz.ptr, yp):
            dev.free(p)
    dev.free(flush)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

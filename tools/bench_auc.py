"""Micro-benchmark of the device AUC (medicalseg_amd/csrc/msk_auc.hip through utils.metric.AucScores) beside the host path
it replaces (device -> host copy of the probabilities of every volume, then utils.metric.auc_roc on numpy).
python tools/bench_auc.py [--iters K] [--cases 0,1,...] [--out FILE]

Cases: 128^3 with C = 2 and C = 3, 1 and 20 volumes; 512 x 512 x 12 with C = 20 (the MRI head), 1 and 10 volumes.
Scores: 'saturated' (msk_softmax_c of N(0, 12^2) logits: many exact 0.0 / 1.0) and 'uniform' (uniform float32 scores).

device rows, per evaluation of the whole set, after 3 warm-up rounds; every figure is the mean of --iters rounds, taken 5
times: median [min, max] of those 5 means.  A round packs every volume again (a sorted buffer scatters differently from a
fresh one) and calls counts().
  pack / sort per pass / count: HIP-event time of the launches (the library's per-tag profile); sort per pass = the
    histogram, scan and scatter launches of one of the four digit passes;
  counts(): wall time of AucScores.counts(): workspace allocation, sort, count, the download of 3 C + 2 words, the free.
host rows: wall time of the D2H copies (Tensor.numpy() per volume, as evaluate(auc_roc=True) does) and of
  np.concatenate + utils.metric.auc_roc, best of 2 (one run where a run takes more than --host-once seconds); the float
  is compared with the device's.
yardstick: the sort moves 12 bytes per key per pass algorithmically (keys read by the histogram, read and written by the
  scatter), 48 bytes per key in all; that traffic over the measured sort time stands beside msk_minmax_norm (a plain
  streaming kernel of this library, 4 bytes read + 4 written per element) over the same number of bytes (at most
  --yardstick-max), timed in the same process."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((128, 128, 128), 2, 1), ((128, 128, 128), 2, 20), ((128, 128, 128), 3, 1), ((128, 128, 128), 3, 20),
         ((512, 512, 12), 20, 1), ((512, 512, 12), 20, 10)]
REPEATS = 5
TAGS = ("auc_pack", "auc_hist", "auc_scan", "auc_scatter", "auc_count")


def volume(dev, shape, ncls, kind, seed):
    """one volume of scores on the device (owned Tensor) and its label (owned IntTensor)"""
    from medicalseg_amd.device import IntTensor, Tensor
    rng = np.random.default_rng(seed)
    V = int(np.prod(shape))
    probs = Tensor.empty(dev, 1, shape[0], shape[1], shape[2], ncls, arena=False)
    if kind == "saturated":
        x = rng.standard_normal((V, ncls), dtype=np.float32) * np.float32(12.0)
        tmp = dev.malloc(x.nbytes)
        dev.h2d(tmp, x)
        dev.call("msk_softmax_c", Tensor(dev, tmp, 1, shape[0], shape[1], shape[2], ncls).msk(), probs.msk())
        dev.free(tmp)
    else:
        dev.h2d(probs.ptr, rng.random((V, ncls), dtype=np.float32))
    lab = rng.integers(0, ncls, (1, 1) + tuple(shape), dtype=np.int32)
    lp = dev.malloc(lab.nbytes)
    dev.h2d(lp, lab)
    return probs, IntTensor(dev, lp, lab.shape), lab


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def fmt(s):
    return f"{s[0]:.3f} [{s[1]:.3f}, {s[2]:.3f}] ms"


def timed(dev, call, iters):
    means = []
    for _ in range(REPEATS):
        tot = 0.0
        for _ in range(iters):
            dev.timer_start()
            call()
            tot += dev.timer_stop()
        means.append(tot / iters)
    return stats(means)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    ap.add_argument("--host-once", type=float, default=20.0)
    ap.add_argument("--yardstick-max", type=float, default=float(4 << 30))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from medicalseg_amd.device import get_device
    from medicalseg_amd.utils import metric
    dev = get_device()
    lines = [f"# device AUC (msk_auc_pack / msk_auc_counts), {dev.name()}, host CPU: {os.cpu_count()} logical CPUs visible",
             f"# device: ms per evaluation of the whole set, median [min, max] of {REPEATS} means of {args.iters} rounds; a round "
             "packs every volume and calls counts()",
             "# host: wall ms of Tensor.numpy() per volume + np.concatenate + utils.metric.auc_roc on numpy"]

    out = open(args.out, "w") if args.out else None

    def emit(s):
        print(s, flush=True)
        if out:               # line by line: a run that is cut short keeps what it measured
            out.write(s + "\n")
            out.flush()

    for s in lines:
        emit(s)
    vp = C.c_void_p
    for ci in (int(c) for c in args.cases.split(",")):
        shape, ncls, nvol = CASES[ci]
        V = int(np.prod(shape))
        keys = V * nvol * ncls
        emit(f"[{shape[0]}x{shape[1]}x{shape[2]}, C = {ncls}, {nvol} volume{'s' if nvol > 1 else ''}]  {keys / 1e6:.1f} M scores, "
             f"{keys * 4 / 1e6:.0f} MB of probabilities")
        for kind in ("saturated", "uniform"):
            vols = [volume(dev, shape, ncls, kind, 100 * ci + v) for v in range(nvol)]
            acc = metric.AucScores(dev, ncls, V * nvol)

            def round_(record=None):
                acc.fill = 0
                for probs, lt, _ in vols:
                    acc.add(probs, lt)
                dev.sync()
                t0 = time.perf_counter()
                c = acc.counts()
                if record is not None:
                    record.append((time.perf_counter() - t0) * 1e3)
                return c

            for _ in range(3):
                counts = round_()
            per_tag = {t: [] for t in TAGS}
            walls = []
            dev.prof_enable(True)
            for _ in range(REPEATS):
                dev.prof_reset()
                rec = []
                for _ in range(args.iters):
                    round_(rec)
                rep = dev.prof_report()
                for t in TAGS:
                    per_tag[t].append(rep.get(t, (0, 0.0))[1] / args.iters)
                walls.append(sum(rec) / args.iters)
            dev.prof_enable(False)
            sort_ms = [(h + s + c) for h, s, c in zip(per_tag["auc_hist"], per_tag["auc_scan"], per_tag["auc_scatter"])]
            dev_auc = metric.auc_from_counts(counts, ncls)
            wall = stats(walls)
            emit(f"  {kind:9s} device  pack {fmt(stats(per_tag['auc_pack']))}   sort per pass {fmt(stats([x / 4 for x in sort_ms]))}"
                 f" (hist {stats(per_tag['auc_hist'])[0] / 4:.3f} + scan {stats(per_tag['auc_scan'])[0] / 4:.3f} + scatter "
                 f"{stats(per_tag['auc_scatter'])[0] / 4:.3f})   count {fmt(stats(per_tag['auc_count']))}   counts() {fmt(wall)}")
            sort_med = stats(sort_ms)[0]
            traffic = 48.0 * keys
            emit(f"  {kind:9s} sort    {traffic / 1e6:.0f} MB algorithmic traffic / {sort_med:.3f} ms = "
                 f"{traffic / (sort_med * 1e-3) / 1e9:.0f} GB/s")
            # host path
            d2h, host, host_auc = [], [], None
            for rep_i in range(2):
                t0 = time.perf_counter()
                hp = [probs.numpy() for probs, _, _ in vols]
                t1 = time.perf_counter()
                host_auc = metric.auc_roc(np.concatenate(hp), np.concatenate([lab for _, _, lab in vols]), num_classes=ncls)
                t2 = time.perf_counter()
                d2h.append((t1 - t0) * 1e3)
                host.append((t2 - t1) * 1e3)
                del hp
                if t2 - t0 > args.host_once:
                    break
            total = min(a + b for a, b in zip(d2h, host))
            emit(f"  {kind:9s} host    d2h {min(d2h):.1f} ms + numpy {min(host):.1f} ms = {total:.1f} ms ({len(host)} run"
                 f"{'s' if len(host) > 1 else ''})   {total / wall[0]:.0f} x the device counts(), "
                 f"{total / (wall[0] + stats(per_tag['auc_pack'])[0]):.0f} x pack + counts()   auc device {dev_auc:.17g} host "
                 f"{host_auc:.17g} equal: {dev_auc == host_auc}")
            acc.free()
            for probs, lt, _ in vols:
                dev.free(probs.ptr)
                dev.free(lt.ptr)
            # yardstick over the same number of bytes
            elems = int(min(traffic, args.yardstick_max) // 8)
            src, dst = dev.malloc(elems * 4), dev.malloc(elems * 4)
            dev.memset(src, 0, elems * 4)
            call = lambda: dev.call("msk_minmax_norm", vp(src), vp(dst), C.c_size_t(elems), 1, C.c_float(0.0), C.c_float(1.0))
            for _ in range(3):
                call()
            y = timed(dev, call, max(args.iters, 5))
            emit(f"  {kind:9s} yardstick msk_minmax_norm over {elems * 8 / 1e6:.0f} MB read + written: {fmt(y)}  "
                 f"{elems * 8 / (y[0] * 1e-3) / 1e9:.0f} GB/s")
            dev.free(src)
            dev.free(dst)
    if out:
        out.close()


if __name__ == "__main__":
    main()

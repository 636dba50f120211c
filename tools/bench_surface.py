"""Micro-benchmark of the exact distance transform and the surface-distance metrics (medicalseg_amd/csrc/msk_edt.hip:
msk_edt3d, msk_surface_count, msk_surface_gather through utils.metric) beside the host path they replace (device ->
host copy of prediction and label, then scipy.ndimage.binary_erosion + distance_transform_edt per class and direction).
python tools/bench_surface.py [--iters K] [--out FILE] [--no-huge]

Sizes: 128^3 (C = 2), 12 x 512 x 512 (C = 20, all 19 foreground classes) and 300 x 512 x 512 (C = 2; no host row: the
host path takes minutes there).  Inputs, resident in HBM: 'blobs' (ellipsoids of every foreground class; the prediction
is another draw that overlaps the label's partly) and 'noise' (independent 50 % noise in prediction and label, class 1).

pass rows: the three launches of msk_edt3d (features = the surface of a class of the label) timed separately by the
library's per-kernel profile (HIP events around every launch): one call per timed class (blobs: every foreground class,
so the row is the mean launch over all of them; noise: class 1), --iters rounds after 3 warm-up rounds, a 1 GiB buffer
written before every round so that the volume comes from HBM; median and [min, max] of 5 such means.  GB/s = the bytes
a pass moves when every line holds a feature (x: 4 read + 8 written per voxel; y, z: 8 read + 8 written) over the
median.  A y or z pass skips the lines without a feature and stores only the values that changed, so on blobs, where a
class fills a small part of the volume, it moves fewer bytes and the figure overstates its traffic: the row says which
share of the y pass's lines (the (z, x) columns) holds a feature.  The noise rows are the dense case (every line).
yardstick rows: msk_minmax_norm (a plain streaming kernel of this library) over 2 * voxels floats = the 16 bytes per
voxel of a y or z pass, timed the same way in the same process.
call rows: wall time of utils.metric.surface_metrics(pred, label, C) on device inputs, download and host sort / sqrt /
percentile included, best and median of --iters calls; next to it the time of the same call on the downloaded arrays
through scipy (d2h + erosion + two distance transforms per class), once, and whether the floats agree."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((128, 128, 128), 2, True), ((12, 512, 512), 20, True), ((300, 512, 512), 2, False)]
FLUSH_BYTES = 1 << 30
REPEATS = 5
PASSES = ("edt_x", "edt_y", "edt_z")
PASS_BYTES = {"edt_x": 12, "edt_y": 16, "edt_z": 16}


def blob_pair(shape, ncls, seed):
    """(pred, label) int32: per foreground class two ellipsoids in the label and a partly overlapping draw in the
    prediction, built slab-wise so that 300 x 512 x 512 needs no float64 grid of the whole volume"""
    rng = np.random.default_rng(seed)
    label, pred = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    ax = [np.arange(s, dtype=np.float32) for s in shape]
    for c in range(1, ncls):
        for k in range(2):
            ctr = [rng.uniform(0.1 * s, 0.9 * s) for s in shape]
            rad = [max(1.5, s * (0.012 / ncls) ** (1 / 3.0) * rng.uniform(0.7, 1.2)) for s in shape]
            for arr, shift in ((label, 0.0), (pred, rng.uniform(-0.4, 0.4))):
                q = [((ax[a] - ctr[a] - shift * rad[a]) / rad[a]) ** 2 for a in range(3)]
                arr[(q[0][:, None, None] + q[1][None, :, None] + q[2][None, None, :]) <= 1.0] = c
    return pred, label


def noise_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) < 0.5).astype(np.int32), (rng.random(shape, dtype=np.float32) < 0.5).astype(np.int32)


def spread(means):
    means = sorted(means)
    return means[len(means) // 2], means[0], means[-1]


def time_passes(dev, call, iters, flush):
    """{tag: (median, min, max)} of REPEATS means of `iters` profiled calls, in ms"""
    per = {p: [] for p in PASSES}
    for r in range(REPEATS):
        dev.prof_reset()
        dev.prof_enable(True)
        for i in range(iters):
            dev.memset(flush, (r * iters + i) & 0xFF, FLUSH_BYTES)
            call()
        dev.sync()
        rep = dev.prof_report()
        dev.prof_enable(False)
        for p in PASSES:
            calls, ms = rep.get(p, (0, 0.0))
            per[p].append(ms / calls if calls else 0.0)
    return {p: spread(v) for p, v in per.items()}


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


def host_metrics(dev, pv, lv, ncls):
    """the path the feature replaces: download both volumes, then per class erosion and two distance transforms"""
    from scipy import ndimage
    t0 = time.perf_counter()
    pred, label = pv.numpy(), lv.numpy()
    t1 = time.perf_counter()
    res = {k: np.full(ncls - 1, np.nan) for k in ("hd", "hd95", "assd")}
    for c in range(1, ncls):
        P, L = pred == c, label == c
        P, L = P & ~ndimage.binary_erosion(P), L & ~ndimage.binary_erosion(L)
        if not P.any() or not L.any():
            continue
        d_pl = np.sort(ndimage.distance_transform_edt(~L)[P])
        d_lp = np.sort(ndimage.distance_transform_edt(~P)[L])
        res["hd"][c - 1] = max(d_pl[-1], d_lp[-1])
        res["hd95"][c - 1] = np.percentile(np.concatenate([d_pl, d_lp]), 95)
        res["assd"][c - 1] = (np.mean(d_pl) + np.mean(d_lp)) / 2
    t2 = time.perf_counter()
    return res, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-huge", action="store_true", help="leave out 300 x 512 x 512")
    args = ap.parse_args()
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.device import get_device
    from medicalseg_amd.utils import metric
    dev = get_device()
    lines = [f"# surface distances (msk_edt3d / msk_surface_count / msk_surface_gather), {dev.name()}, host CPU: "
             f"{os.cpu_count()} logical CPUs visible",
             f"# passes, yardstick: HIP-event ms per launch, median [min, max] of {REPEATS} means of {args.iters} calls, 1 GiB "
             "written before every call; GB/s = algorithmic bytes / median",
             f"# call: wall ms of utils.metric.surface_metrics on device inputs (download included), best / median of {args.iters}; "
             "host: d2h + scipy erosion and distance transforms, once"]
    flush = dev.malloc(FLUSH_BYTES)
    vp = C.c_void_p

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for s in lines:
        print(s, flush=True)
    for shape, ncls, with_host in CASES:
        if args.no_huge and not with_host:
            continue
        vox = int(np.prod(shape))
        d, h, w = shape
        emit(f"[{d}x{h}x{w}, C = {ncls}]  {vox / 1e6:.1f} M voxels")
        src, dst = dev.malloc(vox * 8), dev.malloc(vox * 8)
        dev.memset(src, 0, vox * 8)
        stream = lambda: dev.call("msk_minmax_norm", vp(src), vp(dst), C.c_size_t(2 * vox), 1, C.c_float(0.0), C.c_float(1.0))
        for _ in range(3):
            stream()
        y = time_events(dev, stream, args.iters, flush)
        emit(f"  yardstick msk_minmax_norm, {16 * vox / 1e6:.1f} MB read + written: {y[0]:.4f} [{y[1]:.4f}, {y[2]:.4f}] ms  "
             f"{16 * vox / (y[0] * 1e-3) / 1e9:6.0f} GB/s")
        dev.free(src)
        dev.free(dst)
        for kind in ("blobs", "noise"):
            pred, label = blob_pair(shape, ncls, 7) if kind == "blobs" else noise_pair(shape, 7)
            classes = list(range(1, ncls)) if kind == "blobs" else [1]
            pv, lv = pp.upload(pred), pp.upload(label)
            dist = dev.malloc(vox * 8)
            edt = lambda: [dev.call("msk_edt3d", vp(lv.ptr), d, h, w, c, 1, None, vp(dist)) for c in classes]
            share = float(np.mean([(label == c).any(axis=1).mean() for c in classes]))
            for _ in range(3):
                edt()
            t = time_passes(dev, edt, args.iters, flush)
            dev.free(dist)
            del pred, label
            emit(f"  {kind:5s} passes: mean launch over {len(classes)} class(es); {100 * share:.1f} % of the y pass's lines hold a feature")
            for p in PASSES:
                m = t[p]
                rate = PASS_BYTES[p] * vox / (m[0] * 1e-3) / 1e9 if m[0] > 0 else float("nan")
                emit(f"  {kind:5s} {p}  {m[0]:.4f} [{m[1]:.4f}, {m[2]:.4f}] ms  {rate:6.0f} GB/s of {PASS_BYTES[p]} B/voxel"
                     f"  ({rate / (16 * vox / (y[0] * 1e-3) / 1e9):.2f} of the yardstick's rate)")
            total = sum(t[p][0] for p in PASSES)
            emit(f"  {kind:5s} msk_edt3d = {total:.4f} ms for the three launches")
            run = lambda: metric.surface_metrics(pv, lv, ncls, classes=classes)
            got = run()
            dev.sync()
            wall = []
            for _ in range(args.iters):
                t0 = time.perf_counter()
                got = run()
                wall.append((time.perf_counter() - t0) * 1e3)
            wall.sort()
            nvals = sum(int(np.count_nonzero(metric.surface_mask(a == c))) for a in (pv.numpy(), lv.numpy()) for c in classes) \
                if vox <= 1 << 23 else -1
            emit(f"  {kind:5s} call  surface_metrics, {len(classes)} class(es): best {wall[0]:.2f} ms, median {wall[len(wall) // 2]:.2f} ms"
                 f"  = {wall[len(wall) // 2] / len(classes):.2f} ms per class" + (f"; {nvals} surface values downloaded" if nvals >= 0 else "")
                 + f"; hd95 of class 1 = {got['hd95'][0]:.4f}")
            if with_host:
                want, t_d2h, t_scipy = host_metrics(dev, pv, lv, classes[-1] + 1)
                same = all(np.allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True) for k in ("hd", "hd95", "assd"))
                emit(f"  {kind:5s} host  d2h {t_d2h:.1f} ms + scipy {t_scipy:.1f} ms = {t_d2h + t_scipy:.1f} ms"
                     f"   ({(t_d2h + t_scipy) / wall[len(wall) // 2]:.1f} x the device call's median; same metrics: {same})")
            pv.free()
            lv.free()
    dev.free(flush)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

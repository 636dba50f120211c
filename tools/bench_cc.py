"""Micro-benchmark of the connected-component labelling (medicalseg_amd/csrc/msk_ccl.hip, msk_connected_components3d)
beside the host path it replaces (transforms.transform._connected_components after a device -> host copy).
python tools/bench_cc.py [--iters K] [--out FILE]

Masks: 12 box blobs, 50 % random noise and the 3-D checkerboard (V/2 one-voxel components: the worst case of the
sort), at 128^3 and 12 x 512 x 512, as float32 volumes on the device.

device rows: HIP-event time of one msk_connected_components3d call (all of its launches, no host synchronisation),
mean of --iters after 3 warm-up calls.  'warm' runs the calls back to back (the 8-12 MB mask stays in the 256 MB
last-level cache); 'cold' writes a 1 GiB buffer before every call so the mask comes from HBM.  'stages' is one
profiled warm pass split by launch group (the profile's event brackets add a few us per group).  'py call' is the wall
time of preprocess.connected_components_device, which adds the status read (one synchronisation) and the allocation.
host rows: the wall time of the D2H copy and of _connected_components on this machine's CPU, best of 3."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(128, 128, 128), (12, 512, 512)]
FLUSH_BYTES = 1 << 30


def masks(shape):
    import cc_reference as R
    return [("12 box blobs", R.box_blobs(shape, 12, 0)), ("50% noise", R.noise(shape, 1)),
            ("checkerboard", R.checkerboard(shape))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from medicalseg_amd import preprocess as pp
    from medicalseg_amd.device import get_device
    from medicalseg_amd.transforms.transform import _connected_components
    dev = get_device()
    lines = [f"# connected components, {dev.name()}, host CPU: {os.cpu_count()} logical CPUs visible",
             f"# device: HIP-event ms per msk_connected_components3d call (mean of {args.iters}); warm = back to back, "
             "cold = 1 GiB written before every call",
             "# host: wall ms of the D2H copy and of _connected_components (scipy.ndimage.label + ranking), best of 3"]
    flush = dev.malloc(FLUSH_BYTES)
    st = dev.malloc(64)
    for shape in SHAPES:
        for name, m in masks(shape):
            vol = pp.upload(m)
            out = dev.malloc(vol.size * 4)
            call = lambda: dev.call("msk_connected_components3d", C.c_void_p(vol.ptr), C.c_void_p(out), 1, *shape, 0, 0, 0,
                                    C.c_void_p(st), None)
            for _ in range(3):
                call()
            res = {}
            for mode in ("warm", "cold"):
                tot = 0.0
                for i in range(args.iters):
                    if mode == "cold":
                        dev.memset(flush, i & 0xFF, FLUSH_BYTES)
                    dev.timer_start()
                    call()
                    tot += dev.timer_stop()
                res[mode] = tot / args.iters
            dev.sync()
            dev.prof_reset()
            dev.prof_enable(True)
            call()
            dev.sync()
            stages = dev.prof_report()
            dev.prof_enable(False)
            t0 = time.perf_counter()
            for _ in range(args.iters):
                o = pp.connected_components_device(vol)
                o.free()
            py_ms = (time.perf_counter() - t0) * 1e3 / args.iters
            d2h, host = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                a = vol.numpy()
                t1 = time.perf_counter()
                ref = _connected_components(a)
                t2 = time.perf_counter()
                d2h.append((t1 - t0) * 1e3)
                host.append((t2 - t1) * 1e3)
            got = dev.d2h(out, shape, np.int32)
            same = bool(np.array_equal(got, ref))
            lines.append(f"[{shape[0]}x{shape[1]}x{shape[2]} {name}]  {int(ref.max())} components, device == host: {same}")
            lines.append(f"  device  warm {res['warm']:.3f} ms   cold {res['cold']:.3f} ms   py call {py_ms:.3f} ms")
            lines.append("  stages  " + "  ".join(f"{t} {ms / max(c, 1):.3f}" for t, (c, ms) in sorted(stages.items())))
            lines.append(f"  host    d2h {min(d2h):.1f} ms + _connected_components {min(host):.1f} ms = "
                         f"{min(d2h) + min(host):.1f} ms")
            dev.free(out)
            vol.free()
    dev.free(st)
    dev.free(flush)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

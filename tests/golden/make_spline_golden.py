"""Generate tests/golden/spline_golden.npz by running the REFERENCE's own order-3 resampling in the build container:
medicalseg/transforms/functional.py resize_3d(img, size, order=3) with an int size and with a tuple size, and
tools/preprocess_utils geometry.resample(new_shape=..., order=3).  Only inputs, sizes and expected outputs are stored.

    python tests/golden/make_spline_golden.py

The reference is loaded the way make_transforms_golden.py and make_preprocess_golden.py load it (placeholders for the
absent I/O libraries, a path-only `tools` package, cwd at the reference for its relative open).
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def load_reference():
    sys.dont_write_bytecode = True
    os.chdir(REF)
    for n in ["SimpleITK", "nibabel", "pydicom", "nrrd", "cv2", "visualdl"]:
        try:
            importlib.import_module(n)
        except Exception:
            sys.modules[n] = types.ModuleType(n)
    spec = importlib.util.spec_from_file_location("ref_functional", REF + "/medicalseg/transforms/functional.py")
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    t = types.ModuleType("tools")
    t.__path__ = [os.path.join(REF, "tools")]
    sys.modules["tools"] = t
    from tools.preprocess_utils import resample
    return F, resample


def main():
    F, resample = load_reference()
    rng = np.random.default_rng(20261020)
    out = {}
    # resize_3d: (input shape, size); an int size fixes the shortest side (functional.py:41-46)
    resize = [((7, 9, 6), 9), ((5, 8, 11), 4), ((6, 7, 8), (9, 5, 12)), ((1, 6, 5), (3, 6, 2)), ((10, 4, 9), (10, 9, 1))]
    for i, (shape, size) in enumerate(resize):
        img = (rng.random(shape) * 255).astype(np.float32)
        o = F.resize_3d(img.copy(), size, order=3)
        out[f"rz{i}_img"] = img
        out[f"rz{i}_size"] = np.array([size] if isinstance(size, int) else size, dtype=np.int64)
        out[f"rz{i}_out"] = np.ascontiguousarray(o)
    # geometry.resample: CT-like values, up, down and mixed
    cases = [((8, 9, 7), (12, 6, 14)), ((12, 10, 3), (6, 5, 3)), ((4, 5, 6), (11, 10, 9)), ((9, 2, 13), (4, 7, 13))]
    for i, (sin, sout) in enumerate(cases):
        img = (rng.standard_normal(sin) * 400 - 300).astype(np.float32)
        o, _ = resample(img.copy(), new_shape=list(sout), order=3)
        out[f"rs{i}_img"] = img
        out[f"rs{i}_shape"] = np.array(sout, dtype=np.int64)
        out[f"rs{i}_out"] = np.ascontiguousarray(o)
    assert all(v.dtype != object for v in out.values())
    np.savez_compressed(os.path.join(HERE, "spline_golden.npz"), **out)
    print("wrote", len(out), "arrays,", sum(out[k].size for k in out if k.endswith("_out")), "output voxels")


if __name__ == "__main__":
    main()

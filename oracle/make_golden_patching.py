"""Generate tests/golden/patching.npz with the REFERENCE's own `_prepare_patching` (infer/tile.py of the tree refimport.REF names), executed from its
source as tests/test_infer_tile.py does (infer/tile.py imports the whole inference stack; the function itself needs numpy and math only).

What the fixture pins per case of tests/test_infer_tile.py::test_prepare_patching_matches_reference (seeded uint8 image, window, mask):
the padded image as its shape and the SHA-256 of its bytes (the images run to megabytes), and the patch table bit for bit.

    python oracle/make_golden_patching.py
"""
import hashlib
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from refimport import REF, out_dir  # noqa: E402

CASES = [((270, 270), 270, 80), ((256, 256), 256, 164), ((301, 517), 270, 80), ((1000, 731), 256, 164)]


def case_key(shape, win, msk):
    return "%dx%d_w%d_m%d" % (shape[0], shape[1], win, msk)


def case_image(shape):
    return np.random.default_rng(0).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)


def sha256(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def ref_prepare_patching():
    path = os.path.join(REF, "infer", "tile.py")
    src = open(path).read()
    m = re.search(r"def _prepare_patching\(.*?\n(?=####)", src, re.S)

    class _NP:  # numpy >= 2 dropped the np.lib.pad alias the reference uses (infer/tile.py:71)
        lib = type("lib", (), {"pad": staticmethod(np.pad)})

        def __getattr__(self, k):
            return getattr(np, k)

    ns = {"np": _NP(), "math": math}
    exec(compile(m.group(0), path, "exec"), ns)
    return ns["_prepare_patching"]


if __name__ == "__main__":
    fn = ref_prepare_patching()
    out = {}
    for shape, win, msk in CASES:
        pad, info = fn(case_image(shape), win, msk)
        k = case_key(shape, win, msk)
        out[k + "_pad_shape"] = np.asarray(pad.shape, np.int64)
        out[k + "_pad_sha256"] = sha256(pad)
        out[k + "_info"] = np.asarray(info, np.int64)
    np.savez(os.path.join(out_dir(), "patching.npz"), **out)

"""Generate tests/golden/viz_strip.npz with the REFERENCE's own models/hovernet/run_desc.py viz_step_output (imported through
oracle/refimport.py: reference first on sys.path, `__file__` asserted; a stub cv2, which misc/utils.py imports and the picture never
uses; matplotlib on the Agg backend).

Per case (CASES: map size, image size, nr_types) the fixture holds the seeded inputs -- `<case>_img` uint8 [3,ih,iw,3], `<case>_np`
/ `<case>_hv` / `<case>_tp` as `_true` and `_pred` -- and `<case>_strip`, the reference's picture of them.  The inputs carry what
decides a pixel: values at and beyond the range ends, NaN, +-inf, every type id and ids outside 0..nr_types.  `lut` is the reference's
colour table, `(plt.get_cmap("jet")(np.arange(256))[:, :3] * 255).astype("uint8")`.  Arrays only.

    python tools/make_golden_viz.py       (HVN_GOLDEN_OUT=DIR writes elsewhere: tests/test_viz_strip_host.py)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
from refimport import out_dir, ref_import, use_reference  # noqa: E402

N = 3
# name: (map h, w), (image h, w), nr_types, seed
CASES = {
    "m16": ((16, 16), (24, 24), None, 1),
    "m16t5": ((16, 16), (24, 24), 5, 2),
    "m5x7": ((5, 7), (8, 9), None, 3),
    "m5x7t5": ((5, 7), (8, 9), 5, 4),
}


def case_inputs(name):
    """The `raw_data` of a case, host arrays in the dtypes `valid_step` / `train_step` hand on."""
    (h, w), (ih, iw), nr_types, seed = CASES[name]
    rng = np.random.default_rng(seed)
    # few distinct values per plane (sixteen grey levels per channel, maps in steps of 1/32): the .npz stays small; dense random
    # floats are what tests/test_viz_strip_host.py feeds the live reference
    raw = {"img": (rng.integers(0, 16, (N, ih, iw, 3)) * 17).astype(np.uint8)}
    true_np = rng.integers(0, 2, (N, h, w)).astype(np.int64)
    pred_np = (rng.integers(0, 33, (N, h, w)) / 32).astype(np.float32)
    true_hv = (rng.integers(-32, 33, (N, h, w, 2)) / 32).astype(np.float32)
    pred_hv = (rng.integers(-48, 49, (N, h, w, 2)) / 32).astype(np.float32)                    # a third of them beyond the range
    special = np.array([0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, 0.5, -0.0, 1.0e-40, 255.0 / 256.0, 1.5, -7.0], np.float32)
    pred_np.reshape(-1)[:special.size] = special
    pred_hv.reshape(-1)[:special.size] = special
    true_hv.reshape(-1)[:3] = [-1.0, 1.0, 0.0]
    raw["np"], raw["hv"] = (true_np, pred_np), (true_hv, pred_hv)
    if nr_types is not None:
        true_tp = rng.integers(0, nr_types + 1, (N, h, w)).astype(np.int64)
        pred_tp = rng.integers(0, nr_types + 1, (N, h, w)).astype(np.float32)
        ids = np.arange(-1, nr_types + 2)
        true_tp.reshape(-1)[:ids.size] = ids
        pred_tp.reshape(-1)[-ids.size:] = ids
        raw["tp"] = (true_tp, pred_tp)
    return raw, nr_types


def for_reference(raw):
    """Copies (the reference clamps in place where astype does not copy) with the NP and TP maps as [n,h,w,1]: the reference's
    `aligned_shape` stacks the shapes of img, true_np and pred_np into one array, which numpy >= 1.24 refuses for shapes of unequal
    length; its `colorize` squeezes the axis away again."""
    out = {"img": raw["img"].copy(), "hv": tuple(a.copy() for a in raw["hv"])}
    for k in ("np", "tp"):
        if k in raw:
            out[k] = tuple(a[..., None].copy() for a in raw[k])
    return out


def main():
    use_reference()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    R = ref_import("models.hovernet.run_desc")
    out = {"lut": (plt.get_cmap("jet")(np.arange(256))[:, :3] * 255).astype("uint8")}
    for name in CASES:
        raw, nr_types = case_inputs(name)
        out[name + "_img"] = raw["img"]
        for k in ("np", "hv", "tp"):
            if k in raw:
                out[name + "_" + k + "_true"], out[name + "_" + k + "_pred"] = raw[k]
        with np.errstate(invalid="ignore"):
            strip = R.viz_step_output(for_reference(raw), nr_types)
        assert strip.dtype == np.uint8
        out[name + "_strip"] = strip
    np.savez_compressed(os.path.join(out_dir(), "viz_strip.npz"), **out)


if __name__ == "__main__":
    main()

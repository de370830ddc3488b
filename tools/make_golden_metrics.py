"""Generate tests/golden/metrics_cases.npz with the REFERENCE's own metrics/stats_utils.py and compute_stats.py (imported through
oracle/refimport.py: reference first on sys.path, `__file__` asserted; a stub cv2, which stats_utils imports and never uses).

Per case (`<case>_true`, `<case>_pred`: int32 maps, raw ids, see CASES) the fixture pins, on remap_label(true), remap_label(pred):
    <case>_vals  float64 [13]: get_fast_pq(match_iou 0.3 | 0.5 | 0.7) -> dq, sq, pq each; get_fast_aji; get_fast_aji_plus; then on
                 the raw maps get_dice_1, and on the remapped maps get_fast_dice_2, get_dice_2
    <case>_pairs int64 [2, k]: paired_true / paired_pred of get_fast_pq at 0.5
and over all cases the reference's run_nuclei_inst_stat on .mat files holding the maps: `inst_stat` float64 [6, N] (cases in
sorted file order = `inst_names`) and its printed lines `inst_stdout`.

    python tools/make_golden_metrics.py       (HVN_GOLDEN_OUT=DIR writes elsewhere: tests/test_metrics_golden.py)
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
from refimport import out_dir, ref_import, use_reference  # noqa: E402

# name: (h, w, instances, seed, id_stride, id_base, shift)
CASES = {
    "s64": (64, 64, 12, 1, 1, 0, (2, 1)),
    "s57x91": (57, 91, 18, 2, 1, 0, (1, -2)),
    "s128": (128, 128, 40, 3, 3, 5, (0, 1)),
    "s200x150": (200, 150, 60, 4, 1, 0, (3, 2)),
    "bigids": (96, 96, 20, 5, 11, 2 ** 31 - 1 - 11 * 30, (2, 2)),
    "s256": (256, 256, 120, 6, 1, 0, (2, 1)),
}
MATCH = (0.3, 0.5, 0.7)


def case_maps(name):
    from hover_net_amd.synth import synth_inst_pair

    h, w, k, seed, stride, base, shift = CASES[name]
    return synth_inst_pair(h, w, k, seed=seed, shift=shift, id_stride=stride, id_base=base)


def main():
    use_reference()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    S = ref_import("metrics.stats_utils")
    out = {}
    for name in CASES:
        t, p = case_maps(name)
        rt, rp = S.remap_label(t), S.remap_label(p)
        vals = []
        for mi in MATCH:
            vals += [float(v) for v in S.get_fast_pq(rt, rp, match_iou=mi)[0]]
        vals += [S.get_fast_aji(rt, rp), S.get_fast_aji_plus(rt, rp), S.get_dice_1(t, p), S.get_fast_dice_2(rt, rp), S.get_dice_2(rt, rp)]
        pairs = S.get_fast_pq(rt, rp, match_iou=0.5)[1]
        out[name + "_true"], out[name + "_pred"] = t, p
        out[name + "_vals"] = np.array(vals, np.float64)
        out[name + "_pairs"] = np.stack([np.asarray(pairs[0], np.int64), np.asarray(pairs[1], np.int64)])
    import scipy.io as sio

    CS = ref_import("compute_stats")
    with tempfile.TemporaryDirectory() as d:
        for sub in ("true", "pred"):
            os.makedirs(os.path.join(d, sub))
        for name in CASES:
            for sub in ("true", "pred"):
                sio.savemat(os.path.join(d, sub, name + ".mat"), {"inst_map": out[name + "_" + sub]})
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            inst = CS.run_nuclei_inst_stat(os.path.join(d, "pred"), os.path.join(d, "true"), print_img_stats=True)
        stdout = buf.getvalue().replace(os.path.join(d, "pred"), "<pred_dir>")
    out["inst_stat"] = np.asarray(inst, np.float64)
    out["inst_names"] = np.array(sorted(CASES))
    out["inst_stdout"] = np.array(stdout)
    np.savez_compressed(os.path.join(out_dir(), "metrics_cases.npz"), **out)


if __name__ == "__main__":
    main()

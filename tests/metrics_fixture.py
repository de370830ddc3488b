"""Helpers shared by the CPU and GPU tests of tests/golden/metrics_cases.npz (written by tools/make_golden_metrics.py)."""
import os

import numpy as np

from hover_net_amd import metrics as M

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "metrics_cases.npz")


def cases(d):
    """The case names of a loaded fixture, sorted."""
    return sorted(k[:-5] for k in d.files if k.endswith("_true"))


def case_values(t, p, device):
    """The 13 values and the PQ pairing of a fixture case, in the order tools/make_golden_metrics.py records them, through
    hover_net_amd.metrics on `device`."""
    rt, rp = M.remap_label(t, device=device), M.remap_label(p, device=device)
    vals = []
    for mi in (0.3, 0.5, 0.7):
        vals += [float(v) for v in M.get_fast_pq(rt, rp, match_iou=mi, device=device)[0]]
    vals += [M.get_fast_aji(rt, rp, device=device), M.get_fast_aji_plus(rt, rp, device=device), M.get_dice_1(t, p, device=device),
             M.get_fast_dice_2(rt, rp, device=device), M.get_dice_2(rt, rp, device=device)]
    pairs = M.get_fast_pq(rt, rp, match_iou=0.5, device=device)[1]
    return np.array(vals, np.float64), np.stack([np.asarray(pairs[0], np.int64), np.asarray(pairs[1], np.int64)])

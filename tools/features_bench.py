"""Times the per-nucleus feature pass (hvn_instance_features) against the record-table pass it sits next to (hvn_instance_table, an
existing kernel: the yardstick), on one GPU, and prints a small table plus ONE JSON line.

    python tools/features_bench.py [--reps 30] [--inner 10] [--out FILE]

workloads  tiles  64 maps of 164 x 164 from synth.synth_pred_maps(seed=100, k_lo=2, k_hi=8): bench.py's structured workload
           wsi    one 2048 x 2048 map of the same kind: a whole-slide stage-2 tile (assembled from four 512 x 512 painted blocks,
                  block (r + c) % 4 at block row r, block column c, like tools/contour_bench.py)
Both are post-processed on the device first (hvn_postproc); what is timed starts from the instance maps in HBM.
legs (warm; each sample is --inner back-to-back calls between two HIP events on one stream, divided by --inner; median of --reps
samples, min and max are printed too)
           table_ms         PostProc.table: init + accumulate + finalize of hvn_instance_table (with the type vote, nr_types = 5)
           features_ms      PostProc.features(image=None): the shape sums
           features_rgb_ms  PostProc.features with a uint8 RGB image: + the colour sums
The three legs alternate inside one loop, so that drift on a shared machine hits all alike.  Before anything is timed, `seen` of
every slot is compared with the table's `area` and the colour-free fields of both feature calls with each other.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run(name, n, hw, reps, inner):
    import torch

    from hover_net_amd import features as F
    from hover_net_amd import post_proc as PP
    from hover_net_amd.synth import synth_pred_maps

    dev = torch.device("cuda", 0)
    if hw <= 512:
        pred = torch.from_numpy(synth_pred_maps(n, hw, hw, 5, seed=100, k_lo=2, k_hi=8)[0]).to(dev)
    else:
        assert n == 1 and hw % 512 == 0
        blk = synth_pred_maps(4, 512, 512, 5, seed=100, k_lo=2, k_hi=8)[0]
        g = hw // 512
        pred = torch.from_numpy(np.concatenate([np.concatenate([blk[(r + c) % 4] for c in range(g)], 1) for r in range(g)], 0)[None]).to(dev)
    image = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)).to(dev)
    pp = PP.PostProc(dev)
    inst = pp.separate(pred)
    rec, counts = pp.table(inst, pred, 5)
    max_inst = rec.shape[1]

    # same result first
    rec_h = rec.cpu().numpy().view(PP._REC_DTYPE).reshape(n, max_inst)
    plain = pp.features(inst, rec).cpu().numpy().view(F.FEAT_DTYPE).reshape(n, max_inst)
    rgb = pp.features(inst, rec, image).cpu().numpy().view(F.FEAT_DTYPE).reshape(n, max_inst)
    assert np.array_equal(plain["seen"], rec_h["area"]) and np.array_equal(rgb["seen"], rec_h["area"]), "seen != area"
    for k in ("sxx", "syy", "sxy", "per"):
        assert np.array_equal(plain[k], rgb[k]), k
    assert not plain["csum"].any() and rgb["csum"].any()

    calls = {"table_ms": lambda: pp.table(inst, pred, 5), "features_ms": lambda: pp.features(inst, rec),
             "features_rgb_ms": lambda: pp.features(inst, rec, image)}
    legs = {k: [] for k in calls}
    for it in range(reps + 3):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= 3:                                   # three warm-up rounds
                legs[k].append(e0.elapsed_time(e1) / inner)
    out = {"workload": name, "maps": n, "hw": hw, "slots": n * max_inst, "instances": int(counts.sum()), "reps": reps, "inner": inner}
    out.update({k: stat(v) for k, v in legs.items()})
    t = out["table_ms"]["median"]
    out["features_over_table"] = round(out["features_ms"]["median"] / t, 3)
    out["features_rgb_over_table"] = round(out["features_rgb_ms"]["median"] / t, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "the median is taken over at least 20 samples"
    from hover_net_amd import lib as L

    L.require_gpu()
    res = [run("tiles", 64, 164, a.reps, a.inner), run("wsi", 1, 2048, a.reps, a.inner)]
    lines = ["hvn_instance_features vs hvn_instance_table (ms per call, median [min .. max] of %d samples of %d calls each)" % (a.reps, a.inner)]
    for r in res:
        lines.append("%-5s %d x %d x %d, %d slots, %d instances" % (r["workload"], r["maps"], r["hw"], r["hw"], r["slots"], r["instances"]))
        for k in ("table_ms", "features_ms", "features_rgb_ms"):
            lines.append("    %-16s %8.4f  [%8.4f .. %8.4f]" % (k, r[k]["median"], r[k]["min"], r[k]["max"]))
        lines.append("    features / table = %.3f    features_rgb / table = %.3f" % (r["features_over_table"], r["features_rgb_over_table"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"features_bench": res}))


if __name__ == "__main__":
    main()

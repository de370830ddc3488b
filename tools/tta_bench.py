"""Times the infer_step of BASELINE cfg 2 (original mode, 5 types, batch 32, fp32) with and without test-time augmentation on one GPU,
and the two new launches alone, and prints a small table plus ONE JSON line.

    python tools/tta_bench.py [--reps 20] [--batch 32] [--out profiles/tta_bench.txt]

legs (warm; one sample = one step between two HIP events on the engine's stream; median of --reps samples, min and max are printed too)
           none      run_desc.infer_step_device(tiles, net)                  the plain step
           flips     ... tta="flips"   four views, none of them transposing
           d4        ... tta="d4"      all eight views
The three legs alternate inside one loop, so that drift on a shared machine hits all alike.  tiles/s = batch / median.
kernels    HVN_OP_VIEW (one launch, view 5: flip + quarter turn, the transposing form) and HVN_OP_TTA (one launch, view 5, not the
           last / the last view) on the engine's own buffers: 10 back-to-back launches between two HIP events, divided by 10.
Before anything is timed the d4 result is compared with the float32 numpy oracle (tests/tta_ref.py) on the logits of eight plain
passes: the hv channels must be equal, and the largest np / type-probability error against float64 is printed.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import tta_ref as R
    from hover_net_amd import lib as L
    from hover_net_amd import net_desc, run_desc
    from hover_net_amd import plan as PL
    from hover_net_amd.synth import synth_state_dict, synth_tiles

    L.require_gpu()
    n = a.batch
    net = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    net.load_state_dict(synth_state_dict("original", 5, seed=21), strict=True)
    net = net.to("cuda").eval()
    net.max_batch = n
    tiles_h = synth_tiles(n, 270, seed=22)
    tiles = torch.from_numpy(tiles_h).to("cuda")
    eng = net.engine(n)

    # same result first (three samples are enough for the oracle; the step runs on all)
    m = min(n, 3)
    per = []
    for k in range(8):
        v = np.ascontiguousarray(np.stack([R.view(t, k) for t in tiles_h[:m]]))
        logits, _ = eng.run(torch.from_numpy(v).to("cuda"))
        per.append({b: t.cpu().numpy() for b, t in logits.items()})
    got = run_desc.infer_step_device(tiles[:m], net, tta="d4").cpu().numpy()
    acc = eng._tta_acc[:m].cpu().numpy()
    r32, r64 = R.reduce_f32(per, tuple(range(8))), R.reduce_f64(per, tuple(range(8)))
    assert (got[..., 2:] == r32["hv"]).all(), "hv channels differ from the float32 oracle"
    err = max(np.abs(got[..., 1].astype(np.float64) - r64["np"]).max(), np.abs(acc[..., 3:].astype(np.float64) / 8 - r64["tp"]).max())
    own = max(np.abs(r32["np"] - r64["np"]).max(), np.abs(r32["tp"] - r64["tp"]).max())

    calls = {"none": lambda: run_desc.infer_step_device(tiles, net), "flips": lambda: run_desc.infer_step_device(tiles, net, tta="flips"),
             "d4": lambda: run_desc.infer_step_device(tiles, net, tta="d4")}
    legs = {k: [] for k in calls}
    for it in range(a.reps + 2):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 2:                                   # two warm-up rounds
                legs[k].append(e0.elapsed_time(e1))

    # the two launches alone, on the engine's buffers
    vo, to = L.hvn_op(), L.hvn_op()
    vo.kind, vo._rsv = PL.OP_VIEW, 5
    vo.x.base, vo.y.base = tiles.data_ptr(), eng._tta_scratch.data_ptr()
    for v in (vo.x, vo.y):
        v.h, v.w, v.c = 270, 270, 3
    to.kind, to._rsv, to.cout, to.stride = PL.OP_TTA, 5, 5, 8
    to.x.base, to.res.base, to.w = eng.logits["np"].data_ptr(), eng.logits["hv"].data_ptr(), eng.logits["tp"].data_ptr()
    to.y.base, to.y2.base = eng.pred_map.data_ptr(), eng._tta_acc.data_ptr()
    to.y.h, to.y.w, to.y.c = 80, 80, 4
    run_op, sp = L.lib().hvn_run_op, L.stream_ptr("cuda")

    def launch(op, last):
        to.kw = int(last)
        L.check(run_op(ctypes.addressof(op), n, sp), "hvn_run_op")

    kern = {"view_ms": lambda: launch(vo, 0), "tta_ms": lambda: launch(to, 0), "tta_last_ms": lambda: launch(to, 1)}
    ksamp = {k: [] for k in kern}
    for it in range(a.reps + 2):
        for k, fn in kern.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            if it >= 2:
                ksamp[k].append(e0.elapsed_time(e1) / 10)

    out = {"batch": n, "reps": a.reps, "np_tp_err_vs_f64": float(err), "oracle_f32_err_vs_f64": float(own)}
    out.update({k + "_ms": stat(v) for k, v in legs.items()})
    out.update({k: stat(v) for k, v in ksamp.items()})
    for k in legs:
        out[k + "_tiles_per_s"] = round(1000.0 * n / out[k + "_ms"]["median"], 1)
    lines = ["infer_step with test-time augmentation, cfg 2 (original, 5 types, fp32), batch %d: ms per step, median [min .. max] of %d samples" % (n, a.reps)]
    for k, nv in (("none", 1), ("flips", 4), ("d4", 8)):
        s = out[k + "_ms"]
        lines.append("    tta=%-6s %9.3f  [%9.3f .. %9.3f]   %8.1f tiles/s   %.2f x the plain step (%d views)"
                     % (k, s["median"], s["min"], s["max"], out[k + "_tiles_per_s"], s["median"] / out["none_ms"]["median"], nv))
    lines.append("the launches alone (ms per launch, 10 back-to-back between two HIP events; view 5 = flip + quarter turn)")
    for k in kern:
        s = ksamp[k]
        lines.append("    %-12s %8.4f  [%8.4f .. %8.4f]" % (k, statistics.median(s), min(s), max(s)))
    per_view = out["view_ms"]["median"] + out["tta_ms"]["median"]
    lines.append("    VIEW + TTA per view = %.4f ms = %.2f %% of the plain step" % (per_view, 100.0 * per_view / out["none_ms"]["median"]))
    lines.append("d4 on %d tiles against the numpy oracle: hv bit-equal; np / type probabilities differ from float64 by at most %.3g"
                 " (the float32 oracle itself: %.3g)" % (m, err, own))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tta_bench": out}))


if __name__ == "__main__":
    main()

"""Times the device contour tracer (hvn_trace_contours_device) against the host path it can replace, on one GPU, and prints a
small table plus ONE JSON line.

    python tools/contour_bench.py [--reps 30] [--out FILE]

workloads  tiles  32 maps of 164 x 164 from synth.synth_pred_maps(seed=100, k_lo=2, k_hi=8): bench.py's structured workload
           wsi    one 2048 x 2048 map of the same kind: a whole-slide stage-2 tile (assembled from four 512 x 512 painted blocks,
                  block (r + c) % 4 at block row r, block column c, like tools/wsi_bench.py: painting 2048 x 2048 at once takes minutes)
Both are post-processed on the device first (hvn_postproc + hvn_instance_table); what is timed starts from the instance maps and
the record table in HBM.
legs (warm, median of --reps; min and max are printed too)
           device_trace_ms  PostProc.contours alone: HIP events around the call (count pass, prefix sum, emit pass)
           d2h_pts_offs_ms  copying pts (the offs[-1] points that were traced) and offs into pinned memory, HIP events
           d2h_capacity_ms  copying the WHOLE pts buffer (its default capacity, a quarter of the pixels) and offs: what TilePipeline(to_host=True),
                            WsiInference(device_contours=True) and trace_contours_device copy today, since the total is not known on the host
                            before the copy is enqueued; HIP events
           device_path_ms   the first two in sequence, host clock from the call to the end of the copy (includes the launch overhead)
           host_d2h_inst_ms the path replaced: the int32 instance maps into pinned memory (the host tracer reads them), HIP events
           host_trace_ms    trace_contours_flat per map on those arrays at its default thread count, host clock
           host_path_ms     the sum of the two
The device and the host legs alternate inside one loop, so that drift on a shared machine hits both alike.  The contours of both
paths are compared with == before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run(name, n, hw, reps):
    import torch

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
    pp = PP.PostProc(dev)
    inst = pp.separate(pred)
    rec, counts = pp.table(inst, pred, 5)
    max_inst = rec.shape[1]
    pts, offs, status = pp.contours(inst, rec)
    assert status.cpu().tolist() == [0, 0, -1, 0], status.cpu().tolist()
    total = int(offs[-1])
    inst_pin = torch.empty(inst.shape, dtype=torch.int32, pin_memory=True)
    pts_pin = torch.empty((total, 2), dtype=torch.int32, pin_memory=True)
    offs_pin = torch.empty(offs.shape, dtype=torch.int64, pin_memory=True)
    cap_pin = torch.empty(pts.shape, dtype=torch.int32, pin_memory=True)
    rec_h = rec.cpu().numpy().view(PP._REC_DTYPE).reshape(n, max_inst)

    def host_trace():
        a = inst_pin.numpy()
        return [PP.trace_contours_flat(a[i], rec_h[i]) for i in range(n)]

    # same result first
    inst_pin.copy_(inst)
    want = host_trace()
    got = PP.split_contours(pts.cpu().numpy(), offs.cpu().numpy(), n, max_inst)
    for (gp, go), (wp, wo) in zip(got, want):
        assert np.array_equal(go, wo) and np.array_equal(gp, wp), "device and host contours differ"

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    legs = {k: [] for k in ("device_trace_ms", "d2h_pts_offs_ms", "d2h_capacity_ms", "device_path_ms", "host_d2h_inst_ms", "host_trace_ms")}
    for it in range(reps + 3):
        e = [ev() for _ in range(7)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e[0].record()
        p, o, _ = pp.contours(inst, rec)
        e[1].record()
        pts_pin.copy_(p[:total], non_blocking=True)
        offs_pin.copy_(o, non_blocking=True)
        e[2].record()
        e[2].synchronize()
        t1 = time.perf_counter()
        e[3].record()
        inst_pin.copy_(inst, non_blocking=True)
        e[4].record()
        e[4].synchronize()
        t2 = time.perf_counter()
        host_trace()
        t3 = time.perf_counter()
        e[5].record()
        cap_pin.copy_(p, non_blocking=True)
        offs_pin.copy_(o, non_blocking=True)
        e[6].record()
        e[6].synchronize()
        if it < 3:                                   # warm-up rounds
            continue
        legs["device_trace_ms"].append(e[0].elapsed_time(e[1]))
        legs["d2h_pts_offs_ms"].append(e[1].elapsed_time(e[2]))
        legs["d2h_capacity_ms"].append(e[5].elapsed_time(e[6]))
        legs["device_path_ms"].append((t1 - t0) * 1e3)
        legs["host_d2h_inst_ms"].append(e[3].elapsed_time(e[4]))
        legs["host_trace_ms"].append((t3 - t2) * 1e3)
    res = {k: stat(v) for k, v in legs.items()}
    res["host_path_ms"] = stat([a + b for a, b in zip(legs["host_d2h_inst_ms"], legs["host_trace_ms"])])
    px = n * hw * hw
    res.update({"workload": name, "maps": [n, hw, hw], "max_inst": max_inst, "instances": int(counts.sum()), "points": total,
                "points_per_pixel": round(total / px, 4), "longest_contour": int(np.diff(offs.cpu().numpy()).max()),
                "pts_capacity": int(pts.shape[0]), "d2h_bytes_device_path": total * 8 + offs.numel() * 8,
                "d2h_bytes_capacity": pts.numel() * 4 + offs.numel() * 8, "d2h_bytes_host_path": px * 4,
                "reps": reps})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch

    from hover_net_amd import lib as L

    L.require_gpu()
    rows = [run("tiles", 32, 164, args.reps), run("wsi", 1, 2048, args.reps)]
    lines = ["device contour tracer vs the host path, %s, median [min .. max] ms of %d warm runs" % (torch.cuda.get_device_name(0), args.reps)]
    for r in rows:
        lines.append("%-5s %s  instances %d  points %d  points/pixel %.4f  longest contour %d" % (
            r["workload"], "x".join(map(str, r["maps"])), r["instances"], r["points"], r["points_per_pixel"], r["longest_contour"]))
        for k in ("device_trace_ms", "d2h_pts_offs_ms", "d2h_capacity_ms", "device_path_ms", "host_d2h_inst_ms", "host_trace_ms", "host_path_ms"):
            lines.append("      %-17s %9.4f  [%9.4f .. %9.4f]" % (k, r[k]["median"], r[k]["min"], r[k]["max"]))
    lines.append(json.dumps({"tool": "contour_bench", "host_threads": os.environ.get("HVN_HOST_THREADS", "default"), "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

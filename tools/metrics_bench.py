"""Times the instance-metrics path (hover_net_amd/metrics.py) on two synthetic sets and prints ONE JSON line.

    python tools/metrics_bench.py [--reps 5] [--ref-maps 1]

sets      consep   14 maps of 1000 x 1000, ~600 disk instances each; pred = truth shifted, with merges, splits, misses and
                   spurious instances (hover_net_amd.synth.synth_inst_pair)
          pannuke  256 maps of 256 x 256, ~40 instances each
legs (median of --reps, milliseconds for the whole set; maps resident on the device where there is one)
          device_table_ms  hvn_pair_table over the set (kernels only, CUDA events; groups as metrics.device_triples makes them)
          device_copy_ms   metrics.device_triples: the kernels + copying the K triples per image to the host
          host_half_ms     from those triples to the [N, 6] rows: sort, rank, dense IoU matrices, linear_sum_assignment
          end_to_end_ms    metrics.instance_stats(true, pred) on the device tensors
          host_table_ms    the host restatement of the table alone (metrics.host_triples, np.unique of an int64 key)
          host_e2e_ms      metrics.instance_stats on the host path
reference (only where the reference tree exists): seconds per map of its own get_dice_1 / get_fast_aji / get_fast_pq /
get_fast_aji_plus on the first --ref-maps maps of the consep set.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REF = "/root/reference"


def make_set(name):
    from hover_net_amd.synth import synth_inst_pair

    if name == "consep":
        pairs = [synth_inst_pair(1000, 1000, 600, seed=100 + i, shift=(1 + i % 3, (i % 5) - 2), r_lo=4, r_hi=10) for i in range(14)]
    else:
        pairs = [synth_inst_pair(256, 256, 40, seed=1000 + i, shift=(i % 3, 1 - i % 3)) for i in range(256)]
    return np.stack([t for t, _ in pairs]), np.stack([p for _, p in pairs])


def median_ms(fn, reps, sync=None):
    out = []
    fn()
    for _ in range(reps):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 3)


def device_legs(true, pred, reps):
    import torch

    from hover_net_amd import lib as L
    from hover_net_amd import metrics as M

    dev = torch.device("cuda", 0)
    td, pd = torch.from_numpy(true).to(dev), torch.from_numpy(pred).to(dev)
    n, h, w = true.shape
    per = L.lib().hvn_pair_table_workspace_bytes(1, h, w) + 12 * h * w
    g = max(1, min(n, M.WORKSPACE_BUDGET // per))
    bufs = []
    for i0 in range(0, n, g):
        m = min(g, n - i0)
        need = L.lib().hvn_pair_table_workspace_bytes(m, h, w)
        bufs.append((i0, m, need, torch.empty(need, dtype=torch.uint8, device=dev), torch.empty((m, h * w, 3), dtype=torch.int32, device=dev),
                     torch.empty(m, dtype=torch.int32, device=dev)))
    stream = L.stream_ptr(dev)

    def kernels():
        for i0, m, need, ws, tri, cnt in bufs:
            L.check(L.lib().hvn_pair_table(td[i0:i0 + m].data_ptr(), pd[i0:i0 + m].data_ptr(), m, h, w, tri.data_ptr(), cnt.data_ptr(),
                                           ws.data_ptr(), need, stream), "hvn_pair_table")

    kernels()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        kernels()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    del bufs
    triples = M.device_triples(td, pd, dev)
    k = [len(x) for x in triples]

    def host_half():
        for tr in triples:
            tab = M.PairTable(tr, h * w).ranked()
            M.pq_from_table(tab, 0.5)
            M.dice_1_from_table(tab), M.aji_from_table(tab), M.aji_plus_from_table(tab)

    assert np.array_equal(M.instance_stats(td, pd), M.instance_stats(list(true), list(pred), device="cpu"))
    return {"device_table_ms": round(statistics.median(times), 3),
            "device_copy_ms": median_ms(lambda: M.device_triples(td, pd, dev), reps, torch.cuda.synchronize),
            "host_half_ms": median_ms(host_half, reps),
            "end_to_end_ms": median_ms(lambda: M.instance_stats(td, pd), reps, torch.cuda.synchronize),
            "triples_per_image": int(np.median(k)), "groups": len(range(0, n, g)),
            "table_bytes_read_MB": round(true.nbytes * 2 / 1e6, 1)}


def reference_times(true, pred, n):
    sys.path.insert(0, REF)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    os.environ.setdefault("MPLBACKEND", "Agg")
    import metrics.stats_utils as S

    assert S.__file__.startswith(REF), S.__file__
    out = {}
    for i in range(n):
        t, p = S.remap_label(true[i]), S.remap_label(pred[i])
        for fn in ("get_dice_1", "get_fast_aji", "get_fast_pq", "get_fast_aji_plus"):
            t0 = time.perf_counter()
            getattr(S, fn)(t, p)
            out.setdefault(fn + "_s", []).append(time.perf_counter() - t0)
    return {k: round(statistics.mean(v), 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-maps", type=int, default=1)
    args = ap.parse_args()
    import torch

    from hover_net_amd import metrics as M

    res = {"tool": "metrics_bench", "gpu": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None}
    for name in ("consep", "pannuke"):
        true, pred = make_set(name)
        leg = {"maps": list(true.shape),
               "instances_per_map": int(np.median([len(np.unique(t)) - 1 for t in true])),
               "host_table_ms": median_ms(lambda: [M.host_triples(t, p) for t, p in zip(true, pred)], args.reps),
               "host_e2e_ms": median_ms(lambda: M.instance_stats(list(true), list(pred), device="cpu"), max(1, args.reps // 2))}
        if torch.cuda.is_available():
            leg.update(device_legs(true, pred, args.reps))
        if name == "consep" and args.ref_maps > 0 and os.path.isdir(os.path.join(REF, "metrics")):
            leg["reference_per_map"] = reference_times(true, pred, args.ref_maps)
        res[name] = leg
    print(json.dumps(res))


if __name__ == "__main__":
    main()

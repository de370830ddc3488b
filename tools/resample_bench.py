"""Times the device resampler (hvn_resize_window) against the host statement of the same arithmetic (resample.resize_host) on one
GPU and its host, and prints a small table plus ONE JSON line.

    python tools/resample_bench.py [--reps 5] [--out FILE]

workloads  up    a 5000 x 5000 random source to 10 000 x 10 000 (f = 2, cubic): one chunk of a 20x slide processed at 40x
           down  a 10 000 x 10 000 source to 5000 x 5000 (f = 1/2, linear)
legs (warm; median of --reps, min and max are printed too)
           kernel_ms   hvn_resize_window alone, source and tables resident: HIP events around the one launch
           wrapper_ms  resample.resize_window_device, source resident: tables made on the host and uploaded, then the launch (events)
           copy_ms     a device-to-device copy of the OUTPUT's bytes (torch copy_, events): the machine's copy rate for comparison
           host_s      resample.resize_host on the same input, host clock, ONE run (vectorised numpy, single thread)
bytes      the bytes the algorithm must move: 3 * src pixels read + 3 * dst pixels written (+ the tables); kernel GB/s = bytes /
           kernel_ms; copy GB/s = 2 * output bytes / copy_ms; `of_copy` is their ratio.
The device result is compared with the host result (==, every byte) before anything is timed.
"""
import argparse
import ctypes
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


def run(name, n, f, reps):
    import torch

    from hover_net_amd import lib as L, resample as R

    dev = torch.device("cuda", 0)
    src = np.random.default_rng(5).integers(0, 256, (n, n, 3), dtype=np.uint8)
    m = R.out_size(n, f)
    t0 = time.perf_counter()
    want = R.resize_host(src, f)
    host_s = time.perf_counter() - t0
    src_dev = torch.from_numpy(src).to(dev)
    out = torch.empty((m, m, 3), dtype=torch.uint8, device=dev)
    other = torch.empty_like(out)
    tabs_np = R.window_tables((n, n), f, 0, 0, m, m)
    tabs = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in tabs_np]
    taps = int(tabs_np[1].shape[1])
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def kernel():
        L.check(L.lib().hvn_resize_window(src_dev.data_ptr(), n, n, 3 * n, 0, 0, n, n, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                          tabs[3].data_ptr(), taps, out.data_ptr(), m, m, stream), "hvn_resize_window")

    kernel()
    assert np.array_equal(out.cpu().numpy(), want), "device and host results differ"
    out.zero_()
    R.resize_window_device(src_dev, (0, 0), (n, n), f, 0, 0, m, m, out=out)
    assert np.array_equal(out.cpu().numpy(), want), "wrapper and host results differ"
    del want

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {"kernel_ms": [], "wrapper_ms": [], "copy_ms": []}
    for it in range(reps + 2):                           # the legs alternate inside one loop; two warm-up rounds
        k = timed(kernel)
        w = timed(lambda: R.resize_window_device(src_dev, (0, 0), (n, n), f, 0, 0, m, m, out=out))
        c = timed(lambda: other.copy_(out))
        if it >= 2:
            legs["kernel_ms"].append(k)
            legs["wrapper_ms"].append(w)
            legs["copy_ms"].append(c)
    res = {k: stat(v) for k, v in legs.items()}
    moved = 3 * n * n + 3 * m * m + sum(int(a.nbytes) for a in tabs_np)
    kernel_gbs = moved / (res["kernel_ms"]["median"] * 1e-3) / 1e9
    copy_gbs = 2 * 3 * m * m / (res["copy_ms"]["median"] * 1e-3) / 1e9
    res.update({"workload": name, "source": [n, n], "output": [m, m], "factor": f, "kind": R.kind_of(f), "host_s": round(host_s, 3),
                "bytes_moved": moved, "kernel_GBps": round(kernel_gbs, 1), "copy_GBps": round(copy_gbs, 1),
                "of_copy": round(kernel_gbs / copy_gbs, 4), "reps": reps})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch

    from hover_net_amd import lib as L

    L.require_gpu()
    rows = [run("up", 5000, 2.0, args.reps), run("down", 10000, 0.5, args.reps)]
    lines = ["device resampler vs the host statement, %s, median [min .. max] of %d warm runs" % (torch.cuda.get_device_name(0), args.reps)]
    for r in rows:
        lines.append("%-5s %s -> %s  f %g (%s)  bytes moved %d" % (r["workload"], "x".join(map(str, r["source"])), "x".join(map(str, r["output"])),
                                                                  r["factor"], r["kind"], r["bytes_moved"]))
        for k in ("kernel_ms", "wrapper_ms", "copy_ms"):
            lines.append("      %-12s %10.4f  [%10.4f .. %10.4f]" % (k, r[k]["median"], r[k]["min"], r[k]["max"]))
        lines.append("      %-12s %10.3f  (one run)" % ("host_s", r["host_s"]))
        lines.append("      kernel %.1f GB/s, device copy %.1f GB/s: %.1f %% of the copy rate" % (r["kernel_GBps"], r["copy_GBps"], 100 * r["of_copy"]))
    lines.append(json.dumps({"tool": "resample_bench", "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

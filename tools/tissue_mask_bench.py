"""Times the device tissue mask (csrc/hvn_tissue.hip) against the host heuristic (tissue_mask.simple_get_mask) on one GPU and
its host, and the summed-area box test against the per-box loop, and prints a small table plus ONE JSON line.

    python tools/tissue_mask_bench.py [--reps 7] [--host-reps 3] [--out FILE]

thumbnails  synth.synth_thumbnail(n, n, seed 3): 1250 x 1250 (a 40 000 x 40 000 slide at 1/32) and 3125 x 3125 (100 000 x 100 000);
            the fraction of pixels drawn as tissue is printed with each
legs        host_s        tissue_mask.simple_get_mask(thumb), host clock, median of --host-reps
            device_ms     tissue_mask.simple_get_mask(thumb, device=...): host thumbnail to host mask -- upload, grey + histogram,
                          histogram readback, Otsu on the host, mask kernels, download -- host clock (the call ends in a
                          synchronising copy), median of --reps after two warm-up calls
            gray_hist_ms  hvn_tissue_gray_hist alone, thumbnail resident (HIP events)
            mask_ms       hvn_tissue_mask alone, grey plane and workspace resident (HIP events): two connected-component passes
                          and the dilation, 10 launches and 2 clears
            device legs alternate inside one loop
boxes       the 248 004 patches of a 40 000 x 40 000 slide against the 1250 x 1250 mask: infer_wsi.select_valid (one slice and sum
            per box) and infer_wsi.select_valid_sat (table built inside the call), host clock, median of --host-reps
The device mask is compared with the host mask (==, every byte), and the two box lists with each other, before anything is timed.
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


def stat(xs, nd=4):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run(n, reps, host_reps):
    import torch

    from hover_net_amd import lib as L, tissue_mask as TM
    from hover_net_amd.synth import synth_thumbnail

    dev = torch.device("cuda", 0)
    thumb, frac = synth_thumbnail(n, n, seed=3)
    host = []
    for _ in range(host_reps):
        dt, want = clock(lambda: TM.simple_get_mask(thumb))
        host.append(dt)
    got = TM.simple_get_mask(thumb, device=dev)
    assert np.array_equal(got, want), "device and host masks differ"

    thumb_dev = torch.from_numpy(thumb).to(dev)
    gray, hist = TM.gray_hist_device(thumb_dev)
    t = TM.otsu_from_hist(hist.cpu().numpy())
    need = int(L.lib().hvn_tissue_mask_workspace_bytes(n, n))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    mask = torch.empty((n, n), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def k_gray():
        L.check(L.lib().hvn_tissue_gray_hist(thumb_dev.data_ptr(), n, n, gray.data_ptr(), hist.data_ptr(), stream), "hvn_tissue_gray_hist")

    def k_mask():
        L.check(L.lib().hvn_tissue_mask(gray.data_ptr(), n, n, t, 256, 16384, 16, mask.data_ptr(), None, None, ws.data_ptr(), need, stream),
                "hvn_tissue_mask")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    k_mask()
    assert np.array_equal(mask.cpu().numpy(), want), "hvn_tissue_mask and the host mask differ"
    legs = {"device_ms": [], "gray_hist_ms": [], "mask_ms": []}
    for it in range(reps + 2):                           # the legs alternate inside one loop; two warm-up rounds
        d = 1e3 * clock(lambda: TM.simple_get_mask(thumb, device=dev))[0]
        g = timed(k_gray)
        m = timed(k_mask)
        if it >= 2:
            legs["device_ms"].append(d)
            legs["gray_hist_ms"].append(g)
            legs["mask_ms"].append(m)
    res = {k: stat(v) for k, v in legs.items()}
    res.update({"thumbnail": [n, n], "slide": [32 * n, 32 * n], "tissue_fraction": round(frac, 4), "mask_fraction": round(float(want.mean()), 4),
                "otsu": t, "host_s": stat(host, 3), "reps": reps, "host_reps": host_reps,
                "host_over_device": round(1e3 * statistics.median(host) / statistics.median(legs["device_ms"]), 1)})
    return res, want


def boxes(mask, host_reps):
    from hover_net_amd import infer_wsi

    shape = np.array([32 * mask.shape[0], 32 * mask.shape[1]])
    _, patch = infer_wsi.get_chunk_patch_info(shape, np.array([10000, 10000]), np.array([270, 270]), np.array([80, 80]))
    loop, sat = [], []
    for _ in range(host_reps):
        dt, a = clock(lambda: infer_wsi.select_valid(patch, mask, shape))
        loop.append(dt)
        dt, b = clock(lambda: infer_wsi.select_valid_sat(patch, mask, shape))
        sat.append(dt)
        assert np.array_equal(a, b), "select_valid_sat and select_valid differ"
    return {"slide": shape.tolist(), "patches": int(patch.shape[0]), "kept": int(a.shape[0]), "select_valid_s": stat(loop, 4),
            "select_valid_sat_s": stat(sat, 4), "ratio": round(statistics.median(loop) / statistics.median(sat), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1250, 3125])
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 5 or args.host_reps < 3:
        ap.error("--reps must be at least 5 and --host-reps at least 3")
    import torch

    from hover_net_amd import lib as L

    L.require_gpu()
    rows, masks = [], {}
    for n in args.sizes:
        r, masks[n] = run(n, args.reps, args.host_reps)
        rows.append(r)
    bx = boxes(masks[args.sizes[0]], args.host_reps)
    lines = ["device tissue mask vs the host heuristic, %s and its host (%d CPUs visible), median [min .. max]: %d warm device runs, %d host runs"
             % ("%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), os.cpu_count(), args.reps, args.host_reps)]
    for r in rows:
        lines.append("thumbnail %s (slide %s)  tissue drawn %.1f %%, mask %.1f %%, Otsu %d" % ("x".join(map(str, r["thumbnail"])), "x".join(map(str, r["slide"])),
                                                                                           100 * r["tissue_fraction"], 100 * r["mask_fraction"], r["otsu"]))
        for k in ("host_s", "device_ms", "gray_hist_ms", "mask_ms"):
            lines.append("      %-13s %10.4f  [%10.4f .. %10.4f]" % (k, r[k]["median"], r[k]["min"], r[k]["max"]))
        lines.append("      host / device (end to end): %.1f" % r["host_over_device"])
    lines.append("boxes     %d patches of a %s slide, %d kept" % (bx["patches"], "x".join(map(str, bx["slide"])), bx["kept"]))
    for k in ("select_valid_s", "select_valid_sat_s"):
        lines.append("      %-19s %10.4f  [%10.4f .. %10.4f]" % (k, bx[k]["median"], bx[k]["min"], bx[k]["max"]))
    lines.append("      select_valid / select_valid_sat: %.1f" % bx["ratio"])
    lines.append(json.dumps({"tool": "tissue_mask_bench", "rows": rows, "boxes": bx}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

"""Times Macenko stain normalisation (hover_net_amd/stain.py, csrc/hvn_stain.hip) on one GPU for a 1 000^2 image and a 10 000^2
region, and prints a small table plus ONE JSON line.

    python tools/stain_bench.py [--reps 10] [--out profiles/stain_bench.txt]

Per extent (an H&E-like 500^2 texture of tests/stain_ref.py, tiled): the images' colour list is checked against np.unique and the
normalised bytes against stain.apply_host (on the 1 000^2 image; on a 1 000-row band of the region) before anything is timed.
legs (warm; one sample = the launches between two HIP events on the current stream; median of --reps samples, min and max printed)
    hist      HVN_OP_STAIN_HIST into a clear table                    -> pixels/s (every pixel is one add; merged adds reach memory)
    compact   HVN_OP_STAIN_COMPACT with the clearing flag (three launches over the 64 MB table)
    fit       stain.fit_from_counts on the host (wall clock), and the rows of its list
    apply     HVN_OP_STAIN_APPLY out of place                         -> bytes/s at 6 B per pixel
    copy      a device-to-device copy of the same bytes, timed in the same loop (6 B per pixel as well: 3 read, 3 written)
    network   the plain infer_step of cfg 2 (original, 5 types, fp32, batch 32) -> the time the network needs for the same pixels, one
              80 x 80 output per 270 x 270 patch; the sum hist + compact + fit + apply is printed as a share of it.
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
sys.path.insert(0, os.path.join(REPO, "tests"))


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import stain_ref as R
    from hover_net_amd import lib as L
    from hover_net_amd import net_desc, run_desc, stain
    from hover_net_amd import plan as PL
    from hover_net_amd.synth import synth_state_dict, synth_tiles

    L.require_gpu()
    sp = L.stream_ptr("cuda")
    run_op = L.lib().hvn_run_op

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the network's time per patch
    nb = 32
    net = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    net.load_state_dict(synth_state_dict("original", 5, seed=21), strict=True)
    net = net.to("cuda").eval()
    net.max_batch = nb
    tiles = torch.from_numpy(synth_tiles(nb, 270, seed=22)).to("cuda")
    step = [timed(lambda: run_desc.infer_step_device(tiles, net)) for _ in range(a.reps + 2)][2:]
    ms_per_patch = statistics.median(step) / nb

    texture = R.he_image(500, 500, 7)
    bins = torch.zeros(1 << 24, dtype=torch.int32, device="cuda")
    ws = torch.empty(65536, dtype=torch.uint8, device="cuda")
    status = torch.empty(2, dtype=torch.int64, device="cuda")
    out, lines = {"reps": a.reps, "step_ms_batch32": stat(step)}, []
    lines.append("Macenko stain normalisation on one GPU: ms, median [min .. max] of %d samples; plain infer_step (cfg 2, batch 32) %.3f ms = %.1f tiles/s"
                 % (a.reps, statistics.median(step), 1000.0 / ms_per_patch))
    for edge in (1000, 10000):
        img_h = np.ascontiguousarray(np.tile(texture, (edge // 500, edge // 500, 1)))
        pixels = edge * edge
        x = torch.from_numpy(img_h).to("cuda")
        y = torch.empty_like(x)
        z = torch.empty_like(x)
        cap = min(pixels, 1 << 24)
        lst = torch.empty((cap, 2), dtype=torch.int32, device="cuda")
        hist, comp, app = L.hvn_op(), L.hvn_op(), L.hvn_op()
        hist.kind = PL.OP_STAIN_HIST
        hist.x.base, hist.x.h, hist.x.w, hist.x.c, hist.y.base = x.data_ptr(), edge, edge, 3, bins.data_ptr()
        comp.kind, comp._rsv = PL.OP_STAIN_COMPACT, 1
        comp.x.base, comp.y.base, comp.y.h, comp.y2.base, comp.x2.base = bins.data_ptr(), lst.data_ptr(), cap, status.data_ptr(), ws.data_ptr()
        # the same result first
        keys, counts = stain.colour_counts_device(x)
        k_h, c_h = stain.colour_counts_host(texture)
        assert np.array_equal(keys, k_h) and np.array_equal(counts, c_h * (edge // 500) ** 2), "the device colour list differs from np.unique"
        t0 = time.perf_counter()
        fit = stain.fit_from_counts(keys, counts)
        fit_ms = (time.perf_counter() - t0) * 1000.0
        tab = stain.tables(fit)
        tab_dev = stain.tables_device(tab, "cuda")
        app.kind = PL.OP_STAIN_APPLY
        for v, t in ((app.x, x), (app.y, y)):
            v.base, v.h, v.w, v.c = t.data_ptr(), edge, edge, 3
        app.w = tab_dev.data_ptr()
        L.check(run_op(ctypes.addressof(app), 1, sp), "hvn_run_op")
        assert np.array_equal(y[:1000].cpu().numpy(), stain.apply_host(img_h[:1000], tab)), "the device apply differs from apply_host"

        legs = {"hist": lambda: L.check(run_op(ctypes.addressof(hist), 1, sp), "hvn_run_op"),
                "compact": lambda: L.check(run_op(ctypes.addressof(comp), 1, sp), "hvn_run_op"),     # clears what hist added
                "apply": lambda: L.check(run_op(ctypes.addressof(app), 1, sp), "hvn_run_op"),
                "copy": lambda: z.copy_(x)}
        samp = {k: [] for k in legs}
        for it in range(a.reps + 2):
            for k, fn in legs.items():
                ms = timed(fn)
                if it >= 2:
                    samp[k].append(ms)
        assert int(bins.count_nonzero()) == 0 and [int(v) for v in status.cpu()] == [len(keys), pixels]
        med = {k: statistics.median(v) for k, v in samp.items()}
        net_ms = pixels / 6400.0 * ms_per_patch
        total = med["hist"] + med["compact"] + fit_ms + med["apply"]
        r = {k + "_ms": stat(v) for k, v in samp.items()}
        r.update({"fit_host_ms": round(fit_ms, 3), "colours": int(len(keys)), "hist_pixels_per_s": round(pixels / med["hist"] * 1e3, 0),
                  "apply_bytes_per_s": round(6.0 * pixels / med["apply"] * 1e3, 0), "copy_bytes_per_s": round(6.0 * pixels / med["copy"] * 1e3, 0),
                  "network_ms_same_pixels": round(net_ms, 2), "share_of_network": round(total / net_ms, 5)})
        out["%dx%d" % (edge, edge)] = r
        lines.append("%d x %d (%d pixels, %d colours)" % (edge, edge, pixels, len(keys)))
        for k in ("hist", "compact", "apply", "copy"):
            s = samp[k]
            extra = {"hist": "%.3g pixels/s added" % (pixels / med["hist"] * 1e3), "compact": "64 MB table read twice, cleared",
                     "apply": "%.3g B/s at 6 B per pixel" % (6.0 * pixels / med["apply"] * 1e3),
                     "copy": "%.3g B/s at 6 B per pixel (device-to-device copy of the same bytes)" % (6.0 * pixels / med["copy"] * 1e3)}[k]
            lines.append("    %-8s %9.4f  [%9.4f .. %9.4f]   %s" % (k, med[k], min(s), max(s), extra))
        lines.append("    %-8s %9.4f   host, float64 numpy on %d rows (once)" % ("fit", fit_ms, len(keys)))
        lines.append("    hist + compact + fit + apply = %.3f ms = %.3f %% of the network's %.1f ms for the same pixels (%.0f patches)"
                     % (total, 100.0 * total / net_ms, net_ms, pixels / 6400.0))
        del x, y, z, lst
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"stain_bench": out}))


if __name__ == "__main__":
    main()

"""Times the device overlay writer (hvn_draw_overlay) against the host writer it can replace (viz.visualize_instances_dict), on one
GPU and its host, and prints a small table plus ONE JSON line.

    python tools/overlay_bench.py [--reps 30] [--out FILE]

workloads  image  one 1000 x 1000 image with 600 instances of 24 vertices (octagon-like closed contours, radius 8..14 px)
           tiles  32 images of 164 x 164 with 16 such instances each: bench.py's tile shape
Both carry a type per instance (colours from a 5-row table, no randomness) and draw the centroid dots (draw_dot=True, thickness 2).
legs (warm, median of --reps; min and max are printed too)
           device_draw_ms   viz.draw_overlay_device alone with everything in HBM: HIP events around the call (owner-map clear, mark
                            contours, mark dots, paint)
           device_path_ms   host clock from the call to the end of the copy of the overlays into pinned memory, inputs in HBM (the
                            device-resident route: image uploaded for patch extraction, contours traced on the device)
           dict_path_ms     viz.visualize_instances_dict(device=...) per image, host clock: flatten the dict, upload, draw, download --
                            what InferManager's device_overlay does today
           host_ms          viz.visualize_instances_dict per image on the host, host clock: the default path
The device and the host legs alternate inside one loop, so that drift on a shared machine hits both alike.  The overlays of all
paths are compared with == before anything is timed.  PNG encoding is part of no leg.
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

TYPE_COLOUR = {t: (str(t), c) for t, c in enumerate([(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)])}


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def synth_dicts(n, hw, per_image, vertices, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = {}
        for k in range(per_image):
            c = rng.uniform(0, hw, 2)
            ang = np.linspace(0, 2 * np.pi, vertices, endpoint=False)
            r = rng.uniform(8, 14, vertices)
            d[k + 1] = {"contour": np.stack([c[0] + r * np.cos(ang), c[1] + r * np.sin(ang)], 1).astype(np.int32), "centroid": c,
                        "type": int(rng.integers(0, 5))}
        out.append(d)
    return out


def run(name, n, hw, per_image, reps):
    import torch

    from hover_net_amd import viz

    dev = torch.device("cuda", 0)
    images = np.random.default_rng(7).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    dicts = synth_dicts(n, hw, per_image, 24, seed=11)

    def host():
        return [viz.visualize_instances_dict(images[i], dicts[i], True, TYPE_COLOUR, 2) for i in range(n)]

    def by_dict():
        return [viz.visualize_instances_dict(images[i], dicts[i], True, TYPE_COLOUR, 2, device=dev) for i in range(n)]

    # the batch's flat arrays in HBM: `per_image` slots per image
    flats = [viz.flatten_instances(d, [TYPE_COLOUR[v["type"]][1] for v in d.values()]) for d in dicts]
    pts = torch.from_numpy(np.concatenate([f[0] for f in flats], 0)).to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(np.concatenate([np.diff(f[1]) for f in flats]))]).astype(np.int64)).to(dev)
    rgba = torch.from_numpy(np.concatenate([f[2] for f in flats], 0)).to(dev)
    centres = torch.from_numpy(np.concatenate([f[3] for f in flats], 0)).to(dev)
    img_dev = torch.from_numpy(images).to(dev)
    out_dev = torch.empty_like(img_dev)
    pin = torch.empty(images.shape, dtype=torch.uint8, pin_memory=True)

    # same result first
    want = np.stack(host())
    pin.copy_(viz.draw_overlay_device(img_dev, pts, offs, rgba, centres, out=out_dev))
    assert np.array_equal(pin.numpy(), want), "device and host overlays differ"
    assert np.array_equal(np.stack(by_dict()), want), "dict route and host overlays differ"

    legs = {k: [] for k in ("device_draw_ms", "device_path_ms", "dict_path_ms", "host_ms")}
    for it in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        viz.draw_overlay_device(img_dev, pts, offs, rgba, centres, out=out_dev)
        e1.record()
        pin.copy_(out_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        by_dict()
        t2 = time.perf_counter()
        host()
        t3 = time.perf_counter()
        if it < 3:                                   # warm-up rounds
            continue
        legs["device_draw_ms"].append(e0.elapsed_time(e1))
        legs["device_path_ms"].append((t1 - t0) * 1e3)
        legs["dict_path_ms"].append((t2 - t1) * 1e3)
        legs["host_ms"].append((t3 - t2) * 1e3)
    res = {k: stat(v) for k, v in legs.items()}
    res.update({"workload": name, "images": [n, hw, hw], "instances": n * per_image, "points": int(pts.shape[0]),
                "pixels_drawn": int((want != images).any(-1).sum()), "d2h_bytes": int(images.nbytes), "reps": reps})
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
    rows = [run("image", 1, 1000, 600, args.reps), run("tiles", 32, 164, 16, args.reps)]
    lines = ["device overlay writer vs the host writer, %s, median [min .. max] ms of %d warm runs" % (torch.cuda.get_device_name(0), args.reps)]
    for r in rows:
        lines.append("%-5s %s  instances %d  points %d  pixels drawn %d" % (r["workload"], "x".join(map(str, r["images"])), r["instances"],
                                                                          r["points"], r["pixels_drawn"]))
        for k in ("device_draw_ms", "device_path_ms", "dict_path_ms", "host_ms"):
            lines.append("      %-15s %10.4f  [%10.4f .. %10.4f]" % (k, r[k]["median"], r[k]["min"], r[k]["max"]))
    lines.append(json.dumps({"tool": "overlay_bench", "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

"""Times the per-nucleus texture pass (HVN_OP_INST_TEXTURE, csrc/hvn_texture.hip) on one GPU next to the feature pass it sits beside
(hvn_instance_features with an image: the yardstick) and to its numpy host path, and prints a small table plus ONE JSON line.

    python tools/texture_bench.py [--reps 30] [--inner 10] [--out profiles/texture_bench.txt]

workload   64 maps of 164 x 164 from synth.synth_pred_maps(seed=100, k_lo=2, k_hi=8), bench.py's structured workload, post-processed on
           the device first (hvn_postproc, hvn_instance_table); what is timed starts from the instance maps, the records and the
           image in HBM.  Two images: `smooth`, a chromatin-like smooth field in a narrow band of greys (most pairs of a row land in one
           or two words: the contention the merged form is for), and `noise`, uniform random bytes (every word is hit).
legs (warm; each sample is --inner back-to-back calls between two HIP events on one stream, divided by --inner; median of --reps
samples, min and max are printed too)
           range / fixed            the op as the package issues it: one LDS add per pair
           range_merged / fixed_merged   the other accumulation form: equal keys merged on chip before the LDS add
           features_rgb             PostProc.features with the same image, same maps, same process
           host                     texture.sums_host ("range"), numpy on the same box, wall clock, once
The GPU legs alternate inside one loop, so that drift on a shared machine hits all alike.  Before anything is timed, both forms and
both scales are compared with `sums_host` with == on every word; a difference ends the run.
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


def images(n, hw):
    from scipy import ndimage

    rng = np.random.default_rng(7)
    f = ndimage.gaussian_filter(rng.normal(size=(n, hw, hw)), (0, 3.0, 3.0))
    f = (f - f.min()) / (f.max() - f.min())
    smooth = (60 + 90 * f)[..., None] + rng.normal(scale=3.0, size=(n, hw, hw, 3)) + np.array([30.0, -10.0, 40.0])
    return {"smooth": np.clip(smooth, 0, 255).astype(np.uint8), "noise": rng.integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)}


def run(reps, inner, n=64, hw=164):
    import torch

    from hover_net_amd import post_proc as PP
    from hover_net_amd import texture as TX
    from hover_net_amd.synth import synth_pred_maps

    dev = torch.device("cuda", 0)
    pred = torch.from_numpy(synth_pred_maps(n, hw, hw, 5, seed=100, k_lo=2, k_hi=8)[0]).to(dev)
    pp = PP.PostProc(dev)
    inst = pp.separate(pred)
    rec, counts = pp.table(inst, pred, 5)
    max_inst = rec.shape[1]
    inst_h = inst.cpu().numpy()
    rec_h = rec.cpu().numpy().view(PP._REC_DTYPE).reshape(n, max_inst)
    out = {"maps": n, "hw": hw, "slots": n * max_inst, "instances": int(counts.sum()), "reps": reps, "inner": inner, "images": {}}
    for name, img_h in images(n, hw).items():
        image = torch.from_numpy(img_h).to(dev)
        t0 = time.perf_counter()
        want = {"range": TX.sums_host(inst_h, rec_h, img_h, "range")}
        host_s = time.perf_counter() - t0
        want["fixed"] = TX.sums_host(inst_h, rec_h, img_h, "fixed")
        for scale in ("range", "fixed"):
            for form in (0, 1):
                got = pp.texture(inst, rec, image, scale, form=form).cpu().numpy().view(TX.TEX_DTYPE).reshape(n, max_inst)
                assert got.tobytes() == want[scale].tobytes(), "%s, %s, form %d: the device differs from sums_host" % (name, scale, form)
        calls = {"range": lambda: pp.texture(inst, rec, image, "range"), "range_merged": lambda: pp.texture(inst, rec, image, "range", form=1),
                 "fixed": lambda: pp.texture(inst, rec, image, "fixed"), "fixed_merged": lambda: pp.texture(inst, rec, image, "fixed", form=1),
                 "features_rgb": lambda: pp.features(inst, rec, image)}
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
                if it >= 3:                               # three warm-up rounds
                    legs[k].append(e0.elapsed_time(e1) / inner)
        r = {k: stat(v) for k, v in legs.items()}
        r["host_ms"] = round(host_s * 1e3, 1)
        f = r["features_rgb"]["median"]
        r["range_over_features_rgb"] = round(r["range"]["median"] / f, 3)
        r["fixed_over_features_rgb"] = round(r["fixed"]["median"] / f, 3)
        r["merged_over_plain"] = {"range": round(r["range_merged"]["median"] / r["range"]["median"], 3),
                                  "fixed": round(r["fixed_merged"]["median"] / r["fixed"]["median"], 3)}
        r["pairs"] = int(want["range"]["glcm"].astype(np.int64).sum())
        out["images"][name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "texture_bench.txt"))
    a = ap.parse_args()
    assert a.reps >= 20, "the median is taken over at least 20 samples"
    from hover_net_amd import lib as L

    L.require_gpu()
    res = run(a.reps, a.inner)
    lines = ["HVN_OP_INST_TEXTURE vs hvn_instance_features with an image (ms per call, median [min .. max] of %d samples of %d calls each)"
             % (a.reps, a.inner),
             "%d maps of %d x %d, %d slots, %d instances; device == sums_host on every word, both scales, both forms: yes"
             % (res["maps"], res["hw"], res["hw"], res["slots"], res["instances"])]
    for name, r in res["images"].items():
        lines.append("image `%s`: %d pairs counted" % (name, r["pairs"]))
        for k, what in (("range", "scale range, one LDS add per pair (the product's form)"),
                        ("range_merged", "scale range, equal keys merged before the LDS add"), ("fixed", "scale fixed, one LDS add per pair"),
                        ("fixed_merged", "scale fixed, merged"), ("features_rgb", "hvn_instance_features with the image")):
            lines.append("    %-13s %8.4f  [%8.4f .. %8.4f]   %s" % (k, r[k]["median"], r[k]["min"], r[k]["max"], what))
        lines.append("    range / features_rgb = %.3f   fixed / features_rgb = %.3f   merged / plain = %.3f (range), %.3f (fixed)"
                     % (r["range_over_features_rgb"], r["fixed_over_features_rgb"], r["merged_over_plain"]["range"], r["merged_over_plain"]["fixed"]))
        lines.append("    %-13s %8.1f   texture.sums_host (\"range\"), numpy, once: %.0f times `range`" % ("host", r["host_ms"], r["host_ms"] / r["range"]["median"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"texture_bench": res}))


if __name__ == "__main__":
    main()

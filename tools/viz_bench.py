"""Times the run loop's picture on the device (csrc/hvn_viz.hip) against its host definition, on one GPU and its host, and what
it changes in a validation epoch and in a training step.  Prints a small table plus ONE JSON line.  Records only: no threshold.

    python tools/viz_bench.py [--reps 9] [--out FILE]

strips      8 samples with 5 types (five columns), maps 80 x 80 from 270 x 270 images and 164 x 164 from 256 x 256:
            host_ms       run_desc.viz_step_output on host arrays, host clock
            device_ms     run_desc.viz_step_output_device on device tensors (torch packing + one launch), HIP events
            kernel_ms     hvn_viz_strip alone on packed tensors (viz.strip_device into a given strip), HIP events
            to_host_ms    viz_step_output_device(...).cpu(), host clock (ends in the synchronising copy)
            the strips are compared with == first; the legs alternate inside one loop; median [min .. max] of --reps after 2 warm-ups
valid       one validation epoch of train.run_phases (phase 0, 'original' mode, 5 types) over a synthetic set of 64 patches resident
            in HBM (augment.DevicePatchLoader, batch 16: 4 steps), timed around the valid engine's run between two device syncs:
            default_image   valid_step + AccumulateRawOutput + proc_valid_step_output(image=True)
            device_viz8     valid_step_stats + DeviceValidStats(viz_samples=8)
            device_viz0     valid_step_stats + DeviceValidStats()
            one run_phases call per leg with --reps + 1 epochs; the first epoch (engine builds) is dropped
train       run_desc.train_step at batch 4 on one engine and one resident batch, default raw (five copies to the host per step: the
            parent's step) against extra_info["viz"] = "device"; host clock over 10 steps between two device syncs, per step; the two
            legs alternate; the optimizer is a no-op, so both time the same kernels on the same weights
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
os.environ.setdefault("HVN_TUNE_REPS", "1")


def stat(xs, nd=4):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def raw_inputs(n, hw, img_hw, nr_types, seed):
    rng = np.random.default_rng(seed)
    h, w = hw
    return {"img": rng.integers(0, 256, (n, *img_hw, 3)).astype(np.uint8),
            "np": (rng.integers(0, 2, (n, h, w)).astype(np.int64), rng.random((n, h, w), dtype=np.float32)),
            "hv": ((rng.random((n, h, w, 2), dtype=np.float32) * 2 - 1), (rng.random((n, h, w, 2), dtype=np.float32) * 2.4 - 1.2)),
            "tp": (rng.integers(0, nr_types + 1, (n, h, w)).astype(np.int64), rng.integers(0, nr_types + 1, (n, h, w)).astype(np.float32))}


def strips(hw, img_hw, reps):
    import torch

    from hover_net_amd import run_desc, viz

    nt, n = 5, 8
    raw = raw_inputs(n, hw, img_hw, nt, 1)
    dev = {k: (torch.tensor(v).cuda() if k == "img" else tuple(torch.tensor(a).cuda() for a in v)) for k, v in raw.items()}
    want = run_desc.viz_step_output(raw, nt)
    got = run_desc.viz_step_output_device(dev, nt)
    assert np.array_equal(got.cpu().numpy(), want), "device and host strips differ"
    pred = torch.stack([dev["tp"][1], dev["np"][1], dev["hv"][1][..., 0], dev["hv"][1][..., 1]], -1).contiguous()
    packed = (dev["img"], pred, dev["np"][0].int(), dev["hv"][0], dev["tp"][0].int())
    sel = torch.tensor([(i, i) for i in range(n)], dtype=torch.int32)
    out = torch.zeros_like(got)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    legs = {"host_ms": [], "device_ms": [], "kernel_ms": [], "to_host_ms": []}
    for it in range(reps + 2):
        t = {"host_ms": clock(lambda: run_desc.viz_step_output(raw, nt)),
             "device_ms": events(lambda: run_desc.viz_step_output_device(dev, nt)),
             "kernel_ms": events(lambda: viz.strip_device(*packed, sel.numpy(), out=out, nr_types=nt)),
             "to_host_ms": clock(lambda: run_desc.viz_step_output_device(dev, nt).cpu())}
        if it >= 2:
            for k, v in t.items():
                legs[k].append(v)
    assert np.array_equal(out.cpu().numpy(), want)
    res = {k: stat(v) for k, v in legs.items()}
    res.update({"samples": n, "nr_types": nt, "maps": list(hw), "images": list(img_hw), "strip": list(want.shape), "strip_bytes": int(want.size)})
    return res


def synthetic_patches(p, nt, seed=0):
    from hover_net_amd.synth import synth_inst_pair, synth_tiles

    out = np.zeros((p, 270, 270, 5), np.int32)
    out[..., :3] = synth_tiles(p, 270, seed=seed + 1)
    for i in range(p):
        inst = synth_inst_pair(270, 270, 40, seed=seed + i)[0].astype(np.int32)
        out[i, ..., 3] = inst
        out[i, ..., 4] = np.where(inst > 0, inst % nt + 1, 0)
    return out


def valid_epochs(reps):
    import torch

    from hover_net_amd import run_engine as RE
    from hover_net_amd import train

    mode, nt = "original", 5
    train_set, valid_set = synthetic_patches(16, nt, seed=100), synthetic_patches(64, nt, seed=200)
    times = []
    orig = RE.TriggerEngine.run

    def timed(self, state, event):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        orig(self, state, event)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))

    res = {}
    RE.TriggerEngine.run = timed
    try:
        for leg, kw in (("default_image", {"viz": 8}), ("device_viz8", {"device_valid": True, "viz": 8}), ("device_viz0", {"device_valid": True})):
            cfg = train.get_config(nt, mode)
            cfg["phase_list"] = cfg["phase_list"][:1]
            cfg["phase_list"][0]["batch_size"] = {"train": 16, "valid": 16}
            del times[:]
            hist, _net = train.run_phases(cfg, train.device_loaders(train_set, valid_set, mode, True, seed=3), nr_epochs=reps + 1,
                                          allow_random_frozen_encoder=True, **kw)
            assert len(times) == reps + 1 and all(h["valid_steps"] == 4 for h in hist)
            res[leg] = dict(stat(times[1:], 3), first_epoch_ms=round(times[0], 1))
    finally:
        RE.TriggerEngine.run = orig
    res.update({"patches": 64, "batch": 16, "steps": 4, "mode": mode, "nr_types": nt, "epochs_timed": reps})
    return res


def train_steps(reps):
    import torch

    from hover_net_amd import net_desc, run_desc
    from hover_net_amd.synth import synth_state_dict, synth_train_batch

    class NoStep:
        def step(self):
            pass

    mode, nt, n, k = "original", None, 4, 10
    net = net_desc.create_model(mode=mode, nr_types=nt, input_ch=3, freeze=False)
    net.load_state_dict(synth_state_dict(mode, nt, seed=9), strict=True)
    net = net.to("cuda")
    batch = {key: torch.from_numpy(v).cuda() for key, v in synth_train_batch(n, mode, nt, seed=31).items()}
    loss = {"np": {"bce": 1, "dice": 1}, "hv": {"mse": 1, "msge": 1}}
    infos = {"default_raw": [{"net": {"desc": net, "optimizer": NoStep(), "extra_info": {"loss": loss}}}, {}],
             "device_raw": [{"net": {"desc": net, "optimizer": NoStep(), "extra_info": {"loss": loss, "viz": "device"}}}, {}]}
    legs = {name: [] for name in infos}
    for it in range(reps + 2):
        for name, info in infos.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                run_desc.train_step(batch, info)
            torch.cuda.synchronize()
            if it >= 2:
                legs[name].append(1e3 * (time.perf_counter() - t0) / k)
    res = {name: stat(v, 3) for name, v in legs.items()}
    res.update({"batch": n, "mode": mode, "steps_per_sample": k, "samples": reps,
                "default_minus_device_ms": round(statistics.median(legs["default_raw"]) - statistics.median(legs["device_raw"]), 3)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip", nargs="*", default=[], choices=["strips", "valid", "train"])
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch

    from hover_net_amd import lib as L

    L.require_gpu()
    lines = ["run-loop picture: device against host, %s (%s) and its host (%d CPUs visible); median [min .. max] of %d warm runs"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, os.cpu_count(), args.reps)]
    result = {"tool": "viz_bench", "reps": args.reps}
    if "strips" not in args.skip:
        result["strips"] = [strips((80, 80), (270, 270), args.reps), strips((164, 164), (256, 256), args.reps)]
        for r in result["strips"]:
            lines.append("strip     %d samples, maps %s from images %s, %d types -> %s uint8 (%d bytes)"
                         % (r["samples"], "x".join(map(str, r["maps"])), "x".join(map(str, r["images"])), r["nr_types"], "x".join(map(str, r["strip"])), r["strip_bytes"]))
            for k in ("host_ms", "device_ms", "kernel_ms", "to_host_ms"):
                lines.append("      %-13s %10.4f  [%10.4f .. %10.4f]" % (k, r[k]["median"], r[k]["min"], r[k]["max"]))
    if "valid" not in args.skip:
        v = result["valid"] = valid_epochs(args.reps)
        lines.append("valid     one validation epoch of run_phases: %d resident patches, batch %d (%d steps), '%s' mode, %d types; ms per epoch"
                     % (v["patches"], v["batch"], v["steps"], v["mode"], v["nr_types"]))
        for k in ("default_image", "device_viz8", "device_viz0"):
            lines.append("      %-13s %10.3f  [%10.3f .. %10.3f]   (first epoch, with engine builds: %.1f)" % (k, v[k]["median"], v[k]["min"], v[k]["max"], v[k]["first_epoch_ms"]))
    if "train" not in args.skip:
        t = result["train"] = train_steps(args.reps)
        lines.append("train     run_desc.train_step, batch %d, '%s' mode, no-op optimizer; ms per step over %d steps between two syncs" % (t["batch"], t["mode"], t["steps_per_sample"]))
        for k in ("default_raw", "device_raw"):
            lines.append("      %-13s %10.3f  [%10.3f .. %10.3f]" % (k, t[k]["median"], t[k]["min"], t[k]["max"]))
        lines.append("      default - device (medians): %.3f ms per step" % t["default_minus_device_ms"])
    lines.append(json.dumps(result))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

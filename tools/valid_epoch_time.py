"""Times one validation epoch both ways, in one process on one resident loader, and writes a small text report.

    python tools/valid_epoch_time.py [--patches 256] [--batch 16] [--reps 7] [--out profiles/valid_stats_ab.txt]

default path   run_desc.valid_step + AccumulateRawOutput + ProcessAccumulatedRawOutput(proc_valid_step_output): every batch is
               copied to the host (images, prediction map, targets), kept for the epoch and reduced in numpy
device path    run_desc.valid_step_stats + DeviceValidStats: the statistics are accumulated on the device (valid_stats.ValidStats),
               one copy of 15 numbers per epoch
Both are wired exactly as train.run_phases wires them (device_valid=False / True) on the same synthetic-weight network (fast mode, 5
types) and the same `augment.DevicePatchLoader(mode="valid")` over `--patches` synthetic 256 x 256 patches.

Memory leg (first, device path before default path, so that the default path's arrays cannot raise the device path's figure): per path,
the bytes of raw arrays the engine holds when the epoch ends (`state.epoch_accumulated_output`) and the peak of the process's
resident set (sampled after every step and after the epoch's reduction, plus ru_maxrss where the epoch set a new high-water
mark) over its resident set just before the epoch.
Timing leg: one warm-up epoch per path, then `--reps` epochs per path, ALTERNATING the two; host clock around an epoch that ends in a
device synchronise; median, min, max and spread (max - min) per path.  The two paths' scalars are compared at the end.
"""
import argparse
import os
import resource
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def synth_patches(p, size, seed=0):
    """[p, size, size, 5] int32: random RGB, rectangular "nuclei" with instance ids and types 1..4."""
    rng = np.random.default_rng(seed)
    data = np.zeros((p, size, size, 5), np.int32)
    data[..., :3] = rng.integers(0, 256, (p, size, size, 3), dtype=np.uint8)
    for k in range(p):
        for i in range(1, 40):
            y, x = rng.integers(0, size - 24), rng.integers(0, size - 24)
            data[k, y:y + rng.integers(8, 24), x:x + rng.integers(8, 24), 3:] = (i, rng.integers(1, 5))
    return data


def rss_bytes():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def hwm_bytes():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024


def held_bytes(acc):
    seen, total = set(), 0
    for arrays in acc.values():
        for a in arrays:
            base = a
            while isinstance(getattr(base, "base", None), np.ndarray):      # list(value) holds views of the batch's array
                base = base.base
            if id(base) not in seen:
                seen.add(id(base))
                total += getattr(base, "nbytes", 0)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "valid_stats_ab.txt"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least five repeats per path")

    import torch

    from hover_net_amd import augment, net_desc, run_desc
    from hover_net_amd import run_engine as RE
    from hover_net_amd.synth import synth_state_dict
    from hover_net_amd.valid_stats import ValidStats

    if not torch.cuda.is_available():
        raise SystemExit("valid_epoch_time: no GPU -- nothing is measured without one")
    mode, nt, dev = "fast", 5, "cuda:0"
    torch.cuda.set_device(torch.device(dev))
    net = net_desc.create_model(mode=mode, nr_types=nt, input_ch=3)
    net.load_state_dict(synth_state_dict(mode, nt, seed=3), strict=True)
    net = net.to(dev).eval()
    data = synth_patches(args.patches, 256)
    loader = augment.DevicePatchLoader(data, (256, 256), (164, 164), args.batch, mode="valid", with_type=True, device=dev)
    del data
    run_info = {"net": {"desc": net}}

    def default_engine():
        eng = RE.RunEngine("valid", loader, run_desc.valid_step, run_info)
        eng.add_event_handler(RE.Events.STEP_COMPLETED, RE.AccumulateRawOutput())
        eng.add_event_handler(RE.Events.EPOCH_COMPLETED, RE.ProcessAccumulatedRawOutput(
            lambda raw: run_desc.proc_valid_step_output(raw, nr_types=nt)))
        return eng

    def device_engine():
        stats = ValidStats(nt, dev)
        eng = RE.RunEngine("valid", loader, run_desc.valid_step_stats, dict(run_info, valid_stats=stats))
        eng.add_event_handler(RE.Events.EPOCH_COMPLETED, RE.DeviceValidStats(stats))
        return eng

    def epoch(eng):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(nr_epoch=1, chained=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("validation epoch, default path vs device_valid path (tools/valid_epoch_time.py)")
    say("device: %s; mode %s, %d types, batch %d, %d patches of 256 x 256 -> %d batches, %d pixels of 164 x 164 masks per epoch"
        % (torch.cuda.get_device_name(0), mode, nt, args.batch, args.patches, len(loader), args.patches * 164 * 164))
    engines = {"device": device_engine(), "default": default_engine()}
    # ---- memory leg: device path first ------------------------------------------------------------------------------------------
    epoch(engines["device"])                # builds the inference engine (launch-form timing), loads code objects
    say()
    say("host memory over one epoch (device path measured first):")
    peak = [0]

    class SampleRss(RE.BaseCallbacks):      # after every step and, added last, after the epoch's reduction
        def run(self, state, event):
            peak[0] = max(peak[0], rss_bytes())

    for name in ("device", "default"):
        eng = engines[name]
        eng.add_event_handler(RE.Events.STEP_COMPLETED, SampleRss())
        eng.add_event_handler(RE.Events.EPOCH_COMPLETED, SampleRss())
        before, hwm0, peak[0] = rss_bytes(), hwm_bytes(), 0
        epoch(eng)
        if hwm_bytes() > hwm0:              # the process reached a new high-water mark inside this epoch (between two samples, too)
            peak[0] = max(peak[0], hwm_bytes())
        grow = max(0, peak[0] - before)
        for handlers in eng.event_handler_dict.values():
            handlers[:] = [h for h in handlers if not isinstance(h, SampleRss)]
        held = held_bytes(engines[name].state.epoch_accumulated_output)
        say("  %-8s raw arrays held at the end of the epoch: %12d bytes (%8.1f MiB); peak resident-set growth: %8.1f MiB"
            % (name, held, held / 2 ** 20, grow / 2 ** 20))
    # ---- timing leg: alternate ---------------------------------------------------------------------------------------------------
    for name in ("default", "device"):
        epoch(engines[name])                # warm-up of every shape the timed window uses
    times = {"default": [], "device": []}
    for _ in range(args.reps):
        for name in ("default", "device"):
            times[name].append(epoch(engines[name]))
    say()
    say("epoch time, %d alternating repeats after one warm-up epoch each (host clock, epoch ends in a device synchronise):" % args.reps)
    stat = {}
    for name in ("default", "device"):
        t = [x * 1e3 for x in times[name]]
        stat[name] = (statistics.median(t), min(t), max(t))
        say("  %-8s median %9.2f ms   min %9.2f   max %9.2f   spread (max - min) %8.2f ms   [%s]"
            % (name, stat[name][0], stat[name][1], stat[name][2], stat[name][2] - stat[name][1], " ".join("%.1f" % x for x in t)))
    d_med, spread = stat["device"][0] - stat["default"][0], stat["default"][2] - stat["default"][1]
    say("  device median - default median = %+.2f ms; spread of the default path = %.2f ms -> %s"
        % (d_med, spread, "within the acceptance rule (not above the default by more than its spread)" if d_med <= spread
           else "ABOVE the default path by more than its spread"))
    # ---- same answer -------------------------------------------------------------------------------------------------------------
    a, b = engines["default"].state.tracked_step_output["scalar"], engines["device"].state.tracked_step_output["scalar"]
    say()
    say("scalars of the last epoch (default | device):")
    for k in a:
        say("  %-10s %.17g | %.17g%s" % (k, a[k], b[k], "" if k == "hv_mse" or a[k] == b[k] else "   DIFFERENT"))
    n_terms = 2 * args.patches * 164 * 164
    say("  hv_mse: |difference| %.3g, bound 2 n 2^-53 want = %.3g (n = %d terms)"
        % (abs(a["hv_mse"] - b["hv_mse"]), 2.0 * n_terms * 2.0 ** -53 * a["hv_mse"], n_terms))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

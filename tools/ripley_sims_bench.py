"""Times the random-labelling test of Ripley's cross-type K (hover_net_amd/ripley.py: `sims_device`, csrc/hvn_pairs_sim.hip) on one GPU
against what a user could do without it -- relabel and run HVN_OP_NBR_PAIRS once per simulation -- and prints a small table plus ONE
JSON line.

    python tools/ripley_sims_bench.py [--reps 10] [--size 1000000] [--rmax 150] [--radii 16] [--sims 99,999] [--batches 1,2,4,8,12,16,32]
                                      [--check 20000] [--out profiles/ripley_sims_bench.txt]

Input: the synthetic slide of tools/nbr_bench_util.py (five types), `--radii` equally spaced radii up to `--rmax` (pixels), the window of
the square image that holds the points.  First `sims_device` is checked against `sims_host` with == on `--check` points and 5
simulations, in one batch and in batches of 2 (the host path is the one tests/test_ripley_sims_host.py holds to the oracle); a
difference ends the run.
legs (warm; one sample = the launches of one op between two HIP events on the current stream; median of --reps samples after 2 warm-up
rounds, min and max; the legs take turns)
    grid      HVN_OP_NBR_GRID, once per test
    pairs     HVN_OP_NBR_PAIRS on the same points: the observed counts, and the YARDSTICK -- S of these are S relabelled runs
    per batch size SB of --batches: one HVN_OP_NBR_PAIRS_SIM of SB simulations, and its two launches apart (labels: the permutation, the
              label bytes and cnt; pairs: the geometry once, SB typed adds per counted pair), per batch and per simulation
    total     per S of --sims: grid + pairs + all batches at the module's own batch size, between two events, three times
"""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from nbr_bench_util import points, stat, timed, write_out  # noqa: E402
from ripley_bench import sample  # noqa: E402


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.observed[:4] + (a.pairs_in, a.n_in), b.observed[:4] + (b.pairs_in, b.n_in)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=1000000)
    ap.add_argument("--rmax", type=float, default=150.0)
    ap.add_argument("--radii", type=int, default=16)
    ap.add_argument("--sims", default="99,999")
    ap.add_argument("--batches", default="1,2,4,8,12,16,32")
    ap.add_argument("--check", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hover_net_amd import lib as L
    from hover_net_amd import ripley as RP

    L.require_gpu()
    radii = [a.rmax * (k + 1) / a.radii for k in range(a.radii)]
    default = RP._BATCH
    out, lines = {"reps": a.reps, "batch": default}, []
    lines.append("Random-labelling test of Ripley's K on one GPU: ms, median [min .. max] of %d samples" % a.reps)

    xy, types, side = points(a.check, seed=a.check % 1000 + 3)
    window = RP.window_of((int(np.ceil(side)) + 1, int(np.ceil(side)) + 1))
    host = RP.sims_host(xy, types, radii, window, 5, sims=5, seed=7)
    for sb in (default, 2):
        RP._BATCH = sb
        assert same(RP.sims_device(xy, types, radii, window, 5, sims=5, seed=7), host), "%d points, batches of %d: the device differs from sims_host" % (a.check, sb)
    RP._BATCH = default
    lines.append("%d points, 5 simulations, in one batch and in batches of 2: device == sims_host on all six arrays: yes" % a.check)

    n = a.size
    xy, types, side = points(n, seed=n % 1000 + 3)
    window = RP.window_of((int(np.ceil(side)) + 1, int(np.ceil(side)) + 1))
    ref = None
    per_sim = {}
    lines.append("%d points in %.0f x %.0f px, %d radii up to %g px, 5 types" % (n, side, side, a.radii, a.rmax))
    for sb in (int(s) for s in a.batches.split(",")):
        RP._BATCH = sb
        q = RP.DeviceRipleySims(xy, types, radii, window, 5, sims=sb, seed=1)
        assert q.sb == sb and q.batches == 1
        res = q.run().result()
        if ref is None:
            ref = res
        assert np.array_equal(res.pairs_in[0], ref.pairs_in[0]) and np.array_equal(res.n_in[0], ref.n_in[0]), "simulation 0 depends on the batch size"
        samp = sample([("grid", q.run_grid), ("pairs", q.run_observed), ("sim", q.run_op), ("labels", lambda: q.run_op(0, 1)), ("sim_pairs", lambda: q.run_op(0, 2))], a.reps)
        q.run_op()
        assert same(q.result(), res), "the timed launches changed the result"
        med = {k: statistics.median(v) for k, v in samp.items()}
        per_sim[sb] = med["sim"] / sb
        out["batch,%d" % sb] = dict({k + "_ms": stat(v) for k, v in samp.items()}, per_sim_ms=round(per_sim[sb], 4), yardstick_ratio=round(med["pairs"] / per_sim[sb], 3))
        if sb == int(a.batches.split(",")[0]):
            for k, what in (("grid", "NBR_GRID"), ("pairs", "NBR_PAIRS, the observed counts: the yardstick per simulation")):
                lines.append("    %-14s %10.4f  [%10.4f .. %10.4f]   %s" % (k, med[k], min(samp[k]), max(samp[k]), what))
        lines.append("    SB = %-2d  sim  %10.4f  [%10.4f .. %10.4f]   labels %8.4f + pairs %8.4f; %8.4f per simulation; NBR_PAIRS / that = %.2f"
                     % (sb, med["sim"], min(samp["sim"]), max(samp["sim"]), med["labels"], med["sim_pairs"], per_sim[sb], med["pairs"] / per_sim[sb]))
        del q
    RP._BATCH = default
    best = min(per_sim, key=per_sim.get)
    lines.append("    fastest per simulation: SB = %d; the module's batch size is %d" % (best, default))
    for nsim in (int(s) for s in a.sims.split(",")):
        q = RP.DeviceRipleySims(xy, types, radii, window, 5, sims=nsim, seed=1)
        q.run()
        samp = sample([("pairs", q.run_observed), ("total", q.run)], 3)
        res = q.result()
        assert np.array_equal(res.pairs_in[0], ref.pairs_in[0]) and np.array_equal(res.observed.pairs_in, ref.observed.pairs_in)
        total, yard = statistics.median(samp["total"]), nsim * statistics.median(samp["pairs"])
        out["sims,%d" % nsim] = {"total_ms": stat(samp["total"]), "batch": q.sb, "batches": q.batches, "yardstick_ms": round(yard, 2), "ratio": round(yard / total, 3)}
        lines.append("    S = %-4d total %10.2f  [%10.2f .. %10.2f]   grid + observed + %d batches of %d; %d x NBR_PAIRS = %.2f ms: %.2f times the total"
                     % (nsim, total, min(samp["total"]), max(samp["total"]), q.batches, q.sb, nsim, yard, yard / total))
        del q
    write_out("ripley_sims_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

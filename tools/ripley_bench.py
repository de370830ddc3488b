"""Times the typed pair counts under Ripley's cross-type K (hover_net_amd/ripley.py, csrc/hvn_pairs.hip) on one GPU next to their host
path on the same box, for 10^5 and 10^6 synthetic centroids, and prints a small table plus ONE JSON line.

    python tools/ripley_bench.py [--reps 10] [--sizes 100000,1000000] [--rmax 100,150] [--radii 16] [--out profiles/ripley_bench.txt]

Input: the synthetic slide of tools/nbr_bench_util.py (about one nucleus per 20 x 20 px, 70 % uniform, 30 % in Gaussian clusters, five
types), `--radii` equally spaced radii up to each `--rmax` (pixels), the window of the square image that holds the points.  Per size
and r_max, `pairs_device` is first checked against `pairs_host` with == on all four arrays (the host path is the one
tests/test_ripley_host.py holds to the all-pairs oracle); a difference ends the run.
legs (warm; one sample = the launches of one op between two HIP events on the current stream; median of --reps samples after 2 warm-up
rounds, min and max)
    grid      HVN_OP_NBR_GRID: memset, count, three scan launches, scatter                      -> points/s
    pairs     HVN_OP_NBR_PAIRS: memset of acc, one launch                                       -> candidate tests/s (per point, the points
              in its 3 x 3 cells, counted on the host from the grid)
    query     HVN_OP_NBR_QUERY on the same points and r_max, k = 5: the SAME candidate set    -> candidate tests/s, the yardstick
    host      `pairs_host`, wall clock, once (numpy on the same box)
A last block times the op on 70 000 coincident points of one type, where every add of a wave lands on one bin.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from nbr_bench_util import candidates, points, stat, timed, write_out  # noqa: E402


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def sample(legs, reps):
    """{name: [ms] * reps} for legs = ((name, fn), ..): the legs take turns, two warm-up rounds are dropped."""
    samp = {name: [] for name, _ in legs}
    for it in range(reps + 2):
        for name, fn in legs:
            ms = timed(fn)
            if it >= 2:
                samp[name].append(ms)
    return samp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--rmax", default="100,150", help="largest radius, comma separated")
    ap.add_argument("--radii", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hover_net_amd import lib as L
    from hover_net_amd import neighbours as NB
    from hover_net_amd import ripley as RP

    L.require_gpu()

    out, lines = {"reps": a.reps}, []
    lines.append("Typed pair counts under Ripley's K on one GPU: ms, median [min .. max] of %d samples; host = pairs_host once, wall clock" % a.reps)
    for n in (int(s) for s in a.sizes.split(",")):
        xy, types, side = points(n, seed=n % 1000 + 3)
        window = RP.window_of((int(np.ceil(side)) + 1, int(np.ceil(side)) + 1))
        for rmax in (float(r) for r in a.rmax.split(",")):
            radii = [rmax * (k + 1) / a.radii for k in range(a.radii)]
            q = RP.DeviceRipley(xy, types, radii, window, 5)
            g = q.grid
            q.run_grid()
            q.run_op()
            dev = q.result()
            print("%d points, r_max = %g: device done, host running" % (n, rmax), flush=True)
            t0 = time.perf_counter()
            host = RP.pairs_host(xy, types, radii, window, 5)
            host_s = time.perf_counter() - t0
            assert same(dev, host), "%d points, r_max %g: the device's counts differ from pairs_host's" % (n, rmax)
            nq = NB.DeviceQuery(xy, types, rmax, 5, 5)
            nq.run_grid()
            nq.run_op()
            samp = sample([("grid", q.run_grid), ("pairs", q.run_op), ("query", nq.run_op)], a.reps)
            assert same(q.result(), host), "the timed launches changed the result"
            med = {name: statistics.median(v) for name, v in samp.items()}
            tests = candidates(xy, g)
            counted = int(host.pairs[:, :, -1].sum())
            out["%d,%g" % (n, rmax)] = dict({name + "_ms": stat(v) for name, v in samp.items()}, host_s=round(host_s, 2), equal=True, cells=[g.ncy, g.ncx],
                                            cell_side=g.c, radii=a.radii, candidate_tests=tests, counted_pairs=counted,
                                            pairs_tests_per_s=round(tests / med["pairs"] * 1e3, 0), query_tests_per_s=round(tests / med["query"] * 1e3, 0))
            lines.append("%d points in %.0f x %.0f px, %d radii up to %g px, 5 types, %d x %d cells of %.4f px; %d candidate tests, %d counted pairs; device == host on all four arrays: yes"
                         % (n, side, side, a.radii, rmax, g.ncy, g.ncx, g.c, tests, counted))
            lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %.3g points/s" % ("grid", med["grid"], min(samp["grid"]), max(samp["grid"]), n / med["grid"] * 1e3))
            for name, what in (("pairs", "NBR_PAIRS"), ("query", "NBR_QUERY, k = 5, same points and r_max")):
                lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %s: %.3g candidate tests per second" % (name, med[name], min(samp[name]), max(samp[name]), what, tests / med[name] * 1e3))
            lines.append("    %-8s %10.1f   pairs_host, numpy (once): %.0f times grid + pairs; pairs / query = %.2f"
                         % ("host", host_s * 1e3, host_s * 1e3 / (med["grid"] + med["pairs"]), med["pairs"] / med["query"]))
            del q, nq
    # the worst case for same-address adds: one spot, one type
    n = 70000
    xy = np.tile([[40.0, 30.0]], (n, 1))
    q = RP.DeviceRipley(xy, None, [2.0, 5.0], (0.0, 0.0, 100.0, 50.0))
    q.run_grid()
    q.run_op()
    assert q.result().pairs.tolist() == [[[n * (n - 1)] * 2]], "coincident points: not N (N - 1)"
    samp = sample([("pairs", q.run_op)], a.reps)["pairs"]
    out["coincident,%d" % n] = {"pairs_ms": stat(samp)}
    lines.append("%d coincident points of one type: %d candidate tests, every add on one bin; == N (N - 1): yes" % (n, n * n))
    lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %.3g candidate tests per second" % ("pairs", statistics.median(samp), min(samp), max(samp), n * n / statistics.median(samp) * 1e3))
    write_out("ripley_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

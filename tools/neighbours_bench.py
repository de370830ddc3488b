"""Times the neighbour search (hover_net_amd/neighbours.py, csrc/hvn_neighbours.hip) on one GPU next to its host path on the same
box, for 10^5 and 10^6 synthetic centroids, and prints a small table plus ONE JSON line.

    python tools/neighbours_bench.py [--reps 10] [--sizes 100000,1000000] [--out profiles/neighbours_bench.txt]

Input: tissue-like density, about one nucleus per 20 x 20 px -- 70 % of the points uniform over a square of side 20 sqrt(N), 30 % in
Gaussian clusters (sigma 40 px, 200 points each), five types; radius = 100 px, k = 5.  Per size, `query_device` is first checked
against `query_host` with == on all three arrays (the host path is the one tests/test_neighbours_host.py holds to the O(N^2) oracle);
a difference ends the run.
legs (warm; one sample = the launches of one op between two HIP events on the current stream; median of --reps samples, min and max)
    grid      HVN_OP_NBR_GRID: memset, count, three scan launches, scatter           -> points/s
    query     HVN_OP_NBR_QUERY                                                       -> points/s and distance tests/s (the candidates of
              the 3 x 3 cells of every point, counted on the host from the grid)
    host      `query_host`, wall clock, once (numpy on the same box)
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

from nbr_bench_util import TYPES, candidates, points, stat, timed, write_out  # noqa: E402

RADIUS, K = 100.0, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hover_net_amd import lib as L
    from hover_net_amd import neighbours as NB

    L.require_gpu()

    out, lines = {"reps": a.reps, "radius": RADIUS, "k": K, "types": TYPES}, []
    lines.append("Neighbour search on one GPU, radius %g px, k = %d, %d types: ms, median [min .. max] of %d samples; host = query_host once, wall clock"
                 % (RADIUS, K, TYPES, a.reps))
    for n in (int(s) for s in a.sizes.split(",")):
        xy, types, side = points(n, seed=n % 1000 + 3)
        q = NB.DeviceQuery(xy, types, RADIUS, K, TYPES)
        g = q.grid
        q.run_grid()
        q.run_op()
        dev = q.result()
        print("%d points: device done, host running" % n, flush=True)
        t0 = time.perf_counter()
        host = NB.query_host(xy, types, RADIUS, K, TYPES)
        host_s = time.perf_counter() - t0
        for name in ("count", "knn", "nearest_of_type"):
            assert np.array_equal(dev[name], host[name]), "%d points: the device's %s differs from query_host's" % (n, name)
        samp = {"grid": [], "query": []}
        for it in range(a.reps + 2):
            for name, fn in (("grid", q.run_grid), ("query", q.run_op)):
                ms = timed(fn)
                if it >= 2:
                    samp[name].append(ms)
        again = q.result()
        assert all(np.array_equal(again[name], host[name]) for name in host), "the timed launches changed the result"
        med = {name: statistics.median(v) for name, v in samp.items()}
        tests = candidates(xy, g)
        mean_nb = float(host["count"].sum(1).mean())
        out[str(n)] = {"grid_ms": stat(samp["grid"]), "query_ms": stat(samp["query"]), "host_s": round(host_s, 2), "equal": True, "cells": [g.ncy, g.ncx],
                       "cell_side": g.c, "mean_neighbours": round(mean_nb, 2), "max_neighbours": int(host["count"].sum(1).max()), "distance_tests": tests,
                       "query_points_per_s": round(n / med["query"] * 1e3, 0), "query_tests_per_s": round(tests / med["query"] * 1e3, 0)}
        lines.append("%d points in %.0f x %.0f px, %d x %d cells of %.4f px; %.1f neighbours per point on average, %d at most; device == host: yes"
                     % (n, side, side, g.ncy, g.ncx, g.c, mean_nb, int(host["count"].sum(1).max())))
        lines.append("    %-6s %10.4f  [%10.4f .. %10.4f]   %.3g points/s" % ("grid", med["grid"], min(samp["grid"]), max(samp["grid"]), n / med["grid"] * 1e3))
        lines.append("    %-6s %10.4f  [%10.4f .. %10.4f]   %.3g points/s, %.3g distance tests/s (%d tests in the 3 x 3 cells)"
                     % ("query", med["query"], min(samp["query"]), max(samp["query"]), n / med["query"] * 1e3, tests / med["query"] * 1e3, tests))
        lines.append("    %-6s %10.1f   query_host, numpy (once): %.0f times grid + query" % ("host", host_s * 1e3, host_s * 1e3 / (med["grid"] + med["query"])))
        del q
    write_out("neighbours_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

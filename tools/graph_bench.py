"""Times the cell graph (hover_net_amd/graph.py, csrc/hvn_graph.hip) on one GPU next to its host path on the same box, for 10^6
synthetic centroids, and prints a small table plus ONE JSON line.

    python tools/graph_bench.py [--reps 10] [--sizes 1000000] [--radius 75] [--out profiles/graph_bench.txt]

Input: the slide-like points of tools/nbr_bench_util.py (about one nucleus per 20 x 20 px, 30 % of them in Gaussian clusters); radius =
75 px, inside the 50 - 100 px that cell-graph work uses at 40x.  Per size, `gabriel_device` is first checked against `gabriel_host` with
== on indptr and indices (the host path is the one tests/test_graph_host.py holds to the all-k oracle); a difference ends the run.
legs (warm; one sample = the launches of one leg between two HIP events on the current stream; median of --reps samples, min and max)
    grid      HVN_OP_NBR_GRID: memset, count, three scan launches, scatter                         -> points/s
    count     HVN_OP_NBR_GRAPH, mode 0, with its table of 16 slots per point: degree[N] and first[N][16]   -> triples/s (below)
    cumsum    torch.cumsum of degree into indptr on the device (the readback of E and of the largest degree is not in it)
    compact   the table's used part gathered into `indices` by a boolean mask (torch; it synchronises once for the size)
    count0    HVN_OP_NBR_GRAPH, mode 0, without the table: degree[N] only                          -> triples/s
    fill      HVN_OP_NBR_GRAPH, mode 1, after count0: the same search again, the rows' positions stored   -> triples/s
              count0 + cumsum + fill is the form that DESIGN.md section 8 weighs against count + cumsum + compact; it is also what a
              graph with a degree above 16 takes after its count
    query     HVN_OP_NBR_QUERY on the same grid, k = 5, untyped: the yardstick for the same staging   -> distance tests/s
    host      `gabriel_host`, wall clock, once (numpy on the same box)
A TRIPLE is one (i, j, k) of the definition with j and k neighbours of i: sum over i of n_i^2, n_i the neighbours of i.  The kernel
leaves a pair at its first blocker, so it forms the dot product of only a part of them: triples/s is the rate at which the
neighbourhoods are DISPOSED of, not a count of multiplications.
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

K, WIDTH = 5, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1000000")
    ap.add_argument("--radius", type=float, default=75.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from hover_net_amd import graph as GR
    from hover_net_amd import lib as L
    from hover_net_amd import neighbours as NB

    L.require_gpu()
    radius = a.radius
    out, lines = {"reps": a.reps, "radius": radius, "list_cap": GR.LIST_CAP}, []
    lines.append("Cell graph (Gabriel edges of length <= r) on one GPU, radius %g px: ms, median [min .. max] of %d samples; host = gabriel_host once, wall clock"
                 % (radius, a.reps))
    for n in (int(s) for s in a.sizes.split(",")):
        xy, _types, side = points(n, seed=n % 1000 + 3)
        q = GR.DeviceGraph(xy, radius)
        g = q.grid
        dev = q.run().result()
        nq = NB.DeviceQuery(xy, None, radius, K)
        per_point = nq.run().result()["count"].sum(1).astype(np.int64)
        print("%d points: device done, host running" % n, flush=True)
        t0 = time.perf_counter()
        host = GR.gabriel_host(xy, radius)
        host_s = time.perf_counter() - t0
        assert np.array_equal(dev.indptr, host.indptr) and np.array_equal(dev.indices, host.indices), "%d points: the device's graph differs from gabriel_host's" % n
        assert q.from_table and q.width == WIDTH, "a degree above %d: the table form does not apply to this input" % WIDTH
        two = GR.DeviceGraph(xy, radius, width=0)                # the form without the table: count, then fill
        plain = two.run().result()
        assert not two.from_table and np.array_equal(plain.indptr, host.indptr) and np.array_equal(plain.indices, host.indices), "count + fill differs from gabriel_host"
        cumsum = lambda: torch.cumsum(q.degree, 0, dtype=torch.int64, out=q.indptr[1:])  # noqa: E731
        legs = [("grid", q.run_grid), ("count", q.run_op), ("cumsum", cumsum), ("compact", q.compact), ("count0", two.run_op), ("fill", two.run_fill), ("query", nq.run_op)]
        samp = {name: [] for name, _ in legs}
        for it in range(a.reps + 2):
            for name, fn in legs:
                ms = timed(fn)
                if it >= 2:
                    samp[name].append(ms)
        for d in (q, two):
            again = d.prepare_fill().result() if d is q else d.result()
            assert np.array_equal(again.indptr, host.indptr) and np.array_equal(again.indices, host.indices), "the timed launches changed the result"
        deg = GR.degree(host)
        med = {name: statistics.median(v) for name, v in samp.items()}
        e, triples, tests = int(host.indptr[-1]), int((per_point * per_point).sum()), candidates(xy, g)
        slow = int((per_point > GR.LIST_CAP).sum())
        out[str(n)] = dict({name + "_ms": stat(v) for name, v in samp.items()}, host_s=round(host_s, 2), equal=True, cells=[g.ncy, g.ncx], cell_side=g.c,
                           directed_edges=e, mean_degree=round(e / n, 3), max_degree=int(deg.max()), mean_neighbours=round(float(per_point.mean()), 2),
                           max_neighbours=int(per_point.max()), slow_path_points=slow, triples=triples, distance_tests=tests,
                           count_triples_per_s=round(triples / med["count"] * 1e3, 0), fill_triples_per_s=round(triples / med["fill"] * 1e3, 0))
        table_ms, two_ms = med["count"] + med["cumsum"] + med["compact"], med["count0"] + med["cumsum"] + med["fill"]
        lines.append("%d points in %.0f x %.0f px, %d x %d cells of %.4f px; E = %d directed edges, degree %.2f on average, %d at most; %.1f neighbours per point on average, %d at most (%d points above the on-chip list of %d); device == host: yes"
                     % (n, side, side, g.ncy, g.ncx, g.c, e, e / n, int(deg.max()), float(per_point.mean()), int(per_point.max()), slow, GR.LIST_CAP))
        row = "    %-8s %10.4f  [%10.4f .. %10.4f]   "
        lines.append((row + "%.3g points/s") % ("grid", med["grid"], min(samp["grid"]), max(samp["grid"]), n / med["grid"] * 1e3))
        for name, what in (("count", "NBR_GRAPH count with the table of %d slots per point" % WIDTH), ("count0", "NBR_GRAPH count without the table"),
                           ("fill", "NBR_GRAPH fill")):
            lines.append((row + "%s: %.3g triples/s (%d triples = sum of n_i^2; the early exit skips a part of their dot tests)")
                         % (name, med[name], min(samp[name]), max(samp[name]), what, triples / med[name] * 1e3, triples))
        lines.append((row + "torch.cumsum of degree into indptr") % ("cumsum", med["cumsum"], min(samp["cumsum"]), max(samp["cumsum"])))
        lines.append((row + "the table's used part gathered into indices (torch)") % ("compact", med["compact"], min(samp["compact"]), max(samp["compact"])))
        lines.append("    count + cumsum + compact = %.4f ms (the form in use); count0 + cumsum + fill = %.4f ms (without the table): the first / the second = %.2f"
                     % (table_ms, two_ms, table_ms / two_ms))
        lines.append((row + "NBR_QUERY, k = 5, untyped, same grid: %.3g distance tests/s (%d tests in the 3 x 3 cells); count / this = %.2f")
                     % ("query", med["query"], min(samp["query"]), max(samp["query"]), tests / med["query"] * 1e3, tests, med["count"] / med["query"]))
        lines.append("    %-8s %10.1f   gabriel_host, numpy (once): %.0f times grid + count + cumsum + compact"
                     % ("host", host_s * 1e3, host_s * 1e3 / (med["grid"] + table_ms)))
        del q, nq, two
    write_out("graph_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

"""Times the nucleus density map (hover_net_amd/density.py, csrc/hvn_density.hip) on one GPU next to its host path on the same box, for
10^5 and 10^6 synthetic centroids, and prints a small table plus ONE JSON line.

    python tools/density_bench.py [--reps 10] [--sizes 100000,1000000] [--params 100:32,150:64] [--out profiles/density_bench.txt]

Input: the synthetic slide of tools/nbr_bench_util.py (about one nucleus per 20 x 20 px, 70 % uniform, 30 % in Gaussian clusters, five
types) and the pipeline raster over it (`density.raster_of`: one node per step x step pixels).  Parameters radius:step in pixels.  Per
size and parameter set, `density_device` is first checked against `density_host` with == on the whole array (the host path is the one
tests/test_density_host.py holds to the all-pairs oracle); a difference ends the run.
legs (warm; one sample = the launches of one op between two HIP events on the current stream; median of --reps samples, min and max)
    grid      HVN_OP_NBR_GRID: memset, count, three scan launches, scatter                      -> points/s
    density   HVN_OP_NBR_DENSITY: one launch                                                    -> nodes/s and distance tests/s (per node,
              the points in the 3 x 3 cells around its clamped cell, counted on the host from the grid)
    query     HVN_OP_NBR_QUERY on the same points and radius, k = 5                             -> distance tests/s (per point, the points
              in its 3 x 3 cells), for comparison
    host      `density_host`, wall clock, once (numpy on the same box)
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


def node_tests(xy, g, raster):
    """Distance tests the 3 x 3 search of every node needs: per node, the points in the nine cells around its clamped cell."""
    from hover_net_amd import density as DN
    from hover_net_amd import neighbours as NB

    cx, cy = NB.cells(xy, g)
    per = np.zeros((g.ncy + 2, g.ncx + 2), np.int64)
    np.add.at(per, (cy + 1, cx + 1), 1)
    box = sum(per[1 + dy:g.ncy + 1 + dy, 1 + dx:g.ncx + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    px, py = DN.nodes(raster)
    ncx_, _ = NB.cells(np.stack([px, np.full_like(px, g.y0)], 1), g)
    _, ncy_ = NB.cells(np.stack([np.full_like(py, g.x0), py], 1), g)
    return int(box[ncy_[:, None], ncx_[None, :]].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--params", default="100:32,150:64", help="radius:step, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hover_net_amd import density as DN
    from hover_net_amd import lib as L
    from hover_net_amd import neighbours as NB

    L.require_gpu()

    out, lines = {"reps": a.reps}, []
    lines.append("Nucleus density maps on one GPU: ms, median [min .. max] of %d samples; host = density_host once, wall clock" % a.reps)
    for n in (int(s) for s in a.sizes.split(",")):
        xy, types, side = points(n, seed=n % 1000 + 3)
        for radius, step in ((float(p.split(":")[0]), int(p.split(":")[1])) for p in a.params.split(",")):
            raster = DN.raster_of((int(np.ceil(side)), int(np.ceil(side))), step)
            q = DN.DeviceDensity(xy, types, radius, raster, 5)
            g, raster = q.grid, q.raster
            q.run_grid()
            q.run_op()
            dev = q.result()
            print("%d points, r = %g, step = %d: device done, host running" % (n, radius, step), flush=True)
            t0 = time.perf_counter()
            host = DN.density_host(xy, types, radius, raster, 5)
            host_s = time.perf_counter() - t0
            assert dev.dtype == host.dtype and np.array_equal(dev, host), "%d points: the device's count differs from density_host's" % n
            nq = NB.DeviceQuery(xy, types, radius, 5, 5)
            nq.run_grid()
            nq.run_op()
            samp = {"grid": [], "density": [], "query": []}
            for it in range(a.reps + 2):
                for name, fn in (("grid", q.run_grid), ("density", q.run_op), ("query", nq.run_op)):
                    ms = timed(fn)
                    if it >= 2:
                        samp[name].append(ms)
            assert np.array_equal(q.result(), host), "the timed launches changed the result"
            med = {name: statistics.median(v) for name, v in samp.items()}
            tests, qtests, nodes = node_tests(xy, g, raster), candidates(xy, g), raster.W * raster.H
            out["%d,%g,%d" % (n, radius, step)] = dict(
                grid_ms=stat(samp["grid"]), density_ms=stat(samp["density"]), query_ms=stat(samp["query"]), host_s=round(host_s, 2), equal=True,
                cells=[g.ncy, g.ncx], cell_side=g.c, raster=[raster.H, raster.W], counted=int(host.sum()), distance_tests=tests,
                density_tests_per_s=round(tests / med["density"] * 1e3, 0), query_distance_tests=qtests, query_tests_per_s=round(qtests / med["query"] * 1e3, 0))
            lines.append("%d points in %.0f x %.0f px, radius %g px, step %d px: %d x %d nodes, 5 types, %d x %d cells of %.4f px; mean count per node %.1f; device == host on count: yes"
                         % (n, side, side, radius, step, raster.H, raster.W, g.ncy, g.ncx, g.c, float(host.sum()) / nodes))
            lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %.3g points/s" % ("grid", med["grid"], min(samp["grid"]), max(samp["grid"]), n / med["grid"] * 1e3))
            lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %.3g nodes/s; %d candidate tests in the nodes' 3 x 3 cells, %.3g per second"
                         % ("density", med["density"], min(samp["density"]), max(samp["density"]), nodes / med["density"] * 1e3, tests, tests / med["density"] * 1e3))
            lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   NBR_QUERY, k = 5, same points and radius: %d candidate tests, %.3g per second"
                         % ("query", med["query"], min(samp["query"]), max(samp["query"]), qtests, qtests / med["query"] * 1e3))
            lines.append("    %-8s %10.1f   density_host, numpy (once): %.0f times grid + density" % ("host", host_s * 1e3, host_s * 1e3 / (med["grid"] + med["density"])))
            del q, nq
    write_out("density_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

"""Times nuclei-in-regions (hover_net_amd/regions.py, csrc/hvn_regions.hip) on one GPU next to its host path on the same box, for 10^6
synthetic centroids against about 200 irregular regions of about 500 vertices, and prints a small table plus ONE JSON line.

    python tools/regions_bench.py [--reps 10] [--sizes 1000000] [--regions 200] [--vertices 500] [--cells 20,40,80] [--out profiles/regions_bench.txt]

Input: the synthetic slide of tools/nbr_bench_util.py (about one nucleus per 20 x 20 px, 70 % uniform, 30 % in Gaussian clusters, five
types) and star-shaped regions with a smoothly varying radius of 2 to 10 % of the slide's side, scattered over it (they overlap).
`regions_device` is first checked against `regions_host` with == on all three arrays (the host path is the one
tests/test_regions_host.py holds to the all-edges oracle); a difference ends the run.
legs (warm; one sample = the launches of one op between two HIP events on the current stream; median of --reps samples after 2 warm-up
rounds, min and max)
    grid      HVN_OP_NBR_GRID: memset, count, three scan launches, scatter                      -> points/s
    regions   HVN_OP_NBR_REGIONS: memset of count, one launch                                   -> edge tests/s (per point, the entries of its
              row's list, counted on the host)
    pairs     HVN_OP_NBR_PAIRS on the same points, 16 radii up to 150 px                        -> candidate tests/s, the yardstick
    host      `regions_host`, wall clock, once (numpy on the same box)
then the same op at every cell side of --cells and with ONE row (the brute-force form: every point against every edge), each checked
against the first result.
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


def blobs(n_regions, n_vertices, side, seed):
    """Irregular star-shaped regions: the radius of vertex k is a base radius (2 to 10 % of the side) times a smooth factor in
    [0.6, 1.4]."""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n_vertices) / n_vertices
    regs = []
    for _ in range(n_regions):
        cx, cy = rng.random(2) * side
        base = side * (0.02 + 0.08 * rng.random())
        f = 1.0 + sum(0.4 / 3 * np.sin((h + 2) * a + rng.random() * 6.28) for h in range(3))
        regs.append([[np.stack([cx + base * f * np.cos(a), cy + base * f * np.sin(a)], 1)]])
    return regs


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def sample(legs, reps):
    """{name: [ms] * reps} for legs = ((name, fn), ..): the legs take turns, two warm-up rounds are dropped."""
    samp = {name: [] for name, _ in legs}
    for it in range(reps + 2):
        for name, fn in legs:
            ms = timed(fn)
            if it >= 2:
                samp[name].append(ms)
    return samp


def edge_tests(xy, q, RG):
    """Point-edge tests of a DeviceRegions: per point, the length of its row's list."""
    row_start, _ = RG.bin_rows(xy, q.rs, q.grid)
    per_row = np.bincount(RG._rows_of(xy[:, 1], q.grid), minlength=q.grid.ncy)
    return int((per_row * np.diff(row_start.astype(np.int64))).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1000000")
    ap.add_argument("--regions", type=int, default=200)
    ap.add_argument("--vertices", type=int, default=500)
    ap.add_argument("--cells", default="20,40,80", help="further cell sides to time, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hover_net_amd import lib as L
    from hover_net_amd import regions as RG
    from hover_net_amd import ripley as RP

    L.require_gpu()

    out, lines = {"reps": a.reps}, []
    lines.append("Nuclei in annotated regions on one GPU: ms, median [min .. max] of %d samples; host = regions_host once, wall clock" % a.reps)
    for n in (int(s) for s in a.sizes.split(",")):
        xy, types, side = points(n, seed=n % 1000 + 5)
        rs = RG.RegionSet.from_polygons(blobs(a.regions, a.vertices, side, 7))
        ne = rs.edges.shape[0]
        q = RG.DeviceRegions(xy, types, rs, 5)
        g = q.grid
        q.run_grid()
        q.run_op()
        dev = q.result()
        print("%d points, %d edges: device done, host running" % (n, ne), flush=True)
        t0 = time.perf_counter()
        host = RG.regions_host(xy, types, rs, 5)
        host_s = time.perf_counter() - t0
        assert same(dev, host), "%d points: the device's result differs from regions_host's" % n
        radii = [150.0 * (k + 1) / 16 for k in range(16)]
        pq = RP.DeviceRipley(xy, types, radii, RP.window_of((int(np.ceil(side)) + 1, int(np.ceil(side)) + 1)), 5)
        pq.run_grid()
        pq.run_op()
        samp = sample([("grid", q.run_grid), ("regions", q.run_op), ("pairs", pq.run_op)], a.reps)
        assert same(q.result(), host), "the timed launches changed the result"
        med = {name: statistics.median(v) for name, v in samp.items()}
        tests, ptests = edge_tests(xy, q, RG), candidates(xy, pq.grid)
        key = "%d" % n
        out[key] = dict({name + "_ms": stat(v) for name, v in samp.items()}, host_s=round(host_s, 2), equal=True, rows=g.ncy, cell_side=g.c, regions=len(rs),
                        edges=ne, entries=q.entries, edge_tests=tests, inside=int(host.hits.sum()), regions_tests_per_s=round(tests / med["regions"] * 1e3, 0),
                        pairs_candidate_tests=ptests, pairs_tests_per_s=round(ptests / med["pairs"] * 1e3, 0))
        lines.append("%d points in %.0f x %.0f px, 5 types, %d regions of %d edges in all; %d rows of %.4f px, %d list entries, %d edge tests, %d memberships; device == host on all three arrays: yes"
                     % (n, side, side, len(rs), ne, g.ncy, g.c, q.entries, tests, int(host.hits.sum())))
        lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %.3g points/s" % ("grid", med["grid"], min(samp["grid"]), max(samp["grid"]), n / med["grid"] * 1e3))
        lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   NBR_REGIONS: %.3g edge tests per second" % ("regions", med["regions"], min(samp["regions"]), max(samp["regions"]), tests / med["regions"] * 1e3))
        lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   NBR_PAIRS, 16 radii up to 150 px, same points: %d candidate tests, %.3g per second"
                     % ("pairs", med["pairs"], min(samp["pairs"]), max(samp["pairs"]), ptests, ptests / med["pairs"] * 1e3))
        lines.append("    %-8s %10.1f   regions_host, numpy (once): %.0f times grid + regions" % ("host", host_s * 1e3, host_s * 1e3 / (med["grid"] + med["regions"])))
        del pq
        forms = [("cell %g" % float(c), float(c)) for c in a.cells.split(",") if c] + [("one row", 4.0 * side)]
        for label, cell in forms:
            f = RG.DeviceRegions(xy, types, rs, 5, cell=cell)
            f.run_grid()
            f.run_op()
            assert same(f.result(), host), "%s: the result differs" % label
            ms = sample([("regions", f.run_op)], 3 if label == "one row" else a.reps)["regions"]
            ft = edge_tests(xy, f, RG)
            out[key][label] = {"rows": f.grid.ncy, "cell_side": f.grid.c, "entries": f.entries, "edge_tests": ft, "regions_ms": stat(ms)}
            lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %s: %d rows of %.4f px, %d entries, %d edge tests, %.3g per second; same integers: yes"
                         % ("regions", statistics.median(ms), min(ms), max(ms), label, f.grid.ncy, f.grid.c, f.entries, ft, ft / statistics.median(ms) * 1e3))
            del f
        del q
    write_out("regions_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

"""Times the nucleus clustering (hover_net_amd/clusters.py, csrc/hvn_clusters.hip) on one GPU next to its host path on the same box, for
10^5 and 10^6 synthetic centroids, and prints a small table plus ONE JSON line.

    python tools/clusters_bench.py [--reps 10] [--sizes 100000,1000000] [--params 100:10,25:10] [--out profiles/clusters_bench.txt]

Input: the synthetic slide of tools/nbr_bench_util.py (about one nucleus per 20 x 20 px, 70 % uniform, 30 % in Gaussian clusters).
Parameters: radius 100 px, min_pts 10 (at 125 neighbours per point nearly every point is a core and the slide is ONE cluster: every
union ends on one root, the most contended case of the union-find), and radius 25 px, min_pts 10 (only the Gaussian clusters are dense
enough: thousands of clusters, borders and noise).  Per size and parameter set, `cluster_device` is first checked against `cluster_host`
with == on both arrays (the host path is the one tests/test_clusters_host.py holds to the O(N^2) oracle); a difference ends the run.
legs (warm; one sample = the launches of one op between two HIP events on the current stream; median of --reps samples, min and max)
    grid      HVN_OP_NBR_GRID: memset, count, three scan launches, scatter                      -> points/s
    cluster   HVN_OP_NBR_CLUSTER: degree, link, roots, assign                                  -> points/s and distance tests/s (the
              candidates of the 3 x 3 cells of every point, counted on the host from the grid; the degree pass makes all of them, the
              link pass at most half, the assign pass those of the border points)
    host      `cluster_host`, wall clock, once (numpy on the same box)
    sklearn   sklearn.cluster.DBSCAN(eps, min_samples).fit, wall clock, once, where the library is installed and N <= --sklearn-max
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--params", default="100:10,25:10", help="radius:min_pts, comma separated")
    ap.add_argument("--sklearn-max", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hover_net_amd import clusters as CL
    from hover_net_amd import lib as L

    L.require_gpu()
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None

    out, lines = {"reps": a.reps}, []
    lines.append("Nucleus clusters (DBSCAN) on one GPU: ms, median [min .. max] of %d samples; host = cluster_host once, wall clock" % a.reps)
    for n in (int(s) for s in a.sizes.split(",")):
        xy, _types, side = points(n, seed=n % 1000 + 3)
        for radius, min_pts in ((float(p.split(":")[0]), int(p.split(":")[1])) for p in a.params.split(",")):
            q = CL.DeviceClusters(xy, None, radius, min_pts)
            g = q.grid
            q.run_grid()
            q.run_op()
            dev = q.result()
            print("%d points, r = %g, m = %d: device done, host running" % (n, radius, min_pts), flush=True)
            t0 = time.perf_counter()
            host = CL.cluster_host(xy, None, radius, min_pts)
            host_s = time.perf_counter() - t0
            for name in ("label", "degree"):
                assert np.array_equal(dev[name], host[name]), "%d points: the device's %s differs from cluster_host's" % (n, name)
            samp = {"grid": [], "cluster": []}
            for it in range(a.reps + 2):
                for name, fn in (("grid", q.run_grid), ("cluster", q.run_op)):
                    ms = timed(fn)
                    if it >= 2:
                        samp[name].append(ms)
            again = q.result()
            assert all(np.array_equal(again[name], host[name]) for name in host), "the timed launches changed the result"
            med = {name: statistics.median(v) for name, v in samp.items()}
            tests = candidates(xy, g)
            label, degree = host["label"], host["degree"]
            core = degree >= min_pts
            ids, sizes = np.unique(label[label >= 0], return_counts=True)
            census = {"clusters": int(ids.shape[0]), "cores": int(core.sum()), "borders": int((~core & (label >= 0)).sum()),
                      "noise": int((label < 0).sum()), "largest": int(sizes.max()) if sizes.shape[0] else 0}
            sk_s = None
            if DBSCAN is not None and n <= a.sklearn_max:
                t0 = time.perf_counter()
                db = DBSCAN(eps=radius, min_samples=min_pts).fit(xy)
                sk_s = time.perf_counter() - t0
                census["sklearn_same_cores"] = bool(np.array_equal(np.sort(db.core_sample_indices_), np.nonzero(core)[0]))
            out["%d,%g,%d" % (n, radius, min_pts)] = dict(
                census, grid_ms=stat(samp["grid"]), cluster_ms=stat(samp["cluster"]), host_s=round(host_s, 2), sklearn_s=None if sk_s is None else round(sk_s, 2),
                equal=True, cells=[g.ncy, g.ncx], cell_side=g.c, mean_degree=round(float(degree.mean()), 2), distance_tests=tests,
                cluster_points_per_s=round(n / med["cluster"] * 1e3, 0))
            lines.append("%d points in %.0f x %.0f px, radius %g px, min_pts %d, %d x %d cells of %.4f px; mean degree %.1f; device == host on label and degree: yes"
                         % (n, side, side, radius, min_pts, g.ncy, g.ncx, g.c, float(degree.mean())))
            lines.append("    %d clusters (largest %d), %d cores, %d borders, %d noise" % (census["clusters"], census["largest"], census["cores"], census["borders"], census["noise"]))
            lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %.3g points/s" % ("grid", med["grid"], min(samp["grid"]), max(samp["grid"]), n / med["grid"] * 1e3))
            lines.append("    %-8s %10.4f  [%10.4f .. %10.4f]   %.3g points/s; %d candidate tests in the 3 x 3 cells (%.3g per second of the whole op)"
                         % ("cluster", med["cluster"], min(samp["cluster"]), max(samp["cluster"]), n / med["cluster"] * 1e3, tests, tests / med["cluster"] * 1e3))
            lines.append("    %-8s %10.1f   cluster_host, numpy (once): %.0f times grid + cluster" % ("host", host_s * 1e3, host_s * 1e3 / (med["grid"] + med["cluster"])))
            if sk_s is not None:
                lines.append("    %-8s %10.1f   sklearn DBSCAN.fit (once); the same core set: %s" % ("sklearn", sk_s * 1e3, "yes" if census["sklearn_same_cores"] else "NO"))
            del q
    write_out("clusters_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

"""Times the spanning forest of the cell graph (hover_net_amd/forest.py, csrc/hvn_forest.hip) on one GPU next to its host path and
scipy's minimum spanning tree on the same box, for 10^6 synthetic centroids, and prints a small table plus ONE JSON line.

    python tools/forest_bench.py [--reps 10] [--sizes 1000000] [--radius 75] [--out profiles/forest_bench.txt]

Input: the slide-like points of tools/nbr_bench_util.py and their cell graph at 75 px, as tools/graph_bench.py; the forest runs on the
buffers the DeviceGraph left on the device.  Per size, `DeviceForest` is first checked against `forest_host` with == on component and
edges (the host path is the one tests/test_forest_host.py holds to the scalar Kruskal); a difference ends the run.
legs (warm; one sample = the launches of one leg between two HIP events on the current stream; median of --reps samples after two
warm-ups, min and max; the legs are interleaved)
    forest    HVN_OP_NBR_FOREST, the whole op: the start, max(1, ceil(log2 N)) rounds of four launches of which those after the last
              round that joined anything return at once, the end; no readback inside it                      -> directed edges/s
    readback  the same forest as start / one round / end ops with one readback of the round's count between the rounds, ending at the
              first round that joined nothing: the form DESIGN.md section 8 weighs against the one above
    nofilter  `forest` with the kernel form whose atomic minima are not preceded by a read of the word
    start, round 0 .., end   the parts of `forest`, timed apart (each round is one op of four launches)
    count     HVN_OP_NBR_GRAPH, mode 0, with its table, on the same points: the yardstick
    host      `forest_host`, wall clock, once (numpy on the same box)
    scipy     scipy.sparse.csgraph.minimum_spanning_tree over the same edges with d2 as the weight, wall clock, once (where scipy
              imports; it drops edges of weight 0 and breaks ties as it likes, so its tree is not compared)
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

from nbr_bench_util import points, stat, timed, write_out  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1000000")
    ap.add_argument("--radius", type=float, default=75.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hover_net_amd import forest as FO
    from hover_net_amd import graph as GR
    from hover_net_amd import lib as L
    from hover_net_amd import points as P

    L.require_gpu()
    radius = a.radius
    out, lines = {"reps": a.reps, "radius": radius}, []
    lines.append("Spanning forest of the cell graph (Gabriel edges of length <= r) on one GPU, radius %g px: ms, median [min .. max] of %d samples after 2 warm-ups; host and scipy once, wall clock"
                 % (radius, a.reps))
    for n in (int(s) for s in a.sizes.split(",")):
        xy, _types, side = points(n, seed=n % 1000 + 3)
        q = GR.DeviceGraph(xy, radius).run()
        g = q.result()
        f = FO.DeviceForest(graph=q)
        dev = f.run().result()
        rounds = f.rounds
        print("%d points: device done, host running" % n, flush=True)
        t0 = time.perf_counter()
        host = FO.forest_host(xy, g)
        host_s = time.perf_counter() - t0
        assert np.array_equal(dev.component, host.component) and np.array_equal(dev.edges, host.edges), "%d points: the device's forest differs from forest_host's" % n
        scipy_s = None
        try:
            from scipy.sparse import csr_matrix
            from scipy.sparse.csgraph import minimum_spanning_tree

            i, j = GR.edge_index(g)
            m = csr_matrix((P.d2_of(xy[i, 0], xy[i, 1], xy[j, 0], xy[j, 1]), (i, j)), shape=(n, n))
            t0 = time.perf_counter()
            minimum_spanning_tree(m)
            scipy_s = time.perf_counter() - t0
        except ImportError:
            pass
        slow, plain = FO.DeviceForest(graph=q), FO.DeviceForest(graph=q, no_filter=True)
        for other, what in ((slow.run_with_readbacks(), "one readback per round"), (plain.run(), "no read before the atomics")):
            res = other.result()
            assert np.array_equal(res.component, host.component) and np.array_equal(res.edges, host.edges) and other.rounds == rounds, what
        parts = [("start", f.run_start)] + [("round %d" % r, lambda r=r: f.run_round(r)) for r in range(min(rounds + 1, FO.round_bound(n)))] + [("end", f.run_end)]
        legs = [("forest", f.run), ("readback", slow.run_with_readbacks), ("nofilter", plain.run)] + parts + [("count", q.run_op)]
        samp = {name: [] for name, _ in legs}
        for it in range(a.reps + 2):
            for name, fn in legs:
                ms = timed(fn)
                if it >= 2:
                    samp[name].append(ms)
        for d in (f, slow, plain):
            again = d.result()
            assert np.array_equal(again.component, host.component) and np.array_equal(again.edges, host.edges), "the timed launches changed the result"
        med = {name: statistics.median(v) for name, v in samp.items()}
        e, trees, comps = int(g.indptr[-1]), int(host.edges.shape[0]), FO.n_components(host)
        split_ms = sum(med[name] for name, _ in parts)
        out[str(n)] = dict({name.replace(" ", "_") + "_ms": stat(v) for name, v in samp.items()}, host_s=round(host_s, 2),
                           scipy_s=None if scipy_s is None else round(scipy_s, 2), equal=True, directed_edges=e, forest_edges=trees, components=comps,
                           rounds=rounds, round_bound=FO.round_bound(n), forest_edges_per_s=round(e / med["forest"] * 1e3, 0))
        lines.append("%d points in %.0f x %.0f px; E = %d directed edges; F = %d forest edges, %d components; %d rounds joined something, %d launched; device == host: yes"
                     % (n, side, side, e, trees, comps, rounds, FO.round_bound(n)))
        row = "    %-9s %10.4f  [%10.4f .. %10.4f]   "
        lines.append((row + "NBR_FOREST, the whole op: %.3g directed edges/s") % ("forest", med["forest"], min(samp["forest"]), max(samp["forest"]), e / med["forest"] * 1e3))
        lines.append((row + "start / round / end ops with one readback per round: this / forest = %.2f")
                     % ("readback", med["readback"], min(samp["readback"]), max(samp["readback"]), med["readback"] / med["forest"]))
        lines.append((row + "NBR_FOREST without the read in front of the atomic minima: this / forest = %.2f")
                     % ("nofilter", med["nofilter"], min(samp["nofilter"]), max(samp["nofilter"]), med["nofilter"] / med["forest"]))
        for name, _ in parts:
            lines.append((row + "a part of the op, timed apart") % (name, med[name], min(samp[name]), max(samp[name])))
        lines.append("    the parts sum to %.4f ms; forest - the parts = %.4f ms for the %d rounds that return at once" % (split_ms, med["forest"] - split_ms, FO.round_bound(n) - rounds - 1))
        lines.append((row + "NBR_GRAPH count with its table, same points: forest / this = %.2f") % ("count", med["count"], min(samp["count"]), max(samp["count"]), med["forest"] / med["count"]))
        lines.append("    %-9s %10.1f   forest_host, numpy (once): %.0f times forest" % ("host", host_s * 1e3, host_s * 1e3 / med["forest"]))
        if scipy_s is not None:
            lines.append("    %-9s %10.1f   scipy minimum_spanning_tree on the same edges (once; its tree is not compared): %.0f times forest" % ("scipy", scipy_s * 1e3, scipy_s * 1e3 / med["forest"]))
        del q, f, slow, plain
    write_out("forest_bench", lines, out, a.out)


if __name__ == "__main__":
    main()

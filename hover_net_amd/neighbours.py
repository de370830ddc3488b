"""Nucleus neighbourhoods: typed counts within a radius, the k nearest neighbours and the nearest neighbour of every type -- the
definition of the result, its host form, and the device form that returns the same integers (csrc/hvn_neighbours.hip, DESIGN.md
4.18).  Opt-in everywhere.  numpy only; imports without a GPU.

Inputs: `xy` float64 [N, 2] of (x, y), all finite; `types` int32 [N] in [0, T) or None (then T = 1 and every type is 0); `radius`
r > 0; 1 <= k <= 16; T <= 16.  All arithmetic is IEEE float64, one rounding per operation, no fused multiply-add:

    dx = xj - xi;  dy = yj - yi;  d2(i, j) = (dx * dx) + (dy * dy);  r2 = r * r
    j is a neighbour of i  <=>  j != i and d2(i, j) <= r2

d2 is symmetric bit for bit (negation is exact), so the relation is symmetric.  Outputs per point i, all int32, positions j being row
numbers of `xy`:

    count[i, t]            the number of neighbours of type t
    knn[i, 0..k)           the neighbours in ascending (d2, j) order, the first k, padded with -1
    nearest_of_type[i, t]  the neighbour of type t that is smallest in (d2, j), or -1

Coincident points (d2 == 0, j != i) are neighbours, ordered by j.  Distances are not outputs of the search: `distances` derives
sqrt(d2(i, j)) from returned positions with the formula above, so the device is compared in integers only and every float a user
sees is numpy's.

Three implementations: tests/neighbours_ref.py (O(N^2), the oracle), `query_host` (a uniform grid to gather candidates, then the rule
above: a million points are feasible without a GPU) and `query_device` (HVN_OP_NBR_GRID + HVN_OP_NBR_QUERY).  The three agree with ==.

The grid (`grid`).  x0 = min x, y0 = min y, and the cell of a point is (floor((y - y0) / c), floor((x - x0) / c)), clamped into
[0, ncy) x [0, ncx).  The 3 x 3 cells around a point must hold all its neighbours, and c = r does not achieve that: with r = 1 and
points at x = 0, 1 - 2^-53 and 2, the difference 2 - (1 - 2^-53) rounds to exactly 1.0, the last two points are neighbours, and at
c = 1 they land in cells 0 and 2.  So c = r (1 + 2^-20), or wider.  The argument, per axis:
  * d2 <= r2 gives fl(dx)^2 <= r^2 (1 + 2^-53)^2 up to the rounding of dx * dx, hence |fl(dx)| <= r (1 + 2^-52), and the true
    difference |xj - xi| <= r (1 + 2^-51)  (`_check` refuses a radius whose square is not a normal number, where this would fail);
  * the true cell coordinate u = (x - x0) / c is below the per-axis cap of 4096 cells + 1, and the computed one carries two roundings
    (the subtraction, the division): |fl(u) - u| <= 4097 * 2^-52 < 2^-39;
  * the true coordinates of two neighbours differ by at most r (1 + 2^-51) / c <= (1 + 2^-51) / (1 + 2^-20) < 1 - 2^-21, the computed
    ones by less than 1 - 2^-21 + 2^-38 < 1, so their floors differ by at most 1 (clamping moves both the same way).
The grid is capped at 4096 cells per axis and 2^22 cells in all; c is widened where the extent needs more.  Wider cells are slower,
never wrong.
"""
import numpy as np

from . import points as P
from .points import MARGIN, MAX_AXIS, MAX_CELLS, MAX_N, MAX_T, MIN_R2, Grid, cells, d2_of, grid, r2_of, workspace_bytes  # noqa: F401  (clusters.py, density.py and the tests reach them here)

MAX_K = 16
_PAIRS = 1 << 22                # candidate pairs per round of `query_host`


def _check_k(k):
    if not P.is_integer(k):
        raise TypeError("k must be an integer, got %r" % (k,))
    if not 1 <= int(k) <= MAX_K:
        raise ValueError("k = %d outside 1..%d" % (k, MAX_K))
    return int(k)


def _check(xy, types, radius, k, nr_types):
    """The inputs as the definition names them, or TypeError / ValueError: -> (xy, types | None, r, k, T)."""
    xy, r, k = P.check_xy(xy), P.check_radius(radius), _check_k(k)
    types, t = P.check_types(types, xy.shape[0], nr_types)
    return xy, types, r, k, t


def _empty(n, k, t):
    return {"count": np.zeros((n, t), np.int32), "knn": np.full((n, k), -1, np.int32), "nearest_of_type": np.full((n, t), -1, np.int32)}


def query_host(xy, types, radius, k, nr_types=None):
    """The definition on the host -> {"count": int32 [N, T], "knn": int32 [N, k], "nearest_of_type": int32 [N, T]}.  Candidates
    come from the grid (three contiguous runs of the cell-ordered points per query), in rounds of about 4 million pairs; the rule
    and the two orders are the docstring's."""
    xy, types, r, k, t = _check(xy, types, radius, k, nr_types)
    n = xy.shape[0]
    g = grid(xy, r)
    r2 = r2_of(r)
    order, lo, hi, _, _ = P.candidate_runs(xy, g)
    sx, sy = xy[order, 0], xy[order, 1]
    st = np.zeros(n, np.int64) if types is None else types[order].astype(np.int64)
    out = _empty(n, k, t)
    for a, b, qi, cand, d2 in P.pair_rounds(sx, sy, lo, hi, r2, _PAIRS):
        keep = cand != qi
        qi, cand, d2 = qi[keep], cand[keep], d2[keep]
        j, tj = order[cand], st[cand]
        rows = order[a:b]
        out["count"][rows] = np.bincount((qi - a) * t + tj, minlength=(b - a) * t).reshape(b - a, t)
        o = np.lexsort((j, d2, qi))
        qs = qi[o]
        rank = np.arange(qs.shape[0], dtype=np.int64) - np.searchsorted(qs, np.arange(a, b, dtype=np.int64))[qs - a]
        sel = rank < k
        out["knn"][order[qs[sel]], rank[sel]] = j[o][sel]
        key = (qi * t + tj)[o]
        o = o[np.argsort(key, kind="stable")]          # ascending (i, type, d2, j)
        key = (qi * t + tj)[o]
        head = np.ones(key.shape[0], bool)
        head[1:] = key[1:] != key[:-1]
        out["nearest_of_type"][order[key[head] // t], key[head] % t] = j[o][head]
    return out


# ---- the device ----------------------------------------------------------------------------------
class DeviceQuery(P.DeviceGrid):
    """One device query (`points.DeviceGrid`: `run_grid`, `run_op`, `run`); `result` reads the three arrays back."""

    def __init__(self, xy, types, radius, k, nr_types=None, device="cuda"):
        xy, types, r, k, t = _check(xy, types, radius, k, nr_types)     # raises before anything is allocated or launched
        super().__init__(xy, types, r, device, "query_device", "OP_NBR_QUERY")
        self.k, self.t = k, t
        self.count, self.knn, self.nearest = self.empty((self.n, t)), self.empty((self.n, k)), self.empty((self.n, t))
        op = self._ops[1]
        op.cout, op._rsv = t, k
        op.y.base, op.y2.base, op.res.base = self.count.data_ptr(), self.knn.data_ptr(), self.nearest.data_ptr()

    def result(self):
        return {"count": self.count.cpu().numpy(), "knn": self.knn.cpu().numpy(), "nearest_of_type": self.nearest.cpu().numpy()}


def query_device(xy, types, radius, k, nr_types=None, device="cuda"):
    """`query_host` on the GPU: the same three arrays.  The grid is chosen here on the host; the device builds it and answers the
    query (two ops on the current stream); the one synchronisation is the readback."""
    return DeviceQuery(xy, types, radius, k, nr_types, device).run().result()


def query(xy, types, radius, k, nr_types=None, device=None):
    """`query_host` with device=None, `query_device` on `device` otherwise."""
    return query_host(xy, types, radius, k, nr_types) if device is None else query_device(xy, types, radius, k, nr_types, device)


# ---- what a user reads ---------------------------------------------------------------------------
def distances(xy, idx):
    """float64 distances from point i to the positions idx[i, ...] (`knn` or `nearest_of_type`): sqrt(d2(i, j)) with the
    definition's d2, inf where the index is -1."""
    xy, idx = np.asarray(xy, np.float64), np.asarray(idx)
    if idx.ndim != 2 or idx.shape[0] != xy.shape[0]:
        raise ValueError("idx %s is not [N, m] for xy %s" % (idx.shape, xy.shape))
    j = np.where(idx < 0, 0, idx)
    dx, dy = xy[j, 0] - xy[:, None, 0], xy[j, 1] - xy[:, None, 1]
    return np.where(idx < 0, np.inf, np.sqrt((dx * dx) + (dy * dy)))


def edges(knn):
    """The undirected edge list of the k-nearest graph: unique (min, max) position pairs, sorted; int32 [E, 2]."""
    knn = np.asarray(knn)
    i = np.repeat(np.arange(knn.shape[0], dtype=np.int64), knn.shape[1])
    j = knn.reshape(-1).astype(np.int64)
    i, j = i[j >= 0], j[j >= 0]
    pairs = np.stack([np.minimum(i, j), np.maximum(i, j)], 1)
    return np.unique(pairs, axis=0).astype(np.int32).reshape(-1, 2)


def resolve(spec):
    """What a `neighbours` argument of the pipeline names: None -> None (off), {"radius": r, "k": k} -> (r, k), in pixels of the
    processed image; with "graph": "gabriel" (graph.py: the cell graph at the same radius) -> (r, k, "gabriel"); with "forest": True
    next to it (forest.py: that graph's minimum spanning forest and components) -> (r, k, "gabriel", True).  ValueError / TypeError
    otherwise, before any work."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or set(spec) - {"graph", "forest"} != {"radius", "k"}:
        raise ValueError('neighbours=%r: None or {"radius": r, "k": k} with an optional "graph": "gabriel"' % (spec,))
    if "forest" in spec and (spec["forest"] is not True or "graph" not in spec):
        raise ValueError('neighbours=%r: "forest" is True or absent, and needs "graph"' % (spec,))
    rk = P.check_radius(spec["radius"]), _check_k(spec["k"])
    if "graph" not in spec:
        return rk
    from . import graph as GR

    return rk + (GR.check_kind(spec["graph"]),) + ((True,) if "forest" in spec else ())


def annotate(info, radius, k, nr_types, device=None, graph=None, forest=False):
    """Adds "neighbours" to every entry of an instance dict (`post_proc.process` / `WsiInference.run`) and returns the dict.
    Positions follow dict order; the centroids are the points, entry["type"] the types (nr_types=None: untyped, one column).
    entry["neighbours"] = {"count": [T ints], "knn": [labels], "knn_dist": [floats], "nearest_of_type": [label | None],
    "nearest_of_type_dist": [float | None]}: instance labels instead of positions, the padding of knn removed, plain Python values
    (JSON-serialisable as they are).  graph="gabriel" adds two keys to that dict: "graph": [labels], the nucleus's neighbours in the
    cell graph of graph.py at the same radius, in ascending (d2, j), and "graph_dist": [floats], their distances in that order.
    forest=True, which needs `graph`, adds two more (forest.py): "component": the instance label of the smallest position in the
    nucleus's connected component of that graph, and "tree": [labels], the part of "graph" that lies in the graph's minimum spanning
    forest, in the same order.  The graph is computed once; on a device the forest runs on the graph's own buffers.  An empty dict is
    returned unchanged.  device=None: `query_host` (and `gabriel_host`, `forest_host`)."""
    if forest is not False and (forest is not True or graph is None):
        raise ValueError("forest=%r: True or False, and True needs `graph`" % (forest,))
    if graph is not None:
        from . import graph as GR

        GR.check_kind(graph)
    if not info:
        return info
    labels, xy, types = P.from_info(info, nr_types)
    res = query(xy, types, radius, k, nr_types, device)
    kd, nd = distances(xy, res["knn"]), distances(xy, res["nearest_of_type"])
    count, knn, near = res["count"].tolist(), res["knn"].tolist(), res["nearest_of_type"].tolist()
    kd, nd = kd.tolist(), nd.tolist()
    for i, lab in enumerate(labels):
        m = sum(1 for j in knn[i] if j >= 0)
        info[lab]["neighbours"] = {"count": count[i], "knn": [labels[j] for j in knn[i][:m]], "knn_dist": kd[i][:m],
                                   "nearest_of_type": [labels[j] if j >= 0 else None for j in near[i]],
                                   "nearest_of_type_dist": [d if j >= 0 else None for j, d in zip(near[i], nd[i])]}
    if graph is not None:
        if forest:
            from . import forest as FO

            g, f = FO.of_points(xy, radius, device)
        else:
            g = GR.gabriel(xy, radius, device)
        ptr, idx, dist = g.indptr.tolist(), g.indices.tolist(), GR.lengths(xy, g).tolist()
        for i, lab in enumerate(labels):
            info[lab]["neighbours"]["graph"] = [labels[j] for j in idx[ptr[i]:ptr[i + 1]]]
            info[lab]["neighbours"]["graph_dist"] = dist[ptr[i]:ptr[i + 1]]
        if forest:
            n = len(labels)
            rows, cols = GR.edge_index(g)
            e = f.edges.astype(np.int64)
            in_tree = np.isin(np.minimum(rows, cols) * n + np.maximum(rows, cols), e[:, 0] * n + e[:, 1]).tolist()
            comp = f.component.tolist()
            for i, lab in enumerate(labels):
                info[lab]["neighbours"]["component"] = labels[comp[i]]
                info[lab]["neighbours"]["tree"] = [labels[idx[p]] for p in range(ptr[i], ptr[i + 1]) if in_tree[p]]
    return info

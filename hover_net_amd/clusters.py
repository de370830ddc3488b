"""Nucleus clusters: DBSCAN over the neighbour relation of hover_net_amd/neighbours.py -- the definition of the result, its host
form, and the device form that returns the same integers (csrc/hvn_clusters.hip).  Opt-in everywhere.  numpy only;
imports without a GPU.

Inputs: `xy` float64 [N, 2] of (x, y), all finite; `types` int32 [N] in [0, 16) or None, parallel to `xy`; `radius` r, admissible
exactly where `neighbours._check` admits it; `min_pts` m, an integer in [1, 2^26]; `of_types` None (every point takes part) or a
non-empty collection of types in [0, 16), which needs `types`: a point whose type is not listed is UNSELECTED.

d2 and r2 are those of neighbours.py (float64, one rounding per operation, no fused multiply-add; `neighbours.d2_of` and
`neighbours.r2_of` compute them here), and j is a neighbour of i  <=>  j != i and d2(i, j) <= r2.  Positions are row numbers of `xy`.

    degree[i]  1 + the number of selected neighbours of i for a selected i (the point counts itself, as in sklearn's min_samples);
               0 for an unselected i
    core       i is selected and degree[i] >= m
    cluster    a connected component of the cores under the neighbour relation; its ROOT is the smallest position among its cores,
               and every core gets label = root
    border     selected, not a core, with at least one core neighbour: it takes the label of its (d2, j)-smallest core neighbour j --
               the nearest core, ties by position.  Not the cluster with the smallest root, not whatever a scan visited first.
               A non-core never links two clusters.
    label      -1 for everything else: unselected points and selected points without a core neighbour (noise)

Outputs: `label` and `degree`, int32 [N] each, a function of the inputs alone.  Cores and the partition of the cores coincide with
DBSCAN's (sklearn.cluster.DBSCAN(eps=r, min_samples=m)) wherever no pair sits within rounding of the radius -- that library tests
sqrt(d2) <= r.  The assignment of border points is THIS module's rule: sklearn gives a border point to the cluster whose expansion
reached it first.

Three implementations: tests/clusters_ref.py (O(N^2), the oracle), `cluster_host` (candidates from `neighbours.grid` by
`points.candidate_runs`, in rounds, a vectorised union-find: a million points are feasible without a GPU) and `cluster_device`
(HVN_OP_NBR_GRID + HVN_OP_NBR_CLUSTER).  The three agree with ==.
"""
import numpy as np

from . import neighbours as NB
from . import points as P

MAX_MIN_PTS, MAX_T = 1 << 26, NB.MAX_T


def _check(xy, types, radius, min_pts, of_types):
    """The inputs as the definition names them, or TypeError / ValueError: -> (xy, types | None, r, m, of_types tuple | None)."""
    xy, r = P.check_xy(xy), P.check_radius(radius)
    types, _ = P.check_types(types, xy.shape[0], None)
    return xy, types, r, _check_min_pts(min_pts), _of_types(of_types, types is not None)


def _check_min_pts(min_pts):
    if not P.is_integer(min_pts):
        raise TypeError("min_pts must be an integer, got %r" % (min_pts,))
    if not 1 <= int(min_pts) <= MAX_MIN_PTS:
        raise ValueError("min_pts = %d outside 1..2^26" % min_pts)
    return int(min_pts)


def _of_types(of_types, typed):
    if of_types is None:
        return None
    if isinstance(of_types, (str, bytes)) or not hasattr(of_types, "__iter__"):
        raise TypeError("of_types must be None or a collection of integer types, got %r" % (of_types,))
    of = list(of_types)
    if not all(P.is_integer(t) for t in of):
        raise TypeError("of_types must hold integers, got %r" % (of,))
    if not of or min(of) < 0 or max(of) >= MAX_T:
        raise ValueError("of_types = %r: a non-empty collection of types in [0, %d)" % (of, MAX_T))
    if not typed:
        raise ValueError("of_types = %r needs types" % (of,))
    return tuple(sorted({int(t) for t in of}))


def type_mask(of_types):
    """The type mask of HVN_OP_NBR_CLUSTER: bit t selects type t; -1 selects every point whatever its type."""
    if of_types is None:
        return -1
    return sum(1 << t for t in of_types)


# ---- the host --------------------------------------------------------------------------------------
_PAIRS = 1 << 22                # candidate pairs per round of `cluster_host`


def _merge(comp, u, v):
    """Unites the sets of u[i] and v[i] in `comp`, a forest flattened to its roots (comp[comp] == comp, a root is the smallest slot of
    its set) -> the flattened forest.  Roots are hooked under smaller roots, then pointers are doubled until flat; repeated until no
    edge joins two sets."""
    n = comp.shape[0]
    while True:
        ru, rv = comp[u], comp[v]
        ne = ru != rv
        if not ne.any():
            return comp
        key = np.unique(np.maximum(ru, rv)[ne] * n + np.minimum(ru, rv)[ne])
        u, v = key // n, key % n
        np.minimum.at(comp, u, v)
        while True:
            nxt = comp[comp]
            if np.array_equal(nxt, comp):
                break
            comp = nxt


def cluster_host(xy, types, radius, min_pts, of_types=None):
    """The definition on the host -> {"label": int32 [N], "degree": int32 [N]}.  The selected points are put on `neighbours.grid`;
    one pass over the candidate rounds counts the degrees, a second unites core pairs and keeps every border's nearest core."""
    xy, types, r, m, of = _check(xy, types, radius, min_pts, of_types)
    n = xy.shape[0]
    label, degree = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    sel = np.arange(n) if of is None else np.nonzero(np.isin(types, of))[0]
    if sel.shape[0] == 0:
        return {"label": label, "degree": degree}
    pts = xy[sel]
    r2 = NB.r2_of(r)
    order, lo, hi, _, _ = P.candidate_runs(pts, NB.grid(pts, r))
    ns = order.shape[0]
    sx, sy, pos = pts[order, 0], pts[order, 1], sel[order]        # pos: the position of a slot
    deg = np.zeros(ns, np.int64)
    for _a, _b, qi, _cand, _d2 in P.pair_rounds(sx, sy, lo, hi, r2, _PAIRS):
        deg += np.bincount(qi, minlength=ns)                      # (s, s) is a pair: the point counts itself
    core = deg >= m
    comp, near = np.arange(ns, dtype=np.int64), np.full(ns, -1, np.int64)
    for _a, _b, qi, cand, d2 in P.pair_rounds(sx, sy, lo, hi, r2, _PAIRS):
        to_core = core[cand]
        link = to_core & core[qi] & (cand < qi)
        comp = _merge(comp, qi[link], cand[link])
        b = to_core & ~core[qi]                                   # a border's candidates: cores within the radius
        qb, cb, db = qi[b], cand[b], d2[b]
        o = np.lexsort((pos[cb], db, qb))                         # ascending (query, d2, j)
        qb, cb = qb[o], cb[o]
        head = np.ones(qb.shape[0], bool)
        head[1:] = qb[1:] != qb[:-1]
        near[qb[head]] = cb[head]
    root = np.full(ns, n, np.int64)                               # per flattened root: the smallest position among its cores
    np.minimum.at(root, comp[core], pos[core])
    lab = np.where(core, root[comp], np.where(near >= 0, root[comp[np.maximum(near, 0)]], -1))
    label[pos] = lab
    degree[pos] = deg
    return {"label": label, "degree": degree}


# ---- the device ----------------------------------------------------------------------------------
def cluster_workspace_bytes(n):
    """Bytes of HVN_OP_NBR_CLUSTER's second workspace (include/hvn.h): parent, smallest position per root and degree, by slot."""
    return 12 * n


class DeviceClusters(P.DeviceGrid):
    """One device clustering (`points.DeviceGrid`: `run_grid`, `run_op`, `run`); `result` reads the two arrays back."""

    def __init__(self, xy, types, radius, min_pts, of_types=None, device="cuda"):
        import torch

        xy, types, r, m, of = _check(xy, types, radius, min_pts, of_types)      # raises before anything is allocated or launched
        super().__init__(xy, types, r, device, "cluster_device", "OP_NBR_CLUSTER")
        self.min_pts, self.of_types = m, of
        nbytes2 = cluster_workspace_bytes(self.n)
        self.ws2 = self.empty(nbytes2, torch.uint8)
        self.label, self.degree = self.empty(self.n), self.empty(self.n)
        op = self._ops[1]
        op.cout, op.groups = m, type_mask(of)
        op.y.base, op.y2.base = self.label.data_ptr(), self.degree.data_ptr()
        op.res.base, op.res.sn = self.ws2.data_ptr(), nbytes2

    def result(self):
        return {"label": self.label.cpu().numpy(), "degree": self.degree.cpu().numpy()}


def cluster_device(xy, types, radius, min_pts, of_types=None, device="cuda"):
    """`cluster_host` on the GPU: the same two arrays.  The grid is chosen here on the host; the device builds it and clusters (two
    ops on the current stream); the one synchronisation is the readback."""
    return DeviceClusters(xy, types, radius, min_pts, of_types, device).run().result()


def cluster(xy, types, radius, min_pts, of_types=None, device=None):
    """`cluster_host` with device=None, `cluster_device` on `device` otherwise."""
    return cluster_host(xy, types, radius, min_pts, of_types) if device is None else cluster_device(xy, types, radius, min_pts, of_types, device)


# ---- what a user reads ---------------------------------------------------------------------------
def resolve(spec, typed=True):
    """What a `clusters` argument of the pipeline names: None -> None (off), {"radius": r, "min_pts": m} with an optional
    "types": [ints] -> (r, m, types tuple | None), the radius in pixels of the processed image.  ValueError / TypeError otherwise,
    before any work.  typed=False (a model without a type branch) refuses "types"."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or not {"radius", "min_pts"} <= set(spec) <= {"radius", "min_pts", "types"}:
        raise ValueError('clusters=%r: None or {"radius": r, "min_pts": m} with an optional "types": [ints]' % (spec,))
    r, m = P.check_radius(spec["radius"]), _check_min_pts(spec["min_pts"])
    of = None if spec.get("types") is None else _of_types(spec["types"], True)
    if of is not None and not typed:
        raise ValueError('clusters=%r: "types" needs a model with a type branch' % (spec,))
    return r, m, of


def annotate(info, radius, min_pts, nr_types, of_types=None, device=None):
    """Adds "cluster" to every entry of an instance dict (`post_proc.process` / `WsiInference.run`) and returns the dict.  Positions
    follow dict order; the centroids are the points, entry["type"] the types (nr_types=None: untyped, and `of_types` must be None).
    entry["cluster"] = {"id": the instance label of the cluster's root nucleus | None, "core": bool, "degree": int}: plain Python
    values (JSON-serialisable as they are).  An empty dict is returned unchanged.  device=None: `cluster_host`."""
    if not info:
        return info
    labels, xy, types = P.from_info(info, nr_types)
    res = cluster(xy, types, radius, min_pts, of_types, device)
    lab_of, deg = res["label"].tolist(), res["degree"].tolist()
    for i, lab in enumerate(labels):
        info[lab]["cluster"] = {"id": labels[lab_of[i]] if lab_of[i] >= 0 else None, "core": deg[i] >= min_pts, "degree": deg[i]}
    return info


def summarise(info, nr_types=None):
    """The clusters of an annotated dict -> {id: {"size": members, "n_core": cores among them, "type_count": [T ints] | None,
    "bbox": [[x0, y0], [x1, y1]] of the members' centroids, "centroid": their mean [x, y]}}, ids in order of first appearance; plain
    Python values.  T = nr_types, or the largest type of the dict + 1; None where an entry carries no type."""
    members = {}
    for e in info.values():
        if e["cluster"]["id"] is not None:
            members.setdefault(e["cluster"]["id"], []).append(e)
    kinds = [e["type"] for e in info.values()]
    typed = bool(kinds) and all(t is not None for t in kinds)
    t = None if not typed else int(nr_types) if nr_types is not None else int(max(kinds)) + 1
    out = {}
    for cid, es in members.items():
        xy = np.array([np.asarray(e["centroid"], np.float64).reshape(2) for e in es], np.float64).reshape(-1, 2)
        out[cid] = {"size": len(es), "n_core": sum(1 for e in es if e["cluster"]["core"]),
                    "type_count": None if t is None else np.bincount([int(e["type"]) for e in es], minlength=t).tolist(),
                    "bbox": [xy.min(0).tolist(), xy.max(0).tolist()], "centroid": xy.mean(0).tolist()}
    return out

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

Three implementations: tests/clusters_ref.py (O(N^2), the oracle), `cluster_host` (candidates from `neighbours.grid` /
`neighbours.cells` in rounds, a vectorised union-find: a million points are feasible without a GPU) and `cluster_device`
(HVN_OP_NBR_GRID + HVN_OP_NBR_CLUSTER).  The three agree with ==.
"""
import ctypes

import numpy as np

from . import neighbours as NB

MAX_MIN_PTS, MAX_T = 1 << 26, NB.MAX_T


def _check(xy, types, radius, min_pts, of_types):
    """The inputs as the definition names them, or TypeError / ValueError: -> (xy, types | None, r, m, of_types tuple | None)."""
    xy, types, r, _, _ = NB._check(xy, types, radius, 1, None)
    if isinstance(min_pts, (bool, np.bool_)) or not isinstance(min_pts, (int, np.integer)):
        raise TypeError("min_pts must be an integer, got %r" % (min_pts,))
    if not 1 <= int(min_pts) <= MAX_MIN_PTS:
        raise ValueError("min_pts = %d outside 1..2^26" % min_pts)
    return xy, types, r, int(min_pts), _of_types(of_types, types is not None)


def _of_types(of_types, typed):
    if of_types is None:
        return None
    if isinstance(of_types, (str, bytes)) or not hasattr(of_types, "__iter__"):
        raise TypeError("of_types must be None or a collection of integer types, got %r" % (of_types,))
    of = list(of_types)
    if any(isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) for t in of):
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


def _runs(pts, g):
    """The cell order of `pts` on grid g and, per cell-ordered point (a SLOT), its three contiguous runs of candidate slots
    (`neighbours.query_host`): -> order [n], lo [3, n], hi [3, n]."""
    n = pts.shape[0]
    cx, cy = NB.cells(pts, g)
    cell = cy * g.ncx + cx
    order = np.argsort(cell, kind="stable")
    start = np.zeros(g.ncx * g.ncy + 1, np.int64)
    np.cumsum(np.bincount(cell, minlength=g.ncx * g.ncy), out=start[1:])
    scx, scy = cx[order], cy[order]
    lo, hi = np.empty((3, n), np.int64), np.empty((3, n), np.int64)
    ca, cb = np.maximum(scx - 1, 0), np.minimum(scx + 1, g.ncx - 1)
    for row in range(3):
        yy = scy + (row - 1)
        ok = (yy >= 0) & (yy < g.ncy)
        base = np.clip(yy, 0, g.ncy - 1) * g.ncx
        lo[row] = start[base + ca]
        hi[row] = np.where(ok, start[base + cb + 1], lo[row])
    return order, lo, hi


def _pairs(sx, sy, lo, hi, r2):
    """Rounds of about `_PAIRS` candidate pairs, all candidates of a query in one round: yields (qi, cand, d2) of the pairs with
    d2 <= r2, in slots; (s, s) is among them."""
    n = sx.shape[0]
    ends = np.cumsum((hi - lo).sum(0))
    a = 0
    while a < n:
        b = max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + _PAIRS, side="right")))
        qi, cand = [], []
        for row in range(3):
            lens = hi[row, a:b] - lo[row, a:b]
            first = np.cumsum(lens) - lens
            qi.append(np.repeat(np.arange(a, b, dtype=np.int64), lens))
            cand.append(np.repeat(lo[row, a:b] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64))
        qi, cand = np.concatenate(qi), np.concatenate(cand)
        d2 = NB.d2_of(sx[qi], sy[qi], sx[cand], sy[cand])
        keep = d2 <= r2
        yield qi[keep], cand[keep], d2[keep]
        a = b


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
    order, lo, hi = _runs(pts, NB.grid(pts, r))
    ns = order.shape[0]
    sx, sy, pos = pts[order, 0], pts[order, 1], sel[order]        # pos: the position of a slot
    deg = np.zeros(ns, np.int64)
    for qi, _cand, _d2 in _pairs(sx, sy, lo, hi, r2):
        deg += np.bincount(qi, minlength=ns)                      # (s, s) is a pair: the point counts itself
    core = deg >= m
    comp, near = np.arange(ns, dtype=np.int64), np.full(ns, -1, np.int64)
    for qi, cand, d2 in _pairs(sx, sy, lo, hi, r2):
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


class DeviceClusters:
    """The tensors and the two ops of one device clustering; `run_grid` (the HVN_OP_NBR_GRID of neighbours.py, on `neighbours.grid`)
    and `run_cluster` launch on the current stream without synchronising (tools/clusters_bench.py times them apart), `result`
    reads the two arrays back."""

    def __init__(self, xy, types, radius, min_pts, of_types=None, device="cuda"):
        import torch

        from . import lib as L
        from . import plan as PL

        xy, types, r, m, of = _check(xy, types, radius, min_pts, of_types)      # raises before anything is allocated or launched
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("cluster_device needs a GPU device, got %r" % (device,))
        n, g = xy.shape[0], NB.grid(xy, r)
        self.n, self.min_pts, self.of_types, self.grid = n, m, of, g
        with torch.cuda.device(self.device):
            up = lambda a: torch.from_numpy(a if a.flags.writeable else a.copy()).to(self.device)  # noqa: E731  (torch warns on read-only arrays)
            self.xy = up(xy)
            self.types = None if types is None else up(types)
            self.table = torch.tensor([g.x0, g.y0, g.c, NB.r2_of(r)], dtype=torch.float64, device=self.device)
            nbytes, nbytes2 = NB.workspace_bytes(n, g.ncx * g.ncy), cluster_workspace_bytes(n)
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.ws2 = torch.empty(nbytes2, dtype=torch.uint8, device=self.device)
            self.label = torch.empty(n, dtype=torch.int32, device=self.device)
            self.degree = torch.empty(n, dtype=torch.int32, device=self.device)
        ops = []
        for kind in (PL.OP_NBR_GRID, PL.OP_NBR_CLUSTER):
            op = L.hvn_op()
            op.kind, op.kh, op.kw, op.x.h = kind, g.ncy, g.ncx, n
            op.w, op.x2.base, op.x2.sn = self.table.data_ptr(), self.ws.data_ptr(), nbytes
            ops.append(op)
        ops[0].x.base = self.xy.data_ptr()
        ops[0].res.base = None if self.types is None else self.types.data_ptr()
        ops[1].cout, ops[1].groups = m, type_mask(of)
        ops[1].y.base, ops[1].y2.base = self.label.data_ptr(), self.degree.data_ptr()
        ops[1].res.base, ops[1].res.sn = self.ws2.data_ptr(), nbytes2
        self._ops = ops

    def _run(self, i):
        import torch

        from . import lib as L

        with torch.cuda.device(self.device):
            L.call("hvn_run_op", ctypes.addressof(self._ops[i]), 1, L.stream_ptr(self.device))

    def run_grid(self):
        self._run(0)

    def run_cluster(self):
        self._run(1)

    def result(self):
        return {"label": self.label.cpu().numpy(), "degree": self.degree.cpu().numpy()}


def cluster_device(xy, types, radius, min_pts, of_types=None, device="cuda"):
    """`cluster_host` on the GPU: the same two arrays.  The grid is chosen here on the host; the device builds it and clusters (two
    ops on the current stream); the one synchronisation is the readback."""
    q = DeviceClusters(xy, types, radius, min_pts, of_types, device)
    q.run_grid()
    q.run_cluster()
    return q.result()


def cluster(xy, types, radius, min_pts, of_types=None, device=None):
    """`cluster_host` with device=None, `cluster_device` on `device` otherwise."""
    if device is None:
        return cluster_host(xy, types, radius, min_pts, of_types)
    return cluster_device(xy, types, radius, min_pts, of_types, device)


# ---- what a user reads ---------------------------------------------------------------------------
def resolve(spec, typed=True):
    """What a `clusters` argument of the pipeline names: None -> None (off), {"radius": r, "min_pts": m} with an optional
    "types": [ints] -> (r, m, types tuple | None), the radius in pixels of the processed image.  ValueError / TypeError otherwise,
    before any work.  typed=False (a model without a type branch) refuses "types"."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or not {"radius", "min_pts"} <= set(spec) <= {"radius", "min_pts", "types"}:
        raise ValueError('clusters=%r: None or {"radius": r, "min_pts": m} with an optional "types": [ints]' % (spec,))
    _check(np.zeros((1, 2)), None, spec["radius"], spec["min_pts"], None)
    of = None if spec.get("types") is None else _of_types(spec["types"], True)
    if of is not None and not typed:
        raise ValueError('clusters=%r: "types" needs a model with a type branch' % (spec,))
    return float(spec["radius"]), int(spec["min_pts"]), of


def annotate(info, radius, min_pts, nr_types, of_types=None, device=None):
    """Adds "cluster" to every entry of an instance dict (`post_proc.process` / `WsiInference.run`) and returns the dict.  Positions
    follow dict order; the centroids are the points, entry["type"] the types (nr_types=None: untyped, and `of_types` must be None).
    entry["cluster"] = {"id": the instance label of the cluster's root nucleus | None, "core": bool, "degree": int}: plain Python
    values (JSON-serialisable as they are).  An empty dict is returned unchanged.  device=None: `cluster_host`."""
    if not info:
        return info
    labels = list(info)
    xy = np.array([np.asarray(info[lab]["centroid"], np.float64).reshape(2) for lab in labels], np.float64).reshape(-1, 2)
    types = None
    if nr_types is not None:
        raw = [info[lab]["type"] for lab in labels]
        if any(v is None or isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in raw):
            raise ValueError("nr_types = %r needs an integer type on every entry" % (nr_types,))
        types = np.array(raw, np.int64)
        if types.min() < 0 or types.max() >= nr_types:
            raise ValueError("types outside [0, %d)" % nr_types)
        types = types.astype(np.int32)
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

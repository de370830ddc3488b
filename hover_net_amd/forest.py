"""The minimum spanning forest and the connected components of a cell graph -- the definition of the result, its host form, and the
device form that returns the same integers (csrc/hvn_forest.hip).  Opt-in everywhere.  numpy only; imports without a GPU.

Inputs.  `xy` float64 [N, 2] as `points.check_xy` admits, and a `graph.CellGraph` g over those N positions.  g must be symmetric (j in
row i iff i in row j), free of self-loops, hold no position twice in a row, and have `indices` in [0, N): `check_graph(g, n)` raises
ValueError otherwise, before any work.  Any such graph is admitted, not only Gabriel ones; the order of a row does not matter.

Key.  The key of an undirected edge {i, j} is the triple (d2(i, j), min(i, j), max(i, j)), compared lexicographically, with d2 from
`points.d2_of` (IEEE float64, one rounding per operation, no fused multiply-add).
  * d2 is symmetric bit for bit, >= +0.0 and never NaN for checked xy, so the uint64 bit pattern of d2 orders exactly as the double
    does, and the all-ones word is above every key.
  * Keys are pairwise distinct: a strict total order.  Coincident nuclei (d2 = 0) and lattice ties are ordered by position.

Forest.  Edge e is in the forest iff its two ends are not connected by edges of g with strictly smaller key (the cycle property).
With a strict total order the forest is unique; it is what Kruskal builds when it takes the edges in key order.

Result.  `Forest(component int32 [N], edges int32 [F, 2])`: component[i] is the smallest position in i's connected component of g (the
naming clusters.py uses); `edges` holds the forest's edges as (lo, hi), lo < hi, sorted lexicographically; F = N - the number of
components.  Distances are not outputs: `lengths` derives them on the host from positions, so the device is compared in integers only.

The Euclidean minimum spanning tree is a subgraph of the Gabriel graph, so in exact arithmetic the forest of `graph.gabriel(xy, r)` is
the forest of the whole r-disc graph: the cell graph loses nothing.  That is a remark, not part of the definition.

Three implementations: tests/forest_ref.py (a scalar Kruskal over the edges sorted by key with a plain union-find: the oracle),
`forest_host` (Boruvka rounds in numpy: every component picks its smallest outgoing key, the picks join the forest, the picked
components are merged by pointer jumping; at most ceil(log2 N) rounds) and `forest_device` (HVN_OP_NBR_FOREST: the same rounds on the
GPU, the key's minimum taken as two 64-bit atomic minima, first over the d2 bits and then over (lo << 32 | hi) among the edges that
tie on them).  The three agree with ==.

What a user reads: `n_components`, `component_sizes`, `tree_degree`, `tree_csr`, `lengths`, `summary`, `of_info`, `save` / `load`.  The
pipeline's key is "forest": True next to "graph": "gabriel" inside the `neighbours` argument (neighbours.py: `resolve`, `annotate`).
"""
import collections
import ctypes

import numpy as np

from . import graph as GR
from . import points as P

MAX_E = (1 << 31) - 1

Forest = collections.namedtuple("Forest", "component edges")


def workspace_bytes(n):
    """HVN_NBR_FOREST_WORKSPACE_BYTES(N) of csrc/hvn_kernels.h: best_d2 and best_pair (uint64 [N]), parent, comp, minpos (int32 [N]) and
    64 control words."""
    return 28 * n + 256


def rounds_at(n):
    """HVN_NBR_FOREST_ROUNDS_AT(N): the byte of the workspace at which the int32 count of the rounds that joined anything lies."""
    return 28 * n + 128


def round_bound(n):
    """max(1, ceil(log2 n)): the rounds that suffice for any graph on n points.  Every component that still has an outgoing edge merges
    with at least one other in every round, so the number of such components at least halves."""
    return max(1, int(n - 1).bit_length())


def check_graph(g, n):
    """A graph as the module docstring admits it over n positions, or ValueError: -> (indptr int64 [n + 1], indices int32 [E]), contiguous."""
    indptr, indices = getattr(g, "indptr", None), getattr(g, "indices", None)
    if not isinstance(indptr, np.ndarray) or indptr.dtype != np.int64 or indptr.shape != (n + 1,):
        raise ValueError("indptr must be an int64 numpy array [%d], got %s %s" % (n + 1, getattr(indptr, "dtype", type(indptr).__name__), getattr(indptr, "shape", "")))
    if not isinstance(indices, np.ndarray) or indices.dtype != np.int32 or indices.ndim != 1:
        raise ValueError("indices must be an int32 numpy array [E], got %s %s" % (getattr(indices, "dtype", type(indices).__name__), getattr(indices, "shape", "")))
    e = indices.shape[0]
    if e > MAX_E:
        raise ValueError("%d directed edges reach 2^31" % e)
    if int(indptr[0]) != 0 or int(indptr[-1]) != e or (np.diff(indptr) < 0).any():
        raise ValueError("indptr does not run from 0 to E = %d without falling" % e)
    if e:
        if int(indices.min()) < 0 or int(indices.max()) >= n:
            raise ValueError("indices outside [0, %d)" % n)
        rows, cols = GR._rows(g), indices.astype(np.int64)
        if (rows == cols).any():
            raise ValueError("the graph has a self-loop at position %d" % int(rows[rows == cols][0]))
        fwd = np.sort(rows * n + cols)
        if (fwd[1:] == fwd[:-1]).any():
            raise ValueError("a row of the graph holds a position twice")
        if not np.array_equal(fwd, np.sort(cols * n + rows)):
            raise ValueError("the graph is not symmetric")
    return np.ascontiguousarray(indptr), np.ascontiguousarray(indices)


def _name(comp):
    """component int32 [N] of a labelling by any representative: the smallest position of every class."""
    n = comp.shape[0]
    least = np.full(n, n, np.int64)
    least[comp[::-1]] = np.arange(n - 1, -1, -1, dtype=np.int64)       # of repeated indices the last assignment stays: the smallest position
    return least[comp].astype(np.int32)


def _sorted_edges(lo, hi):
    o = np.lexsort((hi, lo))
    return np.stack([lo[o], hi[o]], 1).astype(np.int32).reshape(-1, 2)


def forest_host(xy, g):
    """The definition on the host -> Forest.  The undirected edges are ranked by key once; a round lets every component pick the
    smallest rank among its outgoing edges, adds the picks to the forest, hooks every picked component to the one its pick leads to
    (of two components that picked the same edge the smaller stays) and flattens the hooks by pointer jumping."""
    xy = P.check_xy(xy)
    n = xy.shape[0]
    indptr, indices = check_graph(g, n)
    rows, cols = GR._rows(GR.CellGraph(indptr, indices)), indices.astype(np.int64)
    keep = rows < cols
    lo, hi = rows[keep], cols[keep]
    d2 = P.d2_of(xy[lo, 0], xy[lo, 1], xy[hi, 0], xy[hi, 1])
    o = np.lexsort((hi, lo, d2.view(np.uint64)))
    lo, hi = lo[o], hi[o]                                        # in key order: an edge's index is its rank
    m = lo.shape[0]
    comp = np.arange(n, dtype=np.int64)
    in_forest = np.zeros(m, bool)
    alive = np.arange(m, dtype=np.int64)
    for _ in range(round_bound(n)):
        cu, cv = comp[lo[alive]], comp[hi[alive]]
        out = cu != cv
        alive, cu, cv = alive[out], cu[out], cv[out]
        if not alive.shape[0]:
            break
        best = np.full(n, m, np.int64)                           # per component the smallest outgoing rank; `alive` ascends, so of
        best[cv[::-1]] = alive[::-1]                             # repeated indices the last assignment -- the smallest rank -- stays
        second = np.full(n, m, np.int64)
        second[cu[::-1]] = alive[::-1]
        best = np.minimum(best, second)
        c = np.nonzero(best < m)[0]
        e = best[c]
        in_forest[e] = True
        a, b = comp[lo[e]], comp[hi[e]]
        other = np.where(a == c, b, a)
        parent = np.arange(n, dtype=np.int64)
        parent[c] = other
        mutual = (parent[other] == c) & (c < other)              # both picked the one edge between them: the smaller stays a root
        parent[c[mutual]] = c[mutual]
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        comp = parent[comp]
    return Forest(_name(comp), _sorted_edges(lo[in_forest], hi[in_forest]))


# ---- the device ----------------------------------------------------------------------------------
class DeviceForest:
    """One device forest.  Built from host arrays (`DeviceForest(xy, g)`: checked, then uploaded) or from a `graph.DeviceGraph` that has
    run (`DeviceForest(graph=q)`: its device xy, indptr and indices are used as they are -- rows in the device's order, which the
    definition does not depend on -- with no upload and no host round trip).  `run` is HVN_OP_NBR_FOREST on the current stream without
    synchronising; `result` reads component, the forest's edges (picked out of `tree` on the device) and `rounds`, the number of rounds
    that joined anything, back.  `run_start`, `run_round(r)` and `run_end` are the op's parts, for tools/forest_bench.py."""

    def __init__(self, xy=None, g=None, device="cuda", graph=None, no_filter=False):
        import torch

        from . import lib as L
        from . import plan as PL

        if graph is not None:
            if xy is not None or g is not None:
                raise ValueError("either host arrays or a DeviceGraph, not both")
            if graph.indices is None:
                raise ValueError("the DeviceGraph has not run")
            self.device, self.n, self.e = graph.device, graph.n, int(graph.e)
            self.xy, self.indptr, self.indices = graph.xy, graph.indptr, graph.indices
        else:
            xy = P.check_xy(xy)                                   # raises before anything is allocated or launched
            indptr, indices = check_graph(g, xy.shape[0])
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise ValueError("forest_device needs a GPU device, got %r" % (device,))
            up = lambda a: torch.from_numpy(a if a.flags.writeable else a.copy()).to(self.device)  # noqa: E731  (torch warns on read-only arrays)
            self.n, self.e = xy.shape[0], indices.shape[0]
            self.xy, self.indptr, self.indices = up(xy), up(indptr), up(indices)
        self.component = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.tree = torch.empty(self.e, dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(workspace_bytes(self.n), dtype=torch.uint8, device=self.device)
        self.rounds = None
        op = L.hvn_op()
        op.kind, op.x.h, op.x.base, op.w = PL.OP_NBR_FOREST, self.n, self.xy.data_ptr(), self.indptr.data_ptr()
        op.res.base, op.res.sn = (self.indices.data_ptr(), self.e) if self.e else (None, 0)
        op.y.base, op.y2.base = self.component.data_ptr(), self.tree.data_ptr() if self.e else None
        op.x2.base, op.x2.sn, op.cout = self.ws.data_ptr(), self.ws.numel(), 1 if no_filter else 0
        self._op = op

    def _run(self, phase, r=0):
        import torch

        from . import lib as L

        self._op._rsv, self._op.stride = phase, r
        with torch.cuda.device(self.device):
            L.call("hvn_run_op", ctypes.addressof(self._op), 1, L.stream_ptr(self.device))

    def run(self):
        self._run(0)
        return self

    def run_start(self):
        self._run(1)

    def run_round(self, r):
        self._run(2, r)

    def run_end(self):
        self._run(3)

    def hooks(self, r):
        """What round r joined, read back from the workspace (a synchronisation)."""
        at = 28 * self.n + 4 * r
        return int(self.ws[at:at + 4].view(self.component.dtype).item())

    def run_with_readbacks(self):
        """The same forest with one readback per round instead of the device's own early exit: the form DESIGN.md section 8 weighs."""
        self.run_start()
        for r in range(round_bound(self.n)):
            self.run_round(r)
            if not self.hooks(r):
                break
        self.run_end()
        return self

    def result(self):
        import torch

        at = rounds_at(self.n)
        self.rounds = int(self.ws[at:at + 4].view(torch.int32).item())
        rows = torch.repeat_interleave(torch.arange(self.n, dtype=torch.int64, device=self.device), self.indptr[1:] - self.indptr[:-1])
        cols = self.indices.to(torch.int64)
        sel = (self.tree != 0) & (rows < cols)
        lo, hi = rows[sel].cpu().numpy(), cols[sel].cpu().numpy()
        return Forest(self.component.cpu().numpy(), _sorted_edges(lo, hi))


def forest_device(xy, g, device="cuda"):
    """`forest_host` on the GPU: the same Forest.  One op on the current stream; the one synchronisation is the readback."""
    return DeviceForest(xy, g, device).run().result()


def forest(xy, g, device=None):
    """`forest_host` with device=None, `forest_device` on `device` otherwise."""
    return forest_host(xy, g) if device is None else forest_device(xy, g, device)


# ---- what a user reads ---------------------------------------------------------------------------
def n_components(f):
    """The number of connected components."""
    return int(np.unique(np.asarray(f.component)).shape[0])


def component_sizes(f):
    """{component name: its number of points} as two arrays -> (names int32 [C] ascending, sizes int64 [C])."""
    names, sizes = np.unique(np.asarray(f.component, np.int32), return_counts=True)
    return names, sizes.astype(np.int64)


def tree_degree(n, f):
    """int32 [n]: the number of forest edges at every point."""
    return np.bincount(np.asarray(f.edges, np.int64).reshape(-1), minlength=n).astype(np.int32)


def tree_csr(xy, n, f):
    """The forest as a `graph.CellGraph` over n positions: every edge in both rows, every row in ascending (d2, j), so that
    `graph.type_edges`, `graph.edge_index` and `graph.lengths` work on it unchanged."""
    xy, e = np.asarray(xy, np.float64), np.asarray(f.edges, np.int64).reshape(-1, 2)
    rows, cols = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    return GR._csr(n, rows, cols, P.d2_of(xy[rows, 0], xy[rows, 1], xy[cols, 0], xy[cols, 1]))


def lengths(xy, f):
    """float64 [F]: sqrt(d2(lo, hi)) of every forest edge in the order of `edges`, with the definition's d2."""
    xy, e = np.asarray(xy, np.float64), np.asarray(f.edges, np.int64).reshape(-1, 2)
    return np.sqrt(P.d2_of(xy[e[:, 0], 0], xy[e[:, 0], 1], xy[e[:, 1], 0], xy[e[:, 1], 1]))


def summary(xy, f):
    """The classic spanning-tree descriptors over L = `lengths(xy, f)`, float64 throughout, as plain Python values:
        edges = F;  components = `n_components(f)`;  mean = sum(L) / F (numpy's L.mean());  std = sqrt(sum((L - mean)^2) / F) (the
        population form, numpy's L.std());  min = min(L);  max = max(L);  min_max_ratio = min / max, None where max = 0;
        disorder = std / (mean + std), None where mean + std = 0.
    With no edge every float field is None."""
    length = lengths(xy, f)
    out = {"edges": int(length.shape[0]), "components": n_components(f)}
    if not length.shape[0]:
        out.update(mean=None, std=None, min=None, max=None, min_max_ratio=None, disorder=None)
        return out
    mean, std, lo, hi = float(length.mean()), float(length.std()), float(length.min()), float(length.max())
    out.update(mean=mean, std=std, min=lo, max=hi, min_max_ratio=lo / hi if hi > 0.0 else None, disorder=std / (mean + std) if mean + std > 0.0 else None)
    return out


def of_points(xy, radius, device=None):
    """The cell graph of checked points at `radius` and its forest -> (CellGraph, Forest).  On a device the graph is one
    `DeviceGraph.run()` and the forest runs on its buffers."""
    if device is None:
        g = GR.gabriel_host(xy, radius)
        return g, forest_host(xy, g)
    q = GR.DeviceGraph(xy, radius, device).run()
    return q.result(), DeviceForest(graph=q).run().result()


def of_info(info, radius, device=None):
    """The cell graph of an instance dict and its forest -> (labels, CellGraph, Forest), as `graph.of_info` names positions and labels.
    An empty dict gives ([], the empty graph, the empty forest)."""
    if not info:
        P.check_radius(radius)
        return [], GR.CellGraph(np.zeros(1, np.int64), np.zeros(0, np.int32)), Forest(np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    labels, xy, _ = P.from_info(info, None)
    return (labels,) + of_points(xy, radius, device)


def save(path, labels, f):
    """(labels, Forest) as an .npz of labels int64 [N], component and edges; no pickle."""
    np.savez(path, labels=np.asarray(labels, np.int64).reshape(-1), component=np.asarray(f.component, np.int32), edges=np.asarray(f.edges, np.int32).reshape(-1, 2))


def load(path):
    """What `save` wrote -> (labels list, Forest)."""
    with np.load(path) as z:
        return z["labels"].tolist(), Forest(z["component"], z["edges"])

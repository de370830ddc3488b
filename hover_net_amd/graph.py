"""The cell graph of nucleus centroids: the Gabriel edges of length <= r -- the definition of the result, its host form, and the device
form that returns the same integers (csrc/hvn_graph.hip).  Opt-in everywhere.  numpy only; imports without a GPU.

Two nuclei are joined iff no third lies in the open disc whose diameter is the segment between them: the subgraph of the Delaunay
triangulation that needs no triangulation and no orientation predicate.  Restricted to edges of length <= r it is a local rule over
the 3 x 3 cells of the neighbour grid.

Inputs as in neighbours.py: `xy` float64 [N, 2] of (x, y), all finite; `radius` r > 0; d2 and r2 as defined there.  All arithmetic is
IEEE float64, one rounding per operation, no fused multiply-add:

    j is a neighbour of i   <=>  j != i and d2(i, j) <= r2                         (neighbours.py)
    dot(i, j, k) = ((xi - xk) * (xj - xk)) + ((yi - yk) * (yj - yk))
    k blocks (i, j)         <=>  k != i, k != j, k is a neighbour of i AND of j, and dot(i, j, k) < 0
    (i, j) is an edge       <=>  j is a neighbour of i and no k blocks (i, j)

  * Symmetry.  dot is symmetric in (i, j) bit for bit, because multiplication commutes, and so is the blocker condition; the neighbour
    relation is symmetric (neighbours.py).  So the edge relation is symmetric: j is in row i iff i is in row j.
  * Open disc, strict <.  A point on the circle does not block.  A point coincident with an endpoint gives dot = 0 (one factor of each
    product is an exact zero), so duplicates never delete edges, and coincident points are joined to each other.  The four corners of a
    lattice square keep both diagonals.  A point strictly between two collinear points blocks them.
  * "Neighbour of both" is part of the definition.  In exact arithmetic it is implied by lying in the disc; stating it makes the
    completeness of the candidates inherit from neighbours.py's grid argument -- every blocker of (i, j) is among the neighbours of i,
    which the 3 x 3 cells of i hold -- and makes a product that overflows harmless, because a NaN or inf d2 is nobody's neighbour.

The result is `CellGraph(indptr int64 [N + 1], indices int32 [E])`: row i = indices[indptr[i]:indptr[i + 1]] lists the graph neighbours
of i in ascending (d2(i, j), j), and E = indptr[N] counts DIRECTED edges (every edge twice).  Positions are row numbers of `xy`.
Distances are not outputs: `lengths` derives them on the host from positions, so the device is compared in integers only.  ValueError
where E would reach 2^31.

Three implementations: tests/graph_ref.py (the lines above over ALL k, no grid: the oracle), `gabriel_host` (candidates from the grid,
`points.candidate_runs` / `pair_rounds`; the blockers of a pair are tried nearest to i first, in rounds of about `_TRIPLES` triples,
and a pair leaves at its first blocker) and `gabriel_device` (HVN_OP_NBR_GRID, then HVN_OP_NBR_GRAPH: the count pass, which also keeps every
row's first 16 edges in a table, a device cumsum, the one readback of E and of the largest degree, and then either the table compacted
on the device or, where a degree exceeds 16, the fill pass into `indices`; the host sorts every row into (d2, j) order).  The three agree with ==.

What a user reads: `degree`, `edge_list`, `edge_index`, `lengths`, `type_edges`, `of_info`, `save` / `load`.  The pipeline's key is
"graph": "gabriel" inside the `neighbours` argument (neighbours.py: `resolve`, `annotate`); the graph's radius is the neighbour radius.
"""
import collections

import numpy as np

from . import points as P

KINDS = ("gabriel",)
MAX_E = (1 << 31) - 1
TABLE_WIDTH = 16                # edges per point that the device's count pass keeps in a fixed-width table; a graph with a larger degree
                                # somewhere takes the fill pass (tests/test_gpu_graph.py has both)
LIST_CAP = 512                  # HVN_NBR_GRAPH_LIST_CAP of csrc/hvn_kernels.h: neighbours of one point that a wave keeps on chip; a point
                                # with more takes the device's slower exact path (tests/test_gpu_graph.py exceeds it)
_PAIRS = 1 << 22                # candidate pairs per round of `gabriel_host`
_TRIPLES = 1 << 22              # (i, j, k) tests per round of `gabriel_host`
_FIRST = 8                      # blockers tried in a pair's first round; doubled every round

CellGraph = collections.namedtuple("CellGraph", "indptr indices")


def _check(xy, radius):
    return P.check_xy(xy), P.check_radius(radius)


def check_kind(kind):
    """A graph kind as the `neighbours` argument names it, or ValueError: -> kind."""
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError('graph=%r: the only cell graph is "gabriel"' % (kind,))
    return kind


def _blocked(xi, yi, xj, yj, sj, xk, yk, sk, r2):
    """Whether k blocks (i, j) for k among the neighbours of i: arrays of triples, s the identities of j and k."""
    with np.errstate(over="ignore", invalid="ignore"):
        dot = ((xi - xk) * (xj - xk)) + ((yi - yk) * (yj - yk))
        return (sk != sj) & (P.d2_of(xj, yj, xk, yk) <= r2) & (dot < 0.0)


def _csr(n, rows, cols, d2):
    """CellGraph of the directed edges (rows[e], cols[e]) with their d2, every row in ascending (d2, j)."""
    if rows.shape[0] > MAX_E:
        raise ValueError("%d directed edges reach 2^31" % rows.shape[0])
    o = np.lexsort((cols, d2, rows))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return CellGraph(indptr, cols[o].astype(np.int32))


def gabriel_host(xy, radius):
    """The definition on the host -> CellGraph.  The neighbour pairs come from the grid in rounds of about 4 million candidate pairs,
    all neighbours of a query in one round and sorted by (d2, j).  The blockers of a pair (i, j) are the neighbours of i; they are
    tried in that order, 8 in the first round, 16 in the next and so on, about 4 million triples at a time, and a pair leaves at its
    first blocker: a blocker lies in the disc, so it is among the nearest to i, and what survives a few rounds is mostly the edges."""
    xy, r = _check(xy, radius)
    n = xy.shape[0]
    g = P.grid(xy, r)
    r2 = P.r2_of(r)
    order, lo, hi, _, _ = P.candidate_runs(xy, g)
    sx, sy = xy[order, 0], xy[order, 1]
    rows, cols, dist = [], [], []
    for a, b, qi, cand, d2 in P.pair_rounds(sx, sy, lo, hi, r2, _PAIRS):
        keep = cand != qi
        qi, cand, d2 = qi[keep], cand[keep], d2[keep]
        o = np.lexsort((order[cand], d2, qi))
        qi, cand, d2 = qi[o], cand[o], d2[o]                 # per query: its neighbours in ascending (d2, j)
        first = np.searchsorted(qi, np.arange(a, b + 1, dtype=np.int64))      # the pairs of query a + u are [first[u], first[u + 1])
        deg = np.diff(first)
        alive = np.arange(qi.shape[0], dtype=np.int64)       # pairs that no blocker tried so far blocks
        edge = np.zeros(qi.shape[0], bool)
        s, width = 0, _FIRST
        while alive.shape[0]:
            done = deg[qi[alive] - a] <= s                   # every neighbour of i has been tried
            edge[alive[done]] = True
            alive = alive[~done]
            nxt = []
            per = max(1, _TRIPLES // width)
            for c in range(0, alive.shape[0], per):
                p = alive[c:c + per]
                u = qi[p] - a
                lens = np.minimum(width, deg[u] - s)
                start = np.cumsum(lens) - lens
                pp = np.repeat(np.arange(p.shape[0], dtype=np.int64), lens)                      # the pair of a triple, within p
                kk = np.repeat(first[u] + s - start, lens) + np.arange(int(lens.sum()), dtype=np.int64)   # its k, as a pair (i, k)
                si, sj, sk = qi[p][pp], cand[p][pp], cand[kk]
                hit = _blocked(sx[si], sy[si], sx[sj], sy[sj], sj, sx[sk], sy[sk], sk, r2)
                nxt.append(p[np.bincount(pp[hit], minlength=p.shape[0]) == 0])
            alive = np.concatenate(nxt) if nxt else alive
            s, width = s + width, 2 * width
        rows.append(order[qi[edge]])
        cols.append(order[cand[edge]])
        dist.append(d2[edge])
    if not rows:
        return _csr(n, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    return _csr(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(dist))


# ---- the device ----------------------------------------------------------------------------------
class DeviceGraph(P.DeviceGrid):
    """One device graph (`points.DeviceGrid`: `run_grid`, `run_op`, `run`).  `run_op` is the COUNT pass, which with `width` > 0 also
    leaves the first `width` edges of every row in the table `first` [N, width]; `prepare_fill` forms indptr on the device and reads E
    and the largest degree back (the one synchronisation).  Where no degree exceeds `width` -- every graph but one with piles of
    coincident or cocircular points -- `indices` is the table's used part, compacted on the device in row order (`compact`), and
    `run_fill` has nothing to do; otherwise `indices` is allocated and `run_fill` is the FILL pass, the search once more.  `result`
    reads both arrays back and sorts every row into (d2, j) order.  width=0: always count, then fill.  tools/graph_bench.py times the
    passes apart."""

    def __init__(self, xy, radius, device="cuda", width=TABLE_WIDTH):
        xy, r = _check(xy, radius)                            # raises before anything is allocated or launched
        if not P.is_integer(width) or not 0 <= width <= 64:
            raise ValueError("width = %r outside 0..64" % (width,))
        super().__init__(xy, None, r, device, "gabriel_device", "OP_NBR_GRAPH")
        import torch

        self.host_xy, self.width = xy, int(width)
        self.degree = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.indptr = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
        self.indices, self.e, self.from_table = None, None, False
        op = self._ops[1]
        op._rsv, op.y.base = 0, self.degree.data_ptr()
        if self.width:
            self.first = self.empty((self.n, self.width))
            self._slot = torch.arange(self.width, dtype=torch.int32, device=self.device)[None, :]
            op.y2.base, op.stride = self.first.data_ptr(), self.width

    def compact(self):
        """The used part of the table, row by row: `indices` of a graph whose largest degree is at most `width`."""
        return self.first[self._slot < self.degree[:, None]]

    def prepare_fill(self):
        import torch

        torch.cumsum(self.degree, 0, dtype=torch.int64, out=self.indptr[1:])
        self.e, top = torch.stack([self.indptr[-1], self.degree.max().to(torch.int64)]).tolist()
        if self.e > MAX_E:
            raise ValueError("%d directed edges reach 2^31" % self.e)
        self.from_table = 0 < self.width and top <= self.width
        if self.from_table:
            self.indices = self.compact()
            return self
        self.indices = self.empty(self.e)
        if len(self._ops) == 2:
            self._ops.append(type(self._ops[1]).from_buffer_copy(self._ops[1]))       # the count op's fields; the fill's own follow
        op = self._ops[2]
        op._rsv, op.stride, op.y.base, op.y.sn, op.y2.base = 1, 0, self.indices.data_ptr(), self.e, self.indptr.data_ptr()
        return self

    def run_fill(self):
        if self.e and not self.from_table:                    # no edge: nothing to fill, and the op refuses an empty `indices`
            self._run(2)

    def run(self):
        self.run_grid()
        self.run_op()
        self.prepare_fill().run_fill()
        return self

    def result(self):
        indptr, cols = self.indptr.cpu().numpy(), self.indices.cpu().numpy().astype(np.int64)
        rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(indptr))
        xy = self.host_xy
        return _csr(self.n, rows, cols, P.d2_of(xy[rows, 0], xy[rows, 1], xy[cols, 0], xy[cols, 1]))


def gabriel_device(xy, radius, device="cuda"):
    """`gabriel_host` on the GPU: the same CellGraph.  The grid is chosen here on the host; the device builds it, counts every point's
    edges, sums the counts and compacts the count pass's table or, where a degree exceeds it, fills the rows in a second search (two or
    three ops and a cumsum on the current stream, one readback of E and the largest degree between them); the rows are put into (d2, j)
    order on the host."""
    return DeviceGraph(xy, radius, device).run().result()


def gabriel(xy, radius, device=None):
    """`gabriel_host` with device=None, `gabriel_device` on `device` otherwise."""
    return gabriel_host(xy, radius) if device is None else gabriel_device(xy, radius, device)


# ---- what a user reads ---------------------------------------------------------------------------
def _rows(g):
    indptr = np.asarray(g.indptr, np.int64)
    return np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))


def degree(g):
    """int32 [N]: the number of graph neighbours of every point."""
    return np.diff(np.asarray(g.indptr, np.int64)).astype(np.int32)


def edge_list(g):
    """The undirected edges: unique (min, max) position pairs, sorted; int32 [E / 2, 2]."""
    i, j = _rows(g), np.asarray(g.indices, np.int64)
    pairs = np.stack([np.minimum(i, j), np.maximum(i, j)], 1)
    return np.unique(pairs, axis=0).astype(np.int32).reshape(-1, 2)


def edge_index(g):
    """The directed edges as int64 [2, E] = (source row, target), in CSR order: the layout graph-network libraries take."""
    return np.stack([_rows(g), np.asarray(g.indices, np.int64)])


def lengths(xy, g):
    """float64 [E]: sqrt(d2(i, j)) of every directed edge in CSR order, with the definition's d2."""
    xy = np.asarray(xy, np.float64)
    i, j = _rows(g), np.asarray(g.indices, np.int64)
    return np.sqrt(P.d2_of(xy[i, 0], xy[i, 1], xy[j, 0], xy[j, 1]))


def type_edges(g, types, nr_types):
    """int64 [T, T]: out[a, b] = the directed edges from a point of type a to one of type b (symmetric; an undirected edge between two
    points of one type counts twice on the diagonal)."""
    types, t = P.check_types(types, np.asarray(g.indptr).shape[0] - 1, nr_types)
    if types is None:
        raise TypeError("type_edges needs the types")
    ti, tj = types[_rows(g)].astype(np.int64), types[np.asarray(g.indices, np.int64)].astype(np.int64)
    return np.bincount(ti * t + tj, minlength=t * t).reshape(t, t).astype(np.int64)


def of_info(info, radius, device=None):
    """The cell graph of an instance dict (`post_proc.process` / `WsiInference.run`) -> (labels, CellGraph): positions follow dict
    order, labels[p] is the instance label at position p, the centroids are the points.  An empty dict gives ([], the empty graph)."""
    if not info:
        P.check_radius(radius)
        return [], CellGraph(np.zeros(1, np.int64), np.zeros(0, np.int32))
    labels, xy, _ = P.from_info(info, None)
    return labels, gabriel(xy, radius, device)


def save(path, labels, g):
    """(labels, CellGraph) as an .npz of labels int64 [N], indptr and indices; no pickle."""
    np.savez(path, labels=np.asarray(labels, np.int64).reshape(-1), indptr=np.asarray(g.indptr, np.int64), indices=np.asarray(g.indices, np.int32))


def load(path):
    """What `save` wrote -> (labels list, CellGraph)."""
    with np.load(path) as z:
        return z["labels"].tolist(), CellGraph(z["indptr"], z["indices"])

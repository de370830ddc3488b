"""The point-pattern layer under neighbours.py, clusters.py, density.py and ripley.py: what the four analyses of nucleus centroids share
on the host, on the device and in the pipeline.  numpy only; imports without a GPU.

The arithmetic (`d2_of`, `r2_of`) and the grid (`grid`, `cells`) are defined in the docstring of neighbours.py, which re-exports them.

Candidates (`candidate_runs`, `pair_rounds`, `round_end`).  Points are put in cell order (a stable sort by cell: a SLOT is a position
in that order).  Cells of one grid row are adjacent there, so the 3 x 3 cells around a slot are three contiguous runs of slots, one per
grid row.  The candidate pairs are tested in rounds of about `pairs` pairs, all candidates of a query in one round; `pairs` is the
caller's own module-level `_PAIRS`, passed at call time.

The device (`DeviceGrid`).  Every analysis is HVN_OP_NBR_GRID, which builds the cell-ordered copies and cell_start in one workspace,
followed by a second op of its own kind that reads them.  `DeviceGrid` uploads the points, chooses the grid, owns that workspace and
fills both ops' common fields; a subclass allocates its outputs and sets its own fields of the second op.

The pipeline (`resolve_specs`, `annotate`, `density_of`, `ripley_of`).  `post_proc.process`, `infer_tile.process_images`, `WsiInference` and the two
managers of infer_manager.py take `neighbours`, `clusters` and, where a map can be returned or written, `density`:
    neighbours  None or {"radius": r, "k": k}: every entry of the instance dict gains "neighbours" (`neighbours.annotate`)
    clusters    None or {"radius": r, "min_pts": m} with an optional "types": [ints], which needs nr_types: every entry gains
                "cluster" (`clusters.annotate`)
    density     None or {"radius": r, "step": s}, `step` an integer >= 1: a `density.DensityMap` of the dict over the image
                (`density.of_info`)
Radii and steps are pixels of the processed image.  A bad spec is refused by `resolve_specs` before any work.  `neighbours` and
`clusters` imply the instance dict.  The analyses run on the FINISHED dict -- on a slide once, on the merged dict in slide
coordinates, so they cross tile seams -- in the order neighbours, clusters, density; on rank 0, where the dict lives, with no
collective; on the GPU where the model is on one, on the host otherwise.
A fourth argument, `ripley` (None or {"radii": [r, ..]} with an optional "window"), is taken by `WsiInference` and the two managers
only: the `ripley.PairCounts` of the finished dict over the image (`ripley.of_info`, here `ripley_of`), made after the other three.  It
is about the slide, not about a nucleus or a place, so it annotates nothing; `PointSpecs` stays the three above, and `ripley.resolve`
resolves the fourth spec, which its users carry beside their PointSpecs.
A fifth, `regions` (None or {"regions": RegionSet | list | GeoJSON path} with an optional "scale"; the managers take {"dir": d} and read
`<d>/<name>.geojson`), is carried the same way: the `regions.RegionCounts` of the finished dict against annotated polygons
(`regions.of_info`, here `regions_of`), made last; every entry gains "region" (`regions.annotate`).
"""
import collections
import ctypes

import numpy as np

MARGIN = 1.0 + 2.0 ** -20
MAX_AXIS, MAX_CELLS = 4096, 1 << 22

Grid = collections.namedtuple("Grid", "x0 y0 c ncx ncy")


def is_number(v):
    """An int or a float, numpy's included, that is not a bool."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def is_integer(v):
    """An int, numpy's included, that is not a bool."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))


def d2_of(xi, yi, xj, yj):
    """d2(i, j) of neighbours.py's docstring for coordinates or arrays of them."""
    dx, dy = xj - xi, yj - yi
    return (dx * dx) + (dy * dy)


def r2_of(r):
    """r2 of neighbours.py's docstring for a checked radius."""
    return r * r


def grid(xy, radius):
    """The grid of neighbours.py's docstring for checked inputs -> Grid(x0, y0, c, ncx, ncy)."""
    x0, y0 = float(xy[:, 0].min()), float(xy[:, 1].min())
    ex, ey = float(xy[:, 0].max()) - x0, float(xy[:, 1].max()) - y0
    c = max(radius * MARGIN, ex / (MAX_AXIS - 1), ey / (MAX_AXIS - 1))
    while True:
        ncx, ncy = int(np.floor(ex / c)) + 1, int(np.floor(ey / c)) + 1
        if ncx <= MAX_AXIS and ncy <= MAX_AXIS and ncx * ncy <= MAX_CELLS:
            return Grid(x0, y0, c, ncx, ncy)
        c *= 1.25


def cells(xy, g):
    """(cx, cy) int64 [N] of every point: floor of the float64 quotient, clamped into the grid."""
    cx = np.clip(np.floor((xy[:, 0] - g.x0) / g.c), 0, g.ncx - 1).astype(np.int64)
    cy = np.clip(np.floor((xy[:, 1] - g.y0) / g.c), 0, g.ncy - 1).astype(np.int64)
    return cx, cy


def from_info(info, nr_types):
    """The points of a non-empty instance dict -> (labels, xy float64 [N, 2], types int32 [N] | None).  Positions follow dict order;
    the centroids are the points, entry["type"] the types (nr_types=None: untyped).  ValueError for an entry without an integer type
    and for a type outside [0, nr_types)."""
    labels = list(info)
    xy = np.array([np.asarray(info[lab]["centroid"], np.float64).reshape(2) for lab in labels], np.float64).reshape(-1, 2)
    types = None
    if nr_types is not None:
        raw = [info[lab]["type"] for lab in labels]
        if not all(is_integer(v) for v in raw):
            raise ValueError("nr_types = %r needs an integer type on every entry" % (nr_types,))
        types = np.array(raw, np.int64)
        if types.min() < 0 or types.max() >= nr_types:
            raise ValueError("types outside [0, %d)" % nr_types)
        types = types.astype(np.int32)
    return labels, xy, types


# ---- candidates on the host ------------------------------------------------------------------------
def candidate_runs(pts, g):
    """The cell order of `pts` on grid g and, per slot, its three runs of candidate slots -> order [n], lo [3, n], hi [3, n], and the
    cells (cx, cy) [n] by position.  A row outside the grid gives an empty run."""
    n = pts.shape[0]
    cx, cy = cells(pts, g)
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
    return order, lo, hi, cx, cy


def round_end(ends, a, pairs):
    """The end b of the round that starts at item a, for the running totals `ends` of the items' pair counts: about `pairs` pairs,
    at least one item (an item larger than `pairs` is a round of its own)."""
    return max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + pairs, side="right")))


def pair_rounds(sx, sy, lo, hi, r2, pairs):
    """Rounds of about `pairs` candidate pairs of `candidate_runs`, all candidates of a query in one round: yields (a, b, qi, cand, d2)
    for the queries [a, b), the pairs with d2 <= r2, in slots; (s, s) is among them."""
    n = sx.shape[0]
    ends = np.cumsum((hi - lo).sum(0))
    a = 0
    while a < n:
        b = round_end(ends, a, pairs)
        qi, cand = [], []
        for row in range(3):
            lens = hi[row, a:b] - lo[row, a:b]
            first = np.cumsum(lens) - lens
            qi.append(np.repeat(np.arange(a, b, dtype=np.int64), lens))
            cand.append(np.repeat(lo[row, a:b] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64))
        qi, cand = np.concatenate(qi), np.concatenate(cand)
        d2 = d2_of(sx[qi], sy[qi], sx[cand], sy[cand])
        keep = d2 <= r2
        yield a, b, qi[keep], cand[keep], d2[keep]
        a = b


# ---- the device ----------------------------------------------------------------------------------
def workspace_bytes(n, n_cells):
    """Bytes of the one workspace of HVN_OP_NBR_GRID and the ops that read it (include/hvn.h, NBR_GRID)."""
    return 24 * n + 4 * (2 * n_cells + 1) + 4096


class DeviceGrid:
    """The uploaded points, the grid workspace and the two ops of one device analysis, for CHECKED xy, types and r: `_ops[0]` is
    HVN_OP_NBR_GRID, `_ops[1]` the op of `kind` (a name of plan.py) with the fields filled that every such op shares.  `name` is the
    caller's function, for the refusal of a device that is no GPU.  `run_grid` and `_run(1)` launch on the current stream without
    synchronising."""

    def __init__(self, xy, types, r, device, name, kind):
        import torch

        from . import lib as L
        from . import plan as PL

        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("%s needs a GPU device, got %r" % (name, device))
        n, g = xy.shape[0], grid(xy, r)
        self.n, self.grid = n, g
        up = lambda a: torch.from_numpy(a if a.flags.writeable else a.copy()).to(self.device)  # noqa: E731  (torch warns on read-only arrays)
        self.xy = up(xy)
        self.types = None if types is None else up(types)
        self.table = torch.tensor([g.x0, g.y0, g.c, r2_of(r)], dtype=torch.float64, device=self.device)
        nbytes = workspace_bytes(n, g.ncx * g.ncy)
        self.ws = self.empty(nbytes, torch.uint8)
        self._ops = []
        for k in (PL.OP_NBR_GRID, getattr(PL, kind)):
            op = L.hvn_op()
            op.kind, op.kh, op.kw, op.x.h = k, g.ncy, g.ncx, n
            op.w, op.x2.base, op.x2.sn = self.table.data_ptr(), self.ws.data_ptr(), nbytes
            self._ops.append(op)
        self._ops[0].x.base = self.xy.data_ptr()
        self._ops[0].res.base = None if self.types is None else self.types.data_ptr()

    def empty(self, shape, dtype=None):
        """An uninitialised tensor on the device, int32 unless told otherwise."""
        import torch

        return torch.empty(shape, dtype=torch.int32 if dtype is None else dtype, device=self.device)

    def _run(self, i):
        import torch

        from . import lib as L

        with torch.cuda.device(self.device):
            L.call("hvn_run_op", ctypes.addressof(self._ops[i]), 1, L.stream_ptr(self.device))

    def run_grid(self):
        self._run(0)


# ---- the pipeline --------------------------------------------------------------------------------
class PointSpecs(collections.namedtuple("PointSpecs", "neighbours clusters density")):
    """The three resolved arguments of the module docstring, None where off: (r, k), (r, m, types tuple | None), (r, step)."""
    __slots__ = ()

    @property
    def any_annotation(self):
        """Whether the instance dict is needed: `neighbours` or `clusters` is on."""
        return self.neighbours is not None or self.clusters is not None


def resolve_specs(neighbours=None, clusters=None, density=None, typed=True):
    """The three arguments as a caller gave them -> PointSpecs, or the ValueError / TypeError of the module's own `resolve`.
    typed=False (a model without a type branch) refuses "types" in `clusters`."""
    from . import clusters as CL
    from . import density as DN
    from . import neighbours as NB

    return PointSpecs(NB.resolve(neighbours), CL.resolve(clusters, typed=typed), DN.resolve(density))


def _device(device):
    return device if device is not None and device.type == "cuda" else None


def annotate(info, specs, nr_types, device):
    """Adds "neighbours", then "cluster", to every entry of a finished instance dict, as `specs` asks, and returns it.  `device`: a
    torch.device or None; the search runs there if it is a GPU and on the host otherwise."""
    from . import clusters as CL
    from . import neighbours as NB

    if specs.neighbours is not None:
        NB.annotate(info, specs.neighbours[0], specs.neighbours[1], nr_types, device=_device(device))
    if specs.clusters is not None:
        CL.annotate(info, specs.clusters[0], specs.clusters[1], nr_types, specs.clusters[2], device=_device(device))
    return info


def density_of(info, size_hw, specs, nr_types, device):
    """The `density.DensityMap` of a finished instance dict over an image of size_hw = (h, w) processed pixels for `specs.density`
    (not None); `device` as in `annotate`."""
    from . import density as DN

    return DN.of_info(info, size_hw, specs.density[0], specs.density[1], nr_types, device=_device(device))


def ripley_of(info, size_hw, spec, nr_types, device):
    """The `ripley.PairCounts` of a finished instance dict over an image of size_hw = (h, w) processed pixels for a resolved `ripley`
    spec (`ripley.resolve`, not None); `device` as in `annotate`."""
    from . import ripley as RP

    return RP.of_info(info, size_hw, spec[0], nr_types, device=_device(device), window=spec[1])


def regions_of(info, rs, nr_types, device):
    """The `regions.RegionCounts` of a finished instance dict for a resolved `regions` spec (`regions.resolve`, not None), with every
    entry annotated ("region"); `device` as in `annotate`."""
    from . import regions as RG

    rc = RG.of_info(info, rs, nr_types, device=_device(device))
    RG.annotate(info, rc)
    return rc

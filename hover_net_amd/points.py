"""The point-pattern layer under neighbours.py, clusters.py, density.py, ripley.py and regions.py: what the five analyses of nucleus
centroids share on the host, on the device and in the pipeline.  numpy only; imports without a GPU.

The arithmetic (`d2_of`, `r2_of`) and the grid (`grid`, `cells`) are defined in the docstring of neighbours.py, which re-exports them.

The inputs (`check_xy`, `check_radius`, `check_types`).  What every analysis admits as points, as a radius and as types; each module's
`_check` calls the ones it needs and adds its own.

Candidates (`candidate_runs`, `pair_rounds`, `round_end`).  Points are put in cell order (a stable sort by cell: a SLOT is a position
in that order).  Cells of one grid row are adjacent there, so the 3 x 3 cells around a slot are three contiguous runs of slots, one per
grid row.  The candidate pairs are tested in rounds of about `pairs` pairs, all candidates of a query in one round; `pairs` is the
caller's own module-level `_PAIRS`, passed at call time.

The device (`DeviceGrid`).  Every analysis is HVN_OP_NBR_GRID, which builds the cell-ordered copies and cell_start in one workspace,
followed by a second op of its own kind that reads them.  `DeviceGrid` uploads the points, chooses the grid, owns that workspace,
fills both ops' common fields and launches them (`run_grid`, `run_op`, `run`); a subclass allocates its outputs, sets its own fields of
the second op and reads them back (`result`).

The pipeline (`ARGS`, `resolve_specs`, `annotate`, `summaries`, `save_results`, `output_dirs`).  Five arguments, None = off, resolved
into one `PointSpecs` by each module's own `resolve`, in this order; a bad spec is refused there, before any work:
    neighbours  {"radius": r, "k": k}: every entry of the instance dict gains "neighbours" (`neighbours.annotate`); with "graph":
                "gabriel" that entry also lists the nucleus's neighbours in the cell graph at the same radius (graph.py), and with
                "forest": True next to it the nucleus's component of that graph and its neighbours in the graph's minimum spanning
                forest (forest.py)
    clusters    {"radius": r, "min_pts": m} with an optional "types": [ints], which needs nr_types: every entry gains "cluster"
                (`clusters.annotate`)
    density     {"radius": r, "step": s}, `step` an integer >= 1: a `density.DensityMap` of the dict over the image (`density.of_info`)
    ripley      {"radii": [r, ..]} with an optional "window": the `ripley.PairCounts` of the dict over the image (`ripley.of_info`);
                with "sims": S and an optional "seed" the `ripley.LabelSims` of the random-labelling test
    regions     {"regions": RegionSet | list | GeoJSON path} with an optional "scale" (the managers take {"dir": d} and read
                `<d>/<name>.geojson`): the `regions.RegionCounts` of the dict against annotated polygons (`regions.of_info`); every
                entry gains "region" (`regions.annotate`); with "margin": [w_0, ..] the result is a `regions.RegionMargins`, which
                adds the `margins.Margins` -- the distance bands around every region's boundary -- and every entry gains "margin" too
Radii, steps and windows are pixels of the processed image.  The first two ANNOTATE (`annotate`) and imply the instance dict;
`post_proc.process` and `infer_tile.process_images` take only them.  The last three are SUMMARIES, one row each of the table
`_SUMMARIES`: the name (which is the field of PointSpecs and of PointResults, the output sub-directory and the module that saves it) and
how to compute it.  `summaries` walks the table into a `PointResults`, `save_results` walks it to write `<sub>/<name>.npz`, `output_dirs`
names the sub-directories that are on; `WsiInference` and the two managers of infer_manager.py use those three and nothing per
analysis.  Everything runs on the FINISHED dict -- on a slide once, on the merged dict in slide coordinates, so it crosses tile seams --
in the order above; on rank 0, where the dict lives, with no collective; on the GPU where the model is on one, on the host otherwise.
"""
import collections
import ctypes
import importlib

import numpy as np

MARGIN = 1.0 + 2.0 ** -20
MAX_AXIS, MAX_CELLS = 4096, 1 << 22
MAX_N, MAX_T = 1 << 26, 16
MIN_R2 = 2.0 ** -1000

Grid = collections.namedtuple("Grid", "x0 y0 c ncx ncy")


def is_number(v):
    """An int or a float, numpy's included, that is not a bool."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def is_integer(v):
    """An int, numpy's included, that is not a bool."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))


def check_xy(xy):
    """Points as neighbours.py's docstring names them, or TypeError / ValueError: -> xy, contiguous."""
    if not isinstance(xy, np.ndarray) or xy.dtype != np.float64:
        raise TypeError("xy must be a float64 numpy array [N, 2], got %s" % (getattr(xy, "dtype", type(xy).__name__),))
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
        raise ValueError("xy must be [N, 2] with N >= 1, got %s" % (xy.shape,))
    if xy.shape[0] > MAX_N:
        raise ValueError("%d points, more than 2^26" % xy.shape[0])
    if not np.isfinite(xy).all():
        raise ValueError("xy holds a coordinate that is not finite")
    with np.errstate(over="ignore"):
        if not np.isfinite(xy.max(0) - xy.min(0)).all():
            raise ValueError("the extent of xy is not a finite float64")
    return np.ascontiguousarray(xy)


def check_radius(radius):
    """A radius as neighbours.py's docstring names it, or TypeError / ValueError: -> float."""
    if not is_number(radius):
        raise TypeError("radius must be a number, got %r" % (radius,))
    r = float(radius)
    if not (r > 0.0 and np.isfinite(r) and np.isfinite(r * r) and r * r >= MIN_R2):
        raise ValueError("radius = %r: it must be positive and its square a normal, finite float64" % (radius,))
    return r


def check_types(types, n, nr_types):
    """The types of n points (None: untyped) and `nr_types` (None: as many as `types` holds) as neighbours.py's docstring names them, or
    TypeError / ValueError: -> (types | None, contiguous; T)."""
    if nr_types is not None and not is_integer(nr_types):
        raise TypeError("nr_types must be an integer or None, got %r" % (nr_types,))
    if types is None:
        t = 1 if nr_types is None else int(nr_types)
    else:
        if not isinstance(types, np.ndarray) or types.dtype != np.int32:
            raise TypeError("types must be an int32 numpy array [N] or None, got %s" % (getattr(types, "dtype", type(types).__name__),))
        if types.shape != (n,):
            raise ValueError("types %s is not parallel to xy %s" % (types.shape, (n, 2)))
        t = int(types.max()) + 1 if nr_types is None else int(nr_types)
    if not 1 <= t <= MAX_T:
        raise ValueError("%d types outside 1..%d" % (t, MAX_T))
    if types is not None and (int(types.min()) < 0 or int(types.max()) >= t):
        raise ValueError("types outside [0, %d)" % t)
    return None if types is None else np.ascontiguousarray(types), t


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
    caller's function, for the refusal of a device that is no GPU.  `run_grid` and `run_op` launch on the current stream without
    synchronising (the tools/*_bench.py time them apart); `run` is both, and `run().result()` a whole analysis, `result` being the
    subclass's readback."""

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

    def run_op(self):
        self._run(1)

    def run(self):
        self.run_grid()
        self.run_op()
        return self


# ---- the pipeline --------------------------------------------------------------------------------
ARGS = ("neighbours", "clusters", "density", "ripley", "regions")


class PointSpecs(collections.namedtuple("PointSpecs", ARGS)):
    """The five resolved arguments of the module docstring, None where off: (r, k), (r, k, "gabriel") or (r, k, "gabriel", True), (r, m, types tuple | None), (r, step),
    (radii tuple, window tuple | None) or (radii, window, sims, seed), a `regions.RegionSet` or `regions.RegionSpec`."""
    __slots__ = ()

    @property
    def any_annotation(self):
        """Whether the instance dict is needed: `neighbours` or `clusters` is on."""
        return self.neighbours is not None or self.clusters is not None


PointResults = collections.namedtuple("PointResults", ARGS[2:])        # what `summaries` returns: None where off


def resolve_specs(neighbours=None, clusters=None, density=None, ripley=None, regions=None, typed=True):
    """The five arguments as a caller gave them -> PointSpecs, or the ValueError / TypeError of the module's own `resolve`.
    typed=False (a model without a type branch) refuses "types" in `clusters`."""
    from . import clusters as CL
    from . import density as DN
    from . import neighbours as NB
    from . import regions as RG
    from . import ripley as RP

    return PointSpecs(NB.resolve(neighbours), CL.resolve(clusters, typed=typed), DN.resolve(density), RP.resolve(ripley), RG.resolve(regions))


def _device(device):
    return device if device is not None and device.type == "cuda" else None


def annotate(info, specs, nr_types, device):
    """Adds "neighbours", then "cluster", to every entry of a finished instance dict, as `specs` asks, and returns it.  `device`: a
    torch.device or None; the search runs there if it is a GPU and on the host otherwise."""
    from . import clusters as CL
    from . import neighbours as NB

    if specs.neighbours is not None:
        NB.annotate(info, specs.neighbours[0], specs.neighbours[1], nr_types, device=_device(device), graph=specs.neighbours[2] if len(specs.neighbours) >= 3 else None,
                    forest=len(specs.neighbours) == 4)
    if specs.clusters is not None:
        CL.annotate(info, specs.clusters[0], specs.clusters[1], nr_types, specs.clusters[2], device=_device(device))
    return info


def _density(info, size_hw, spec, nr_types, device):
    from . import density as DN

    return DN.of_info(info, size_hw, spec[0], spec[1], nr_types, device=device)


def _ripley(info, size_hw, spec, nr_types, device):
    from . import ripley as RP

    sims, seed = spec[2:] if len(spec) == 4 else (None, 0)
    return RP.of_info(info, size_hw, spec[0], nr_types, device=device, window=spec[1], sims=sims, seed=seed)


def _regions(info, _size_hw, rs, nr_types, device):
    from . import regions as RG

    rc = RG.of_info(info, rs, nr_types, device=device)
    RG.annotate(info, rc)
    return rc


# The summaries in the order they are computed and written.  The name is the field of PointSpecs and of PointResults, the output
# sub-directory, and the module whose `save(path, result)` writes the result.
_SUMMARIES = (("density", _density), ("ripley", _ripley), ("regions", _regions))


def summaries(info, size_hw, specs, nr_types, device):
    """PointResults(density, ripley, regions) of a finished instance dict over an image of size_hw = (h, w) processed pixels, as
    `specs` asks and None where it does not; with regions every entry gains "region".  `device` as in `annotate`."""
    return PointResults(*(None if getattr(specs, name) is None else of(info, size_hw, getattr(specs, name), nr_types, _device(device))
                          for name, of in _SUMMARIES))


def save_results(output_dir, name, results):
    """Writes `<output_dir>/<sub>/<name>.npz` for every result of a PointResults that is not None, with its module's `save`."""
    for sub, _ in _SUMMARIES:
        if getattr(results, sub) is not None:
            importlib.import_module("." + sub, __package__).save("%s/%s/%s.npz" % (output_dir, sub, name), getattr(results, sub))


def output_dirs(specs):
    """The sub-directories `save_results` writes into for `specs`: the summaries that are on."""
    return tuple(sub for sub, _ in _SUMMARIES if getattr(specs, sub) is not None)

"""Nuclei in annotated regions: which annotation polygons hold which nucleus, and how many nuclei of every type each region holds -- the
definition of the result, its host form, and the device form that returns the same integers (csrc/hvn_regions.hip).
Opt-in everywhere.  numpy only; imports without a GPU.

Regions.  A REGION is a list of polygons; a polygon is a list of rings, the first the exterior and the others holes, as in GeoJSON; a
ring is >= 3 finite float64 vertices (x, y), and a closing vertex that repeats the first is dropped.  G regions, G in 1..4096.

Edges.  Every ring edge (the last vertex joins the first) is made CANONICAL on the host: its endpoints are ordered so that ay < by.  An
edge with ay == by is dropped: it can never straddle a point.  The canonical edges are numbered in region order (region, polygon,
ring, vertex); E is their count, E <= 2^22.  `RegionSet.edges` is float64 [E, 4] = (ax, ay, bx, by), `edge_region` int32 [E].

Points.  `xy` float64 [N, 2] of (x, y) and `types` int32 [N] in [0, T) or None, admissible exactly where `neighbours._check` admits them
(N in 1..2^26, all finite, T <= 16).

The crossing rule.  Point P = (px, py) CROSSES the edge (ax, ay, bx, by) iff

    ay <= py  and  py < by                                      pure comparisons
    (px - ax) * (by - ay)  <  (bx - ax) * (py - ay)             IEEE float64, one rounding per operation, no fused multiply-add:
                                                                four differences, two products, and the products are COMPARED,
                                                                never subtracted

Membership.  P is inside region g iff it crosses an odd number of g's edges: even-odd over all rings of all polygons of g, so holes
and multipolygons need no special case.  The result, all int32:

    first[i]     the smallest g with point i inside, -1 if none
    hits[i]      the number of regions point i is inside (annotations overlap: a ROI around a tumour outline)
    count[g, t]  the number of points of type t inside region g (<= N <= 2^26; a type outside [0, T) is counted nowhere but the point
                 still gets first / hits -- this layer refuses such types, the device op still behaves)

Two properties of the definition (tests/test_regions_host.py checks both):
  (a) it is true point-in-polygon on exact inputs: on integer coordinates below 2^25 every difference and every product is exact, and
      the rule is the sign of the exact cross product on the half-open span ay <= py < by: a point is inside iff a ray towards -x
      meets the boundary an odd number of times, and a vertex belongs to exactly one of the two edges that meet in it;
  (b) shared edges are watertight: an edge that two regions share is stored in ONE orientation whichever way either ring runs, so
      both make the bit-identical decision on it, for any float64 vertices.  A point is never inside both neighbours of a
      tessellation, nor (inside the tessellated area) in neither.
Both sides of the product comparison are monotone in px, so an edge is a threshold on each scanline.

Floats are host only.  `area[g]` is the shoelace area of every polygon's exterior minus that of its holes, summed over the polygons of
g: the GeoJSON convention (holes lie inside their exterior, polygons of a region do not overlap), documented as such and NOT used by
membership.  `per_area(rc)` = count / area.

Three implementations: tests/regions_ref.py (all points x all edges, the definition's own inequalities: the oracle), `regions_host` and
`regions_device` (HVN_OP_NBR_GRID + HVN_OP_NBR_REGIONS).  The three agree with ==.

Row binning, shared by the host and the device form (`bin_rows`).  The points get the grid of points.py; its row of a y is
    row(y) = clamp(floor((y - y0) / c), 0, ncy - 1)
which is monotone in y (subtraction, division and floor are).  Every grid row gets the list of the edges with row(ay) <= row <=
row(by), in edge order, hence in region order.  A point with ay <= py < by has row(ay) <= row(py) <= row(by), so the list of a
point's row holds every edge the point can cross: the binning is exact, and edges that reach outside the points' extent land in the
clamped end rows.  The cell side (`cell_side`) aims at 256 points per row -- the workgroup of the kernel -- and grows by 1.25 until the lists
hold at most 8 E + ncy entries; an explicit `cell` replaces the aim, not the bound.  A wide cell (one row) is the brute-force form.

The lists' cull (`listed`), exact and by comparisons alone.  An edge is left out of every list when no point at all can cross it:
  * by <= min y or ay > max y of the points: the straddle test fails for every point;
  * max(ax, bx) <= min x of the points: with px >= ax, px >= bx and ay <= py < by, rounding being monotone, u = fl(px - ax) >= 0,
    d = fl(by - ay) > 0, 0 <= v = fl(py - ay) <= d and w = fl(bx - ax) <= u; for w <= 0 the right side fl(w v) <= 0 <= fl(u d), for
    w > 0 the exact products obey u d >= w v and so do their roundings: the left side is never below the right.
Without it the edges of a region that sticks out above or below the points would all pile up in the first or the last row.  The
oracle culls nothing.

The pipeline (`resolve`, `of_info`, `annotate`, `save`): `regions` = None or {"regions": RegionSet | list of regions | GeoJSON path or
dict} with an optional "scale", which multiplies every vertex once, in float64, before canonicalisation (QuPath exports level-0
pixels; the pipeline's points are pixels at proc_mag).  An optional "margin": [w_0, ..] (ascending widths in pixels of the processed
image, margins.py) adds the distance bands around every region's boundary: `resolve` then returns a `RegionSpec` (the RegionSet and the
widths), `of_info` of it a `RegionMargins` (the RegionCounts and the `margins.Margins`), `annotate` of that also sets "margin" on every
entry and `save` adds the margin_* arrays.  Without the key everything is as it was.
"""
import collections
import json
import os

import numpy as np

from . import points as P

MAX_G, MAX_E, MAX_T = 4096, 1 << 22, P.MAX_T
ROW_POINTS = 256                # points per grid row that `cell_side` aims at: the kernel's workgroup
_PAIRS = 1 << 22                # point-edge pairs per round of `regions_host`

RegionCounts = collections.namedtuple("RegionCounts", "first hits count names area")
RegionSpec = collections.namedtuple("RegionSpec", "regions widths")            # what `resolve` returns for a spec with "margin"
RegionMargins = collections.namedtuple("RegionMargins", "counts margins")      # what `of_info` returns for a RegionSpec


def max_entries(n_edges, ncy):
    """The bound on the row lists' total length."""
    return 8 * n_edges + ncy


def _check_scale(scale):
    if not P.is_number(scale):
        raise TypeError("scale must be a number, got %r" % (scale,))
    s = float(scale)
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError("scale = %r: it must be positive and finite" % (scale,))
    return s


def _check_ring(ring, where, scale):
    """One ring -> float64 [n, 2], scaled, without a repeated closing vertex; TypeError / ValueError."""
    if isinstance(ring, (str, bytes)) or not hasattr(ring, "__len__"):
        raise TypeError("%s: a ring is a sequence of (x, y), got %r" % (where, ring))
    pts = []
    if isinstance(ring, np.ndarray) and ring.ndim == 2 and ring.shape[1] >= 2 and ring.dtype.kind in "fiu":
        pts, ring = ring[:, :2].astype(np.float64), ()
    for v in ring:
        if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) < 2:
            raise TypeError("%s: a vertex is (x, y), got %r" % (where, v))
        if not (P.is_number(v[0]) and P.is_number(v[1])):
            raise TypeError("%s: a vertex holds numbers, got %r" % (where, v))
        pts.append((float(v[0]), float(v[1])))
    a = np.array(pts, np.float64).reshape(-1, 2)
    if not np.isfinite(a).all():
        raise ValueError("%s: a vertex is not finite" % where)
    with np.errstate(over="ignore"):
        a = a * scale
    if not np.isfinite(a).all():
        raise ValueError("%s: a scaled vertex is not finite" % where)
    if a.shape[0] >= 2 and (a[0] == a[-1]).all():
        a = a[:-1]
    if a.shape[0] < 3:
        raise ValueError("%s: a ring of %d vertices, fewer than 3" % (where, a.shape[0]))
    return a


def _check_polygons(regions, names, scale):
    """The regions as the definition names them -> (names, polygons as nested lists of float64 [n, 2] rings), or TypeError /
    ValueError, before any edge is made."""
    scale = _check_scale(scale)
    if isinstance(regions, (str, bytes, dict)) or not hasattr(regions, "__len__"):
        raise TypeError("regions must be a list of regions (lists of polygons, lists of rings), got %r" % (type(regions).__name__,))
    if not 1 <= len(regions) <= MAX_G:
        raise ValueError("%d regions outside 1..%d" % (len(regions), MAX_G))
    if names is None:
        names = ["region%d" % k for k in range(len(regions))]
    names = list(names)
    if len(names) != len(regions) or not all(isinstance(s, str) for s in names):
        raise ValueError("names must be %d strings" % len(regions))
    out, edges = [], 0
    for k, region in enumerate(regions):
        if isinstance(region, (str, bytes, dict)) or not hasattr(region, "__len__"):
            raise TypeError("region %d: a list of polygons, got %r" % (k, region))
        polys = []
        for p, poly in enumerate(region):
            if isinstance(poly, (str, bytes, dict)) or not hasattr(poly, "__len__") or len(poly) < 1:
                raise TypeError("region %d, polygon %d: a non-empty list of rings, got %r" % (k, p, poly))
            rings = [_check_ring(ring, "region %d, polygon %d, ring %d" % (k, p, i), scale) for i, ring in enumerate(poly)]
            edges += sum(r.shape[0] for r in rings)
            polys.append(rings)
        out.append(polys)
    if edges > MAX_E:
        raise ValueError("%d ring edges, more than 2^22" % edges)
    return names, out


def _ring_area(r):
    x, y = r[:, 0], r[:, 1]
    return abs(float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))) * 0.5


class RegionSet:
    """G named regions: `names` (list of str), `polygons` (per region a list of polygons, each a list of float64 [n, 2] rings, scaled),
    the canonical edge table `edges` float64 [E, 4] = (ax, ay, bx, by) with ay < by, `edge_region` int32 [E], ascending, and `area`
    float64 [G] (the module docstring's).  Built by `from_polygons` or `from_geojson`; read-only afterwards."""

    def __init__(self, names, polygons):
        self.names, self.polygons = list(names), polygons
        ea, eb, eg = [], [], []
        area = np.zeros(len(polygons), np.float64)
        for g, polys in enumerate(polygons):
            for rings in polys:
                for i, r in enumerate(rings):
                    area[g] += _ring_area(r) if i == 0 else -_ring_area(r)
                    ea.append(r)
                    eb.append(np.roll(r, -1, 0))
                    eg.append(np.full(r.shape[0], g, np.int32))
        a, b, eg = np.concatenate(ea), np.concatenate(eb), np.concatenate(eg)
        keep = a[:, 1] != b[:, 1]
        a, b, eg = a[keep], b[keep], eg[keep]
        swap = (a[:, 1] > b[:, 1])[:, None]
        self.edges = np.ascontiguousarray(np.concatenate([np.where(swap, b, a), np.where(swap, a, b)], 1))
        self.edge_region = np.ascontiguousarray(eg)
        self.area = area
        for arr in (self.edges, self.edge_region, self.area):
            arr.setflags(write=False)

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_polygons(cls, regions, names=None, scale=1.0):
        """`regions`: a list of regions, each a list of polygons, each a list of rings, each a sequence of (x, y).  `scale` multiplies
        every vertex once, in float64, before the edges are made canonical."""
        names, polygons = _check_polygons(regions, names, scale)
        return cls(names, polygons)

    @classmethod
    def from_geojson(cls, src, scale=1.0):
        """A GeoJSON `FeatureCollection`, a bare `Feature` or a bare geometry of type `Polygon` or `MultiPolygon`, as a dict or the path
        of a file (stdlib json).  One region per feature; its name is `properties.name`, else `properties.classification.name`, else
        "region<k>".  Any other geometry type is a ValueError that names it."""
        if isinstance(src, (str, bytes, os.PathLike)):
            with open(src) as handle:
                src = json.load(handle)
        if not isinstance(src, dict) or "type" not in src:
            raise ValueError("GeoJSON: an object with a \"type\" is needed, got %r" % (type(src).__name__,))
        if src["type"] == "FeatureCollection":
            feats = list(src.get("features") or [])
        else:
            feats = [src]
        regions, names = [], []
        for k, f in enumerate(feats):
            if not isinstance(f, dict):
                raise ValueError("GeoJSON: feature %d is %r" % (k, type(f).__name__))
            geom, props = (f.get("geometry"), f.get("properties") or {}) if f.get("type") == "Feature" else (f, {})
            kind = geom.get("type") if isinstance(geom, dict) else None
            if kind == "Polygon":
                regions.append([geom["coordinates"]])
            elif kind == "MultiPolygon":
                regions.append(list(geom["coordinates"]))
            else:
                raise ValueError("GeoJSON: feature %d has geometry type %r; only Polygon and MultiPolygon are regions" % (k, kind))
            name = props.get("name")
            if name is None and isinstance(props.get("classification"), dict):
                name = props["classification"].get("name")
            names.append(str(name) if name is not None else "region%d" % k)
        return cls.from_polygons(regions, names, scale)


def as_regions(rs, scale=1.0):
    """A RegionSet from what a caller may give: a RegionSet (scale must then be 1), a list of regions, a GeoJSON dict or a path."""
    if isinstance(rs, RegionSet):
        if _check_scale(scale) != 1.0:
            raise ValueError("a RegionSet is already scaled: scale = %r" % (scale,))
        return rs
    if isinstance(rs, (str, bytes, os.PathLike, dict)):
        _check_scale(scale)
        return RegionSet.from_geojson(rs, scale)
    return RegionSet.from_polygons(rs, None, scale)


def _check_set(rs):
    if not isinstance(rs, RegionSet):
        raise TypeError("rs must be a RegionSet (RegionSet.from_polygons / from_geojson), got %r" % (type(rs).__name__,))


def _check_counts(rs, types, n, nr_types):
    """The types of n points and the size of a RegionSet, or TypeError / ValueError: -> (types | None, T)."""
    types, t = P.check_types(types, n, nr_types)
    if len(rs) > MAX_G or rs.edges.shape[0] > MAX_E:
        raise ValueError("%d regions of %d edges, more than %d or 2^22" % (len(rs), rs.edges.shape[0], MAX_G))
    return types, t


def _check(xy, types, rs, nr_types, cell=None):
    """The inputs as the definition names them, or TypeError / ValueError, before any work: -> (xy, types | None, rs, T, cell | None)."""
    _check_set(rs)
    if cell is not None:
        cell = P.check_radius(cell)                                 # a cell side is admissible where a radius is
    xy = P.check_xy(xy)
    types, t = _check_counts(rs, types, xy.shape[0], nr_types)
    return xy, types, rs, t, cell


# ---- the rows ------------------------------------------------------------------------------------
def _rows_of(y, g):
    """row(y) of the module docstring for float64 [n] -> int64 [n]: the formula of `points.cells`."""
    with np.errstate(over="ignore"):
        return np.clip(np.floor((y - g.y0) / g.c), 0, g.ncy - 1).astype(np.int64)


def listed(xy, rs):
    """bool [E]: the edges that enter the row lists -- all but those the module docstring's cull proves no point can cross."""
    e = rs.edges
    return (e[:, 3] > xy[:, 1].min()) & (e[:, 1] <= xy[:, 1].max()) & (np.maximum(e[:, 0], e[:, 2]) > xy[:, 0].min())


def cell_side(xy, rs, cell=None):
    """The `radius` to hand to `points.grid` -> (r, Grid): about ROW_POINTS points per grid row (or `cell`), grown by 1.25 until the row
    lists hold at most 8 E + ncy entries."""
    n = xy.shape[0]
    ey = float(xy[:, 1].max()) - float(xy[:, 1].min())
    ex = float(xy[:, 0].max()) - float(xy[:, 0].min())
    r = cell if cell is not None else ey / max(1.0, min(float(P.MAX_AXIS - 1), n / float(ROW_POINTS)))
    if not (r * r >= P.MIN_R2 and np.isfinite(r * r)):               # all points on one scanline, or an absurd extent: one row
        r = max(1.0, ex, ey)
    e = rs.edges[listed(xy, rs)]
    while True:
        g = P.grid(xy, r)
        spans = _rows_of(e[:, 3], g) - _rows_of(e[:, 1], g) + 1
        if int(spans.sum()) <= max_entries(rs.edges.shape[0], g.ncy):
            return r, g
        r *= 1.25


def bin_rows(xy, rs, g):
    """The row lists of the module docstring on grid g -> (row_start int32 [ncy + 1], entries int32 [M]): the edges of row k are
    entries[row_start[k]:row_start[k + 1]], ascending, hence in region order.  M may be 0: then no point is in any region."""
    keep = np.flatnonzero(listed(xy, rs))
    r0, r1 = _rows_of(rs.edges[keep, 1], g), _rows_of(rs.edges[keep, 3], g)
    lens = r1 - r0 + 1
    m = int(lens.sum())
    edge = np.repeat(keep, lens)
    row = np.repeat(r0 - (np.cumsum(lens) - lens), lens) + np.arange(m, dtype=np.int64)
    order = np.argsort(row, kind="stable")                          # stable: ascending edge numbers inside a row
    start = np.zeros(g.ncy + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=g.ncy), out=start[1:])
    return start.astype(np.int32), edge[order].astype(np.int32)


def crosses(px, py, e):
    """The crossing rule for broadcastable point coordinates and edge columns e = (ax, ay, bx, by) -> bool."""
    ax, ay, bx, by = e
    with np.errstate(over="ignore", invalid="ignore"):
        return (ay <= py) & (py < by) & ((px - ax) * (by - ay) < (bx - ax) * (py - ay))


def _zero(n, g, t, rs):
    return RegionCounts(np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros((g, t), np.int32), list(rs.names), rs.area.copy())


# ---- the host --------------------------------------------------------------------------------------
def regions_host(xy, types, rs, nr_types=None, cell=None):
    """The definition on the host -> RegionCounts.  The points of one grid row are tested against that row's edge list only, in
    rounds of about 4 million point-edge pairs; the parity per region is a sum over the list's run of that region."""
    xy, types, rs, t, cell = _check(xy, types, rs, nr_types, cell)
    n, ng = xy.shape[0], len(rs)
    out = _zero(n, ng, t, rs)
    if not listed(xy, rs).any():
        return out
    _, g = cell_side(xy, rs, cell)
    row_start, entries = bin_rows(xy, rs, g)
    prow = _rows_of(xy[:, 1], g)
    order = np.argsort(prow, kind="stable")
    pstart = np.zeros(g.ncy + 1, np.int64)
    np.cumsum(np.bincount(prow, minlength=g.ncy), out=pstart[1:])
    ti = np.zeros(n, np.int64) if types is None else types.astype(np.int64)
    count = np.zeros(ng * t, np.int64)
    for k in np.flatnonzero((np.diff(pstart) > 0) & (np.diff(row_start) > 0)):
        idx = entries[row_start[k]:row_start[k + 1]]
        e = rs.edges[idx]
        eg = rs.edge_region[idx].astype(np.int64)
        head = np.flatnonzero(np.concatenate([[True], eg[1:] != eg[:-1]]))       # the runs of one region each
        regs = eg[head]
        step = max(1, _PAIRS // idx.shape[0])
        for a in range(int(pstart[k]), int(pstart[k + 1]), step):
            pts = order[a:min(a + step, int(pstart[k + 1]))]
            c = crosses(xy[pts, 0][:, None], xy[pts, 1][:, None], (e[:, 0], e[:, 1], e[:, 2], e[:, 3]))
            inside = (np.add.reduceat(c.astype(np.int32), head, axis=1) & 1).astype(bool)          # [points, runs]
            out.hits[pts] = inside.sum(1)
            any_in = inside.any(1)
            out.first[pts[any_in]] = regs[inside.argmax(1)[any_in]]
            pi, ri = np.nonzero(inside)
            count += np.bincount(regs[ri] * t + ti[pts[pi]], minlength=ng * t)
    out.count[...] = count.reshape(ng, t)
    return out


# ---- the device ----------------------------------------------------------------------------------
class NothingToTest(ValueError):
    """No edge of the regions can be crossed by any of the points (all horizontal, or all culled)."""


class DeviceRegions(P.DeviceGrid):
    """One device membership count (`points.DeviceGrid`: `run_grid`, `run_op`, `run`; on the grid of `cell_side`); `result` reads the one
    output buffer back.  The op writes every element of it: nothing is cleared here.  Regions without a single listed edge are refused with `NothingToTest`
    (`regions_device` launches nothing for them)."""

    def __init__(self, xy, types, rs, nr_types=None, device="cuda", cell=None):
        xy, types, rs, t, cell = _check(xy, types, rs, nr_types, cell)          # raises before anything is allocated or launched
        import torch

        if torch.device(device).type != "cuda":
            raise ValueError("regions_device needs a GPU device, got %r" % (device,))
        if not listed(xy, rs).any():
            raise NothingToTest("the regions have no edge that a point could cross: nothing to launch")
        r, g = cell_side(xy, rs, cell)
        super().__init__(xy, types, r, device, "regions_device", "OP_NBR_REGIONS")
        assert self.grid == g
        row_start, entries = bin_rows(xy, rs, g)
        self.t, self.rs, self.entries = t, rs, int(entries.shape[0])
        n, ng = xy.shape[0], len(rs)
        self.edges = torch.from_numpy(rs.edges.copy()).to(self.device)
        self.edge_region = torch.from_numpy(rs.edge_region.copy()).to(self.device)
        self.rows = torch.from_numpy(np.concatenate([row_start, entries])).to(self.device)
        self.out = self.empty(2 * n + ng * t)
        op = self._ops[1]
        op.cout, op._rsv, op.bias = t, ng, self.edges.data_ptr()
        op.res.base, op.res.h = self.edge_region.data_ptr(), rs.edges.shape[0]
        op.y2.base, op.y2.sn = self.rows.data_ptr(), self.entries
        op.y.base = self.out.data_ptr()

    def result(self):
        out = self.out.cpu().numpy()
        n = self.n
        return RegionCounts(out[:n].copy(), out[n:2 * n].copy(), out[2 * n:].reshape(len(self.rs), self.t).copy(), list(self.rs.names), self.rs.area.copy())


def regions_device(xy, types, rs, nr_types=None, device="cuda", cell=None):
    """`regions_host` on the GPU: the same integers.  The grid and the row lists are made here on the host; the device builds the grid
    and tests (two ops on the current stream); the one synchronisation is the readback.  Regions without a listed edge launch nothing."""
    try:
        return DeviceRegions(xy, types, rs, nr_types, device, cell).run().result()
    except NothingToTest:
        xy, types, rs, t, _ = _check(xy, types, rs, nr_types, cell)
        return _zero(xy.shape[0], len(rs), t, rs)


def regions(xy, types, rs, nr_types=None, device=None, cell=None):
    """`regions_host` with device=None, `regions_device` on `device` otherwise."""
    return regions_host(xy, types, rs, nr_types, cell) if device is None else regions_device(xy, types, rs, nr_types, device, cell)


# ---- what a user reads ---------------------------------------------------------------------------
def resolve(spec):
    """What a `regions` argument of the pipeline names: None -> None (off), {"regions": RegionSet | list of regions | GeoJSON dict or
    path} with an optional "scale" -> RegionSet; with a "margin": [w_0, ..] (margins.py's widths) -> RegionSpec(RegionSet, widths).
    ValueError / TypeError otherwise, before any work (the widths before the regions are read)."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or "regions" not in spec or not set(spec) <= {"regions", "scale", "margin"}:
        raise ValueError('regions=%r: None or {"regions": RegionSet | list | path} with an optional "scale" and an optional "margin"' % (spec,))
    if "margin" not in spec:
        return as_regions(spec["regions"], spec.get("scale", 1.0))
    from . import margins as MG

    widths = MG.check_widths(spec["margin"])
    return RegionSpec(as_regions(spec["regions"], spec.get("scale", 1.0)), widths)


def of_info(info, rs, nr_types, device=None):
    """The RegionCounts of an instance dict (`post_proc.process` / `process_images` / `WsiInference.run`): the centroids are the points,
    entry["type"] the types, as in `neighbours.annotate` (nr_types=None: untyped, T = 1); first / hits follow dict order.  An empty dict
    gives zero counts.  device=None: `regions_host`.  A RegionSpec for `rs` gives RegionMargins(that RegionCounts, the `margins.Margins`
    of the same dict for the spec's widths)."""
    if isinstance(rs, RegionSpec):
        from . import margins as MG

        return RegionMargins(of_info(info, rs.regions, nr_types, device), MG.of_info(info, rs.regions, rs.widths, nr_types, device))
    _check_set(rs)
    _, t = _check_counts(rs, None, 0, nr_types)
    if not info:
        return _zero(0, len(rs), t, rs)
    _, xy, types = P.from_info(info, nr_types)
    return regions(xy, types, rs, nr_types, device)


def annotate(info, rc):
    """Every entry of the dict that `rc` was made of gains "region": the int `first` of its nucleus (-1: in no region).  With a
    RegionMargins every entry also gains "margin": {"region": the name of the nearest region within the largest width | None,
    "distance": the distance to its boundary, negative inside it | None}."""
    if isinstance(rc, RegionMargins):
        from . import margins as MG

        annotate(info, rc.counts)
        m = rc.margins
        if len(info) != m.near.shape[0]:
            raise ValueError("%d entries, %d points in the Margins" % (len(info), m.near.shape[0]))
        for entry, g, d in zip(info.values(), m.near.tolist(), MG.signed_distance(m).tolist()):
            entry["margin"] = {"region": m.names[g] if g >= 0 else None, "distance": float(d) if g >= 0 else None}
        return info
    if len(info) != rc.first.shape[0]:
        raise ValueError("%d entries, %d points in the RegionCounts" % (len(info), rc.first.shape[0]))
    for entry, f in zip(info.values(), rc.first.tolist()):
        entry["region"] = int(f)
    return info


def per_area(rc):
    """float64 [G, T]: count / area, NaN where a region's area is 0."""
    out = np.full(rc.count.shape, np.nan)
    area = np.broadcast_to(np.asarray(rc.area, np.float64)[:, None], rc.count.shape)
    np.divide(rc.count.astype(np.float64), area, out=out, where=area > 0)
    return out


def save(path, rc):
    """A RegionCounts as an .npz of its five fields (what the managers write under regions/); a RegionMargins adds margin_widths,
    margin_count, margin_near, margin_d2 and margin_inside."""
    extra = {}
    if isinstance(rc, RegionMargins):
        rc, m = rc
        extra = dict(margin_widths=np.asarray(m.widths, np.float64), margin_count=m.count, margin_near=m.near, margin_d2=m.near_d2, margin_inside=m.near_inside)
    np.savez_compressed(path, count=rc.count, first=rc.first, hits=rc.hits, names=np.array(list(rc.names), dtype=np.str_).reshape(-1),
                        area=np.asarray(rc.area, np.float64), **extra)

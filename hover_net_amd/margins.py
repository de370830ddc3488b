"""Nuclei by distance to an annotation's boundary: the invasive margin.  For every nucleus the nearest annotated region within a
largest width W, its squared distance to that region's boundary and the side it lies on, and per region the typed counts of the nuclei
within each of B widths, inside and outside -- the definition of the result, its host form, and the device form that returns the same
numbers (csrc/hvn_margins.hip).  Opt-in everywhere.  numpy only; imports without a GPU.

Inputs.  A `regions.RegionSet`; points `xy` float64 [N, 2] and `types` int32 [N] or None, admissible exactly where `regions._check`
admits them; WIDTHS w_0 < w_1 < .. < w_{B-1}, B in 1..16, each admissible where `points.check_radius` admits a radius.
w2_k = w_k * w_k (`points.r2_of`), W = w_{B-1}.

Segments (`segments`).  EVERY ring edge of `RegionSet.polygons` (the last vertex of a ring joins the first), horizontal ones included
-- `RegionSet.edges` drops those, so it is no description of the boundary -- in region order (region, polygon, ring, vertex); S is
their count, S <= 2^22.  The endpoints of a segment (ax, ay, bx, by) are ordered so that (ay, ax) <= (by, bx) lexicographically: for
a non-horizontal edge that is exactly the orientation regions.py stores, and an edge that two regions share is one bit-identical
segment in both.  The BOX of a segment is made once, on the host:
    (fl(xlo - W), fl(ylo - W), fl(xhi + W), fl(yhi + W))        xlo = min(ax, bx), xhi = max(ax, bx), ylo = ay, yhi = by

Distance.  IEEE float64, one rounding per operation, nothing fused.  For a point (px, py) and a segment:
    ux = bx - ax   uy = by - ay   vx = px - ax   vy = py - ay
    dot  = ux*vx + uy*vy          len2 = ux*ux + uy*uy
    dot <= 0     : d2 = vx*vx + vy*vy
    dot >= len2  : d2 = (px-bx)*(px-bx) + (py-by)*(py-by)
    otherwise    : c = ux*vy - uy*vx ;  d2 = (c*c) / len2        (len2 > 0 here: the only division)
A segment is NEAR a point iff the point lies in its box -- box[0] <= px <= box[2] and box[1] <= py <= box[3], comparisons only, a NaN
compares false on both sides -- and d2 <= w2_{B-1}.  The box test is PART OF THE DEFINITION, and the oracle applies it too: it is what
makes binning by rows exact without an error analysis of d2.  It differs from the geometric truth (d <= W) only for points within
rounding of W of the box: a point whose true distance is W up to a few ulps may fall on the other side of fl(xlo - W).

Per (point i, region g):
    inside     the parity of `regions.crosses` over g's segments (a horizontal one is never crossed): the membership of regions.py
    dmin2      the minimum of d2 over g's near segments, +inf if there are none

The result `Margins`, its integers exact:
    near[i]         int32    the region with the smallest dmin2 <= w2_{B-1}, ties to the smallest g; -1 if there is none
    near_d2[i]      float64  that dmin2, +inf if there is none
    near_inside[i]  int32    1 or 0 with respect to that region, -1 if there is none
    count[g, side, k, t]  int32  the points of type t with dmin2(i, g) <= w2_k; side 0 is outside g, side 1 inside; cumulative in k,
                    as `ripley.PairCounts` is in r.  A point near several regions is counted for each.  types None: T = 1.
    widths, names   the widths (tuple of float) and the regions' names
`rings(m)` are the first differences over k, `signed_distance(m)` is -sqrt(near_d2) inside and +sqrt(near_d2) outside (NaN where near
< 0; the one square root, host only), `profile(m, g)` the [2 B, T] table a margin plot is drawn from: the rings from the deepest inside
band to the farthest outside band.

Three implementations: tests/margins_ref.py (all points x all segments in scalar Python floats, the lines above: the oracle),
`margins_host` and `margins_device` (HVN_OP_NBR_GRID + HVN_OP_NBR_MARGINS).  The three agree with ==, near_d2 included.

Row lists, shared by the host and the device form (`bin_rows`): the scheme of `regions.bin_rows` with the dilated span.  A segment
enters every grid row k with row(box[1]) <= k <= row(box[3]); row is monotone, so the list of a point's row holds every segment whose
box contains the point, and every segment the point can cross, because ay <= py < by implies box[1] <= py <= box[3] (W > 0 and
rounding is monotone).  The entries of a row ascend, hence are in region order.  The cell side (`cell_side`) is that of
`regions.cell_side`, grown by 1.25 until the lists hold at most 8 S + ncy entries.

The lists' cull (`listed`), exact and by comparisons alone.  A segment whose box misses the points' bounding box is near no point;
it is left out of every list unless a point can still CROSS it.  A box that misses above, below or on the left cannot be crossed
(regions.py's cull: by <= min y, ay > max y, max(ax, bx) <= min x, each implied by the box's miss).  A box that misses on the RIGHT can:
the crossing rule counts the edges to the right of a point, so the far side of a large region decides the parity of a point near its
left side.  Such a segment stays listed, by regions.py's own three comparisons.  The lists may be empty (M = 0): the result is then all
-1 / +inf / 0.  The oracle culls nothing.

The pipeline: `regions.resolve` takes an optional "margin": [w_0, ..] in the `regions` spec (pixels of the processed image) and the
result of `regions.of_info` then carries a `Margins` beside the `RegionCounts` (regions.py).
"""
import collections

import numpy as np

from . import points as P
from . import regions as RG

MAX_B, MAX_S = 16, 1 << 22
_PAIRS = 1 << 20                # point-segment pairs per round of `margins_host`

Margins = collections.namedtuple("Margins", "near near_d2 near_inside count widths names")


def max_entries(n_segments, ncy):
    """The bound on the row lists' total length."""
    return 8 * n_segments + ncy


def check_widths(widths):
    """The widths as the module docstring names them -> tuple of float, or TypeError / ValueError."""
    if isinstance(widths, (str, bytes, dict)) or not hasattr(widths, "__len__"):
        raise TypeError("margin widths must be a sequence of numbers, got %r" % (widths,))
    if not 1 <= len(widths) <= MAX_B:
        raise ValueError("%d margin widths outside 1..%d" % (len(widths), MAX_B))
    for w in widths:
        if not P.is_number(w):
            raise TypeError("a margin width must be a number, got %r" % (w,))
    out = tuple(P.check_radius(w) for w in widths)
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("margin widths %r are not strictly ascending" % (list(widths),))
    return out


def _check(xy, types, rs, widths, nr_types, cell=None):
    """The inputs as the definition names them, or TypeError / ValueError, before any work: -> (xy, types | None, rs, T, cell | None,
    widths)."""
    RG._check_set(rs)
    widths = check_widths(widths)
    xy, types, rs, t, cell = RG._check(xy, types, rs, nr_types, cell)
    if sum(r.shape[0] for polys in rs.polygons for rings in polys for r in rings) > MAX_S:
        raise ValueError("more than 2^22 ring edges")
    return xy, types, rs, t, cell, widths


# ---- the segments ----------------------------------------------------------------------------------
def segments(rs, width):
    """The segment table float64 [S, 4] = (ax, ay, bx, by) with (ay, ax) <= (by, bx), the region of each segment int32 [S], ascending,
    and the boxes float64 [S, 4] for the largest width `width` (the module docstring's)."""
    ea, eb, eg = [], [], []
    for g, polys in enumerate(rs.polygons):
        for rings in polys:
            for r in rings:
                ea.append(r)
                eb.append(np.roll(r, -1, 0))
                eg.append(np.full(r.shape[0], g, np.int32))
    a, b, eg = np.concatenate(ea), np.concatenate(eb), np.concatenate(eg)
    swap = ((a[:, 1] > b[:, 1]) | ((a[:, 1] == b[:, 1]) & (a[:, 0] > b[:, 0])))[:, None]
    seg = np.ascontiguousarray(np.concatenate([np.where(swap, b, a), np.where(swap, a, b)], 1))
    w = float(width)
    with np.errstate(over="ignore"):
        box = np.stack([np.minimum(seg[:, 0], seg[:, 2]) - w, seg[:, 1] - w, np.maximum(seg[:, 0], seg[:, 2]) + w, seg[:, 3] + w], 1)
    return seg, np.ascontiguousarray(eg), np.ascontiguousarray(box)


def d2_of(px, py, s):
    """d2 of the module docstring for broadcastable point coordinates and segment columns s = (ax, ay, bx, by)."""
    ax, ay, bx, by = s
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ux, uy, vx, vy = bx - ax, by - ay, px - ax, py - ay
        dot, len2 = ux * vx + uy * vy, ux * ux + uy * uy
        wx, wy = px - bx, py - by
        c = ux * vy - uy * vx
        return np.where(dot <= 0, vx * vx + vy * vy, np.where(dot >= len2, wx * wx + wy * wy, (c * c) / len2))


def in_box(px, py, b):
    """The box test for broadcastable point coordinates and box columns b -> bool."""
    return (b[0] <= px) & (px <= b[2]) & (b[1] <= py) & (py <= b[3])


# ---- the rows --------------------------------------------------------------------------------------
def listed(xy, seg, box):
    """bool [S]: the segments that enter the row lists -- those whose box meets the points' bounding box, and those a point could
    still cross (the module docstring's cull)."""
    x0, y0, x1, y1 = xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()
    near = (box[:, 0] <= x1) & (box[:, 2] >= x0) & (box[:, 1] <= y1) & (box[:, 3] >= y0)
    cross = (seg[:, 1] < seg[:, 3]) & (seg[:, 3] > y0) & (seg[:, 1] <= y1) & (np.maximum(seg[:, 0], seg[:, 2]) > x0)
    return near | cross


def cell_side(xy, box, keep, cell=None):
    """The `radius` to hand to `points.grid` -> (r, Grid): `regions.cell_side` over the dilated spans of the listed segments."""
    n, s = xy.shape[0], box.shape[0]
    ey = float(xy[:, 1].max()) - float(xy[:, 1].min())
    ex = float(xy[:, 0].max()) - float(xy[:, 0].min())
    r = cell if cell is not None else ey / max(1.0, min(float(P.MAX_AXIS - 1), n / float(RG.ROW_POINTS)))
    if not (r * r >= P.MIN_R2 and np.isfinite(r * r)):               # all points on one scanline, or an absurd extent: one row
        r = max(1.0, ex, ey)
    b = box[keep]
    while True:
        g = P.grid(xy, r)
        spans = RG._rows_of(b[:, 3], g) - RG._rows_of(b[:, 1], g) + 1
        if int(spans.sum()) <= max_entries(s, g.ncy):
            return r, g
        r *= 1.25


def bin_rows(box, keep, g):
    """The row lists of the module docstring on grid g -> (row_start int32 [ncy + 1], entries int32 [M]): the segments of row k are
    entries[row_start[k]:row_start[k + 1]], ascending, hence in region order.  M may be 0."""
    keep = np.flatnonzero(keep)
    r0, r1 = RG._rows_of(box[keep, 1], g), RG._rows_of(box[keep, 3], g)
    lens = r1 - r0 + 1
    m = int(lens.sum())
    seg = np.repeat(keep, lens)
    row = np.repeat(r0 - (np.cumsum(lens) - lens), lens) + np.arange(m, dtype=np.int64)
    order = np.argsort(row, kind="stable")                          # stable: ascending segment numbers inside a row
    start = np.zeros(g.ncy + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=g.ncy), out=start[1:])
    return start.astype(np.int32), seg[order].astype(np.int32)


def _none(n, ng, b, t, widths, rs):
    return Margins(np.full(n, -1, np.int32), np.full(n, np.inf, np.float64), np.full(n, -1, np.int32), np.zeros((ng, 2, b, t), np.int32),
                   tuple(widths), list(rs.names))


def _cumulative(hist, ng, b, t):
    """count [G, 2, B, T] int32 from the ring counts in the device's layout: an integer running sum over k."""
    return np.cumsum(np.asarray(hist, np.int64).reshape(ng, 2, b, t), axis=2).astype(np.int32)


# ---- the host --------------------------------------------------------------------------------------
def margins_host(xy, types, rs, widths, nr_types=None, cell=None):
    """The definition on the host -> Margins.  The points of one grid row are tested against that row's segment list only, in rounds
    of about a million point-segment pairs; parity and minimum per region run over the list's run of that region.  The points of a
    row are taken in ascending x, so a round's points span [xa, xb]: a segment with box[2] < xa is near none of them and crossed by
    none (max(ax, bx) <= box[2] < px: the cull of regions.py) and is skipped; one with box[0] > xb is near none and only its crossings
    are tested.  Comparisons alone: the numbers do not change."""
    xy, types, rs, t, cell, widths = _check(xy, types, rs, widths, nr_types, cell)
    n, ng, nb = xy.shape[0], len(rs), len(widths)
    out = _none(n, ng, nb, t, widths, rs)
    seg, sreg, box = segments(rs, widths[-1])
    keep = listed(xy, seg, box)
    if not keep.any():
        return out
    w2 = np.array([P.r2_of(w) for w in widths], np.float64)
    _, g = cell_side(xy, box, keep, cell)
    row_start, entries = bin_rows(box, keep, g)
    prow = RG._rows_of(xy[:, 1], g)
    order = np.lexsort((xy[:, 0], prow))                             # by row, then by x
    pstart = np.zeros(g.ncy + 1, np.int64)
    np.cumsum(np.bincount(prow, minlength=g.ncy), out=pstart[1:])
    ti = np.zeros(n, np.int64) if types is None else types.astype(np.int64)
    hist = np.zeros(ng * 2 * nb * t, np.int64)
    for k in np.flatnonzero((np.diff(pstart) > 0) & (np.diff(row_start) > 0)):
        idx = entries[row_start[k]:row_start[k + 1]]
        row_s, row_b, row_g = seg[idx].T, box[idx].T, sreg[idx].astype(np.int64)
        step = max(1, _PAIRS // idx.shape[0])
        for a in range(int(pstart[k]), int(pstart[k + 1]), step):
            pts = order[a:min(a + step, int(pstart[k + 1]))]
            px, py = xy[pts, 0][:, None], xy[pts, 1][:, None]
            live = np.flatnonzero(row_b[2] >= px[0, 0])             # px ascends: px[0] is xa, px[-1] is xb
            if live.shape[0] == 0:
                continue
            s, b, eg = row_s[:, live], row_b[:, live], row_g[live]
            head = np.flatnonzero(np.concatenate([[True], eg[1:] != eg[:-1]]))   # the runs of one region each
            regs = eg[head]
            inside = np.add.reduceat(RG.crosses(px, py, s).astype(np.int32), head, axis=1) & 1          # [points, runs]
            d2 = np.full((pts.shape[0], live.shape[0]), np.inf)
            cols = np.flatnonzero(b[0] <= px[-1, 0])
            if cols.shape[0]:
                d = d2_of(px, py, s[:, cols])
                with np.errstate(invalid="ignore"):
                    d2[:, cols] = np.where(in_box(px, py, b[:, cols]) & (d <= w2[-1]), d, np.inf)
            dmin = np.minimum.reduceat(d2, head, axis=1)                                               # [points, runs]
            rows = np.arange(pts.shape[0])
            j = dmin.argmin(1)                                      # the first minimum: the smallest region
            best = dmin[rows, j]
            has = best <= w2[-1]
            out.near[pts[has]] = regs[j[has]]
            out.near_d2[pts[has]] = best[has]
            out.near_inside[pts[has]] = inside[rows, j][has]
            pi, ri = np.nonzero(dmin <= w2[-1])
            kmin = np.searchsorted(w2, dmin[pi, ri], side="left")   # the first k with dmin2 <= w2_k
            hist += np.bincount(((regs[ri] * 2 + inside[pi, ri]) * nb + kmin) * t + ti[pts[pi]], minlength=hist.shape[0])
    out.count[...] = _cumulative(hist, ng, nb, t)
    return out


# ---- the device ----------------------------------------------------------------------------------
class DeviceMargins(P.DeviceGrid):
    """One device margin profile (`points.DeviceGrid`: `run_grid`, `run_op`, `run`; on the grid of `cell_side`); `result` reads the one
    output buffer back.  The op writes every element of it: nothing is cleared here.  Empty row lists (M = 0) are run like any other:
    the op then writes the all-none result.  cull=False selects the kernel form without the x-cull of the staged tile (the same
    numbers; tools/margins_bench.py times the two)."""

    def __init__(self, xy, types, rs, widths, nr_types=None, device="cuda", cell=None, cull=True):
        xy, types, rs, t, cell, widths = _check(xy, types, rs, widths, nr_types, cell)          # raises before anything is allocated or launched
        import torch

        if torch.device(device).type != "cuda":
            raise ValueError("margins_device needs a GPU device, got %r" % (device,))
        seg, sreg, box = segments(rs, widths[-1])
        keep = listed(xy, seg, box)
        r, g = cell_side(xy, box, keep, cell)
        super().__init__(xy, types, r, device, "margins_device", "OP_NBR_MARGINS")
        assert self.grid == g
        row_start, entries = bin_rows(box, keep, g)
        self.t, self.rs, self.widths, self.entries = t, rs, widths, int(entries.shape[0])
        n, ng, nb = xy.shape[0], len(rs), len(widths)
        self.seg = torch.from_numpy(np.ascontiguousarray(np.concatenate([seg, box], 1))).to(self.device)
        self.seg_region = torch.from_numpy(sreg).to(self.device)
        self.w2 = torch.tensor([P.r2_of(w) for w in widths], dtype=torch.float64, device=self.device)
        self.rows = torch.from_numpy(np.concatenate([row_start, entries])).to(self.device)
        self.out = self.empty(4 * n + 2 * ng * nb * t)
        op = self._ops[1]
        op.cout, op._rsv, op.cout2, op.bias, op.w2, op.stride = t, ng, nb, self.seg.data_ptr(), self.w2.data_ptr(), 0 if cull else 1
        op.res.base, op.res.h = self.seg_region.data_ptr(), seg.shape[0]
        op.y2.base, op.y2.sn = self.rows.data_ptr(), self.entries
        op.y.base, op.y.sn = self.out.data_ptr(), 4 * self.out.numel()

    def result(self):
        out = self.out.cpu().numpy()
        n, ng, nb = self.n, len(self.rs), len(self.widths)
        return Margins(out[2 * n:3 * n].copy(), out[:2 * n].view(np.float64).copy(), out[3 * n:4 * n].copy(),
                       _cumulative(out[4 * n:], ng, nb, self.t), tuple(self.widths), list(self.rs.names))


def margins_device(xy, types, rs, widths, nr_types=None, device="cuda", cell=None):
    """`margins_host` on the GPU: the same numbers.  The segments, their boxes, the grid and the row lists are made here on the host;
    the device builds the grid and tests (two ops on the current stream); the one synchronisation is the readback."""
    return DeviceMargins(xy, types, rs, widths, nr_types, device, cell).run().result()


def margins(xy, types, rs, widths, nr_types=None, device=None, cell=None):
    """`margins_host` with device=None, `margins_device` on `device` otherwise."""
    return margins_host(xy, types, rs, widths, nr_types, cell) if device is None else margins_device(xy, types, rs, widths, nr_types, device, cell)


# ---- what a user reads ---------------------------------------------------------------------------
def of_info(info, rs, widths, nr_types, device=None):
    """The Margins of an instance dict, as `regions.of_info` reads it (centroids, entry["type"], dict order).  An empty dict gives
    zero counts."""
    RG._check_set(rs)
    widths = check_widths(widths)
    _, t = RG._check_counts(rs, None, 0, nr_types)
    if not info:
        return _none(0, len(rs), len(widths), t, widths, rs)
    _, xy, types = P.from_info(info, nr_types)
    return margins(xy, types, rs, widths, nr_types, device)


def rings(m):
    """int32 [G, 2, B, T]: the points in band k alone -- w_{k-1} < distance <= w_k, band 0 from the boundary itself."""
    return np.diff(m.count, axis=2, prepend=0).astype(np.int32)


def signed_distance(m):
    """float64 [N]: the distance to the boundary of the nearest region, negative inside it, NaN where near < 0."""
    d = np.full(m.near.shape, np.nan)
    has = m.near >= 0
    d[has] = np.where(m.near_inside[has] == 1, -1.0, 1.0) * np.sqrt(m.near_d2[has])
    return d


def profile(m, g):
    """int32 [2 B, T] for region g: the rings from the deepest inside band (row 0) to the farthest outside band (row 2 B - 1)."""
    r = rings(m)[g]
    return np.concatenate([r[1, ::-1], r[0]], 0)

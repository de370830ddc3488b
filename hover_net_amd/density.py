"""Nucleus density maps: the number of nuclei of every type within a radius of every node of a regular raster -- the definition of the
result, its host form, and the device form that returns the same integers (csrc/hvn_density.hip).  Opt-in
everywhere.  numpy only; imports without a GPU.

Inputs: `xy` float64 [N, 2] of (x, y) and `types` int32 [N] in [0, T) or None (then T = 1 and every type is 0), admissible exactly
where `neighbours._check` admits them (N in 1..2^26, all finite, T <= 16); `radius` r, likewise; a raster (ox, oy, s, W, H): `ox`, `oy`
finite, `s` > 0 finite, `W`, `H` integers in 1..16384 with T H W <= 2^28, and ox + (W - 1) s, oy + (H - 1) s finite.  All arithmetic
is IEEE float64, one rounding per operation, no fused multiply-add:

    px(u) = ox + (u * s);  py(v) = oy + (v * s)                       u in [0, W), v in [0, H), converted exactly
    dx = xj - px(u);  dy = yj - py(v);  d2 = (dx * dx) + (dy * dy);  r2 = r * r          (`neighbours.d2_of`, `neighbours.r2_of`)
    count[t, v, u] = #{ j : types[j] == t and d2 <= r2 }

A point that sits exactly on a node (d2 == 0) is counted: nodes are not points, so there is no j != i here.  A type outside [0, T) is
counted in no channel (this layer refuses such types; the device op still behaves).  The output is `count`, int32 [T, H, W], a
function of the inputs alone.

Three implementations: tests/density_ref.py (all (node, point) pairs in chunks, the oracle), `density_host` (a scatter of every point
over the nodes of its bounding box: a million points on a 512 x 512 raster are feasible without a GPU) and `density_device`
(HVN_OP_NBR_GRID + HVN_OP_NBR_DENSITY).  The three agree with ==.

The window of `density_host`.  px is non-decreasing in u (u * s, its rounding and the addition are monotone), so the nodes a point
can reach on one axis are a contiguous run, found by bisection on the float64 node positions themselves -- no division by s, hence
nothing to argue about origins far larger than the step, where neighbouring nodes round to one position.  With B = fl(r (1 + 2^-40))
the run is  pred(fl(x - B)) <= p <= succ(fl(x + B))  (pred, succ: the neighbouring float64).  Why it holds every node with d2 <= r2:
  * d2 <= r2 gives |fl(dx)| <= r (1 + 2^-52) (neighbours.py, first step of its argument; `_check` refuses a radius whose square is
    not a normal number), and B > r (1 + 2^-41) exceeds that;
  * let z = x - B as a real number and f = fl(z).  z is at least as near to f as to pred(f), so z > pred(f).  A node p < pred(f)
    has x - p > B as real numbers, rounding is monotone and B is a float64, so fl(x - p) >= B > r (1 + 2^-52): the test fails.  The
    upper end is the mirror image.  An overflow of x -+ B gives an infinite bound, which excludes nothing.
Wider windows are slower, never wrong: every pair of the window is still decided by d2 <= r2.

The grid of `density_device` is `neighbours.grid(xy, r)`, built from the POINTS, unchanged; a node's cell comes from the same formula
and the same clamp (csrc: hvn_nbr_axis).  Nodes may lie far outside the points' extent.  The 3 x 3 cells around the clamped node cell
still hold every point with d2 <= r2:
  * a point's own cell needs no clamp (the grid spans the extent), so clamping moves the node's cell TOWARDS the cells of the points,
    never away from one: a difference of at most one cell per axis before the clamp is at most one after it;
  * the per-axis argument of neighbours.py uses nothing about i but that (xi, yi) are float64 and |xj - xi| <= r (1 + 2^-51), so it
    applies to any node that has a neighbour at all: such a node lies within r (1 + 2^-51) of the extent, its true cell coordinate is
    in (-1, 4097) and the two computed coordinates differ by less than 1;
  * a node without a neighbour only sees candidates that fail the test, whichever cells the clamp gave it.

The pipeline raster (`raster_of`, `of_info`) for an image of h x w processed pixels and an integer step >= 1: W = ceil(w / step),
H = ceil(h / step), ox = oy = (step - 1) / 2 (exact), s = step: node (u, v) is the centre of the pixel block [u step, (u + 1) step) x
[v step, (v + 1) step), so the map lines up with the image downsampled by `step`.
"""
import collections
import math

import numpy as np

from . import neighbours as NB
from . import points as P

MAX_AXIS, MAX_NODES, MAX_T = 16384, 1 << 28, NB.MAX_T
_PAIRS = 1 << 22                # (node, point) pairs per round of `density_host`
_WIDEN = 1.0 + 2.0 ** -40       # B = r * _WIDEN in the module docstring

workspace_bytes = NB.workspace_bytes        # the one workspace of HVN_OP_NBR_GRID, which HVN_OP_NBR_DENSITY reads

Raster = collections.namedtuple("Raster", "ox oy s W H")
DensityMap = collections.namedtuple("DensityMap", "count origin step radius")


def _check_raster(raster, t):
    """A raster as the definition names it, for T = t channels, or TypeError / ValueError: -> Raster of floats and ints."""
    if isinstance(raster, (str, bytes)) or not hasattr(raster, "__len__") or len(raster) != 5:
        raise TypeError("raster must be (ox, oy, s, W, H), got %r" % (raster,))
    ox, oy, s, w, h = raster
    if not (P.is_number(ox) and P.is_number(oy) and P.is_number(s)):
        raise TypeError("raster (ox, oy, s) must be numbers, got %r" % ((ox, oy, s),))
    if not (P.is_integer(w) and P.is_integer(h)):
        raise TypeError("raster (W, H) must be integers, got %r" % ((w, h),))
    ox, oy, s, w, h = float(ox), float(oy), float(s), int(w), int(h)
    if not (np.isfinite(ox) and np.isfinite(oy)):
        raise ValueError("raster origin (%r, %r) is not finite" % (ox, oy))
    if not (s > 0.0 and np.isfinite(s)):
        raise ValueError("raster step = %r: it must be positive and finite" % (s,))
    if not (1 <= w <= MAX_AXIS and 1 <= h <= MAX_AXIS):
        raise ValueError("a raster of %d x %d nodes: each axis must be in 1..%d" % (h, w, MAX_AXIS))
    if t * h * w > MAX_NODES:
        raise ValueError("%d planes of %d x %d nodes, more than 2^28 in all" % (t, h, w))
    with np.errstate(over="ignore", invalid="ignore"):
        last = np.array([ox, oy]) + (np.array([w - 1.0, h - 1.0]) * s)
    if not np.isfinite(last).all():
        raise ValueError("the last node of the raster is not at a finite float64")
    return Raster(ox, oy, s, w, h)


def _check(xy, types, radius, raster, nr_types):
    """The inputs as the definition names them, or TypeError / ValueError: -> (xy, types | None, r, Raster, T)."""
    xy, r = P.check_xy(xy), P.check_radius(radius)
    types, t = P.check_types(types, xy.shape[0], nr_types)
    return xy, types, r, _check_raster(raster, t), t


def nodes(raster):
    """(px float64 [W], py float64 [H]): the docstring's node positions of a checked raster."""
    return raster.ox + (np.arange(raster.W, dtype=np.float64) * raster.s), raster.oy + (np.arange(raster.H, dtype=np.float64) * raster.s)


def _window(p, x, b):
    """Per point, the run [a, e) of the sorted node positions p that the module docstring's window holds."""
    with np.errstate(over="ignore"):
        lo, hi = np.nextafter(x - b, -np.inf), np.nextafter(x + b, np.inf)
    return np.searchsorted(p, lo, side="left").astype(np.int64), np.searchsorted(p, hi, side="right").astype(np.int64)


# ---- the host --------------------------------------------------------------------------------------
def density_host(xy, types, radius, raster, nr_types=None):
    """The definition on the host -> count int32 [T, H, W].  Every point is scattered over the nodes of its window (module docstring),
    in rounds of about 4 million (node, point) pairs; a point whose window alone is larger is worked off in bands of node rows."""
    xy, types, r, ra, t = _check(xy, types, radius, raster, nr_types)
    n, (px, py) = xy.shape[0], nodes(ra)
    r2 = NB.r2_of(r)
    ua, ub = _window(px, xy[:, 0], r * _WIDEN)
    va, vb = _window(py, xy[:, 1], r * _WIDEN)
    wl, hl = ub - ua, vb - va
    tj = np.zeros(n, np.int64) if types is None else types.astype(np.int64)
    flat = np.zeros(t * ra.H * ra.W, np.int32)

    def scatter(idx, ua_, wl_, va_, hl_):
        """Items (point idx[i], nodes [ua_[i], ua_[i] + wl_[i]) x [va_[i], va_[i] + hl_[i])): every pair is tested and counted."""
        area = wl_ * hl_
        total = int(area.sum())
        if total == 0:
            return
        it = np.repeat(np.arange(idx.shape[0], dtype=np.int64), area)
        k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(area) - area, area)     # the pair's number inside its item
        u, v, j = ua_[it] + k % wl_[it], va_[it] + k // wl_[it], idx[it]
        keep = NB.d2_of(px[u], py[v], xy[j, 0], xy[j, 1]) <= r2
        key, cnt = np.unique((tj[j[keep]] * ra.H + v[keep]) * ra.W + u[keep], return_counts=True)
        flat[key] += cnt.astype(np.int32)

    area = wl * hl
    ends = np.cumsum(area)
    a = 0
    while a < n:
        b = P.round_end(ends, a, _PAIRS)
        if b == a + 1 and area[a] > _PAIRS:
            rows = max(1, _PAIRS // int(wl[a]))
            for v0 in range(int(va[a]), int(vb[a]), rows):
                scatter(np.array([a]), ua[a:b], wl[a:b], np.array([v0]), np.array([min(rows, int(vb[a]) - v0)]))
        else:
            scatter(np.arange(a, b, dtype=np.int64), ua[a:b], wl[a:b], va[a:b], hl[a:b])
        a = b
    return flat.reshape(t, ra.H, ra.W)


# ---- the device ----------------------------------------------------------------------------------
class DeviceDensity(P.DeviceGrid):
    """One device density map (`points.DeviceGrid`: `run_grid`, `run_op`, `run`; the grid is that of the points); `result` reads the
    map back.  The op writes every element of `count`: nothing is cleared here."""

    def __init__(self, xy, types, radius, raster, nr_types=None, device="cuda"):
        import torch

        xy, types, r, ra, t = _check(xy, types, radius, raster, nr_types)      # raises before anything is allocated or launched
        super().__init__(xy, types, r, device, "density_device", "OP_NBR_DENSITY")
        self.t, self.raster = t, ra
        self.raster_table = torch.tensor([ra.ox, ra.oy, ra.s], dtype=torch.float64, device=self.device)
        self.count = self.empty((t, ra.H, ra.W))
        op = self._ops[1]
        op.cout, op.bias = t, self.raster_table.data_ptr()
        op.y.base, op.y.h, op.y.w = self.count.data_ptr(), ra.H, ra.W

    def result(self):
        return self.count.cpu().numpy()


def density_device(xy, types, radius, raster, nr_types=None, device="cuda"):
    """`density_host` on the GPU: the same array.  The grid is chosen here on the host; the device builds it and counts (two ops on
    the current stream); the one synchronisation is the readback."""
    return DeviceDensity(xy, types, radius, raster, nr_types, device).run().result()


def density(xy, types, radius, raster, nr_types=None, device=None):
    """`density_host` with device=None, `density_device` on `device` otherwise."""
    return density_host(xy, types, radius, raster, nr_types) if device is None else density_device(xy, types, radius, raster, nr_types, device)


# ---- what a user reads ---------------------------------------------------------------------------
def resolve(spec):
    """What a `density` argument of the pipeline names: None -> None (off), {"radius": r, "step": s} -> (r, s): the radius in pixels
    of the processed image, the step an integer >= 1 of such pixels between nodes.  ValueError / TypeError otherwise, before any
    work."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or set(spec) != {"radius", "step"}:
        raise ValueError('density=%r: None or {"radius": r, "step": s}' % (spec,))
    r = P.check_radius(spec["radius"])
    if not P.is_integer(spec["step"]):
        raise TypeError("step must be an integer, got %r" % (spec["step"],))
    if int(spec["step"]) < 1:
        raise ValueError("step = %d, below 1" % spec["step"])
    return r, int(spec["step"])


def raster_of(size_hw, step):
    """The pipeline raster of the module docstring for an image of size_hw = (h, w) processed pixels."""
    h, w = (int(v) for v in size_hw)
    if not P.is_integer(step) or int(step) < 1:
        raise ValueError("step = %r: an integer >= 1" % (step,))
    if h < 1 or w < 1:
        raise ValueError("an image of %d x %d pixels" % (h, w))
    step = int(step)
    o = (step - 1) / 2.0
    return Raster(o, o, float(step), -(-w // step), -(-h // step))


def of_info(info, size_hw, radius, step, nr_types, device=None):
    """The density map of an instance dict (`post_proc.process` / `process_images` / `WsiInference.run`) over an image of
    size_hw = (h, w) processed pixels -> DensityMap(count int32 [T, H, W], origin (ox, oy), step, radius) on the pipeline raster.
    The centroids are the points, entry["type"] the types, as in `neighbours.annotate` (nr_types=None: untyped, T = 1).  An empty dict
    gives an all-zero map.  device=None: `density_host`."""
    ra = raster_of(size_hw, step)
    P.check_radius(radius)
    _, t = P.check_types(None, 0, nr_types)
    ra = _check_raster(ra, t)
    if not info:
        return DensityMap(np.zeros((t, ra.H, ra.W), np.int32), (ra.ox, ra.oy), int(step), float(radius))
    _, xy, types = P.from_info(info, nr_types)
    return DensityMap(density(xy, types, radius, ra, nr_types, device), (ra.ox, ra.oy), int(step), float(radius))


def save(path, dm):
    """A DensityMap as an .npz of `count`, `origin`, `step`, `radius` (what the managers write under density/)."""
    np.savez_compressed(path, count=dm.count, origin=np.asarray(dm.origin, np.float64), step=np.int64(dm.step), radius=np.float64(dm.radius))


def _count(dm):
    return np.asarray(dm.count if isinstance(dm, DensityMap) else dm)


def total(dm):
    """The sum over the channels of a DensityMap (or of a count array [T, H, W]): int64 [H, W]."""
    return _count(dm).sum(0, dtype=np.int64)


def fraction(dm, t):
    """float64 [H, W]: count[t] / total, NaN where the total is 0."""
    c, tot = _count(dm), total(dm)
    out = np.full(tot.shape, np.nan)
    np.divide(c[t].astype(np.float64), tot.astype(np.float64), out=out, where=tot > 0)
    return out


def per_area(dm, mpp):
    """float64 [T, H, W]: nuclei per mm^2 of the disc pi r^2 around every node, for `mpp` microns per processed pixel."""
    if not P.is_number(mpp) or not (mpp > 0 and np.isfinite(mpp)):
        raise ValueError("mpp = %r: microns per pixel, positive and finite" % (mpp,))
    r_mm = float(dm.radius) * float(mpp) / 1000.0
    return dm.count.astype(np.float64) / (math.pi * r_mm * r_mm)


def hot_spots(plane, n, min_sep):
    """The n densest nodes of an integer plane [H, W], at least `min_sep` nodes apart -> int64 rows (v, u, count).  Nodes are visited
    in order (-count, v, u); a node is accepted unless its count is 0 or an accepted node lies within `min_sep` nodes of it
    (dv^2 + du^2 <= min_sep^2, in integers); at most n are accepted."""
    plane = np.asarray(plane)
    if plane.ndim != 2 or plane.dtype.kind not in "iu":
        raise ValueError("hot_spots takes an integer plane [H, W], got %s %s" % (plane.dtype, plane.shape))
    if not P.is_integer(n) or n < 0 or not P.is_integer(min_sep) or min_sep < 0:
        raise ValueError("n = %r and min_sep = %r must be non-negative integers" % (n, min_sep))
    v, u = np.nonzero(plane > 0)
    c = plane[v, u].astype(np.int64)
    o = np.lexsort((u, v, -c))
    v, u, c = v[o].astype(np.int64), u[o].astype(np.int64), c[o]
    out, sep2 = np.zeros((0, 3), np.int64), int(min_sep) * int(min_sep)
    for i in range(v.shape[0]):
        if out.shape[0] >= n:
            break
        if out.shape[0] and ((out[:, 0] - v[i]) ** 2 + (out[:, 1] - u[i]) ** 2 <= sep2).any():
            continue
        out = np.concatenate([out, np.array([[v[i], u[i], c[i]]], np.int64)])
    return out

"""Cross-type Ripley K: the number of ordered pairs of nuclei of types (a, b) within each of a list of radii, with the border edge
correction -- the definition of the result, its host form, and the device form that returns the same integers (csrc/hvn_pairs.hip,
DESIGN.md 4.21).  Opt-in everywhere.  numpy only; imports without a GPU.

Inputs: `xy` float64 [N, 2] of (x, y) and `types` int32 [N] in [0, T) or None (then T = 1 and every type is 0), admissible exactly
where `neighbours._check` admits them (N in 1..2^26, all finite, T <= 16); `radii`: 1..32 finite numbers > 0, strictly ascending,
r_0 < .. < r_{R-1}, each admissible as a radius of neighbours.py; `window` = (wx0, wy0, wx1, wy1), finite, wx0 < wx1 and wy0 < wy1;
T = nr_types (1 when untyped) with T T R <= 4096.  All arithmetic is IEEE float64, one rounding per operation, no fused multiply-add:

    r2_k = r_k * r_k                                                     (`points.r2_of`)
    dx = xj - xi;  dy = yj - yi;  d2 = (dx * dx) + (dy * dy)             (`points.d2_of`)
    kmin(i, j) = the smallest k with d2 <= r2_k                          (d2 > r2_{R-1}: none, the pair is not counted)
    b_i = min(x_i - wx0, wx1 - x_i, y_i - wy0, wy1 - y_i)                each term one subtraction
    m_i = #{ k : r_k <= b_i }                                            a prefix of the radii, because they ascend

A point on or outside the window's edge has m_i = 0; it still counts as a j.  The result, all int64:

    pairs[a, b, k]     = #{ (i, j) : j != i, type_i = a, type_j = b, d2 <= r2_k }
    pairs_in[a, b, k]  = the same with the added condition b_i >= r_k       (the border method: i lies at least r_k inside the window)
    n[a]               = the number of points of type a
    n_in[a, k]         = #{ i : type_i = a, b_i >= r_k }

A type outside [0, T) lands in no bin, as i or as j (this layer refuses such types; the device op still behaves).  Coincident points
(d2 == 0, j != i) are pairs at every radius.  pairs[a, b] == pairs[b, a], because d2 is symmetric bit for bit; pairs_in need not be.

The accumulator.  Both forms count into acc int64 [2, T, T, R], per pair with a kmin:
    acc[0, a, b, kmin] += 1
    acc[1, a, b, kmin] += 1  and, where m_i < R,  acc[1, a, b, m_i] -= 1          only if kmin < m_i
and pairs, pairs_in = acc.cumsum(-1).  Plane 1 is a difference array: its running sum at k counts the pairs with kmin <= k < m_i, and
kmin <= k is d2 <= r2_k (r2 does not descend), k < m_i is r_k <= b_i.

Three implementations: tests/ripley_ref.py (all pairs in chunks, the definition's own inequalities per k: the oracle), `pairs_host`
(`points.candidate_runs` / `pair_rounds` on the grid `points.grid(xy, r_{R-1})`, so the 3 x 3-cell argument of neighbours.py holds
unchanged; kmin and m_i by bisection) and `pairs_device` (HVN_OP_NBR_GRID + HVN_OP_NBR_PAIRS).  The three agree with ==.  n and n_in
are O(N R) numpy on the host in every form.

Floats (`K`, `L`, `rings`) are plain numpy on those integers, on the host only:
    K[a, b, k] = area * pairs_in[a, b, k] / (n_in[a, k] * n[b])           NaN where the denominator is 0
with area = the window's by default.  For a == b the denominator uses n[b], not n[b] - 1: the intensity estimate is n / area for
every type alike, so K of one type and K across types are on one scale (the difference is a factor (n - 1) / n).  L = sqrt(K / pi);
`rings` are the counts between consecutive radii, the integers behind a pair-correlation curve.

The pipeline (`resolve`, `window_of`, `of_info`): `ripley` = None or {"radii": [r, ..]} with an optional "window": (wx0, wy0, wx1,
wy1); without it the window of an image of h x w processed pixels is (-0.5, -0.5, w - 0.5, h - 0.5), the extent of the pixels with
their centres on the integers: exact, and of area h w.
"""
import collections
import math

import numpy as np

from . import points as P

MAX_R, MAX_BINS, MAX_T = 32, 4096, P.MAX_T
_PAIRS = 1 << 22                # candidate pairs per round of `pairs_host`

PairCounts = collections.namedtuple("PairCounts", "pairs pairs_in n n_in radii window")


def _check_radii(radii):
    """1..32 radii, each one neighbours.py admits, strictly ascending -> float64 [R], or TypeError / ValueError."""
    if isinstance(radii, (str, bytes)) or not hasattr(radii, "__len__"):
        raise TypeError("radii must be a sequence of numbers, got %r" % (radii,))
    radii = list(radii)
    if not 1 <= len(radii) <= MAX_R:
        raise ValueError("%d radii outside 1..%d" % (len(radii), MAX_R))
    out = np.array([P.check_radius(r) for r in radii], np.float64)
    if not (np.diff(out) > 0.0).all():
        raise ValueError("radii %r are not strictly ascending" % (radii,))
    return out


def _check_window(window):
    """(wx0, wy0, wx1, wy1), finite, wx0 < wx1 and wy0 < wy1 -> a tuple of floats, or TypeError / ValueError."""
    if isinstance(window, (str, bytes)) or not hasattr(window, "__len__") or len(window) != 4:
        raise TypeError("window must be (wx0, wy0, wx1, wy1), got %r" % (window,))
    if not all(P.is_number(v) for v in window):
        raise TypeError("window must hold numbers, got %r" % (window,))
    w = tuple(float(v) for v in window)
    if not np.isfinite(w).all():
        raise ValueError("window %r is not finite" % (window,))
    if not (w[0] < w[2] and w[1] < w[3]):
        raise ValueError("window %r: wx0 < wx1 and wy0 < wy1" % (window,))
    return w


def _check(xy, types, radii, window, nr_types):
    """The inputs as the definition names them, or TypeError / ValueError: -> (xy, types | None, radii float64 [R], window, T)."""
    rr, xy = _check_radii(radii), P.check_xy(xy)
    types, t = P.check_types(types, xy.shape[0], nr_types)
    return xy, types, rr, _check_bins(window, t, rr), t


def _check_bins(window, t, rr):
    """A checked window, for t types and the checked radii rr whose bins are not too many."""
    win = _check_window(window)
    if t * t * rr.shape[0] > MAX_BINS:
        raise ValueError("%d x %d types and %d radii, more than %d bins" % (t, t, rr.shape[0], MAX_BINS))
    return win


def border(xy, window):
    """b of the definition for checked inputs: float64 [N]."""
    wx0, wy0, wx1, wy1 = window
    return np.minimum(np.minimum(xy[:, 0] - wx0, wx1 - xy[:, 0]), np.minimum(xy[:, 1] - wy0, wy1 - xy[:, 1]))


def _m_of(xy, rr, window):
    """m of the definition: int64 [N]."""
    return np.searchsorted(rr, border(xy, window), side="right").astype(np.int64)


def _finish(acc, xy, types, rr, window, t):
    """PairCounts of a filled accumulator: the running sums, and n, n_in on the host."""
    acc = np.asarray(acc, np.int64).reshape(2, t, t, rr.shape[0])
    ti = np.zeros(xy.shape[0], np.int64) if types is None else types.astype(np.int64)
    ok = (ti >= 0) & (ti < t)
    n = np.bincount(ti[ok], minlength=t).astype(np.int64)
    inside = border(xy, window)[:, None] >= rr[None, :]                           # [N, R]
    n_in = np.zeros((t, rr.shape[0]), np.int64)
    np.add.at(n_in, ti[ok], inside[ok].astype(np.int64))
    return PairCounts(acc[0].cumsum(-1), acc[1].cumsum(-1), n, n_in, rr.copy(), tuple(window))


# ---- the host --------------------------------------------------------------------------------------
def pairs_host(xy, types, radii, window, nr_types=None):
    """The definition on the host -> PairCounts.  Candidates come from the grid of the largest radius (three contiguous runs of the
    cell-ordered points per query), in rounds of about 4 million pairs; kmin and m are bisections, the accumulator the docstring's."""
    xy, types, rr, win, t = _check(xy, types, radii, window, nr_types)
    n, nr = xy.shape[0], rr.shape[0]
    r2 = P.r2_of(rr)
    g = P.grid(xy, float(rr[-1]))
    order, lo, hi, _, _ = P.candidate_runs(xy, g)
    sx, sy = xy[order, 0], xy[order, 1]
    st = np.zeros(n, np.int64) if types is None else types[order].astype(np.int64)
    sm = _m_of(xy, rr, win)[order]
    acc = np.zeros(2 * t * t * nr, np.int64)
    plane = t * t * nr
    for _a, _b, qi, cand, d2 in P.pair_rounds(sx, sy, lo, hi, float(r2[-1]), _PAIRS):
        keep = cand != qi
        qi, cand, d2 = qi[keep], cand[keep], d2[keep]
        kmin = np.searchsorted(r2, d2, side="left").astype(np.int64)
        row, m = (st[qi] * t + st[cand]) * nr, sm[qi]
        acc[:plane] += np.bincount(row + kmin, minlength=plane)
        inner = kmin < m
        acc[plane:] += np.bincount((row + kmin)[inner], minlength=plane)
        drop = inner & (m < nr)
        acc[plane:] -= np.bincount((row + m)[drop], minlength=plane)
    return _finish(acc, xy, types, rr, win, t)


# ---- the device ----------------------------------------------------------------------------------
class DeviceRipley(P.DeviceGrid):
    """One device pair count (`points.DeviceGrid`: `run_grid`, `run_op`, `run`; on the grid of the largest radius); `result` reads the
    accumulator back and finishes it on the host.  The op writes every element of `acc`: nothing is cleared here."""

    def __init__(self, xy, types, radii, window, nr_types=None, device="cuda"):
        import torch

        xy, types, rr, win, t = _check(xy, types, radii, window, nr_types)      # raises before anything is allocated or launched
        super().__init__(xy, types, float(rr[-1]), device, "pairs_device", "OP_NBR_PAIRS")
        self.t, self.radii, self.window, self._xy, self._types = t, rr, win, xy, types
        self.rt = torch.tensor(list(win) + rr.tolist() + P.r2_of(rr).tolist(), dtype=torch.float64, device=self.device)
        self.acc = self.empty((2, t, t, rr.shape[0]), torch.int64)
        op = self._ops[1]
        op.cout, op._rsv, op.bias = t, rr.shape[0], self.rt.data_ptr()
        op.y.base = self.acc.data_ptr()

    def result(self):
        return _finish(self.acc.cpu().numpy(), self._xy, self._types, self.radii, self.window, self.t)


def pairs_device(xy, types, radii, window, nr_types=None, device="cuda"):
    """`pairs_host` on the GPU: the same integers.  The grid is chosen here on the host; the device builds it and counts (two ops on
    the current stream); the one synchronisation is the readback of the accumulator."""
    return DeviceRipley(xy, types, radii, window, nr_types, device).run().result()


def pairs(xy, types, radii, window, nr_types=None, device=None):
    """`pairs_host` with device=None, `pairs_device` on `device` otherwise."""
    return pairs_host(xy, types, radii, window, nr_types) if device is None else pairs_device(xy, types, radii, window, nr_types, device)


# ---- what a user reads ---------------------------------------------------------------------------
def resolve(spec):
    """What a `ripley` argument of the pipeline names: None -> None (off), {"radii": [r, ..]} with an optional "window": (wx0, wy0,
    wx1, wy1) -> (radii tuple, window tuple | None), in pixels of the processed image; without a window the image's own is used
    (`window_of`).  ValueError / TypeError otherwise, before any work."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or "radii" not in spec or not set(spec) <= {"radii", "window"}:
        raise ValueError('ripley=%r: None or {"radii": [r, ..]} with an optional "window"' % (spec,))
    rr = _check_radii(spec["radii"])
    win = None if spec.get("window") is None else _check_window(spec["window"])
    return tuple(rr.tolist()), win


def window_of(size_hw):
    """The window of an image of size_hw = (h, w) processed pixels: the extent of the pixels, their centres on the integers."""
    h, w = (int(v) for v in size_hw)
    if h < 1 or w < 1:
        raise ValueError("an image of %d x %d pixels" % (h, w))
    return (-0.5, -0.5, w - 0.5, h - 0.5)


def of_info(info, size_hw, radii, nr_types, device=None, window=None):
    """The PairCounts of an instance dict (`post_proc.process` / `process_images` / `WsiInference.run`) over an image of size_hw =
    (h, w) processed pixels, with `window_of(size_hw)` unless a window is given.  The centroids are the points, entry["type"] the
    types, as in `neighbours.annotate` (nr_types=None: untyped, T = 1).  An empty dict gives zeros.  device=None: `pairs_host`."""
    win = window_of(size_hw) if window is None else window
    rr, (_, t) = _check_radii(radii), P.check_types(None, 0, nr_types)
    win = _check_bins(win, t, rr)
    if not info:
        z = np.zeros((t, t, rr.shape[0]), np.int64)
        return PairCounts(z, z.copy(), np.zeros(t, np.int64), np.zeros((t, rr.shape[0]), np.int64), rr, win)
    _, xy, types = P.from_info(info, nr_types)
    return pairs(xy, types, rr, win, nr_types, device)


def area_of(window):
    return (window[2] - window[0]) * (window[3] - window[1])


def K(pc, area=None):
    """float64 [T, T, R]: area * pairs_in[a, b, k] / (n_in[a, k] * n[b]), NaN where the denominator is 0; `area` defaults to the
    window's.  n[b], not n[b] - 1, also for a == b (module docstring)."""
    area = area_of(pc.window) if area is None else float(area)
    den = pc.n_in[:, None, :].astype(np.float64) * pc.n[None, :, None].astype(np.float64)
    out = np.full(den.shape, np.nan)
    np.divide(area * pc.pairs_in.astype(np.float64), den, out=out, where=den > 0)
    return out


def L(pc, area=None):
    """float64 [T, T, R]: sqrt(K / pi); a random pattern has L(r) = r."""
    return np.sqrt(K(pc, area) / math.pi)


def rings(pc):
    """int64 [T, T, R]: pairs_in between consecutive radii (r_{k-1}, r_k], the first from 0: np.diff with a leading 0.  Note that the
    set of admitted i shrinks with k, so a ring is a difference of two border-corrected counts, not a count of its own."""
    return np.diff(pc.pairs_in, axis=-1, prepend=0)


def save(path, pc):
    """A PairCounts as an .npz of its six fields (what the managers write under ripley/)."""
    np.savez_compressed(path, pairs=pc.pairs, pairs_in=pc.pairs_in, n=pc.n, n_in=pc.n_in, radii=np.asarray(pc.radii, np.float64),
                        window=np.asarray(pc.window, np.float64))

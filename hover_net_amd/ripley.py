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
their centres on the integers: exact, and of area h w.  With "sims": S (and an optional "seed") the result is a `LabelSims`.

Significance: the random-labelling test.  L(r) = r is the benchmark of a homogeneous pattern only; nuclei are clumped,
so whether a count exceeds chance is asked of the SAME positions with the types permuted among them, S times.  Inputs as above, plus
`sims` = S in 1..9999 and `seed` in [0, 2^64); integer arithmetic is uint64 with wrap-around; the result depends on (xy, types, radii,
window, nr_types, seed) and on nothing else, and simulation s is the same whatever S is.

    mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31        (splitmix64's finaliser)
    key[s][p] = mix(mix(seed + 0x9E3779B97F4A7C15 * (s + 1)) + p)          p = 0..7; formed on the host (`round_keys`), uploaded
    b = max(2, bit_length(N - 1));  hl = b // 2;  hh = b - hl
    F_s(x) on [0, 2^b):  lo = x & (2^hl - 1);  hi = x >> hl;  for p = 0..7:  hi ^= mix(lo + key[s][p]) & (2^hh - 1) if p is even,
                         lo ^= mix(hi + key[s][p]) & (2^hl - 1) if p is odd;  the result is (hi << hl) | lo
    pi_s(i) = the first of F_s(i), F_s(F_s(i)), .. below N                  (`permutation`)
    type_s[i] = types[pi_s(i)]                                             i the point's position in xy

Every round is an involution, so F_s is a bijection of [0, 2^b) and pi_s, by cycle walking, one of [0, N): nothing is sorted or stored.
The walk ends after at most 2^b - N + 1 steps (the cycle of a value below N holds at most the 2^b - N values that are not, then one that
is); fewer than 2 are expected, since 2^b < 2 N for N >= 3.  Untyped points (T = 1) give the observed counts in every simulation.  The
result, int64:
    pairs_in[s, a, b, k], n_in[s, a, k] = pairs_in and n_in of the definition above under labelling s
n and the uncorrected `pairs` are not simulated: n is invariant, and K, L and rings read pairs_in only.  `LabelSims` = (observed, pairs_in,
n_in, seed), `observed` the unchanged PairCounts of the true labels.  Three implementations: tests/ripley_sims_ref.py (scalar Python
integers for the permutation, the all-pairs oracle per labelling), `sims_host` (the candidate geometry of `pairs_host` once per round and
per chunk of simulations) and `sims_device` (HVN_OP_NBR_GRID once, HVN_OP_NBR_PAIRS for the observed counts, then HVN_OP_NBR_PAIRS_SIM per
batch of simulations: csrc/hvn_pairs_sim.hip tests a pair's geometry once per batch and makes only the typed adds per simulation).  Both
count, per simulation, plane 1 of the accumulator above and cnt[a][m] = the points of type a with m_i = m, from which n_in[a, k] is the
sum of cnt[a][m] over m > k.  The three agree with ==.

`K_sims`, `envelope` and `p_value` are plain numpy on those integers: K's formula per simulation, the rank-th smallest and largest K_s per
bin (a pointwise two-sided level of 2 rank / (S + 1)), and the Monte-Carlo p-value (1 + #{s : K_s >= K_obs}) / (S + 1), ties counted.
"""
import collections
import ctypes
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


# ---- random labelling: the host ----------------------------------------------------------------------
MAX_SIMS = 9999
_HOST_SIMS = 32                 # simulations per pass over the candidate geometry in `sims_host`
_BATCH = 8                      # simulations per HVN_OP_NBR_PAIRS_SIM, where the histograms fit (`batch_of`): the fastest measured
_GOLDEN, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)

LabelSims = collections.namedtuple("LabelSims", "observed pairs_in n_in seed")


def _check_sims(sims, seed):
    """S in 1..9999 and a seed in [0, 2^64) -> (int, int), or TypeError / ValueError."""
    if not P.is_integer(sims) or not P.is_integer(seed):
        raise TypeError("sims and seed must be integers, got %r and %r" % (sims, seed))
    if not 1 <= int(sims) <= MAX_SIMS:
        raise ValueError("sims = %r outside 1..%d" % (sims, MAX_SIMS))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed = %r outside [0, 2^64)" % (seed,))
    return int(sims), int(seed)


def _mix(z):
    """mix of the docstring on a uint64 array (which wraps around)."""
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def round_keys(seed, sims):
    """key of the docstring: uint64 [S, 8]."""
    s = np.arange(1, sims + 1, dtype=np.uint64)
    return _mix(_mix(np.array([seed], np.uint64) + _GOLDEN * s)[:, None] + np.arange(8, dtype=np.uint64)[None, :])


def _walk(n, keys_s):
    """pi_s of the docstring for the eight keys of one simulation -> (int64 [n], the longest walk)."""
    b = max(2, (n - 1).bit_length())
    hl = b // 2
    ml, mh = np.uint64((1 << hl) - 1), np.uint64((1 << (b - hl)) - 1)
    keys_s = np.asarray(keys_s, np.uint64)
    out, idx, x, steps = np.empty(n, np.int64), np.arange(n), np.arange(n, dtype=np.uint64), 0
    while idx.size:
        lo, hi = x & ml, x >> np.uint64(hl)
        for p in range(0, 8, 2):
            hi = hi ^ (_mix(lo + keys_s[p]) & mh)
            lo = lo ^ (_mix(hi + keys_s[p + 1]) & ml)
        x = (hi << np.uint64(hl)) | lo
        steps += 1
        if steps > (1 << b) - n + 1:
            raise AssertionError("the walk of %d points passed %d steps" % (n, (1 << b) - n + 1))
        done = x < np.uint64(n)
        out[idx[done]] = x[done].astype(np.int64)
        idx, x = idx[~done], x[~done]
    return out, steps


def permutation(n, keys_s):
    """pi_s of the docstring, a permutation of [0, n), for the eight round keys of one simulation: int64 [n]."""
    return _walk(int(n), keys_s)[0]


def _n_in_of(cnt):
    """n_in [.., T, R] of cnt [.., T, R + 1]: the points of type a with m > k."""
    return np.ascontiguousarray(cnt[..., ::-1].cumsum(-1)[..., ::-1][..., 1:])


def sims_host(xy, types, radii, window, nr_types=None, sims=None, seed=0):
    """The random-labelling test on the host -> LabelSims.  The candidates and their kmin, m are formed once per round and per chunk of
    `_HOST_SIMS` simulations; each simulation then costs the typed bincounts of plane 1 only."""
    xy, types, rr, win, t = _check(xy, types, radii, window, nr_types)
    nsim, seed = _check_sims(sims, seed)
    observed = pairs_host(xy, types, rr, win, t)
    n, nr = xy.shape[0], rr.shape[0]
    keys = round_keys(seed, nsim)
    r2 = P.r2_of(rr)
    order, lo, hi, _, _ = P.candidate_runs(xy, P.grid(xy, float(rr[-1])))
    sx, sy = xy[order, 0], xy[order, 1]
    m_pos = _m_of(xy, rr, win)
    sm = m_pos[order]
    base = np.zeros(n, np.int64) if types is None else types.astype(np.int64)
    plane = t * t * nr
    acc, cnt = np.zeros((nsim, plane), np.int64), np.zeros((nsim, t, nr + 1), np.int64)
    for s0 in range(0, nsim, _HOST_SIMS):
        lab = np.stack([base[permutation(n, keys[s])] for s in range(s0, min(nsim, s0 + _HOST_SIMS))])       # by position
        for j in range(lab.shape[0]):
            cnt[s0 + j] = np.bincount(lab[j] * (nr + 1) + m_pos, minlength=t * (nr + 1)).reshape(t, nr + 1)
        st = lab[:, order]
        for _a, _b, qi, cand, d2 in P.pair_rounds(sx, sy, lo, hi, float(r2[-1]), _PAIRS):
            kmin = np.searchsorted(r2, d2, side="left").astype(np.int64)
            keep = (cand != qi) & (kmin < sm[qi])
            qi, cand, kmin = qi[keep], cand[keep], kmin[keep]
            m = sm[qi]
            drop = m < nr
            for j in range(lab.shape[0]):
                row = (st[j, qi] * t + st[j, cand]) * nr
                acc[s0 + j] += np.bincount(row + kmin, minlength=plane) - np.bincount((row + m)[drop], minlength=plane)
    return LabelSims(observed, acc.reshape(nsim, t, t, nr).cumsum(-1), _n_in_of(cnt), seed)


# ---- random labelling: the device --------------------------------------------------------------------
_MAX_SB, _MAX_LDS = 32, 140 * 1024          # HVN_NBR_PAIRS_SIM_MAX_SB, HVN_NBR_PAIRS_SIM_MAX_LDS of csrc/hvn_kernels.h


def _lds_bytes(sb, bins):
    """HVN_NBR_PAIRS_SIM_LDS_BYTES: SB histograms, and a label word per four simulations for 1024 staged candidates and 256 lanes."""
    return 4 * sb * bins + 4 * (1024 + 256) * ((sb + 3) // 4)


def batch_of(t, nr):
    """SB, the simulations of one HVN_OP_NBR_PAIRS_SIM: `_BATCH`, or as many as fit a workgroup's LDS (8 at the cap of 4096 bins)."""
    sb = max(1, min(int(_BATCH), _MAX_SB))
    while sb > 1 and _lds_bytes(sb, t * t * nr) > _MAX_LDS:
        sb -= 1
    return sb


class DeviceRipleySims(P.DeviceGrid):
    """The random-labelling test on the device (`points.DeviceGrid`, on the grid of the largest radius, built once): `run_observed` is
    HVN_OP_NBR_PAIRS for the true labels, `run_op(batch)` HVN_OP_NBR_PAIRS_SIM for the simulations [batch SB, (batch + 1) SB) -- the
    last batch may be short -- and `run` all of them; `result` reads the integers back and finishes them on the host.  The ops write
    every element of their outputs: nothing is cleared here."""

    def __init__(self, xy, types, radii, window, nr_types=None, sims=None, seed=0, device="cuda"):
        import torch

        from . import lib as L
        from . import plan as PL

        xy, types, rr, win, t = _check(xy, types, radii, window, nr_types)      # raises before anything is allocated or launched
        nsim, seed = _check_sims(sims, seed)
        super().__init__(xy, types, float(rr[-1]), device, "sims_device", "OP_NBR_PAIRS_SIM")
        nr = rr.shape[0]
        self.t, self.radii, self.window, self.sims, self.seed, self._xy, self._types = t, rr, win, nsim, seed, xy, types
        self.sb = batch_of(t, nr)
        self.batches = (nsim + self.sb - 1) // self.sb
        self.rt = torch.tensor(list(win) + rr.tolist() + P.r2_of(rr).tolist(), dtype=torch.float64, device=self.device)
        self.keys = torch.from_numpy(round_keys(seed, nsim).view(np.int64)).to(self.device)         # the bits of the uint64 keys
        self.labels = self.empty((xy.shape[0], (self.sb + 3) // 4))
        self.acc = self.empty((2, t, t, nr), torch.int64)
        self.out = self.empty((nsim, t * t * nr + t * (nr + 1)), torch.int64)
        op = self._ops[1]
        op.cout, op._rsv, op.bias = t, nr, self.rt.data_ptr()
        op.res.base = None if self.types is None else self.types.data_ptr()
        op.y2.base, op.y2.sn = self.labels.data_ptr(), 4 * self.labels.numel()
        obs = L.hvn_op()                                                        # HVN_OP_NBR_PAIRS on the same grid and tables
        ctypes.memmove(ctypes.addressof(obs), ctypes.addressof(op), ctypes.sizeof(obs))
        obs.kind, obs.y.base = PL.OP_NBR_PAIRS, self.acc.data_ptr()
        self._ops.append(obs)

    def run_observed(self):
        self._run(2)

    def run_op(self, batch=0, phase=0):
        """The op of one batch; phase 1 and 2 are its two launches alone (the labels, the pairs), for timing."""
        op, s0 = self._ops[1], batch * self.sb
        if not 0 <= s0 < self.sims:
            raise ValueError("batch %r outside 0..%d" % (batch, self.batches - 1))
        op.nbatch, op.stride = min(self.sb, self.sims - s0), phase
        op.w2, op.y.base = self.keys[s0].data_ptr(), self.out[s0].data_ptr()
        self._run(1)

    def run(self):
        self.run_grid()
        self.run_observed()
        for batch in range(self.batches):
            self.run_op(batch)
        return self

    def result(self):
        t, nr = self.t, self.radii.shape[0]
        out = self.out.cpu().numpy()
        observed = _finish(self.acc.cpu().numpy(), self._xy, self._types, self.radii, self.window, t)
        return LabelSims(observed, out[:, :t * t * nr].reshape(self.sims, t, t, nr).cumsum(-1),
                         _n_in_of(out[:, t * t * nr:].reshape(self.sims, t, nr + 1)), self.seed)


def sims_device(xy, types, radii, window, nr_types=None, sims=None, seed=0, device="cuda"):
    """`sims_host` on the GPU: the same integers.  The grid is built once; the one synchronisation is the readback."""
    return DeviceRipleySims(xy, types, radii, window, nr_types, sims, seed, device).run().result()


def sims(xy, types, radii, window, nr_types=None, sims=None, seed=0, device=None):  # noqa: A002  (the argument is the issue's name)
    """`sims_host` with device=None, `sims_device` on `device` otherwise."""
    if device is None:
        return sims_host(xy, types, radii, window, nr_types, sims, seed)
    return sims_device(xy, types, radii, window, nr_types, sims, seed, device)


# ---- what a user reads ---------------------------------------------------------------------------
def resolve(spec):
    """What a `ripley` argument of the pipeline names: None -> None (off), {"radii": [r, ..]} with an optional "window": (wx0, wy0,
    wx1, wy1) -> (radii tuple, window tuple | None), in pixels of the processed image; without a window the image's own is used
    (`window_of`).  With "sims": S in 1..9999 and an optional "seed" in [0, 2^64) (default 0; refused without "sims") -> (radii, window,
    sims, seed): the random-labelling test.  ValueError / TypeError otherwise, before any work."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or "radii" not in spec or not set(spec) <= {"radii", "window", "sims", "seed"} or ("seed" in spec and "sims" not in spec):
        raise ValueError('ripley=%r: None or {"radii": [r, ..]} with an optional "window", and "sims" with an optional "seed"' % (spec,))
    rr = _check_radii(spec["radii"])
    win = None if spec.get("window") is None else _check_window(spec["window"])
    if "sims" not in spec:
        return tuple(rr.tolist()), win
    return (tuple(rr.tolist()), win) + _check_sims(spec["sims"], spec.get("seed", 0))


def window_of(size_hw):
    """The window of an image of size_hw = (h, w) processed pixels: the extent of the pixels, their centres on the integers."""
    h, w = (int(v) for v in size_hw)
    if h < 1 or w < 1:
        raise ValueError("an image of %d x %d pixels" % (h, w))
    return (-0.5, -0.5, w - 0.5, h - 0.5)


def of_info(info, size_hw, radii, nr_types, device=None, window=None, sims=None, seed=0):  # noqa: A002
    """The PairCounts of an instance dict (`post_proc.process` / `process_images` / `WsiInference.run`) over an image of size_hw =
    (h, w) processed pixels, with `window_of(size_hw)` unless a window is given.  The centroids are the points, entry["type"] the
    types, as in `neighbours.annotate` (nr_types=None: untyped, T = 1).  An empty dict gives zeros.  device=None: `pairs_host`.  With
    `sims` = S the LabelSims of the random-labelling test instead (`sims_host` / `sims_device`), zeros of its shapes for an empty dict."""
    win = window_of(size_hw) if window is None else window
    rr, (_, t) = _check_radii(radii), P.check_types(None, 0, nr_types)
    win = _check_bins(win, t, rr)
    if sims is not None:
        sims, seed = _check_sims(sims, seed)
    if not info:
        z = np.zeros((t, t, rr.shape[0]), np.int64)
        pc = PairCounts(z, z.copy(), np.zeros(t, np.int64), np.zeros((t, rr.shape[0]), np.int64), rr, win)
        return pc if sims is None else LabelSims(pc, np.zeros((sims,) + z.shape, np.int64), np.zeros((sims,) + pc.n_in.shape, np.int64), seed)
    _, xy, types = P.from_info(info, nr_types)
    if sims is None:
        return pairs(xy, types, rr, win, nr_types, device)
    if device is None:
        return sims_host(xy, types, rr, win, nr_types, sims, seed)
    return sims_device(xy, types, rr, win, nr_types, sims, seed, device)


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


def K_sims(ls, area=None):
    """float64 [S, T, T, R]: `K`'s formula per simulation, with n_in[s] and the invariant n[b]; NaN where the denominator is 0."""
    area = area_of(ls.observed.window) if area is None else float(area)
    den = ls.n_in[:, :, None, :].astype(np.float64) * ls.observed.n[None, None, :, None].astype(np.float64)
    out = np.full(den.shape, np.nan)
    np.divide(area * ls.pairs_in.astype(np.float64), den, out=out, where=den > 0)
    return out


def envelope(ls, rank=1, area=None):
    """(lo, hi), float64 [T, T, R] each: the rank-th smallest and the rank-th largest K_s per bin, a pointwise two-sided envelope of
    level 2 rank / (S + 1).  A bin is NaN where any simulation is NaN."""
    k = K_sims(ls, area)
    if not P.is_integer(rank) or not 1 <= rank <= k.shape[0]:
        raise ValueError("rank = %r outside 1..%d" % (rank, k.shape[0]))
    bad = np.isnan(k).any(0)
    k = np.sort(k, axis=0)                                       # NaN sorts last; those bins are masked below
    return np.where(bad, np.nan, k[rank - 1]), np.where(bad, np.nan, k[k.shape[0] - rank])


def p_value(ls, side, area=None):
    """float64 [T, T, R]: the Monte-Carlo p-value of the observed K per bin, (1 + #{s : K_s >= K_obs}) / (S + 1) for side "greater"
    (more pairs than random labelling gives), <= for "less"; ties count.  NaN where the observed K or any simulation is NaN."""
    if side not in ("greater", "less"):
        raise ValueError('side = %r: "greater" or "less"' % (side,))
    k, obs = K_sims(ls, area), K(ls.observed, area)
    bad = np.isnan(k).any(0) | np.isnan(obs)
    with np.errstate(invalid="ignore"):
        hits = ((k >= obs[None]) if side == "greater" else (k <= obs[None])).sum(0)
    return np.where(bad, np.nan, (1.0 + hits) / (k.shape[0] + 1.0))


def save(path, pc):
    """A PairCounts as an .npz of its six fields (what the managers write under ripley/); a LabelSims as those of its observed counts
    plus `sim_pairs_in`, `sim_n_in` and `seed`."""
    extra = {}
    if isinstance(pc, LabelSims):
        extra = {"sim_pairs_in": pc.pairs_in, "sim_n_in": pc.n_in, "seed": np.uint64(pc.seed)}
        pc = pc.observed
    np.savez_compressed(path, pairs=pc.pairs, pairs_in=pc.pairs_in, n=pc.n, n_in=pc.n_in, radii=np.asarray(pc.radii, np.float64),
                        window=np.asarray(pc.window, np.float64), **extra)

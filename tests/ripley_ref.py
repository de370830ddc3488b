"""The oracle of hover_net_amd/ripley.py: a chunked numpy transcription of its definition over ALL ordered pairs, with the definition's
own inequalities per k (d2 <= r2_k, b_i >= r_k) -- no kmin, no difference array, no grid -- and the cases that
tests/test_ripley_host.py and tests/test_gpu_ripley.py share (each built once, with its oracle result).  Every case has at most 4500
points."""
import functools

import numpy as np

import neighbours_ref as NR

_CHUNK = 1 << 21            # (i, j) pairs per chunk


def pairs(xy, types, radii, window, nr_types):
    """-> (pairs [T, T, R], pairs_in [T, T, R], n [T], n_in [T, R]), all int64, as the docstring of hover_net_amd/ripley.py defines them.
    A type outside [0, T) lands in no bin."""
    xy = np.asarray(xy, np.float64)
    n, t = xy.shape[0], int(nr_types)
    rr = np.asarray(radii, np.float64)
    r2 = rr * rr
    wx0, wy0, wx1, wy1 = (np.float64(v) for v in window)
    types = np.zeros(n, np.int64) if types is None else np.asarray(types, np.int64)
    of_type = (types[:, None] == np.arange(t)[None, :]).astype(np.float64)        # [N, T]; counts below 2^53 are exact
    b = np.minimum(np.minimum(xy[:, 0] - wx0, wx1 - xy[:, 0]), np.minimum(xy[:, 1] - wy0, wy1 - xy[:, 1]))
    out, out_in = np.zeros((t, t, rr.shape[0])), np.zeros((t, t, rr.shape[0]))
    step = max(1, _CHUNK // n)
    for a in range(0, n, step):
        e = min(n, a + step)
        dx = xy[None, :, 0] - xy[a:e, None, 0]
        dy = xy[None, :, 1] - xy[a:e, None, 1]
        d2 = (dx * dx) + (dy * dy)
        other = np.arange(n)[None, :] != np.arange(a, e)[:, None]                 # j != i
        for k in range(rr.shape[0]):
            per_i = ((d2 <= r2[k]) & other).astype(np.float64) @ of_type          # [chunk, T]: neighbours of type b of point i
            out[:, :, k] += of_type[a:e].T @ per_i
            out_in[:, :, k] += (of_type[a:e] * (b[a:e] >= rr[k])[:, None]).T @ per_i
    n_in = of_type.T @ (b[:, None] >= rr[None, :]).astype(np.float64)
    return out.astype(np.int64), out_in.astype(np.int64), of_type.sum(0).astype(np.int64), n_in.astype(np.int64)


def assert_same(got, want, what=""):
    """A PairCounts against the oracle's four arrays, with ==."""
    for name, g, w in zip(("pairs", "pairs_in", "n", "n_in"), got[:4], want):
        assert isinstance(g, np.ndarray) and g.dtype == np.int64 and g.shape == w.shape, (what, name, getattr(g, "dtype", None), getattr(g, "shape", None))
        assert (g == w).all(), (what, name, np.argwhere(g != w)[:5].tolist())


# ---- the cases: name -> (xy, types | None, radii, window, nr_types) -------------------------------------------------------------
def _uniform(seed, n, x0, x1, y0, y1, t):
    rng = np.random.default_rng(seed)
    xy = np.stack([x0 + rng.random(n) * (x1 - x0), y0 + rng.random(n) * (y1 - y0)], 1)
    types = None
    if t is not None:
        types = rng.integers(0, t, n).astype(np.int32)
        types[:t] = np.arange(t)                                # every type occurs
    return xy, types


LATTICE_RADII = (3.0, 5.0, 7.5, 12.0)


def _lattice():
    """The integer lattice 40 x 30 in a shuffled order; offsets (3, 4) and (5, 0) lie exactly on the radius 5."""
    yy, xx = np.mgrid[0:30, 0:40]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
    xy = np.ascontiguousarray(xy[np.random.default_rng(51).permutation(xy.shape[0])])
    return xy, ((xy[:, 0] + 2 * xy[:, 1]) % 3).astype(np.int32), LATTICE_RADII, (-0.5, -0.5, 39.5, 29.5), 3


def _rounding():
    """2 - (1 - 2^-53) rounds to 1.0: the last two points are a pair at r = 1, two cells apart at c = r."""
    return np.array([[0.0, 0.0], [1.0 - 2.0 ** -53, 0.0], [2.0, 0.0], [0.0, 7.0]]), None, (1.0,), (-1.0, -1.0, 3.0, 8.0), 1


EDGE_POINT = 0


def _edge():
    """Point 0 at (3, 10) in the window (0, 0, 20, 20): b = 3 = r_1 exactly, so it is inside at k = 0, 1 and not at k = 2.  Point 1 sits
    ON the window's edge (b = 0), point 2 at b = 2 = r_0."""
    xy, types = _uniform(52, 400, 0.0, 20.0, 0.0, 20.0, 2)
    xy[0], xy[1], xy[2] = (3.0, 10.0), (0.0, 12.0), (9.0, 18.0)
    xy[3], xy[4] = (3.0, 11.5), (0.5, 12.0)                     # a neighbour for each of the first two
    return xy, types, (2.0, 3.0, 4.5), (0.0, 0.0, 20.0, 20.0), 2


def _outside():
    xy, types = _uniform(53, 900, -10.0, 60.0, -10.0, 60.0, 4)
    return xy, types, (2.0, 4.0, 6.0, 9.0), (0.0, 0.0, 50.0, 50.0), 4


def _widened():
    xy, types, _r, _k, t = NR._widened()
    return xy, types, (0.25, 0.75, 1.0), (0.0, 0.0, 1.0e6, 1.0e6), t


def _one_point():
    return np.array([[3.5, -2.25]]), None, (1.0, 2.0), (0.0, -5.0, 7.0, 0.0), 1


def _one_radius():
    xy, types = _uniform(54, 500, 0.0, 100.0, 0.0, 80.0, 3)
    return xy, types, (7.0,), (0.0, 0.0, 100.0, 80.0), 3


def _r32():
    xy, types = _uniform(55, 600, 0.0, 90.0, 0.0, 90.0, 2)
    return xy, types, tuple(0.75 * (k + 1) for k in range(32)), (0.0, 0.0, 90.0, 90.0), 2


def _typed(seed, t, nr):
    xy, types = _uniform(seed, 700, 0.0, 100.0, 0.0, 100.0, t)
    return xy, types, tuple(9.0 * (k + 1) / nr for k in range(nr)), (0.0, 0.0, 100.0, 100.0), 1 if t is None else t


def _crowded():
    """3000 points on (5, 5) and 1500 on (17, 5), untyped: with r_max = 10 they fill cells 0 and 1 of a 2 x 1 grid, a run holds 4500
    candidates (five staging tiles), the groups are 12 apart, and every counted pair has d2 = 0: every add lands on bin 0."""
    xy = np.concatenate([np.tile([[5.0, 5.0]], (3000, 1)), np.tile([[17.0, 5.0]], (1500, 1))])
    return xy, None, (4.0, 10.0), (0.0, 0.0, 22.0, 10.0), 1


CASES = {"lattice": _lattice, "rounding": _rounding, "edge": _edge, "outside": _outside, "widened": _widened, "one_point": _one_point,
         "one_radius": _one_radius, "r32": _r32, "untyped": lambda: _typed(56, None, 5), "nine_types": lambda: _typed(57, 9, 32),
         "sixteen_types": lambda: _typed(58, 16, 16), "crowded": _crowded}


def assert_case_facts(name, res):
    """What each case is there for, asserted on a result (oracle tuple or PairCounts), so that no case passes vacuously."""
    from hover_net_amd import neighbours as NB

    (xy, types, radii, window, t), _ = case(name)
    pr, pin, n, n_in = res[:4]
    nr = len(radii)
    assert pr.shape == pin.shape == (t, t, nr) and n.shape == (t,) and n_in.shape == (t, nr)
    assert (pin <= pr).all() and (pin >= 0).all() and (np.diff(pr, axis=-1) >= 0).all() and int(n.sum()) == xy.shape[0]
    g = NB.grid(xy, radii[-1])
    if name == "lattice":
        d2 = NR.d2_matrix(xy)
        assert int((d2 == 25.0).sum()) > 0 and 3 * 3 + 4 * 4 == 25 and radii[1] == 5.0
        assert int(pr[:, :, 1].sum()) == int((d2 <= 25.0).sum()) - xy.shape[0]         # the 12 offsets ON the radius are counted
        assert int(pr[:, :, 1].sum()) > int((d2 < 25.0).sum()) - xy.shape[0]
        inner = (xy[:, 0] >= 11.5) & (xy[:, 0] <= 27.5) & (xy[:, 1] >= 11.5) & (xy[:, 1] <= 17.5)       # 12 inside the window
        assert int(n_in[:, 3].sum()) == int(inner.sum()) == 16 * 6 and int(pin[:, :, 3].sum()) == 16 * 6 * 440      # 441 lattice points within 12
    elif name == "rounding":
        assert xy[2, 0] - xy[1, 0] == 1.0 and xy[1, 0] < 1.0 and pr.reshape(-1).tolist() == [4]
    elif name == "edge":
        b = np.minimum(np.minimum(xy[:, 0] - window[0], window[2] - xy[:, 0]), np.minimum(xy[:, 1] - window[1], window[3] - xy[:, 1]))
        assert b[0] == radii[1] and b[1] == 0.0 and b[2] == radii[0]
        alone = pairs(xy[[0, 3]], types[[0, 3]] * 0, radii, window, 1)               # the pair (0, 3) at distance 1.5 on its own, both at b = 3: in at r = 3, out at 4.5
        assert alone[0].reshape(-1).tolist() == [2, 2, 2] and alone[1].reshape(-1).tolist() == [2, 2, 0] and alone[3].tolist() == [[2, 2, 0]]
        assert (pin < pr).any()
    elif name == "outside":
        out = (xy[:, 0] < window[0]) | (xy[:, 0] > window[2]) | (xy[:, 1] < window[1]) | (xy[:, 1] > window[3])
        assert 100 < int(out.sum()) < 600 and int(n_in[:, 0].sum()) < int((~out).sum()) and int(pin.sum()) > 0
        inside_only = pairs(xy[~out], types[~out], radii, window, t)
        assert int(pr.sum()) > int(inside_only[0].sum())                               # points outside count, as i and as j, in `pairs`;
        assert (pin == inside_only[1]).all()                                            # none is within r_k of an i that lies r_k inside
    elif name == "widened":
        assert g.c > radii[-1] * NB.MARGIN and g.c > 100.0 * radii[-1]
        assert int(pr[:, :, 0].sum()) == 0 and int(pr[:, :, 1].sum()) == 2 * NR.PLANTED   # planted twins at distance 0.5, as far as float64 holds it at 10^6
    elif name == "one_point":
        assert not pr.any() and not pin.any() and n.tolist() == [1] and n_in.tolist() == [[1, 1]]
    elif name == "one_radius":
        assert nr == 1 and int(pr.sum()) > 500 and not (pr - pr.transpose(1, 0, 2)).any()
    elif name == "r32":
        assert nr == 32 and int(pr[:, :, 0].sum()) > 0 and (np.diff(pr.sum((0, 1))) > 0).all()
    elif name in ("untyped", "nine_types", "sixteen_types"):
        assert t == {"untyped": 1, "nine_types": 9, "sixteen_types": 16}[name] and t * t * nr <= 4096 and (n > 0).all()
        assert (pr[:, :, -1] > 0).mean() > 0.9
    elif name == "crowded":
        assert (g.ncx, g.ncy) == (2, 1) and xy.shape[0] == 4500
        assert pr.reshape(-1).tolist() == [3000 * 2999 + 1500 * 1499] * 2 and pin.reshape(-1).tolist() == [3000 * 2999 + 1500 * 1499, 0]
    else:
        raise AssertionError("no facts for %s" % name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(args, oracle result) of a case; built once per process and shared: treat both as read-only."""
    args = CASES[name]()
    want = pairs(*args)
    for a in (args[0], args[1]) + want:
        if a is not None:
            a.setflags(write=False)
    return args, want

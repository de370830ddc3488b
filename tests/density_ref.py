"""The oracle of hover_net_amd/density.py: a chunked numpy transcription of its definition over ALL (node, point) pairs and nothing
cleverer, and the cases that tests/test_density_host.py and tests/test_gpu_density.py share (each built once, with its oracle
result).  Every case has at most 4500 points and 128 x 128 nodes."""
import functools
from fractions import Fraction

import numpy as np

import neighbours_ref as NR

_CHUNK = 1 << 22            # (node, point) pairs per chunk


def density(xy, types, radius, raster, nr_types):
    """px = ox + (u * s); py = oy + (v * s); dx = xj - px; dy = yj - py; d2 = (dx * dx) + (dy * dy);
    count[t, v, u] = #{ j : types[j] == t and d2 <= r * r }.  -> int32 [T, H, W].  A type outside [0, T) lands in no channel."""
    xy = np.asarray(xy, np.float64)
    n = xy.shape[0]
    ox, oy, s, w, h = raster
    ox, oy, s = np.float64(ox), np.float64(oy), np.float64(s)
    types = np.zeros(n, np.int64) if types is None else np.asarray(types, np.int64)
    px = ox + (np.arange(w, dtype=np.float64) * s)
    py = oy + (np.arange(h, dtype=np.float64) * s)
    nx, ny = np.tile(px, h), np.repeat(py, w)                   # node v * W + u
    r2 = np.float64(radius) * np.float64(radius)
    of_type = (types[:, None] == np.arange(nr_types)[None, :]).astype(np.float64)      # [N, T]; counts below 2^53 are exact
    out = np.zeros((h * w, nr_types), np.float64)
    step = max(1, _CHUNK // n)
    for a in range(0, h * w, step):
        dx = xy[None, :, 0] - nx[a:a + step, None]
        dy = xy[None, :, 1] - ny[a:a + step, None]
        d2 = (dx * dx) + (dy * dy)
        out[a:a + step] = (d2 <= r2).astype(np.float64) @ of_type
    return np.ascontiguousarray(out.T).reshape(nr_types, h, w).astype(np.int32)


def assert_same(got, want, what=""):
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == want.shape, (what, getattr(got, "dtype", None), getattr(got, "shape", None))
    assert (got == want).all(), (what, np.argwhere(got != want)[:5].tolist())


# ---- the cases: name -> (xy, types | None, radius, (ox, oy, s, W, H), nr_types) ---------------------------------------------------
def _uniform(seed, n, x0, x1, y0, y1, t):
    rng = np.random.default_rng(seed)
    xy = np.stack([x0 + rng.random(n) * (x1 - x0), y0 + rng.random(n) * (y1 - y0)], 1)
    return xy, (None if t is None else rng.integers(0, t, n).astype(np.int32))


def _lattice():
    yy, xx = np.mgrid[0:30, 0:40]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
    o = np.random.default_rng(21).permutation(xy.shape[0])
    xy = np.ascontiguousarray(xy[o])
    return xy, ((xy[:, 0] + xy[:, 1]) % 3).astype(np.int32), 5.0, (0.0, 0.0, 2.0, 20, 15), 3


def _rounding():
    return np.array([[1.0 - 2.0 ** -53, 0.0]]), None, 1.0, (0.0, 0.0, 1.0, 3, 1), 1


def _outside():
    xy, types = _uniform(22, 500, 100.0, 200.0, 100.0, 200.0, 4)
    return xy, types, 60.0, (-1000.0, -1000.0, 50.0, 48, 48), 4


INSIDE_WINDOW = (150.0, 250.0)


def _inside():
    xy, types = _uniform(23, 1500, 0.0, 400.0, 0.0, 400.0, 3)
    return xy, types, 25.0, (150.0, 150.0, 10.0, 11, 11), 3


def _fine():
    xy, types = _uniform(24, 800, 0.0, 200.0, 0.0, 200.0, 2)
    return xy, types, 16.0, (60.5, 60.5, 1.0, 48, 48), 2                  # s = r / 16: a block of 16 x 16 nodes is narrower than a cell


def _coarse():
    xy, types = _uniform(25, 2000, 0.0, 1280.0, 0.0, 1280.0, 3)
    return xy, types, 4.0, (10.0, 10.0, 20.0, 64, 64), 3                  # s = 5 r: a block of 16 nodes spans 80 grid rows


CROWD_NODE = (8, 8)


def _crowded():
    """3000 points on (5, 5), 1500 on (17, 5): with r = 10 they fill cells 0 and 1 of a 2 x 1 grid, so a run holds 4500 candidates
    (five staging tiles).  Node (8, 8) of the raster is (5, 5) exactly."""
    xy = np.concatenate([np.tile([[5.0, 5.0]], (3000, 1)), np.tile([[17.0, 5.0]], (1500, 1))])
    return xy, (np.arange(4500) % 5).astype(np.int32), 10.0, (-3.0, -3.0, 1.0, 32, 16), 5


def _widened():
    xy, types, _r, _k, t = NR._widened()
    return xy, types, 1.0, (float(xy[0, 0]) - 2.0, float(xy[0, 1]) - 2.0, 0.25, 17, 17), t


def _one_point_one_node():
    return np.array([[3.5, -2.25]]), None, 1.0, (3.0, -2.0, 1.0, 1, 1), 1


def _row():
    xy, types = _uniform(26, 1000, 0.0, 1000.0, -3.0, 3.0, 2)
    return xy, types, 4.0, (0.0, 0.0, 1.0, 1000, 1), 2


def _column():
    xy, types = _uniform(27, 1000, -3.0, 3.0, 0.0, 1000.0, 2)
    return xy, types, 4.0, (0.0, 0.0, 1.0, 1, 1000), 2


def _ragged():
    xy, types = _uniform(28, 1500, 0.0, 370.0, 0.0, 190.0, 4)
    return xy, types, 18.0, (0.0, 0.0, 10.0, 37, 19), 4


def _inexact_step():
    ox, oy = 1.0e6 + 0.3, 2.0e6 + 0.3
    xy, types = _uniform(29, 1200, ox - 0.3, ox + 4.2, oy - 0.3, oy + 3.2, 2)
    return xy, types, 0.25, (ox, oy, 0.1, 40, 30), 2


def _typed(seed, t):
    xy, types = _uniform(seed, 600, 0.0, 100.0, 0.0, 100.0, t)
    if types is not None:
        types[:t] = np.arange(t)                                # every type occurs
    return xy, types, 9.0, (0.0, 0.0, 4.0, 26, 26), 1 if t is None else t


CASES = {"lattice": _lattice, "rounding": _rounding, "outside": _outside, "inside": _inside, "fine": _fine, "coarse": _coarse,
         "crowded": _crowded, "widened": _widened, "one_point_one_node": _one_point_one_node, "row": _row, "column": _column,
         "ragged": _ragged, "inexact_step": _inexact_step, "untyped": lambda: _typed(30, None), "nine_types": lambda: _typed(31, 9),
         "sixteen_types": lambda: _typed(32, 16)}


def assert_case_facts(name, res):
    """What each case is there for, asserted on a result (oracle, host or device), so that no case passes vacuously."""
    from hover_net_amd import neighbours as NB

    (xy, types, r, raster, t), _ = case(name)
    ox, oy, s, w, h = raster
    assert res.shape == (t, h, w) and (res >= 0).all()
    per_node = res.sum(0, dtype=np.int64)
    g = NB.grid(xy, r)
    px, py = ox + (np.arange(w, dtype=np.float64) * s), oy + (np.arange(h, dtype=np.float64) * s)
    if name == "lattice":
        assert int((NR.d2_matrix(xy) == r * r).sum()) > 0 and 3 * 3 + 4 * 4 == r * r       # offsets (3, 4) and (5, 0) sit on the radius
        assert per_node[5, 5] == 81 and per_node[7, 10] == 81                              # interior nodes (10, 10) and (20, 14)
        assert res[:, 5, 5].tolist() == [28, 28, 25]                                       # types (x + y) % 3 around (10, 10)
    elif name == "rounding":
        assert xy[0, 0] - 2.0 == -1.0 and xy[0, 0] < 1.0                                   # fl(dx) = -1 for node u = 2
        assert res.reshape(-1).tolist() == [1, 1, 1]
    elif name == "outside":
        ux, uy = np.floor((px - g.x0) / g.c), np.floor((py - g.y0) / g.c)
        assert (ux < -1).any() and (uy < -1).any() and (ux > g.ncx).any() and (uy > g.ncy).any()
        far = ((uy < -1) | (uy > g.ncy))[:, None] | ((ux < -1) | (ux > g.ncx))[None, :]
        assert far.sum() > 1000 and not per_node[far].any() and per_node.sum() > 0
    elif name == "inside":
        assert xy.min() < INSIDE_WINDOW[0] - r and xy.max() > INSIDE_WINDOW[1] + r and px[0] == py[0] == INSIDE_WINDOW[0] and px[-1] == py[-1] == INSIDE_WINDOW[1]
        out = xy[xy[:, 0] < INSIDE_WINDOW[0]]                                              # points left of the window
        dx, dy = out[:, 0] - px[0], out[:, 1] - py[5]
        reach = int(((dx * dx) + (dy * dy) <= r * r).sum())
        assert reach >= 1 and per_node[5, 0] > reach                                       # edge node (u = 0, v = 5) counts them, and others
    elif name == "fine":
        assert s == r / 16 and 16 * s < g.c and per_node.min() >= 1
    elif name == "coarse":
        assert s == 5 * r and (w, h) == (64, 64) and 16 * s > 16 * g.c
        assert (per_node == 0).mean() > 0.5 and (per_node > 0).sum() >= 50
    elif name == "crowded":
        v, u = CROWD_NODE
        assert (px[u], py[v]) == (5.0, 5.0) and (g.ncx, g.ncy) == (2, 1) and xy.shape[0] == 4500
        assert per_node[v, u] >= 3000 and per_node.max() == 4500 and res[:, v, u].tolist() == [600] * 5
    elif name == "widened":
        assert g.c > r * NB.MARGIN and g.c > 100.0 * r
        assert per_node[8, 8] == 2 and per_node.max() == 2                                 # node (8, 8) is at point 0; its planted twin is 0.5 away
    elif name == "one_point_one_node":
        assert res.tolist() == [[[1]]]
    elif name in ("row", "column"):
        assert (w, h) == ((1000, 1) if name == "row" else (1, 1000)) and per_node.max() >= 8 and (per_node > 0).mean() > 0.9
    elif name == "ragged":
        assert (w, h) == (37, 19) and per_node.min() >= 1
    elif name == "inexact_step":
        assert any(Fraction(float(u)) * Fraction(s) != Fraction(float(u) * s) for u in range(w))       # u * s rounds for some u
        assert per_node.sum() > 500 and per_node.min() < per_node.max()
    elif name == "untyped":
        assert types is None and t == 1 and per_node.sum() > 1000
    elif name in ("nine_types", "sixteen_types"):
        assert t == (9 if name == "nine_types" else 16) and (res.reshape(t, -1).sum(1) > 0).all()
    else:
        raise AssertionError("no facts for %s" % name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(args, oracle result) of a case; built once per process and shared: treat both as read-only."""
    args = CASES[name]()
    want = density(*args)
    for a in (args[0], args[1], want):
        if a is not None:
            a.setflags(write=False)
    return args, want

"""The oracle of hover_net_amd/neighbours.py: an O(N^2) numpy transcription of its definition and nothing cleverer, and the cases that
tests/test_neighbours_host.py and tests/test_gpu_neighbours.py share (each built once, with its oracle result)."""
import functools

import numpy as np


def query(xy, types, radius, k, nr_types):
    """dx = xj - xi; dy = yj - yi; d2 = (dx * dx) + (dy * dy); neighbour <=> j != i and d2 <= r * r.  -> count, knn, nearest_of_type."""
    xy = np.asarray(xy, np.float64)
    n = xy.shape[0]
    types = np.zeros(n, np.int64) if types is None else np.asarray(types, np.int64)
    dx = xy[None, :, 0] - xy[:, None, 0]
    dy = xy[None, :, 1] - xy[:, None, 1]
    d2 = (dx * dx) + (dy * dy)
    r2 = np.float64(radius) * np.float64(radius)
    count = np.zeros((n, nr_types), np.int32)
    knn = np.full((n, k), -1, np.int32)
    nearest = np.full((n, nr_types), -1, np.int32)
    for i in range(n):
        js = np.nonzero(d2[i] <= r2)[0]
        js = js[js != i]
        js = js[np.lexsort((js, d2[i, js]))]            # ascending (d2, j)
        knn[i, :min(k, js.shape[0])] = js[:k]
        for t in range(nr_types):
            of_t = js[types[js] == t]
            count[i, t] = of_t.shape[0]
            if of_t.shape[0]:
                nearest[i, t] = of_t[0]                  # js is in ascending (d2, j)
    return {"count": count, "knn": knn, "nearest_of_type": nearest}


def d2_matrix(xy):
    dx = xy[None, :, 0] - xy[:, None, 0]
    dy = xy[None, :, 1] - xy[:, None, 1]
    return (dx * dx) + (dy * dy)


def assert_same(got, want, what=""):
    for name in ("count", "knn", "nearest_of_type"):
        assert got[name].dtype == np.int32 and got[name].shape == want[name].shape, (what, name, got[name].dtype, got[name].shape)
        assert (got[name] == want[name]).all(), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


# ---- the cases: name -> (xy, types | None, radius, k, nr_types) -----------------------------------------------------------------
def _random2000():
    rng = np.random.default_rng(14)          # a seed at which every point has at least five neighbours within 25
    return rng.random((2000, 2)) * np.array([500.0, 400.0]), rng.integers(0, 5, 2000).astype(np.int32)


def _lattice():
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:30, 0:40]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64) * 5.0
    xy = xy[rng.permutation(xy.shape[0])]
    return xy, rng.integers(0, 5, xy.shape[0]).astype(np.int32), 25.0, 8, 5


def _random():
    xy, types = _random2000()
    return xy, types, 25.0, 5, 5


def _slide():
    xy, types = _random2000()
    xy = np.round(xy * 2.0) / 2.0 + np.array([98304.0, 65536.0])
    xy[100:110] = xy[0]
    return xy, types, 12.5, 4, 5


def _rounding():
    return np.array([[0.0, 0.0], [1.0 - 2.0 ** -53, 0.0], [2.0, 0.0], [0.0, 7.0]]), None, 1.0, 2, 1


def _crowded():
    """3000 points in one cell, each with 2999 neighbours: three staging tiles of 1024 candidates, twelve workgroups of 256 queries."""
    rng = np.random.default_rng(5)
    return rng.random((3000, 2)) * 10.0, rng.integers(0, 16, 3000).astype(np.int32), 50.0, 16, 16


def _one_point():
    return np.array([[3.5, -2.25]]), None, 1.0, 3, 1


def _two_far_points():
    return np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([1, 0], np.int32), 4.999, 1, 2


def _k_above_every_neighbourhood():
    return np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [40.0, 40.0]]), np.array([2, 0, 2, 1], np.int32), 1.5, 16, 3


def _untyped():
    rng = np.random.default_rng(6)
    return rng.random((300, 2)) * 60.0, None, 7.0, 6, 1


def _one_type_given():
    rng = np.random.default_rng(7)
    return rng.random((300, 2)) * 60.0, np.zeros(300, np.int32), 7.0, 6, 1


PLANTED = 20


def _widened():
    """500 points over 10^6 x 10^6 with r = 1: the extent needs 10^6 cells per axis, the caps allow 2048 x 2048, so c is widened.  Rows
    500 + i is planted 0.5 away from row i."""
    rng = np.random.default_rng(8)
    xy = rng.random((500, 2)) * 1.0e6
    xy = np.concatenate([xy, xy[:PLANTED] + np.array([0.3, 0.4])])
    return xy, rng.integers(0, 3, xy.shape[0]).astype(np.int32), 1.0, 3, 3


BORDER_R = 3.0


def _borders():
    """Points at x0 + m * c (x0 = y0 = 0) for the c the module chooses, and one ulp either side, on both axes."""
    c = BORDER_R * (1.0 + 2.0 ** -20)
    xs = [0.0]
    for m in range(1, 7):
        v = m * c
        xs += [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]
    ys = [0.0] + [f(c) for f in (lambda v: np.nextafter(v, -np.inf), lambda v: v, lambda v: np.nextafter(v, np.inf))] + [2 * c, 2.5 * c]
    xy = np.array([[x, y] for y in ys for x in xs], np.float64)
    return xy, (np.arange(xy.shape[0]) % 4).astype(np.int32), BORDER_R, 16, 4


CASES = {"lattice": _lattice, "random": _random, "slide": _slide, "rounding": _rounding, "crowded": _crowded, "one_point": _one_point,
         "two_far_points": _two_far_points, "k_above_every_neighbourhood": _k_above_every_neighbourhood, "untyped": _untyped,
         "one_type_given": _one_type_given, "widened": _widened, "borders": _borders}


def assert_case_facts(name, res):
    """What each case is there for, asserted on a result (oracle, host or device), so that no case passes vacuously.  The figures
    were computed with `query` above."""
    from hover_net_amd import neighbours as NB

    (xy, _types, r, _k, _t), _ = case(name)
    count, knn, nearest = res["count"], res["knn"], res["nearest_of_type"]
    per_point = count.sum(1)
    g = NB.grid(xy, r)
    if name == "lattice":
        assert int((d2_matrix(xy) == r * r).sum()) == 11836                 # ordered pairs at exactly the radius
        assert (knn >= 0).all() and int(per_point.max()) == 80
    elif name == "random":
        assert (knn >= 0).all() and int(per_point.sum()) == 37344           # mean 18.672
        assert int((nearest < 0).sum()) == 238                              # 2.4 % of (i, t) have no neighbour of that type
    elif name == "slide":
        assert int((knn < 0).any(1).sum()) == 641                           # rows that carry padding
        assert knn[0].tolist() == [100, 101, 102, 103] and knn[100].tolist() == [0, 101, 102, 103] and knn[109].tolist() == [0, 100, 101, 102]
        assert not d2_matrix(xy[[0] + list(range(100, 110))]).any()
    elif name == "rounding":
        assert knn.tolist() == [[1, -1], [0, 2], [1, -1], [-1, -1]]
    elif name == "crowded":
        assert (g.ncx, g.ncy) == (1, 1) and (per_point == 2999).all() and (knn >= 0).all() and (nearest >= 0).all()
    elif name == "widened":
        assert g.c > 100.0 * r and g.ncx <= 4096 and g.ncy <= 4096 and g.ncx * g.ncy <= 1 << 22
        assert knn[:PLANTED, 0].tolist() == list(range(500, 500 + PLANTED)) and knn[500:, 0].tolist() == list(range(PLANTED))
    elif name == "borders":
        assert (g.x0, g.y0, g.c) == (0.0, 0.0, BORDER_R * (1.0 + 2.0 ** -20)) and (g.ncx, g.ncy) == (7, 3)
        assert int(per_point.max()) == 8
    elif name in ("one_point", "two_far_points"):
        assert not count.any() and (knn == -1).all() and (nearest == -1).all()
    elif name == "k_above_every_neighbourhood":
        assert knn[:, :2].tolist() == [[1, 2], [0, 2], [0, 1], [-1, -1]] and (knn[:, 2:] == -1).all()
    else:
        assert count.shape[1] == 1 and per_point.min() >= 1


@functools.lru_cache(maxsize=None)
def case(name):
    """(args, oracle result) of a case; built once per process and shared: treat both as read-only."""
    args = CASES[name]()
    want = query(*args)
    for a in (args[0], args[1]) + tuple(want.values()):
        if a is not None:
            a.setflags(write=False)
    return args, want

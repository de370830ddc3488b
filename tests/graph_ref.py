"""The oracle of hover_net_amd/graph.py: its definition over ALL k, with no grid and nothing cleverer (cubic), and the cases that
tests/test_graph_host.py and tests/test_gpu_graph.py share (each built once, with its oracle result).  The points and radii are those of
tests/neighbours_ref.py's cases."""
import functools

import numpy as np

import neighbours_ref as NR


def gabriel(xy, radius):
    """j is a neighbour of i <=> j != i and d2(i, j) <= r * r; k blocks (i, j) <=> k != i, k != j, k is a neighbour of i and of j and
    ((xi - xk) * (xj - xk)) + ((yi - yk) * (yj - yk)) < 0; (i, j) is an edge <=> j is a neighbour of i and no k blocks it.
    -> (indptr int64 [N + 1], indices int32 [E]), every row in ascending (d2, j)."""
    xy = np.asarray(xy, np.float64)
    n = xy.shape[0]
    x, y = xy[:, 0], xy[:, 1]
    d2 = NR.d2_matrix(xy)
    nbr = d2 <= np.float64(radius) * np.float64(radius)
    nbr[np.arange(n), np.arange(n)] = False
    every = np.arange(n)
    indptr, rows = np.zeros(n + 1, np.int64), []
    for i in range(n):
        js = np.nonzero(nbr[i])[0]
        js = js[np.lexsort((js, d2[i, js]))]            # ascending (d2, j)
        with np.errstate(over="ignore", invalid="ignore"):
            dot = ((x[i] - x[None, :]) * (x[js, None] - x[None, :])) + ((y[i] - y[None, :]) * (y[js, None] - y[None, :]))     # [j, k]
        blocks = (every[None, :] != i) & (every[None, :] != js[:, None]) & nbr[i][None, :] & nbr[js] & (dot < 0.0)
        rows.append(js[~blocks.any(1)])
        indptr[i + 1] = indptr[i] + rows[-1].shape[0]
    return indptr, np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)


def assert_same(got, want, what=""):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32, (what, got[0].dtype, got[1].dtype)
    assert got[0].shape == want[0].shape and (got[0] == want[0]).all(), (what, "indptr", np.argwhere(got[0] != want[0])[:5].tolist())
    assert got[1].shape == want[1].shape and (got[1] == want[1]).all(), (what, "indices", np.argwhere(got[1] != want[1])[:5].tolist())


def is_symmetric(g):
    indptr, indices = np.asarray(g[0], np.int64), np.asarray(g[1], np.int64)
    n = indptr.shape[0] - 1
    i = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    return np.array_equal(np.sort(i * n + indices), np.sort(indices * n + i))


def _collinear():
    """50 points on a line, spacing 1.5, in shuffled order; every point within 4 spacings is a neighbour, only the adjacent ones are joined."""
    rng = np.random.default_rng(3)
    t = np.arange(50, dtype=np.float64)[rng.permutation(50)]
    return np.stack([10.0 + 1.5 * t, 4.0 + 0.75 * t], 1), 7.0


def _piles(a, b):
    """Two coincident piles of a and b points, 3 apart: everybody is everybody's neighbour at r = 5 and nobody blocks."""
    xy = np.zeros((a + b, 2))
    xy[:a] = (7.0, 2.5)
    xy[a:] = (10.0, 2.5)
    return xy, 5.0


def piles_graph(a, b):
    """The closed form for `_piles`: every row holds all others, the own pile first (d2 = 0), each by j."""
    n = a + b
    indptr = np.arange(n + 1, dtype=np.int64) * (n - 1)
    first, second = np.arange(a), np.arange(a, n)
    rows = [np.concatenate([first[first != i], second]) if i < a else np.concatenate([second[second != i], first]) for i in range(n)]
    return indptr, np.concatenate(rows).astype(np.int32)


def _dense1100():
    return np.random.default_rng(5).random((1100, 2)) * 10.0, 50.0


NAMES = ("random", "slide", "lattice", "untyped", "borders", "widened", "rounding", "one_point", "two_far_points")
EXTRA = {"collinear": _collinear, "dense1100": _dense1100}
# directed edges, (smallest, largest) degree or None: computed with `gabriel` above
FACTS = {"random": (7838, (1, 8)), "slide": (5640, (None, 14)), "lattice": (9184, (3, 8)), "untyped": (1074, None), "borders": (402, None),
         "widened": (40, None), "rounding": (4, None), "one_point": (0, (0, 0)), "two_far_points": (0, (0, 0)), "collinear": (98, (1, 2)),
         "dense1100": (4258, (1, 8))}


def points(name):
    """(xy, radius) of a case."""
    if name in EXTRA:
        return EXTRA[name]()
    (xy, _types, r, _k, _t), _ = NR.case(name)
    return xy, r


def assert_case_facts(name, g):
    """What each case is there for, asserted on a result (oracle, host or device), so that no case passes vacuously."""
    xy, r = points(name)
    indptr, indices = np.asarray(g[0]), np.asarray(g[1])
    deg = np.diff(indptr)
    edges, span = FACTS[name]
    assert indptr.shape == (xy.shape[0] + 1,) and indptr[0] == 0 and int(indptr[-1]) == indices.shape[0] == edges, (name, int(indptr[-1]))
    if span is not None:
        assert int(deg.max()) == span[1] and (span[0] is None or int(deg.min()) == span[0]), (name, int(deg.min()), int(deg.max()))
    assert is_symmetric(g), name
    if name in NR.CASES:
        knn = NR.case(name)[1]["knn"]
        has = knn[:, 0] >= 0                                      # the nearest neighbour is always a graph neighbour, and the first
        assert (deg[has] >= 1).all() and (indices[indptr[:-1][has]] == knn[has, 0]).all() and (deg[~has] == 0).all(), name
    if name == "lattice":                                         # 30 x 40 points: the axial edges and both diagonals of every square, twice each
        assert edges == 2 * (30 * 39 + 29 * 40) + 2 * 2 * 29 * 39
    elif name == "widened":
        assert edges == 2 * NR.PLANTED and indices[indptr[:-1][:NR.PLANTED]].tolist() == list(range(500, 500 + NR.PLANTED))
    elif name == "rounding":
        assert [indices[indptr[i]:indptr[i + 1]].tolist() for i in range(4)] == [[1], [0, 2], [1], []]
    elif name == "slide":                                         # ten coincident points: joined to each other, ordered by j
        assert indices[indptr[0]:indptr[0] + 10].tolist() == list(range(100, 110)) and indices[indptr[105]:indptr[105] + 3].tolist() == [0, 100, 101]
    elif name == "collinear":
        assert edges == 2 * 49


@functools.lru_cache(maxsize=None)
def case(name):
    """((xy, radius), oracle result) of a case; built once per process and shared: treat both as read-only."""
    xy, r = points(name)
    want = gabriel(xy, r)
    for a in (xy,) + want:
        a.setflags(write=False)
    return (xy, r), want

"""The oracle of hover_net_amd/forest.py: a scalar Kruskal over the edges sorted by key with a plain union-find and nothing cleverer, and
the cases that tests/test_forest_host.py and tests/test_gpu_forest.py share (each built once, with its oracle result).  The points are
those of tests/graph_ref.py with their Gabriel graphs, plus the cases made here."""
import functools

import numpy as np

import graph_ref as G
from hover_net_amd import graph as GR


def kruskal(xy, g):
    """key{i, j} = (d2(i, j), min(i, j), max(i, j)) with dx = xj - xi, dy = yj - yi, d2 = (dx * dx) + (dy * dy); the edges in ascending key;
    an edge joins the forest iff its ends are not yet connected.  The root of a union is its smaller position, so a root names its
    component.  -> (component int32 [N], edges int32 [F, 2] as (lo, hi), sorted)."""
    pts = np.asarray(xy, np.float64).tolist()
    indptr, indices = np.asarray(g[0]).tolist(), np.asarray(g[1]).tolist()
    n = len(pts)
    keys = []
    for i in range(n):
        for j in indices[indptr[i]:indptr[i + 1]]:
            if i < j:
                dx, dy = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1]
                keys.append(((dx * dx) + (dy * dy), i, j))
    keys.sort()
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    edges = []
    for _d2, i, j in keys:
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
            edges.append((i, j))
    edges.sort()
    return np.array([find(i) for i in range(n)], np.int32), np.array(edges, np.int32).reshape(-1, 2)


def assert_same(got, want, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32, (what, got[0].dtype, got[1].dtype)
    assert got[0].shape == want[0].shape and (got[0] == want[0]).all(), (what, "component", np.argwhere(got[0] != want[0])[:5].tolist())
    assert got[1].shape == want[1].shape and (got[1] == want[1]).all(), (what, "edges", np.argwhere(got[1] != want[1])[:5].tolist())


def _line(x):
    return np.stack([np.asarray(x, np.float64), np.zeros(len(x))], 1)


def _ruler1024():
    """1024 points on a line; the gap after point i (1-based) is 1 + v2(i) / 64, v2 the 2-adic valuation: every point's smallest gap is the
    one to its partner in a block of 2, then every pair's to its partner in a block of 4, ..: the components merge strictly pairwise, one
    level per round, ten rounds."""
    gaps = [1.0 + ((i & -i).bit_length() - 1) / 64.0 for i in range(1, 1024)]
    return _line(np.concatenate([[0.0], np.cumsum(gaps)])), 1.5


def _chain1000():
    """1000 points on a line with gaps 1 + i / 4096: every point's smallest edge is the one to its left, so round 1 hooks one chain 999 deep."""
    return _line(np.concatenate([[0.0], np.cumsum(1.0 + np.arange(999) / 4096.0)])), 2.0


def _tiedline():
    return _line(np.arange(1000.0)), 1.5


def _permuted(make, order):
    xy, r = make()
    return np.ascontiguousarray(xy[order(xy.shape[0])]), r


LINES = {"ruler1024": _ruler1024, "chain1000": _chain1000, "tiedline": _tiedline,
         "ruler1024_shuffled": lambda: _permuted(_ruler1024, np.random.default_rng(21).permutation),
         "chain1000_reversed": lambda: _permuted(_chain1000, lambda n: np.arange(n - 1, -1, -1)),
         "tiedline_shuffled": lambda: _permuted(_tiedline, np.random.default_rng(22).permutation)}
NAMES = G.NAMES + ("collinear", "dense1100", "piles") + tuple(LINES)
PILES = (40, 25)
# N, undirected edges of the graph, F, components: pinned with `kruskal` above
FACTS = {"random": (2000, 3919, 1999, 1), "slide": (2000, 2820, 1955, 45), "lattice": (1200, 4592, 1199, 1), "untyped": (300, 537, 299, 1),
         "borders": (114, 201, 93, 21), "widened": (520, 20, 20, 500), "rounding": (4, 2, 2, 2), "one_point": (1, 0, 0, 1),
         "two_far_points": (2, 0, 0, 2), "collinear": (50, 49, 49, 1), "dense1100": (1100, 2129, 1099, 1), "piles": (65, 2080, 64, 1),
         "ruler1024": (1024, 1023, 1023, 1), "chain1000": (1000, 999, 999, 1), "tiedline": (1000, 999, 999, 1)}
ROUNDS = {"random": 6, "ruler1024": 10, "ruler1024_shuffled": 10}      # the rounds that join anything, where a case is there for them


def graph_of(name):
    """(xy, CellGraph) of a case.  `dense1100` and the lines take their graph from `gabriel_host`, which tests/test_graph_host.py holds
    to the cubic oracle; `piles` takes the closed form."""
    if name == "piles":
        return G._piles(*PILES)[0], GR.CellGraph(*G.piles_graph(*PILES))
    if name in LINES or name == "dense1100":
        xy, r = LINES[name]() if name in LINES else G.points(name)
        return xy, GR.gabriel_host(xy, r)
    (xy, _r), g = G.case(name)
    return xy, GR.CellGraph(*g)


def tied_d2(xy, g):
    """The undirected edges beyond the first of every d2 value: the edges minus the distinct d2 among them."""
    e = GR.edge_list(g).astype(np.int64)
    dx, dy = xy[e[:, 1], 0] - xy[e[:, 0], 0], xy[e[:, 1], 1] - xy[e[:, 0], 1]
    return int(e.shape[0] - np.unique((dx * dx) + (dy * dy)).shape[0])


def assert_case_facts(name, xy, g, f):
    """What each case is there for, asserted on a result (oracle, host or device), so that no case passes vacuously."""
    component, edges = np.asarray(f[0]), np.asarray(f[1])
    n, undirected, forest_edges, components = FACTS[name.split("_shuffled")[0].split("_reversed")[0]]
    assert xy.shape == (n, 2) and int(g.indptr[-1]) == 2 * undirected, (name, xy.shape, int(g.indptr[-1]))
    assert component.shape == (n,) and edges.shape == (forest_edges, 2) and np.unique(component).shape[0] == components, (name, edges.shape)
    assert forest_edges == n - components and (component <= np.arange(n)).all() and (component[component] == component).all(), name
    assert (edges[:, 0] < edges[:, 1]).all() and (component[edges[:, 0]] == component[edges[:, 1]]).all(), name
    if name == "random":
        assert tied_d2(xy, g) == 0
    elif name == "slide":
        assert tied_d2(xy, g) == 2605 and (component[100:110] == component[0]).all()
    elif name == "lattice":
        assert tied_d2(xy, g) == undirected - 2                  # two values in all, the side and the diagonal: the position decides everything
    elif name == "piles":                                         # the star at 0 over pile one, the edge (0, 40), the star at 40 over pile two
        a, b = PILES
        want = [[0, j] for j in range(1, a + 1)] + [[a, j] for j in range(a + 1, a + b)]
        assert edges.tolist() == sorted(want) and not component.any()
    elif name.startswith(("ruler1024", "chain1000", "tiedline")):
        order = np.argsort(xy[:, 0])                              # the forest is the line itself
        want = np.sort(np.stack([order[:-1], order[1:]], 1), 1)
        assert edges.tolist() == sorted(want.tolist()) and not component.any()
        if name.startswith("tiedline"):
            assert tied_d2(xy, g) == undirected - 1              # one value
    elif name == "widened":
        assert edges.tolist() == [[i, 500 + i] for i in range(G.NR.PLANTED)]
    elif name == "rounding":
        assert edges.tolist() == [[0, 1], [1, 2]] and component.tolist() == [0, 0, 0, 3]


@functools.lru_cache(maxsize=None)
def case(name):
    """((xy, CellGraph), oracle result) of a case; built once per process and shared: treat all of it as read-only."""
    xy, g = graph_of(name)
    want = kruskal(xy, g)
    for a in (xy, g.indptr, g.indices) + want:
        a.setflags(write=False)
    return (xy, g), want

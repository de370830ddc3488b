"""The oracle of hover_net_amd/clusters.py: an O(N^2) numpy transcription of its definition and nothing cleverer (the dense d2 matrix,
scipy's connected components on the core sub-graph, a lexsort per border point), and the cases that tests/test_clusters_host.py and
tests/test_gpu_clusters.py share (each built once, with its oracle result)."""
import functools

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import neighbours_ref as NR


def cluster(xy, types, radius, min_pts, of_types=None):
    """degree = 1 + selected neighbours (d2 <= r * r, j != i); core <=> selected and degree >= m; a cluster = a connected component of
    the cores, named by its smallest position; a selected non-core takes the label of its (d2, j)-smallest core neighbour.
    -> label, degree."""
    xy = np.asarray(xy, np.float64)
    n = xy.shape[0]
    sel = np.ones(n, bool) if of_types is None else np.isin(np.asarray(types), list(of_types))
    d2 = NR.d2_matrix(xy)
    r2 = np.float64(radius) * np.float64(radius)
    nb = (d2 <= r2) & ~np.eye(n, dtype=bool) & sel[None, :] & sel[:, None]
    degree = np.where(sel, 1 + nb.sum(1), 0).astype(np.int32)
    core = sel & (degree >= min_pts)
    label = np.full(n, -1, np.int32)
    cores = np.nonzero(core)[0]
    if cores.shape[0]:
        _, comp = connected_components(csr_matrix(nb[np.ix_(cores, cores)]), directed=False)
        root = np.full(comp.max() + 1, n, np.int64)
        np.minimum.at(root, comp, cores)                    # the smallest position among a component's cores
        label[cores] = root[comp]
    for i in np.nonzero(sel & ~core)[0]:
        js = np.nonzero(nb[i] & core)[0]
        if js.shape[0]:
            label[i] = label[js[np.lexsort((js, d2[i, js]))[0]]]
    return {"label": label, "degree": degree}


def assert_same(got, want, what=""):
    for name in ("label", "degree"):
        assert got[name].dtype == np.int32 and got[name].shape == want[name].shape, (what, name, got[name].dtype, got[name].shape)
        assert (got[name] == want[name]).all(), (what, name, np.argwhere(got[name] != want[name])[:5].ravel().tolist())


# ---- the cases: name -> (xy, types | None, radius, min_pts, of_types) -------------------------------------------------------------
def _snake():
    """A boustrophedon chain at spacing exactly 1.0: 40 rows of 100 points, the rows 3 apart and joined by two connector points at
    the row ends, 4078 points, shuffled.  With r = 1, m = 3 every point but the two chain ends is a core (itself and two neighbours):
    the deep-tree case of a union-find, the worst case of label propagation."""
    pts = []
    for row in range(40):
        xs = range(100) if row % 2 == 0 else range(99, -1, -1)
        pts += [(float(x), 3.0 * row) for x in xs]
        if row < 39:
            end = 99.0 if row % 2 == 0 else 0.0
            pts += [(end, 3.0 * row + 1.0), (end, 3.0 * row + 2.0)]
    xy = np.array(pts, np.float64)
    return np.ascontiguousarray(xy[np.random.default_rng(3).permutation(xy.shape[0])])


BRIDGE_ROOTS = (1, 2)


def _bridge():
    """Two five-point clumps (the corners of the unit square and its centre) at x offsets 0 and 6, and a bridge point (3.5, 0) at
    position 0.  With r = 2.5, m = 5 every clump point is a core and the clumps are two clusters ((1, 0) and (6, 0) are 5 apart).  The
    bridge is at d2 == 6.25 from (1, 0) and from (6, 0) and further from everything else: degree 3, a border, and the tie goes to
    the smaller position.  Position 1 is a left core that is NOT (1, 0), so the left cluster's root is 1; position 2 is (6, 0), the right
    cluster's root; (1, 0) comes last.  The tie therefore goes to position 2: the nearest core belongs to the cluster with the LARGER
    root, and the bridge must not merge the clumps."""
    left = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.5)]
    right = [(x + 6.0, y) for x, y in left]
    rows = [(3.5, 0.0), left[0], right[0]] + left[2:] + right[1:] + [left[1]]
    return np.array(rows, np.float64)


def _random():
    xy, _ = NR._random2000()
    return xy, None, 12.0, 4, None


def _typed():
    xy, types = NR._random2000()
    return xy, types, 20.0, 4, (1, 3)


def _lattice(m):
    xy = NR._lattice()[0]
    return xy, None, 5.0, m, None


def _crowded(r, m):
    return NR._crowded()[0], None, r, m, None


def _slide():
    return NR._slide()[0], None, 12.5, 4, None


def _untyped_singletons():
    return NR._untyped()[0], None, 3.0, 1, None


CASES = {"random": _random, "typed": _typed, "lattice_m5": lambda: _lattice(5), "lattice_m6": lambda: _lattice(6),
         "snake": lambda: (_snake(), None, 1.0, 3, None),
         "crowded_all": lambda: _crowded(50.0, 3000), "crowded_none": lambda: _crowded(50.0, 3001), "crowded_fine": lambda: _crowded(0.2, 4),
         "slide": _slide, "bridge": lambda: (_bridge(), None, 2.5, 5, None),
         "widened": lambda: (NR._widened()[0], None, 1.0, 2, None), "borders": lambda: (NR._borders()[0], None, NR.BORDER_R, 3, None),
         "one_point_m1": lambda: (NR._one_point()[0], None, 1.0, 1, None), "one_point_m2": lambda: (NR._one_point()[0], None, 1.0, 2, None),
         "two_far_points": lambda: (NR._two_far_points()[0], None, 4.999, 1, None), "min_pts_1": _untyped_singletons}


def census(args, res):
    """(clusters, cores, borders, noise, unselected, largest cluster) of a result."""
    xy, types, _r, m, of = args
    label, degree = res["label"], res["degree"]
    sel = np.ones(xy.shape[0], bool) if of is None else np.isin(types, list(of))
    core = degree >= m
    ids, sizes = np.unique(label[label >= 0], return_counts=True)
    return (int(ids.shape[0]), int(core.sum()), int((sel & ~core & (label >= 0)).sum()), int((sel & (label < 0)).sum()), int((~sel).sum()),
            int(sizes.max()) if sizes.shape[0] else 0)


def assert_case_facts(name, res):
    """What each case is there for, asserted on a result (oracle, host or device), so that no case passes vacuously.  The figures
    were computed with `cluster` above."""
    args, _ = case(name)
    xy, types, r, m, of = args
    label, degree = res["label"], res["degree"]
    n = xy.shape[0]
    got = census(args, res)
    core = degree >= m
    assert (label[core] >= 0).all() and (label < n).all() and (label >= -1).all()
    roots = np.unique(label[label >= 0])
    assert (label[roots] == roots).all() and core[roots].all()              # a label is the position of a core of that cluster
    if name == "random":
        assert got == (54, 1613, 271, 116, 0, 445)
        d = np.sqrt(NR.d2_matrix(xy))
        assert np.abs(d - r).min() > 1.0e-4                                 # no pair within rounding of the radius: comparable with sklearn
    elif name == "typed":
        assert got[:5] == (19, 675, 90, 17, 1218)
        out = ~np.isin(types, list(of))
        assert (label[out] == -1).all() and not degree[out].any() and (degree[~out] >= 1).all()
    elif name == "lattice_m5":
        assert int((NR.d2_matrix(xy) == r * r).sum()) == 2 * (39 * 30 + 29 * 40)     # every lattice edge sits at exactly the radius
        assert got == (1, 1064, 132, 4, 0, 1196)
        corners = np.nonzero(((xy[:, 0] == 0) | (xy[:, 0] == 195)) & ((xy[:, 1] == 0) | (xy[:, 1] == 145)))[0]
        assert corners.shape[0] == 4 and (label[corners] == -1).all() and (degree[corners] == 3).all()
    elif name == "lattice_m6":
        assert got == (0, 0, 0, 1200, 0, 0) and int(degree.max()) == 5
    elif name == "snake":
        assert n == 4078 and got == (1, 4076, 2, 0, 0, 4078)
        ends = np.nonzero(degree == 2)[0]
        assert sorted(map(tuple, xy[ends].tolist())) == [(0.0, 0.0), (0.0, 117.0)] and (label == np.nonzero(core)[0].min()).all()
    elif name == "crowded_all":
        assert got == (1, 3000, 0, 0, 0, 3000) and (label == 0).all() and (degree == 3000).all()
    elif name == "crowded_none":
        assert got == (0, 0, 0, 3000, 0, 0) and (degree == 3000).all()
    elif name == "crowded_fine":
        assert got[:4] == (146, 2109, 550, 341)
    elif name == "slide":
        assert got[:4] == (32, 1710, 211, 79)
        same = [0] + list(range(100, 110))
        assert not NR.d2_matrix(xy[same]).any() and len(set(label[same].tolist())) == 1 and len(set(degree[same].tolist())) == 1
    elif name == "bridge":
        d2 = NR.d2_matrix(xy)[0]
        assert d2[2] == 6.25 and d2[n - 1] == 6.25 and (np.delete(d2, [0, 2, n - 1]) > 6.25).all()
        assert got[:4] == (2, 10, 1, 0) and degree[0] == 3 and tuple(np.unique(label[1:]).tolist()) == BRIDGE_ROOTS
        assert label[n - 1] == 1 and label[2] == 2                            # the two nearest cores lie in different clusters,
        assert label[0] == 2                                                  # and the tie goes to position 2: the LARGER root
    elif name == "widened":
        assert got[:4] == (NR.PLANTED, 2 * NR.PLANTED, 0, 500 - NR.PLANTED) and got[5] == 2
        assert label[:NR.PLANTED].tolist() == list(range(NR.PLANTED)) == label[500:].tolist()
    elif name == "borders":
        assert got[0] == 19 and got[3] == 3
    elif name == "one_point_m1":
        assert label.tolist() == [0] and degree.tolist() == [1]
    elif name == "one_point_m2":
        assert label.tolist() == [-1] and degree.tolist() == [1]
    elif name == "two_far_points":
        assert label.tolist() == [0, 1] and degree.tolist() == [1, 1]        # d = 5 > 4.999: two singletons at m = 1
    elif name == "min_pts_1":
        assert core.all() and got == (84, 300, 0, 0, 0, 25) and int((degree == 1).sum()) == 33
        lone = degree == 1
        assert (label[lone] == np.nonzero(lone)[0]).all()                    # an isolated point is a singleton cluster named by itself
    else:
        raise AssertionError("no facts for %s" % name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(args, oracle result) of a case; built once per process and shared: treat both as read-only."""
    args = CASES[name]()
    want = cluster(*args)
    for a in (args[0], args[1]) + tuple(want.values()):
        if a is not None:
            a.setflags(write=False)
    return args, want

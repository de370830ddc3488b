"""The oracle of hover_net_amd/regions.py: ALL points against ALL edges with the definition's own inequalities -- no rows, no cull, no
edge table of the module's: the edges are made canonical here, ring by ring, in plain Python -- and the cases that
tests/test_regions_host.py and tests/test_gpu_regions.py share (each built once, with its oracle result).  Every case runs in well
under a second."""
import functools

import numpy as np


def canonical_edges(polygons):
    """The canonical edges of regions given as nested lists of [n, 2] rings (no repeated closing vertex) -> a list of
    (ax, ay, bx, by, g) with ay < by, in region order; horizontal edges are dropped."""
    out = []
    for g, polys in enumerate(polygons):
        for rings in polys:
            for ring in rings:
                n = len(ring)
                for i in range(n):
                    (x0, y0), (x1, y1) = ring[i], ring[(i + 1) % n]
                    if y0 == y1:
                        continue
                    out.append((x0, y0, x1, y1, g) if y0 < y1 else (x1, y1, x0, y0, g))
    return out


def inside(xy, polygons):
    """bool [G, N]: point i is inside region g -- it crosses an odd number of g's edges."""
    px, py = np.asarray(xy[:, 0], np.float64), np.asarray(xy[:, 1], np.float64)
    par = np.zeros((len(polygons), xy.shape[0]), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for ax, ay, bx, by, g in canonical_edges(polygons):
            ax, ay, bx, by = np.float64(ax), np.float64(ay), np.float64(bx), np.float64(by)
            par[g] ^= (ay <= py) & (py < by) & ((px - ax) * (by - ay) < (bx - ax) * (py - ay))
    return par


def regions(xy, types, polygons, nr_types):
    """-> (first [N], hits [N], count [G, T]), all int32, as the docstring of hover_net_amd/regions.py defines them.  A type outside
    [0, T) is counted nowhere."""
    n, t = xy.shape[0], int(nr_types)
    par = inside(xy, polygons)
    hits = par.sum(0).astype(np.int32)
    first = np.where(hits > 0, par.argmax(0), -1).astype(np.int32)
    types = np.zeros(n, np.int64) if types is None else np.asarray(types, np.int64)
    count = np.zeros((len(polygons), t), np.int32)
    for k in range(t):
        count[:, k] = (par & (types == k)[None, :]).sum(1)
    return first, hits, count


def assert_same(got, want, what=""):
    """A RegionCounts against the oracle's three arrays, with ==."""
    for name, g, w in zip(("first", "hits", "count"), got[:3], want):
        assert isinstance(g, np.ndarray) and g.dtype == np.int32 and g.shape == w.shape, (what, name, getattr(g, "dtype", None), getattr(g, "shape", None))
        assert (g == w).all(), (what, name, np.argwhere(g != w)[:5].tolist())


# ---- the cases: name -> (xy, types | None, RegionSet, nr_types, cell | None) -------------------------------------------------
def _rs(regs, **kw):
    from hover_net_amd import regions as RG

    return RG.RegionSet.from_polygons(regs, **kw)


def _uniform(seed, n, x0, x1, y0, y1, t):
    rng = np.random.default_rng(seed)
    xy = np.stack([x0 + rng.random(n) * (x1 - x0), y0 + rng.random(n) * (y1 - y0)], 1)
    types = None
    if t is not None:
        types = rng.integers(0, t, n).astype(np.int32)
        types[:t] = np.arange(t)                                # every type occurs
    return xy, types


def _lattice(x0, x1, y0, y1, step, seed):
    """Every (x, y) of the lattice of `step` over [x0, x1] x [y0, y1], shuffled."""
    xs, ys = np.arange(x0, x1 + step / 2, step), np.arange(y0, y1 + step / 2, step)
    xy = np.stack([np.repeat(xs, ys.shape[0]), np.tile(ys, xs.shape[0])], 1).astype(np.float64)
    return np.ascontiguousarray(xy[np.random.default_rng(seed).permutation(xy.shape[0])])


def _square(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _circle(cx, cy, r, n, phase=0.0001):
    a = 2.0 * np.pi * np.arange(n) / n + phase
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)


TRIANGLE = [(2.0, 1.0), (17.0, 3.0), (6.0, 14.0)]


def _triangle(n):
    """One region, N at the workgroup's edge; the first point is inside."""
    xy, types = _uniform(60 + n, n, 0.0, 20.0, 0.0, 16.0, 2 if n > 1 else None)
    xy[0] = (8.0, 6.0)
    return xy, types, _rs([[[TRIANGLE]]]), None if n == 1 else 2, None


HOLE_VERTICES = [(3.0, 3.0), (7.0, 3.0), (7.0, 7.0), (3.0, 7.0)]


def _hole():
    """Region 0: a square with a square hole.  Region 1: two squares, the second with a hole.  The half-integer lattice holds every
    vertex, the holes' among them."""
    r0 = [[_square(0.0, 0.0, 10.0, 10.0), HOLE_VERTICES]]
    r1 = [[_square(12.0, 0.0, 16.0, 4.0)], [_square(12.0, 6.0, 16.0, 10.0), _square(13.0, 7.0, 15.0, 9.0)]]
    xy = _lattice(-1.0, 17.0, -1.0, 11.0, 0.5, 61)
    return xy, ((2 * xy[:, 0] + 2 * xy[:, 1]) % 3).astype(np.int32), _rs([r0, r1], names=["ring", "pair"]), 3, None


def _overlap():
    """A quadrilateral inside a big square, and a square that cuts both: hits in 0..3, and (24, 24) lies in all three."""
    regs = [[[[(10.0, 10.0), (28.0, 12.0), (26.0, 27.0), (12.0, 25.0)]]], [[_square(20.0, 20.0, 40.0, 40.0)]], [[_square(0.0, 0.0, 30.0, 30.0)]]]
    xy, types = _uniform(62, 600, -5.0, 45.0, -5.0, 45.0, 4)
    xy[0] = (24.0, 24.0)
    return xy, types, _rs(regs), 4, None


def tessellation(jitter=None):
    """128 triangles that tile [0, 64]^2: the 8 x 8 squares of side 8 with their interior corners moved by integers in [-3, 3] (or by
    `jitter(shape)`), each cut along a diagonal, the diagonals alternating -> (regions, vertices [9, 9, 2])."""
    v = np.stack(np.meshgrid(np.arange(9) * 8.0, np.arange(9) * 8.0, indexing="ij"), -1)
    rng = np.random.default_rng(63)
    v[1:8, 1:8] += rng.integers(-3, 4, (7, 7, 2)).astype(np.float64) if jitter is None else jitter((7, 7, 2))
    regs = []
    for i in range(8):
        for j in range(8):
            a, b, c, d = (tuple(v[i, j]), tuple(v[i + 1, j]), tuple(v[i + 1, j + 1]), tuple(v[i, j + 1]))
            tris = ([a, b, c], [a, c, d]) if (i + j) % 2 == 0 else ([a, b, d], [b, c, d])
            regs += [[[list(t)]] for t in tris]
    return regs, v


def _tessellation():
    regs, _ = tessellation()
    return _lattice(-2.0, 66.0, -2.0, 66.0, 1.0, 64), None, _rs(regs), 1, None


HALF_OPEN = [(0.0, 0.0), (8.0, 0.0), (8.0, 6.0), (4.0, 10.0), (0.0, 6.0)]


def _half_open():
    """A house with vertical walls x = 0 and x = 8 for y in [0, 6]: the half-integer lattice has points with py == ay and py == by of
    every edge, and points ON both walls."""
    return _lattice(-1.0, 9.0, -1.0, 11.0, 0.5, 65), None, _rs([[[HALF_OPEN]]]), 1, None


LONG_RING_TILE = 512            # the kernel's RG_TILE


def _long_ring():
    """One row (the cell is wider than the extent), so its list is the edge table: region 0 a circle of 3000 edges (five tiles and 440
    entries), region 1 a diamond of 4 edges (its boundaries fall inside tile 5), region 2 a circle of 580 edges that ends with the
    last entry of tile 6 (3584 = 7 x 512), region 3 a triangle that starts tile 7."""
    regs = [[[_circle(0.0, 0.0, 50.0, 3000)]], [[[(20.0, 15.0), (25.0, 20.0), (20.0, 25.0), (15.0, 20.0)]]], [[_circle(-15.0, -10.0, 12.0, 580)]],
            [[[(-40.0, 30.0), (-20.0, 33.0), (-33.0, 48.0)]]]]
    xy, types = _uniform(66, 2000, -60.0, 60.0, -60.0, 60.0, 3)
    return xy, types, _rs(regs), 3, 1.0e4


def _many_regions():
    """G = 4096, the cap: squares of side 0.8 on the 64 x 64 integer lattice."""
    regs = [[[_square(float(i), float(j), i + 0.8, j + 0.8)]] for j in range(64) for i in range(64)]
    xy, types = _uniform(67, 3000, 0.0, 64.0, 0.0, 64.0, 2)
    return xy, types, _rs(regs), 2, None


def _tall_edge():
    """400 points over 10^6 x 10^6 with a cell side of 1 asked for: the grid is widened to some 1700 rows, and the two edges of the sliver
    (region 0) are listed in every one of them.  Region 1, a circle of 2000 edges, keeps 8 E above the entries of the sliver."""
    regs = [[[[(4.0e5, -10.0), (4.6e5, -10.0), (4.2e5, 1.0e6 + 10.0)]]], [[_circle(5.0e5, 5.0e5, 2.0e5, 2000)]]]
    xy, types = _uniform(68, 400, 0.0, 1.0e6, 0.0, 1.0e6, 2)
    return xy, types, _rs(regs), 2, 1.0


def _far_outside():
    """Regions wholly above, below, left of and right of the points' extent (their edges land in the clamped end rows), one around all
    points and one among them."""
    regs = [[[_square(20.0, 500.0, 80.0, 600.0)]], [[_square(20.0, -600.0, 80.0, -500.0)]], [[_square(-600.0, 20.0, -500.0, 80.0)]],
            [[_square(500.0, 20.0, 600.0, 80.0)]], [[_square(-1000.0, -1000.0, 1000.0, 1000.0)]], [[[(30.0, 30.0), (70.0, 35.0), (50.0, 75.0)]]]]
    xy, types = _uniform(69, 700, 0.0, 100.0, 0.0, 100.0, 3)
    return xy, types, _rs(regs, names=["above", "below", "left", "right", "around", "among"]), 3, None


def _degenerate():
    """A ring whose edges are all horizontal: no canonical edge at all."""
    xy, types = _uniform(70, 300, 0.0, 10.0, 0.0, 10.0, 2)
    return xy, types, _rs([[[[(0.0, 5.0), (10.0, 5.0), (4.0, 5.0)]]]]), 2, None


def _sixteen_types():
    regs = [[[_square(0.0, 0.0, 60.0, 60.0)]], [[_circle(50.0, 50.0, 30.0, 40)]], [[[(10.0, 80.0), (90.0, 60.0), (70.0, 95.0)]]],
            [[_square(40.0, 0.0, 100.0, 45.0), _square(60.0, 10.0, 80.0, 30.0)]], [[_circle(20.0, 30.0, 15.0, 7)], [_circle(80.0, 80.0, 12.0, 9)]]]
    xy, types = _uniform(71, 2500, 0.0, 100.0, 0.0, 100.0, 16)
    return xy, types, _rs(regs), 16, None


CASES = {"triangle_1": lambda: _triangle(1), "triangle_255": lambda: _triangle(255), "triangle_256": lambda: _triangle(256),
         "triangle_257": lambda: _triangle(257), "hole": _hole, "overlap": _overlap, "tessellation": _tessellation, "half_open": _half_open,
         "long_ring": _long_ring, "many_regions": _many_regions, "tall_edge": _tall_edge, "far_outside": _far_outside, "degenerate": _degenerate,
         "sixteen_types": _sixteen_types}


def assert_case_facts(name, res):
    """What each case is there for, asserted on a result (oracle tuple or RegionCounts), so that no case passes vacuously."""
    from hover_net_amd import regions as RG

    (xy, types, rs, nr_types, cell), _ = case(name)
    first, hits, count = res[:3]
    n, t = xy.shape[0], 1 if nr_types is None else nr_types
    assert first.shape == hits.shape == (n,) and count.shape == (len(rs), t)
    assert ((first >= 0) == (hits > 0)).all() and first.max() < len(rs) and int(count.sum()) == int(hits.sum())
    px, py = xy[:, 0], xy[:, 1]
    if name.startswith("triangle"):
        assert n == int(name.split("_")[1]) and first[0] == 0 and rs.edges.shape == (3, 4) and (n == 1 or 0 < int(hits.sum()) < n)
    elif name == "hole":
        at = lambda x, y: int(hits[(px == x) & (py == y)][0])  # noqa: E731
        assert [at(*v) for v in HOLE_VERTICES] == [0, 1, 1, 1]          # the hole is half-open too: only its lowest-left corner is in it
        assert at(5.0, 5.0) == 0 and at(1.0, 1.0) == 1 and at(14.0, 8.0) == 0 and at(12.5, 6.5) == 1 and at(14.0, 2.0) == 1 and at(14.0, 5.0) == 0
        assert rs.area.tolist() == [100.0 - 16.0, 16.0 + 16.0 - 4.0]
    elif name == "overlap":
        assert sorted(set(hits.tolist())) == [0, 1, 2, 3] and hits[0] == 3 and first[0] == 0
        assert ((hits == 1) & (first == 2)).any() and ((hits == 1) & (first == 1)).any() and ((hits == 2) & (first == 1)).any()
    elif name == "tessellation":
        into = (px >= 0) & (px < 64) & (py >= 0) & (py < 64)
        assert len(rs) == 128 and int(into.sum()) == 64 * 64 and (hits[into] == 1).all() and (hits[~into] == 0).all()
    elif name == "half_open":
        at = lambda x, y: int(hits[(px == x) & (py == y)][0])  # noqa: E731
        assert at(0.0, 3.0) == 1 and at(8.0, 3.0) == 0                  # on the left wall: inside; on the right wall: outside
        assert at(4.0, 0.0) == 1 and at(4.0, 10.0) == 0 and at(0.0, 0.0) == 1 and at(8.0, 0.0) == 0 and at(0.0, 6.0) == 1 and at(8.0, 6.0) == 0
        assert at(4.0, 6.0) == 1 and at(2.0, 8.0) == 1 and at(6.0, 8.0) == 0 and at(-0.5, 3.0) == 0
    elif name == "long_ring":
        ends = np.cumsum(np.bincount(rs.edge_region)).tolist()
        assert ends == [3000, 3004, 3584, 3587] and 3584 == 7 * LONG_RING_TILE and 3000 % LONG_RING_TILE not in (0, LONG_RING_TILE - 4)
        assert RG.cell_side(xy, rs, cell)[1].ncy == 1 and (count.sum(1) > 0).all() and (hits == 2).any()
    elif name == "many_regions":
        assert len(rs) == RG.MAX_G == 4096 and rs.edges.shape[0] == 8192 and hits.max() == 1 and 1500 < int(hits.sum()) < 2300
        assert int((count.sum(1) > 0).sum()) > 1000
    elif name == "tall_edge":
        g = RG.cell_side(xy, rs, cell)[1]
        r0, r1 = RG._rows_of(rs.edges[:2, 1], g), RG._rows_of(rs.edges[:2, 3], g)
        assert g.ncy > 1500 and g.c > 100.0 and r0.tolist() == [0, 0] and r1.tolist() == [g.ncy - 1] * 2 and (rs.edge_region[:2] == 0).all()
        assert int(count[0].sum()) > 3 and int(count[1].sum()) > 20
    elif name == "far_outside":
        assert not count[:4].any() and int(count[4].sum()) == n and 0 < int(count[5].sum()) < n and (first[hits == 2] == 4).all()
        assert RG.cell_side(xy, rs, cell)[1].ncy > 1
    elif name == "degenerate":
        assert rs.edges.shape == (0, 4) and not hits.any() and (first == -1).all() and not count.any()
    elif name == "sixteen_types":
        assert t == 16 and (count > 0).all() and hits.max() >= 2
    else:
        raise AssertionError("no facts for %s" % name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(args, oracle result) of a case; built once per process and shared: treat both as read-only."""
    args = CASES[name]()
    xy, types, rs, nr_types, _cell = args
    want = regions(xy, types, rs.polygons, 1 if nr_types is None else nr_types)
    for a in (xy, types) + want:
        if a is not None:
            a.setflags(write=False)
    return args, want

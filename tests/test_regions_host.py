"""CPU tests of hover_net_amd/regions.py: `regions_host` against the all-edges oracle tests/regions_ref.py with ==, the two properties
of the definition (true point-in-polygon on exact inputs, watertight shared edges), GeoJSON, scale, the derived forms (`resolve`,
`of_info`, `annotate`, `save`, `per_area`), the Python refusals and the C refusals of HVN_OP_NBR_REGIONS, which the library decides
before any launch."""
import ctypes
import json

import numpy as np
import pytest
import torch

import regions_ref as R
from hover_net_amd import neighbours as NB
from hover_net_amd import regions as RG


# -- 1: host == oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_host_equals_oracle(name):
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = RG.regions_host(*args)
    R.assert_same(got, want, name)
    assert got.names == args[2].names and (got.area == args[2].area).all()
    R.assert_same(RG.regions(*args[:4], device=None, cell=args[4]), want, name)


@pytest.mark.parametrize("name", ["hole", "tessellation", "long_ring", "sixteen_types"])
@pytest.mark.parametrize("cell", [0.75, 7.0, 1.0e5])
def test_the_cell_side_changes_nothing(name, cell):
    """Many rows, a few rows, one row (the brute-force form): the same integers."""
    (xy, types, rs, t, _), want = R.case(name)
    R.assert_same(RG.regions_host(xy, types, rs, t, cell), want, name)


def test_row_lists_hold_every_edge_a_point_can_cross():
    """`bin_rows` on the widened grid of `tall_edge`: every (point, edge) pair with ay <= py < by has the edge in the list of the
    point's row, the lists ascend, and their total length respects the bound."""
    (xy, _types, rs, _t, cell), _ = R.case("tall_edge")
    _, g = RG.cell_side(xy, rs, cell)
    row_start, entries = RG.bin_rows(xy, rs, g)
    assert row_start.dtype == entries.dtype == np.int32 and row_start[0] == 0 and row_start[-1] == entries.shape[0] <= RG.max_entries(rs.edges.shape[0], g.ncy)
    prow = RG._rows_of(xy[:, 1], g)
    assert (prow == NB.cells(xy, g)[1]).all()                       # the row of a point is its cell's
    straddle = (rs.edges[None, :, 1] <= xy[:, None, 1]) & (xy[:, None, 1] < rs.edges[None, :, 3])
    for i, e in zip(*np.nonzero(straddle)):
        lst = entries[row_start[prow[i]]:row_start[prow[i] + 1]]
        assert e in lst
    for k in range(g.ncy):
        assert (np.diff(entries[row_start[k]:row_start[k + 1]]) > 0).all()


@pytest.mark.parametrize("name", ["far_outside", "overlap", "tall_edge", "sixteen_types", "long_ring"])
def test_the_lists_cull_drops_only_edges_that_no_point_crosses(name):
    """`listed` against the crossing rule itself, all points x all edges: an edge that is left out is crossed by no point."""
    (xy, _types, rs, _t, _cell), _ = R.case(name)
    keep = RG.listed(xy, rs)
    e = rs.edges
    c = RG.crosses(xy[:, 0][:, None], xy[:, 1][:, None], (e[:, 0], e[:, 1], e[:, 2], e[:, 3]))
    assert not c[:, ~keep].any() and c[:, keep].any()
    if name == "far_outside":        # above, below and left are gone, and the left side of `around`; right stays (every point lies left of it)
        assert [int(keep[rs.edge_region == g].sum()) for g in range(6)] == [0, 0, 0, 2, 1, 3]


def test_regions_that_no_point_can_reach_launch_nothing(monkeypatch):
    """All edges culled: zeros on both paths, and the device form does not get as far as the library."""
    from hover_net_amd import lib as L

    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(L, "lib", no_work)
    monkeypatch.setattr(L, "call", no_work)
    xy, types = R._uniform(73, 300, 0.0, 10.0, 0.0, 10.0, 2)
    rs = RG.RegionSet.from_polygons([[[R._square(2.0, 20.0, 8.0, 30.0)]], [[R._square(-9.0, 2.0, -1.0, 8.0)]]])
    assert rs.edges.shape[0] == 4 and not RG.listed(xy, rs).any()
    for got in (RG.regions_host(xy, types, rs, 2), RG.regions_device(xy, types, rs, 2)):
        R.assert_same(got, R.regions(xy, types, rs.polygons, 2), "unreachable")
        assert not got.hits.any() and not got.count.any() and (got.first == -1).all()
    with pytest.raises(RG.NothingToTest):
        RG.DeviceRegions(xy, types, rs, 2)


# -- 2: the two properties of the definition ---------------------------------------------------------------------
def _star(cx, cy, radii, n, s, salt):
    """An integer star polygon: n vertices around (cx, cy) at the radii in turn, scaled by s, each moved by a few units."""
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        r = radii[k % len(radii)]
        out.append((int(round((cx + r * np.cos(a)) * s)) + (k * 7919 + salt) % 1013, int(round((cy + r * np.sin(a)) * s)) + (k * 104729 + salt) % 997))
    return out


def _pnpoly_int(px, py, rings):
    """Even-odd point-in-polygon in Python integers over the rings AS GIVEN (no canonical edges): a ray towards +x meets edge (i, j)
    when the edge straddles py half-openly and px lies left of it, decided by exact cross-multiplication."""
    inside = False
    for ring in rings:
        n = len(ring)
        for i in range(n):
            (xi, yi), (xj, yj) = ring[i], ring[(i + 1) % n]
            if (yi > py) != (yj > py):
                lhs, rhs = (px - xi) * (yj - yi), (xj - xi) * (py - yi)
                if (lhs < rhs) if yj > yi else (lhs > rhs):
                    inside = not inside
    return inside


def test_property_a_true_point_in_polygon_on_exact_inputs():
    """Star polygons with holes on integer coordinates below 2^25, where every difference and product is exact in float64: the rule is
    exact point-in-polygon, on a 100 x 100 lattice and on every vertex."""
    s = 330000
    r0 = [_star(50, 50, (45, 18), 20, s, 1), _star(50, 50, (12, 5), 8, s, 2)]
    r1 = [_star(30, 65, (28, 9, 20), 18, s, 3), _star(30, 65, (6, 3), 6, s, 4), _star(70, 30, (4, 2), 10, s, 5)]     # the last ring lies outside the star: even-odd takes it as an island
    rings = r0 + r1
    assert max(max(abs(x), abs(y)) for ring in rings for x, y in ring) < 2 ** 25
    pts = [(i * s, j * s) for i in range(100) for j in range(100)] + [v for ring in rings for v in ring]
    assert max(max(p) for p in pts) < 2 ** 25
    rs = RG.RegionSet.from_polygons([[r0], [r1]])
    xy = np.array(pts, np.float64)
    got = RG.regions_host(xy, None, rs)
    want = np.array([[_pnpoly_int(px, py, r) for r in (r0, r1)] for px, py in pts])
    assert 1500 < int(want[:, 0].sum()) < 6000 and 500 < int(want[:, 1].sum()) < 4000
    assert (got.hits == want.sum(1)).all()
    assert (got.first == np.where(want[:, 0], 0, np.where(want[:, 1], 1, -1))).all()
    assert (R.inside(xy, rs.polygons).T == want).all()                # the oracle too


def test_property_b_shared_edges_are_watertight():
    """The integer tessellation puts every lattice point of [0, 64)^2 in exactly one triangle (tests/regions_ref.py asserts it on the
    case).  Here the same tessellation with irrational-scaled, jittered vertices: 200 000 random points, every vertex and every edge
    midpoint are never in two triangles, because a shared edge is stored in one orientation and decides the same for both."""
    rng = np.random.default_rng(72)
    regs, v = R.tessellation(jitter=lambda shape: (rng.random(shape) * 6.0 - 3.0) * np.sqrt(0.5))
    scale = float(np.pi)
    rs = RG.RegionSet.from_polygons(regs, scale=scale)
    assert len(rs) == 128
    # every interior edge occurs twice in the table, bit for bit, once per neighbour
    uniq, times = np.unique(rs.edges, axis=0, return_counts=True)
    assert sorted(set(times.tolist())) == [1, 2] and int((times == 2).sum()) > 150
    mids = [(np.asarray(t[0][0][i]) + np.asarray(t[0][0][(i + 1) % 3])) * 0.5 * scale for t in regs for i in range(3)]
    xy = np.concatenate([rng.random((200000, 2)) * 66.0 * scale - scale, v.reshape(-1, 2) * scale, np.array(mids)])
    got = RG.regions_host(xy, None, rs)
    assert set(got.hits.tolist()) == {0, 1}
    inner = (xy[:200000] > 0.0).all(1) & (xy[:200000] < 64.0 * scale).all(1)
    assert (got.hits[:200000][inner] == 1).all() and not got.hits[:200000][~inner].any()
    assert int(got.count.sum()) == int(got.hits.sum()) and (got.count[:, 0] > 0).all()


# -- 3: GeoJSON and scale ----------------------------------------------------------------------------------------
SQ = [[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0], [0.0, 0.0]]          # closed, as GeoJSON writes rings
HOLE = [[3.0, 3.0], [7.0, 3.0], [7.0, 7.0], [3.0, 7.0], [3.0, 3.0]]
TRI = [[20.0, 0.0], [30.0, 0.0], [25.0, 9.0], [20.0, 0.0]]
COLLECTION = {"type": "FeatureCollection", "features": [
    {"type": "Feature", "properties": {"name": "tumour"}, "geometry": {"type": "Polygon", "coordinates": [SQ, HOLE]}},
    {"type": "Feature", "properties": {"classification": {"name": "stroma", "colorRGB": -1}}, "geometry": {"type": "MultiPolygon", "coordinates": [[TRI], [[[40.0, 0.0], [44.0, 0.0], [44.0, 4.0, 0.0], [40.0, 4.0]]]]}},
    {"type": "Feature", "properties": None, "geometry": {"type": "Polygon", "coordinates": [TRI]}}]}


def _same_set(a, b):
    assert a.names == b.names and (a.edges == b.edges).all() and (a.edge_region == b.edge_region).all() and (a.area == b.area).all()


def test_from_geojson_equals_from_polygons(tmp_path):
    want = RG.RegionSet.from_polygons([[[SQ[:-1], HOLE[:-1]]], [[TRI[:-1]], [[(40.0, 0.0), (44.0, 0.0), (44.0, 4.0), (40.0, 4.0)]]], [[TRI]]],
                                      names=["tumour", "stroma", "region2"])
    assert want.edges.shape == (2 + 2 + 2 + 2 + 2, 4) and want.edge_region.tolist() == [0] * 4 + [1] * 4 + [2] * 2       # the horizontal edges are gone
    assert want.edges.dtype == np.float64
    assert (want.edges[:, 1] < want.edges[:, 3]).all() and want.area.tolist() == [84.0, 45.0 + 16.0, 45.0]
    _same_set(RG.RegionSet.from_geojson(COLLECTION), want)
    path = tmp_path / "a.geojson"
    path.write_text(json.dumps(COLLECTION))
    _same_set(RG.RegionSet.from_geojson(str(path)), want)
    _same_set(RG.RegionSet.from_geojson(path), want)
    _same_set(RG.as_regions(str(path)), want)
    one = RG.RegionSet.from_geojson(COLLECTION["features"][0])               # a bare Feature
    assert one.names == ["tumour"] and (one.edges == want.edges[:4]).all()
    bare = RG.RegionSet.from_geojson({"type": "MultiPolygon", "coordinates": [[TRI]]})      # a bare geometry
    assert bare.names == ["region0"] and (bare.edges == want.edges[4:6]).all()
    for kind in ("Point", "LineString", "GeometryCollection"):
        with pytest.raises(ValueError, match=kind):
            RG.RegionSet.from_geojson({"type": "Feature", "properties": {}, "geometry": {"type": kind, "coordinates": [1.0, 2.0]}})
    with pytest.raises(ValueError, match="None"):
        RG.RegionSet.from_geojson({"type": "Feature", "properties": {}, "geometry": None})
    with pytest.raises(ValueError):
        RG.RegionSet.from_geojson({"type": "FeatureCollection", "features": []})        # no region at all
    with pytest.raises(ValueError):
        RG.RegionSet.from_geojson([1, 2])


def test_scale_multiplies_every_vertex_once():
    third = 1.0 / 3.0
    a = RG.RegionSet.from_geojson(COLLECTION, scale=third)
    b = RG.RegionSet.from_polygons([[[(np.array(SQ) * third).tolist(), (np.array(HOLE) * third).tolist()]],
                                    [[(np.array(TRI) * third).tolist()], [[(40.0 * third, 0.0), (44.0 * third, 0.0), (44.0 * third, 4.0 * third), (40.0 * third, 4.0 * third)]]],
                                    [[(np.array(TRI) * third).tolist()]]], names=a.names)
    _same_set(a, b)
    xy = np.array([[1.0, 1.0], [5.0, 5.0], [2.0, 2.0], [25.0, 3.0]])
    assert RG.regions_host(xy, None, RG.RegionSet.from_geojson(COLLECTION)).first.tolist() == [0, -1, 0, 1]
    assert RG.regions_host(xy * 0.25, None, RG.RegionSet.from_geojson(COLLECTION, scale=0.25)).first.tolist() == [0, -1, 0, 1]     # a power of two: exact
    assert RG.regions_host(xy, None, RG.RegionSet.from_geojson(COLLECTION, scale=0.25)).first.tolist() == [-1, -1, 0, -1]      # (1, 1) now lies in the hole [0.75, 1.75]^2
    assert RG.resolve({"regions": COLLECTION, "scale": 0.25}).area.tolist() == [84.0 / 16, 61.0 / 16, 45.0 / 16]


# -- 4: refusals -------------------------------------------------------------------------------------------------
T3 = [(0.0, 0.0), (4.0, 0.0), (0.0, 3.0)]
BAD_SETS = [([[[[(0.0, 0.0), (1.0, np.nan), (0.0, 1.0)]]]], {}, ValueError), ([[[[(0.0, 0.0), (np.inf, 0.0), (0.0, 1.0)]]]], {}, ValueError),
            ([[[[(0.0, 0.0), (1.0, 1.0)]]]], {}, ValueError), ([[[[(0.0, 0.0), (1.0, 1.0), (0.0, 0.0)]]]], {}, ValueError),       # two vertices once the closing one is dropped
            ([[[T3, [(1.0, 1.0)]]]], {}, ValueError), ([], {}, ValueError), ([[[T3]]] * 4097, {}, ValueError),
            ([[[[(0.0, 0.0), (True, 0.0), (0.0, 1.0)]]]], {}, TypeError), ([[[[(0.0, 0.0), ("1", 0.0), (0.0, 1.0)]]]], {}, TypeError),
            ([[[[(0.0, 0.0), (1.0,), (0.0, 1.0)]]]], {}, TypeError), ([[[5.0]]], {}, TypeError), ([[5.0]], {}, TypeError), ([5.0], {}, TypeError),
            ("abc", {}, TypeError), ([[[T3]]], {"scale": 0.0}, ValueError), ([[[T3]]], {"scale": -1.0}, ValueError), ([[[T3]]], {"scale": np.inf}, ValueError),
            ([[[T3]]], {"scale": True}, TypeError), ([[[T3]]], {"scale": "2"}, TypeError), ([[[[(1e308, 0.0), (0.0, 1.0), (1.0, 1.0)]]]], {"scale": 10.0}, ValueError),
            ([[[T3]]], {"names": ["a", "b"]}, ValueError), ([[[T3]]], {"names": [3]}, ValueError)]


@pytest.mark.parametrize("regs,kw,exc", BAD_SETS, ids=[str(i) for i in range(len(BAD_SETS))])
def test_bad_regions_are_refused_before_any_edge_is_made(regs, kw, exc, monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(RG.RegionSet, "__init__", no_work)
    with pytest.raises(exc):
        RG.RegionSet.from_polygons(regs, **kw)


def test_too_many_edges_are_refused_and_the_caps_admitted(monkeypatch):
    monkeypatch.setattr(RG, "MAX_E", 10)
    ring11 = [(float(k), float(k * k)) for k in range(11)]
    with pytest.raises(ValueError, match="edges"):
        RG.RegionSet.from_polygons([[[ring11]]])
    assert RG.RegionSet.from_polygons([[[ring11[:10]]]]).edges.shape == (10, 4)
    monkeypatch.undo()
    assert len(RG.RegionSet.from_polygons([[[T3]]] * 4096)) == 4096 == RG.MAX_G and RG.MAX_E == 1 << 22


GOOD = dict(xy=np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 2.0]]), types=np.array([0, 1, 1], np.int32), rs=RG.RegionSet.from_polygons([[[T3]]]), nr_types=2, cell=None)
BAD = [("xy", GOOD["xy"].astype(np.float32), TypeError), ("xy", GOOD["xy"].tolist(), TypeError), ("xy", np.zeros((3, 3)), ValueError), ("xy", np.zeros((0, 2)), ValueError),
       ("xy", np.array([[0.0, 0.0], [np.nan, 1.0], [0.5, 2.0]]), ValueError), ("xy", np.array([[0.0, 0.0], [np.inf, 1.0], [0.5, 2.0]]), ValueError),
       ("xy", np.array([[-1e308, 0.0], [1e308, 1.0], [0.5, 2.0]]), ValueError), ("types", GOOD["types"].astype(np.int64), TypeError), ("types", [0, 1, 1], TypeError),
       ("types", np.array([0, 1], np.int32), ValueError), ("types", np.array([0, 2, 1], np.int32), ValueError), ("types", np.array([0, -1, 1], np.int32), ValueError),
       ("nr_types", 17, ValueError), ("nr_types", 0, ValueError), ("nr_types", 2.0, TypeError), ("nr_types", True, TypeError),
       ("rs", [[[T3]]], TypeError), ("rs", None, TypeError), ("rs", "a.geojson", TypeError),
       ("cell", 0.0, ValueError), ("cell", -2.0, ValueError), ("cell", np.inf, ValueError), ("cell", np.nan, ValueError), ("cell", True, TypeError), ("cell", "3", TypeError)]


@pytest.mark.parametrize("field,value,exc", BAD, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BAD)])
def test_python_refusals_precede_any_work(field, value, exc, monkeypatch):
    """Both paths refuse in `_check`: before a grid is chosen and, for the device form, before anything is allocated or launched."""
    from hover_net_amd import lib as L
    from hover_net_amd import points as P

    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(L, "lib", no_work)
    monkeypatch.setattr(L, "call", no_work)
    monkeypatch.setattr(P, "grid", no_work)
    monkeypatch.setattr(RG, "bin_rows", no_work)
    args = dict(GOOD, **{field: value})
    for fn in (RG.regions_host, RG.regions_device):
        with pytest.raises(exc):
            fn(args["xy"], args["types"], args["rs"], args["nr_types"], cell=args["cell"])
    with pytest.raises(exc):
        RG.regions(args["xy"], args["types"], args["rs"], args["nr_types"], device="cuda", cell=args["cell"])


def test_a_device_that_is_no_gpu_is_refused():
    with pytest.raises(ValueError, match="GPU"):
        RG.regions_device(GOOD["xy"], GOOD["types"], GOOD["rs"], 2, device="cpu")
    with pytest.raises(ValueError, match="GPU"):
        RG.regions_device(*R.case("degenerate")[0][:4], device="cpu")


def _op():
    """A well-formed REGIONS op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.x.h = PL.OP_NBR_REGIONS, ncy, ncx, n
    op.w, op.x2.base, op.x2.sn = P(1), P(2), NB.workspace_bytes(n, ncy * ncx)
    op.cout, op._rsv, op.bias = 5, 12, P(3)
    op.res.base, op.res.h = P(4), 700
    op.y2.base, op.y2.sn = P(6), 1500
    op.y.base = P(5)
    return op


# one entry per refusal that include/hvn.h lists for NBR_REGIONS: (field, value, status)
REGIONS_REFUSALS = [("y.base", None, -1), ("bias", None, -1), ("res.base", None, -1), ("y2.base", None, -1), ("y.base", 0x15000002, -1), ("res.base", 0x14000001, -1),
                    ("y2.base", 0x16000002, -1), ("bias", 0x13000004, -1), ("cout", 0, -1), ("cout", 17, -1), ("cout", -3, -1), ("_rsv", 0, -1), ("_rsv", -1, -1),
                    ("res.h", 0, -1), ("res.h", -7, -1), ("y2.sn", 0, -1), ("y2.sn", -1, -1), ("_rsv", 4097, -4), ("res.h", (1 << 22) + 1, -4),
                    ("y2.sn", 8 * 700 + 30 + 1, -4), ("y2.sn", 1 << 40, -4)]
SHARED_REFUSALS = [("w", None, -1), ("x2.base", None, -1), ("w", 0x11000004, -1), ("x2.base", 0x12000004, -1), ("x.h", 0, -1), ("x.h", -5, -1),
                   ("kh", 0, -1), ("kw", -1, -1), ("x.h", (1 << 26) + 1, -4), ("kh", 4097, -4), ("kw", 4097, -4), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4),
                   ("x2.sn", 0, -4)]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_op_kind_19_is_in_the_header_and_the_plan():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    assert PL.OP_NBR_REGIONS == 19 and "HVN_OP_NBR_REGIONS = 19" in open(L.HEADER).read() and "hvn_regions.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                      # no new export


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_REGIONS list: its status, a text that leads with the op's name, decided before any launch
    (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as tests/test_ripley_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_regions:") and b"unknown op kind" not in err, (rc, err)

    for path, value, code in REGIONS_REFUSALS + SHARED_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 1, code)
    refused(_op(), 2, -1)                                            # batch must be 1
    op = _op()
    op.kh, op.kw = 2049, 2049                                        # each axis allowed, 2^22 cells exceeded
    op.x2.sn = 1 << 40
    refused(op, 1, -4)
    op = _op()
    op._rsv, op.res.h, op.y2.sn = 4096, 1 << 22, 8 * (1 << 22) + 30  # the caps themselves pass the op's own checks: the next refusal is the shared one
    op.x.h = 0
    rc = l.hvn_run_op(ctypes.byref(op), 1, None)
    assert rc == -1 and l.hvn_last_error().startswith(b"nbr_regions: N = 0")
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1)                                             # an all-zero op is refused by name


def test_c_refusals_leave_the_output_untouched_on_the_host_side():
    """The refusals above return before the launcher is entered; here the same with a real host buffer standing in for the output:
    a refused REGIONS does not write it (the op that runs writes EVERY element)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    buf = np.full(2 * 1000 + 12 * 5, 0x5A5A5A5A, np.int32)
    for path, value in (("cout", 0), ("_rsv", 0), ("_rsv", 5000), ("res.h", 0), ("y2.sn", 0), ("x.h", 0), ("x2.sn", 8), ("kh", 5000), ("bias", None)):
        op = _op()
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()


# -- 5: what a user reads -----------------------------------------------------------------------------------------
def _stub_info(typed=False):
    return {1: {"bbox": np.array([[2, 3], [8, 9]]), "centroid": np.array([5.5, 4.5]), "contour": np.array([[3, 2], [3, 7], [8, 7], [8, 2]], np.int32),
                "type_prob": 0.9 if typed else None, "type": 1 if typed else None},
            4: {"bbox": np.array([[12, 10], [20, 15]]), "centroid": np.array([12.0, 15.5]), "contour": np.array([[10, 12], [10, 19], [14, 19], [14, 12]], np.int32),
                "type_prob": 0.8 if typed else None, "type": 2 if typed else None},
            9: {"bbox": np.array([[14, 12], [20, 18]]), "centroid": np.array([15.0, 19.5]), "contour": np.array([[12, 14], [12, 19], [17, 19], [17, 14]], np.int32),
                "type_prob": 0.7 if typed else None, "type": 1 if typed else None}}


STUB_GEOJSON = {"type": "FeatureCollection", "features": [
    {"type": "Feature", "properties": {"name": "roi"}, "geometry": {"type": "Polygon", "coordinates": [[[0, 0], [40, 0], [40, 17], [0, 17], [0, 0]]]}},
    {"type": "Feature", "properties": {"name": "core"}, "geometry": {"type": "Polygon", "coordinates": [[[10, 14], [20, 14], [20, 30], [10, 30]]]}}]}


def test_resolve():
    rs = RG.RegionSet.from_geojson(STUB_GEOJSON)
    assert RG.resolve(None) is None and RG.resolve({"regions": rs}) is rs
    _same_set(RG.resolve({"regions": STUB_GEOJSON}), rs)
    _same_set(RG.resolve({"regions": [[[[(0, 0), (40, 0), (40, 17), (0, 17)]]], [[[(10, 14), (20, 14), (20, 30), (10, 30)]]]]}),
              RG.RegionSet.from_polygons(rs.polygons))
    assert RG.resolve({"regions": STUB_GEOJSON, "scale": 2.0}).area.tolist() == [4 * 680.0, 4 * 160.0]
    for bad, exc in (({"region": rs}, ValueError), ({"regions": rs, "radius": 1.0}, ValueError), (rs, ValueError), ({"regions": rs, "scale": 2.0}, ValueError),
                     ({"regions": 5}, TypeError), ({"regions": STUB_GEOJSON, "scale": "x"}, TypeError), ({"regions": STUB_GEOJSON, "scale": 0}, ValueError)):
        with pytest.raises(exc):
            RG.resolve(bad)


def test_of_info_annotate_save_and_per_area(tmp_path):
    rs = RG.RegionSet.from_geojson(STUB_GEOJSON)
    empty = RG.of_info({}, rs, 3)
    assert empty.first.shape == empty.hits.shape == (0,) and empty.count.tolist() == [[0, 0, 0]] * 2 and empty.names == ["roi", "core"]
    assert RG.annotate({}, empty) == {}
    info = _stub_info(typed=True)
    rc = RG.of_info(info, rs, 3)
    assert rc.first.tolist() == [0, 0, 1] and rc.hits.tolist() == [1, 2, 1] and rc.count.tolist() == [[0, 1, 1], [0, 1, 1]]
    assert rc.first.dtype == rc.hits.dtype == rc.count.dtype == np.int32 and rc.area.tolist() == [680.0, 160.0]
    untyped = RG.of_info(_stub_info(), rs, None)
    assert untyped.count.tolist() == [[2], [2]] and untyped.first.tolist() == rc.first.tolist()
    keys = {lab: set(e) for lab, e in info.items()}
    assert RG.annotate(info, rc) is info and [e["region"] for e in info.values()] == [0, 0, 1]
    assert all(type(e["region"]) is int and set(e) == keys[lab] | {"region"} for lab, e in info.items())
    with pytest.raises(ValueError):
        RG.annotate({1: {}}, rc)
    assert RG.per_area(rc).tolist() == [[0.0, 1 / 680.0, 1 / 680.0], [0.0, 1 / 160.0, 1 / 160.0]]
    flat = RG.RegionCounts(rc.first, rc.hits, rc.count, rc.names, np.array([680.0, 0.0]))
    assert np.isnan(RG.per_area(flat)[1]).all() and not np.isnan(RG.per_area(flat)[0]).any()
    RG.save(tmp_path / "r.npz", rc)
    with np.load(tmp_path / "r.npz") as z:                           # no pickle
        assert sorted(z.files) == ["area", "count", "first", "hits", "names"]
        assert z["names"].tolist() == ["roi", "core"] and z["area"].tolist() == [680.0, 160.0]
        for name in ("first", "hits", "count"):
            assert z[name].dtype == np.int32 and (z[name] == getattr(rc, name)).all()


# -- the managers, with the GPU call replaced by a stub (the GPU runs are in tests/test_gpu_regions.py) -------------------------
def _load(path):
    with np.load(path) as z:
        assert sorted(z.files) == ["area", "count", "first", "hits", "names"]
        return RG.RegionCounts(z["first"], z["hits"], z["count"], z["names"].tolist(), z["area"])


def test_process_file_list_writes_regions_npz(tmp_path, caplog):
    from hover_net_amd import infer_manager as im

    inp, ann = tmp_path / "in", tmp_path / "ann"
    inp.mkdir()
    ann.mkdir()
    for name in "ab":
        np.save(inp / (name + ".npy"), np.random.default_rng(0).integers(0, 256, (40, 50, 3), dtype=np.uint8))
    (ann / "a.geojson").write_text(json.dumps(STUB_GEOJSON))         # none for b

    def process(images):
        return [(np.zeros(i.shape[:2], np.int32), _stub_info()) for i in images]

    mgr = im.InferManager({"model_args": {"nr_types": None, "mode": "original"}, "model_path": None}, process_fn=process)
    text = {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out)}
        if flag:
            args["regions"] = {"dir": str(ann)}
        with caplog.at_level("WARNING"):
            assert mgr.process_file_list(args) == ["a", "b"]
        assert (out / "regions").exists() == flag
        text[flag] = {name: json.load(open(out / "json" / (name + ".json"))) for name in "ab"}
        raw = open(out / "json" / "b.json").read()
        text[flag, "b"] = raw
    assert text[True, "b"] == text[False, "b"]                       # the image without a file: json byte-identical, nothing written, logged
    assert not (tmp_path / "out1" / "regions" / "b.npz").exists() and "b.geojson is missing" in caplog.text
    rc = _load(tmp_path / "out1" / "regions" / "a.npz")
    R.assert_same(rc, RG.of_info(_stub_info(), RG.RegionSet.from_geojson(STUB_GEOJSON), None)[:3], "tile manager")
    assert rc.first.tolist() == [0, 0, 1] and rc.names == ["roi", "core"]
    nuc = text[True]["a"]["nuc"]
    assert [nuc[k]["region"] for k in ("1", "4", "9")] == [0, 0, 1]
    assert {k: {f: v for f, v in e.items() if f != "region"} for k, e in nuc.items()} == text[False]["a"]["nuc"]
    half = tmp_path / "half"
    assert mgr.process_file_list({"input_dir": str(inp), "output_dir": str(half), "regions": {"dir": str(ann), "scale": 0.5}}) == ["a", "b"]
    assert _load(half / "regions" / "a.npz").first.tolist() == [0, -1, -1] and _load(half / "regions" / "a.npz").area.tolist() == [170.0, 40.0]
    for bad, exc in (({"path": str(ann)}, ValueError), ({"dir": 5}, ValueError), ({"dir": str(ann), "scale": 0.0}, ValueError), ({"dir": str(ann), "scale": "2"}, TypeError),
                     (str(ann), ValueError)):
        with pytest.raises(exc):
            mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "regions": bad})
    assert not (tmp_path / "bad").exists()                           # refused before any file is touched


def test_process_wsi_list_writes_regions_npz(tmp_path, caplog):
    from hover_net_amd import infer_manager as im

    inp, ann = tmp_path / "slides", tmp_path / "ann"
    inp.mkdir()
    ann.mkdir()
    for name in "st":
        np.save(inp / (name + ".npy"), np.random.default_rng(1).integers(30, 120, (64, 96, 3), dtype=np.uint8))
    (ann / "s.geojson").write_text(json.dumps(STUB_GEOJSON))
    mgr = im.WsiManager({"model_args": {"nr_types": None, "mode": "fast"}, "model_path": None}, wsi_fn=lambda slide, mask: (None, _stub_info()))
    text = {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out)}
        if flag:
            args["regions"] = {"dir": str(ann)}
        with caplog.at_level("WARNING"):
            assert mgr.process_wsi_list(args) == {"s": "done", "t": "done"}
        assert (out / "regions").exists() == flag
        text[flag] = {name: open(out / (name + ".json")).read() for name in "st"}
    assert text[True]["t"] == text[False]["t"] and not (tmp_path / "out1" / "regions" / "t.npz").exists() and "t.geojson is missing" in caplog.text
    rc = _load(tmp_path / "out1" / "regions" / "s.npz")
    assert rc.first.tolist() == [0, 0, 1] and rc.hits.tolist() == [1, 2, 1] and rc.count.tolist() == [[2], [2]]
    assert [e["region"] for e in json.loads(text[True]["s"])["nuc"].values()] == [0, 0, 1]
    with pytest.raises(ValueError):
        mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "regions": {"dirs": str(ann)}})
    assert not (tmp_path / "bad").exists()

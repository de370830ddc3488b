"""CPU tests of hover_net_amd/margins.py: `margins_host` against the all-segments oracle tests/margins_ref.py with == (near_d2 included),
exact geometry on small integers, the row lists and their cull, the host helpers, the Python refusals and the C refusals of
HVN_OP_NBR_MARGINS (decided before any launch), and the "margin" key of the `regions` spec through `resolve`, `of_info`, `annotate`,
`save` and the two managers."""
import ctypes
import json

import numpy as np
import pytest
import torch

import margins_ref as M
import regions_ref as R
from hover_net_amd import margins as MG
from hover_net_amd import neighbours as NB
from hover_net_amd import regions as RG


def _run(args, **kw):
    return MG.margins_host(*args[:4], nr_types=args[4], cell=kw.get("cell", args[5]))


# -- 1: host == oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_host_equals_oracle(name):
    args, want = M.case(name)
    M.assert_case_facts(name, want)
    got = _run(args)
    M.assert_same(got, want, name)
    assert got.widths == tuple(float(w) for w in args[3]) and got.names == args[2].names
    M.assert_same(MG.margins(*args[:4], nr_types=args[4], device=None, cell=args[5]), want, name)


@pytest.mark.parametrize("name", ["hole", "overlap", "long_ring", "sixteen_by_sixteen", "random_1", "outside"])
@pytest.mark.parametrize("cell", [0.75, 7.0, 1.0e5])
def test_the_cell_side_changes_nothing(name, cell):
    """Many rows, a few rows, one row (the brute-force form): the same numbers."""
    args, want = M.case(name)
    M.assert_same(_run(args, cell=cell), want, name)


def test_horizontal_edges_are_boundary():
    """(5, -3) is 3 from the horizontal edge y = 0 of [0, 10]^2, not sqrt(34) from a corner: `RegionSet.edges` has no such edge, the
    segment table does."""
    (xy, _t, rs, widths, _n, _c), want = M.case("square_exact")
    seg, sreg, box = MG.segments(rs, widths[-1])
    assert rs.edges.shape == (2, 4) and seg.shape == (4, 4) and sreg.tolist() == [0] * 4 and seg.dtype == box.dtype == np.float64 and sreg.dtype == np.int32
    assert seg.tolist() == [[0.0, 0.0, 10.0, 0.0], [10.0, 0.0, 10.0, 10.0], [0.0, 10.0, 10.0, 10.0], [0.0, 0.0, 0.0, 10.0]]
    assert box.tolist() == [[-5.0, -5.0, 15.0, 5.0], [5.0, -5.0, 15.0, 15.0], [-5.0, 5.0, 15.0, 15.0], [-5.0, -5.0, 5.0, 15.0]]
    assert want[1][0] == 9.0 and want[1][0] != 34.0
    only_vertical = [s for s in M.segments_of(rs.polygons) if s[1] != s[3]]
    assert min(M.d2_of(5.0, -3.0, *s[:4]) for s in only_vertical) == 34.0


def test_non_horizontal_segments_are_the_edges_of_regions_py():
    """The orientation of a non-horizontal segment is exactly the canonical edge's, so `inside` is the membership of regions.py."""
    for name in ("random_1", "hole", "long_ring"):
        rs = M.case(name)[0][2]
        seg, sreg, _ = MG.segments(rs, 1.0)
        keep = seg[:, 1] != seg[:, 3]
        assert (seg[keep] == rs.edges).all() and (sreg[keep] == rs.edge_region).all()
        assert ((seg[:, 1] < seg[:, 3]) | ((seg[:, 1] == seg[:, 3]) & (seg[:, 0] <= seg[:, 2]))).all() and (np.diff(sreg) >= 0).all()


def test_a_shared_edge_is_one_segment_and_gives_one_distance():
    """The edge x = 10 that the two regions of `shared_edge` share is bit-identical in both, so each region alone gives the same
    near_d2 for the points nearest to it, from either side, and together the smaller region keeps the tie."""
    (xy, _t, rs, widths, _n, _c), want = M.case("shared_edge")
    seg, sreg, _ = MG.segments(rs, widths[-1])
    a, b = seg[sreg == 0], seg[sreg == 1]
    assert sum((a == row).all(1).any() for row in b) == 1
    alone = [MG.margins_host(xy, None, RG.RegionSet.from_polygons([rs.polygons[g]]), widths) for g in (0, 1)]
    assert (alone[0].near_d2 == alone[1].near_d2).all() and (alone[0].near == 0).all() and (alone[1].near == 0).all()
    assert (want[0] == 0).all() and (want[1] == alone[0].near_d2).all()
    assert (alone[0].near_inside[:17] == 1).all() and (alone[1].near_inside[:17] == 0).all() and (alone[1].near_inside[17:34] == 1).all()


@pytest.mark.parametrize("name", ["hole", "overlap", "outside", "random_2", "sixteen_by_sixteen"])
def test_inside_is_the_membership_of_regions_py(name):
    """near_inside equals membership in the near region as the crossing rule of regions.py gives it (its oracle and its host form), and
    the inside counts at the largest width never exceed the region's count."""
    (xy, types, rs, widths, t, _c), want = M.case(name)
    got = _run(M.case(name)[0])
    member = R.inside(xy, rs.polygons)                              # [G, N], all points x all canonical edges
    has = got.near >= 0
    assert has.any() and (got.near_inside[has] == member[got.near[has], np.flatnonzero(has)]).all()
    rc = RG.regions_host(xy, types, rs, t)
    assert (got.count[:, 1, -1, :] <= rc.count).all() and (rc.first[has & (got.near_inside == 1)] >= 0).all()


def test_row_lists_hold_every_segment_whose_box_holds_the_point():
    """`bin_rows` on the grids of three cases: every (point, segment) pair with the point in the segment's box, or the point crossing
    the segment, has the segment in the list of the point's row; the lists ascend; their total length respects the bound."""
    for name in ("many_rows", "outside", "random_3"):
        (xy, _t, rs, widths, _n, cell), _ = M.case(name)
        seg, sreg, box = MG.segments(rs, widths[-1])
        keep = MG.listed(xy, seg, box)
        _, g = MG.cell_side(xy, box, keep, cell)
        row_start, entries = MG.bin_rows(box, keep, g)
        assert row_start.dtype == entries.dtype == np.int32 and row_start[0] == 0 and row_start[-1] == entries.shape[0] <= MG.max_entries(seg.shape[0], g.ncy)
        prow = RG._rows_of(xy[:, 1], g)
        assert (prow == NB.cells(xy, g)[1]).all()
        px, py = xy[:, 0][:, None], xy[:, 1][:, None]
        need = MG.in_box(px, py, box.T) | RG.crosses(px, py, seg.T)
        lists = [set(entries[row_start[k]:row_start[k + 1]].tolist()) for k in range(g.ncy)]
        assert need.any() and all(s in lists[prow[i]] for i, s in zip(*np.nonzero(need)))
        assert all((np.diff(entries[row_start[k]:row_start[k + 1]]) > 0).all() for k in range(g.ncy))


@pytest.mark.parametrize("name", ["far", "outside", "overlap", "many_rows"])
def test_the_lists_cull_drops_only_segments_that_no_point_is_near_or_crosses(name):
    (xy, _t, rs, widths, _n, _c), _ = M.case(name)
    seg, _sreg, box = MG.segments(rs, widths[-1])
    keep = MG.listed(xy, seg, box)
    px, py = xy[:, 0][:, None], xy[:, 1][:, None]
    need = MG.in_box(px, py, box.T) | RG.crosses(px, py, seg.T)
    assert not need[:, ~keep].any() and (~keep).any() == (name in ("far", "outside"))


def test_empty_lists_launch_and_compute_nothing_on_the_host(monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work was started")

    args, want = M.case("far")
    monkeypatch.setattr(MG, "bin_rows", no_work)
    monkeypatch.setattr(MG, "d2_of", no_work)
    M.assert_same(_run(args), want, "far")


# -- 2: the helpers on a hand-computed case ----------------------------------------------------------------------
def test_rings_signed_distance_and_profile():
    """`square_exact`, widths 1 / 3 / 5: outside the square one point on it, one at 3, three at 5; inside three on or 1 from the
    boundary and one at 5."""
    args, _ = M.case("square_exact")
    m = _run(args)
    assert m.count[0, :, :, 0].tolist() == [[1, 2, 5], [3, 3, 4]]
    assert MG.rings(m)[0, :, :, 0].tolist() == [[1, 1, 3], [3, 0, 1]] and MG.rings(m).dtype == np.int32
    d = MG.signed_distance(m)
    assert d[[0, 1, 2, 5, 8, 9]].tolist() == [3.0, 5.0, -5.0, 5.0, 5.0, -1.0] and np.isnan(d[[6, 10]]).all() and (d[[3, 4, 7]] == 0.0).all()
    assert MG.profile(m, 0)[:, 0].tolist() == [1, 0, 3, 1, 1, 3] and MG.profile(m, 0).shape == (6, 1)
    typed = MG.margins_host(args[0], (np.arange(11) % 2).astype(np.int32), args[2], args[3], 2)
    assert (typed.count.sum(-1) == m.count[..., 0]).all() and MG.profile(typed, 0).shape == (6, 2) and (MG.profile(typed, 0).sum(1) == MG.profile(m, 0)[:, 0]).all()


# -- 3: refusals -------------------------------------------------------------------------------------------------
T3 = [(0.0, 0.0), (4.0, 0.0), (0.0, 3.0)]
GOOD = dict(xy=np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 2.0]]), types=np.array([0, 1, 1], np.int32), rs=RG.RegionSet.from_polygons([[[T3]]]), widths=[0.5, 1.0],
            nr_types=2, cell=None)
BAD_WIDTHS = [([], ValueError), (list(range(1, 18)), ValueError), ([1.0, 1.0], ValueError), ([2.0, 1.0], ValueError), ([0.0, 1.0], ValueError), ([-1.0], ValueError),
              ([np.nan], ValueError), ([1.0, np.inf], ValueError), ([1e200], ValueError), ([1e-300], ValueError), ([True], TypeError), (["1"], TypeError),
              ([None], TypeError), (2.0, TypeError), ("12", TypeError), (None, TypeError), ({"w": 1.0}, TypeError)]
BAD = [("widths", w, exc) for w, exc in BAD_WIDTHS] + [
    ("xy", GOOD["xy"].astype(np.float32), TypeError), ("xy", np.zeros((0, 2)), ValueError), ("xy", np.array([[0.0, 0.0], [np.nan, 1.0], [0.5, 2.0]]), ValueError),
    ("types", GOOD["types"].astype(np.int64), TypeError), ("types", np.array([0, 2, 1], np.int32), ValueError), ("nr_types", 17, ValueError), ("nr_types", 2.0, TypeError),
    ("rs", [[[T3]]], TypeError), ("rs", None, TypeError), ("cell", 0.0, ValueError), ("cell", np.nan, ValueError), ("cell", "3", TypeError)]


@pytest.mark.parametrize("field,value,exc", BAD, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BAD)])
def test_python_refusals_precede_any_work(field, value, exc, monkeypatch):
    """Both paths refuse in `_check`: before a segment is made and, for the device form, before anything is allocated or launched."""
    from hover_net_amd import lib as L
    from hover_net_amd import points as P

    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(L, "lib", no_work)
    monkeypatch.setattr(L, "call", no_work)
    monkeypatch.setattr(P, "grid", no_work)
    monkeypatch.setattr(MG, "segments", no_work)
    args = dict(GOOD, **{field: value})
    for fn in (MG.margins_host, MG.margins_device):
        with pytest.raises(exc):
            fn(args["xy"], args["types"], args["rs"], args["widths"], args["nr_types"], cell=args["cell"])
    with pytest.raises(exc):
        MG.margins(args["xy"], args["types"], args["rs"], args["widths"], args["nr_types"], device="cuda", cell=args["cell"])


def test_the_caps_are_admitted_and_a_device_that_is_no_gpu_is_refused():
    assert MG.check_widths(range(1, 17)) == tuple(float(k) for k in range(1, 17)) and MG.check_widths(np.array([0.5, 2.0])) == (0.5, 2.0)
    assert MG.check_widths((3,)) == (3.0,) and MG.MAX_B == 16 and MG.MAX_S == 1 << 22
    with pytest.raises(ValueError, match="margins_device needs a GPU"):
        MG.margins_device(GOOD["xy"], GOOD["types"], GOOD["rs"], GOOD["widths"], 2, device="cpu")


def test_too_many_segments_are_refused(monkeypatch):
    monkeypatch.setattr(MG, "MAX_S", 2)
    with pytest.raises(ValueError, match="ring edges"):
        MG.margins_host(GOOD["xy"], None, GOOD["rs"], [1.0])


def _op():
    """A well-formed MARGINS op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.x.h = PL.OP_NBR_MARGINS, ncy, ncx, n
    op.w, op.x2.base, op.x2.sn = P(1), P(2), NB.workspace_bytes(n, ncy * ncx)
    op.cout, op._rsv, op.cout2, op.bias, op.w2 = 5, 12, 3, P(3), P(7)
    op.res.base, op.res.h = P(4), 700
    op.y2.base, op.y2.sn = P(6), 1500
    op.y.base, op.y.sn = P(5), 16 * n + 8 * 12 * 3 * 5
    return op


# one entry per refusal that include/hvn.h lists for NBR_MARGINS: (field, value, status, a word of its text)
MARGINS_REFUSALS = [("y.base", None, -1, b"null"), ("bias", None, -1, b"segment table"), ("w2", None, -1, b"widths"), ("res.base", None, -1, b"segment regions"),
                    ("y2.base", None, -1, b"row lists"), ("y.base", 0x15000004, -1, b"misaligned"), ("res.base", 0x14000001, -1, b"misaligned"),
                    ("y2.base", 0x16000002, -1, b"misaligned"), ("bias", 0x13000004, -1, b"misaligned"), ("w2", 0x17000004, -1, b"misaligned"),
                    ("cout", 0, -1, b"types"), ("cout", 17, -1, b"types"), ("cout", -3, -1, b"types"), ("cout2", 0, -1, b"widths outside"), ("cout2", 17, -1, b"widths outside"),
                    ("cout2", -1, -1, b"widths outside"), ("_rsv", 0, -1, b"regions"), ("_rsv", -1, -1, b"regions"), ("_rsv", 4097, -4, b"regions"),
                    ("res.h", 0, -1, b"segments"), ("res.h", -7, -1, b"segments"), ("res.h", (1 << 22) + 1, -4, b"2^22"), ("y2.sn", -1, -1, b"entries"),
                    ("y2.sn", 8 * 700 + 30 + 1, -4, b"8 S + kh"), ("y2.sn", 1 << 40, -4, b"8 S + kh"), ("y.sn", 16 * 1000 + 8 * 12 * 3 * 5 - 1, -4, b"output of"),
                    ("y.sn", 0, -4, b"output of")]
SHARED_REFUSALS = [("w", None, -1, b"null"), ("x2.base", None, -1, b"null"), ("w", 0x11000004, -1, b"misaligned"), ("x2.base", 0x12000004, -1, b"misaligned"),
                   ("x.h", 0, -1, b"N = 0"), ("x.h", -5, -1, b"N ="), ("kh", 0, -1, b"grid"), ("kw", -1, -1, b"grid"), ("x.h", (1 << 26) + 1, -4, b"2^26"),
                   ("kh", 4097, -4, b"grid"), ("kw", 4097, -4, b"grid"), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4, b"workspace"), ("x2.sn", 0, -4, b"workspace")]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_op_kind_21_is_in_the_header_the_plan_and_the_sources():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    header = open(L.HEADER).read()
    assert PL.OP_NBR_MARGINS == 21 and "HVN_OP_NBR_MARGINS = 21" in header and " NBR_MARGINS " in header and "hvn_margins.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                      # no new export: the op goes through hvn_run_op
    kernels = open(L.CSRC + "/hvn_kernels.h").read()
    assert "struct NbrMarginsArgs" in kernels and "HVN_NBR_MARGINS_MAX_B 16" in kernels and "HVN_NBR_MARGINS_MAX_G 4096" in kernels and "HVN_NBR_MARGINS_MAX_S (1 << 22)" in kernels


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_MARGINS list: its status and a text of its own that leads with the op's name, decided before
    any launch (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as
    tests/test_regions_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code, word):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_margins:") and word in err and b"unknown op kind" not in err, (rc, err, word)

    for path, value, code, word in MARGINS_REFUSALS + SHARED_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 1, code, word)
    refused(_op(), 2, -1, b"batch")                                  # batch must be 1
    op = _op()
    op._rsv, op.cout, op.cout2, op.res.h, op.y2.sn, op.y.sn = 4096, 16, 16, 1 << 22, 8 * (1 << 22) + 30, 1 << 40   # the caps pass the op's own checks:
    op.x.h = 0                                                                                                      # the next refusal is the shared one
    refused(op, 1, -1, b"N = 0")
    op = _op()
    op.y2.sn, op.x.h = 0, 0                                          # empty row lists are no refusal
    refused(op, 1, -1, b"N = 0")
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1, b"null")                                    # an all-zero op is refused by name


def test_c_refusals_leave_the_output_untouched_on_the_host_side():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    buf = np.full(4 * 1000 + 2 * 12 * 3 * 5, 0x5A5A5A5A, np.int32)
    for path, value in (("cout", 0), ("cout2", 0), ("_rsv", 5000), ("res.h", 0), ("y2.sn", -1), ("x.h", 0), ("x2.sn", 8), ("kh", 5000), ("bias", None), ("y.sn", 100)):
        op = _op()
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()


# -- 4: the "margin" key of the regions spec ---------------------------------------------------------------------
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
# by hand, widths 2 / 5: nucleus 1 is 4.5 inside roi; 4 is 1.5 inside both (the tie goes to roi); 9 is 2.5 outside roi and 5 inside core
STUB_MARGIN = [{"region": "roi", "distance": -4.5}, {"region": "roi", "distance": -1.5}, {"region": "roi", "distance": 2.5}]
STUB_COUNT = [[[[0], [1]], [[1], [2]]], [[[0], [0]], [[1], [2]]]]
MARGIN_FILES = ["area", "count", "first", "hits", "margin_count", "margin_d2", "margin_inside", "margin_near", "margin_widths", "names"]


def test_resolve_with_and_without_margin():
    rs = RG.RegionSet.from_geojson(STUB_GEOJSON)
    assert RG.resolve({"regions": rs}) is rs and isinstance(RG.resolve({"regions": STUB_GEOJSON, "scale": 2.0}), RG.RegionSet)
    spec = RG.resolve({"regions": rs, "margin": [2, 5.0]})
    assert isinstance(spec, RG.RegionSpec) and spec.regions is rs and spec.widths == (2.0, 5.0) and spec._fields == ("regions", "widths")
    assert RG.resolve({"regions": STUB_GEOJSON, "scale": 0.5, "margin": (1.5,)}).regions.area.tolist() == [170.0, 40.0]
    for margin, exc in BAD_WIDTHS:
        with pytest.raises(exc):
            RG.resolve({"regions": rs, "margin": margin})
    with pytest.raises(ValueError):
        RG.resolve({"regions": rs, "margins": [1.0]})


def test_a_bad_margin_is_refused_before_the_regions_are_read(monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(RG, "as_regions", no_work)
    with pytest.raises(ValueError):
        RG.resolve({"regions": "/nowhere/at/all.geojson", "margin": [3.0, 2.0]})


def test_without_margin_everything_is_as_before(tmp_path):
    """The same spec with and without going through `resolve`: RegionCounts, only "region" on the entries, the same five arrays in a
    byte-identical file."""
    rs = RG.RegionSet.from_geojson(STUB_GEOJSON)
    spec = RG.resolve({"regions": STUB_GEOJSON})
    assert type(spec) is RG.RegionSet
    a, b = RG.of_info(_stub_info(True), spec, 3), RG.of_info(_stub_info(True), rs, 3)
    assert type(a) is RG.RegionCounts and a._fields == ("first", "hits", "count", "names", "area")
    assert a.first.tolist() == [0, 0, 1] and a.hits.tolist() == [1, 2, 1] and a.count.tolist() == [[0, 1, 1], [0, 1, 1]]
    R.assert_same(a, b[:3])
    info = _stub_info(True)
    keys = {lab: set(e) for lab, e in info.items()}
    RG.annotate(info, a)
    assert all(set(e) == keys[lab] | {"region"} for lab, e in info.items())
    RG.save(tmp_path / "a.npz", a)
    RG.save(tmp_path / "b.npz", b)
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    with np.load(tmp_path / "a.npz") as z:
        assert sorted(z.files) == ["area", "count", "first", "hits", "names"]


def test_of_info_annotate_and_save_with_margin(tmp_path):
    spec = RG.resolve({"regions": STUB_GEOJSON, "margin": [2.0, 5.0]})
    empty = RG.of_info({}, spec, 3)
    assert isinstance(empty, RG.RegionMargins) and empty.margins.near.shape == (0,) and empty.margins.count.shape == (2, 2, 2, 3) and not empty.margins.count.any()
    assert RG.annotate({}, empty) == {}
    info = _stub_info()
    res = RG.of_info(info, spec, None)
    assert isinstance(res, RG.RegionMargins) and res._fields == ("counts", "margins") and isinstance(res.counts, RG.RegionCounts) and isinstance(res.margins, MG.Margins)
    R.assert_same(res.counts, RG.of_info(_stub_info(), spec.regions, None)[:3])
    m = res.margins
    assert m.near.tolist() == [0, 0, 0] and m.near_d2.tolist() == [20.25, 2.25, 6.25] and m.near_inside.tolist() == [1, 1, 0] and m.count.tolist() == STUB_COUNT
    assert m.widths == (2.0, 5.0) and m.names == ["roi", "core"]
    want = M.margins(np.array([[5.5, 4.5], [12.0, 15.5], [15.0, 19.5]]), None, spec.regions.polygons, (2.0, 5.0), 1)
    M.assert_same(m, want, "stub")
    typed = RG.of_info(_stub_info(True), spec, 3).margins
    assert typed.count.shape == (2, 2, 2, 3) and (typed.count.sum(-1) == m.count[..., 0]).all() and typed.count[0, 1, :, 2].tolist() == [1, 1]
    keys = {lab: set(e) for lab, e in info.items()}
    assert RG.annotate(info, res) is info and [e["margin"] for e in info.values()] == STUB_MARGIN and [e["region"] for e in info.values()] == [0, 0, 1]
    assert all(set(e) == keys[lab] | {"region", "margin"} and type(e["margin"]["distance"]) is float for lab, e in info.items())
    none = RG.of_info(_stub_info(), RG.resolve({"regions": STUB_GEOJSON, "margin": [0.25]}), None)
    assert [e["margin"] for e in RG.annotate(_stub_info(), none).values()] == [{"region": None, "distance": None}] * 3
    with pytest.raises(ValueError):
        RG.annotate({1: {}}, res)
    RG.save(tmp_path / "m.npz", res)
    with np.load(tmp_path / "m.npz") as z:                           # no pickle
        assert sorted(z.files) == MARGIN_FILES
        assert z["margin_widths"].tolist() == [2.0, 5.0] and z["margin_count"].tolist() == STUB_COUNT and z["margin_count"].dtype == np.int32
        assert z["margin_near"].tolist() == [0, 0, 0] and z["margin_d2"].tolist() == [20.25, 2.25, 6.25] and z["margin_inside"].tolist() == [1, 1, 0]
        assert z["first"].tolist() == [0, 0, 1] and z["names"].tolist() == ["roi", "core"]


def test_points_summaries_pass_the_pair_on():
    from hover_net_amd import points as PT

    specs = PT.resolve_specs(regions={"regions": STUB_GEOJSON, "margin": [2.0, 5.0]})
    assert isinstance(specs.regions, RG.RegionSpec) and PT.output_dirs(specs) == ("regions",)
    info = _stub_info()
    res = PT.summaries(info, (40, 50), specs, None, None)
    assert isinstance(res.regions, RG.RegionMargins) and [e["margin"] for e in info.values()] == STUB_MARGIN


# -- the managers, with the GPU call replaced by a stub (the GPU runs are in tests/test_gpu_margins.py) -------------------------
def test_process_file_list_writes_the_margin(tmp_path):
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
    out = {}
    for key, regions in (("plain", {"dir": str(ann)}), ("margin", {"dir": str(ann), "margin": [2.0, 5.0]})):
        out[key] = tmp_path / key
        assert mgr.process_file_list({"input_dir": str(inp), "output_dir": str(out[key]), "regions": regions}) == ["a", "b"]
    assert (out["plain"] / "json" / "b.json").read_bytes() == (out["margin"] / "json" / "b.json").read_bytes() and not (out["margin"] / "regions" / "b.npz").exists()
    with np.load(out["plain"] / "regions" / "a.npz") as z:
        assert sorted(z.files) == ["area", "count", "first", "hits", "names"]
    with np.load(out["margin"] / "regions" / "a.npz") as z:
        assert sorted(z.files) == MARGIN_FILES and z["margin_count"].tolist() == STUB_COUNT and z["margin_d2"].tolist() == [20.25, 2.25, 6.25] and z["first"].tolist() == [0, 0, 1]
    plain, marg = (json.load(open(out[k] / "json" / "a.json"))["nuc"] for k in ("plain", "margin"))
    assert [marg[k]["margin"] for k in ("1", "4", "9")] == STUB_MARGIN and not any("margin" in e for e in plain.values())
    assert {k: {f: v for f, v in e.items() if f != "margin"} for k, e in marg.items()} == plain
    for bad, exc in (({"dir": str(ann), "margin": [5.0, 2.0]}, ValueError), ({"dir": str(ann), "margin": []}, ValueError), ({"dir": str(ann), "margin": 3.0}, TypeError),
                     ({"dir": str(ann), "margin": ["2"]}, TypeError), ({"dir": str(ann), "margins": [2.0]}, ValueError)):
        with pytest.raises(exc):
            mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "regions": bad})
    assert not (tmp_path / "bad").exists()                           # refused before any file is touched


def test_process_wsi_list_writes_the_margin(tmp_path):
    from hover_net_amd import infer_manager as im

    inp, ann = tmp_path / "slides", tmp_path / "ann"
    inp.mkdir()
    ann.mkdir()
    np.save(inp / "s.npy", np.random.default_rng(1).integers(30, 120, (64, 96, 3), dtype=np.uint8))
    (ann / "s.geojson").write_text(json.dumps(STUB_GEOJSON))
    mgr = im.WsiManager({"model_args": {"nr_types": None, "mode": "fast"}, "model_path": None}, wsi_fn=lambda slide, mask: (None, _stub_info()))
    out = {}
    for key, regions in (("plain", {"dir": str(ann)}), ("margin", {"dir": str(ann), "margin": [2.0, 5.0]})):
        out[key] = tmp_path / key
        assert mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(out[key]), "regions": regions}) == {"s": "done"}
    with np.load(out["plain"] / "regions" / "s.npz") as z:
        assert sorted(z.files) == ["area", "count", "first", "hits", "names"]
    with np.load(out["margin"] / "regions" / "s.npz") as z:
        assert sorted(z.files) == MARGIN_FILES and z["margin_count"].tolist() == STUB_COUNT and z["margin_near"].tolist() == [0, 0, 0]
    plain, marg = (json.loads((out[k] / "s.json").read_text())["nuc"] for k in ("plain", "margin"))
    assert [e["margin"] for e in marg.values()] == STUB_MARGIN and [e["region"] for e in marg.values()] == [0, 0, 1]
    assert {k: {f: v for f, v in e.items() if f != "margin"} for k, e in marg.items()} == plain
    with pytest.raises(ValueError):
        mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "regions": {"dir": str(ann), "margin": [1.0, 1.0]}})
    assert not (tmp_path / "bad").exists()

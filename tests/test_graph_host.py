"""The cell graph on the CPU (hover_net_amd/graph.py): `gabriel_host` against the all-k oracle tests/graph_ref.py with ==, the oracle itself
against scipy's Delaunay triangulation, the helpers, the "graph" key of the `neighbours` argument through `resolve`, `annotate` and both
managers (the GPU call replaced by a stub), and every refusal that include/hvn.h lists for HVN_OP_NBR_GRAPH."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import graph_ref as G
from hover_net_amd import graph as GR
from hover_net_amd import neighbours as NB
from hover_net_amd import points as P


# -- 1: host == oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES + ("collinear", "dense1100"))
def test_host_equals_oracle(name):
    """`dense1100` is one cell with 1099 neighbours per point (its oracle takes a quarter of a minute); `collinear` keeps the 49 links
    of a chain out of 50 points that all see four others each way."""
    (xy, r), want = G.case(name)
    G.assert_case_facts(name, want)
    got = GR.gabriel_host(xy, r)
    assert isinstance(got, GR.CellGraph) and got._fields == ("indptr", "indices")
    G.assert_same(got, want, name)
    G.assert_case_facts(name, got)
    G.assert_same(GR.gabriel(xy, r), want, name)


def test_the_rounds_change_nothing(monkeypatch):
    """Tiny rounds of pairs and of triples: many rounds per case, single-pair chunks included."""
    (xy, r), want = G.case("untyped")
    monkeypatch.setattr(GR, "_PAIRS", 50)
    monkeypatch.setattr(GR, "_TRIPLES", 9)
    monkeypatch.setattr(GR, "_FIRST", 1)
    G.assert_same(GR.gabriel_host(xy, r), want, "tiny rounds")


def test_the_oracle_gives_a_subgraph_of_the_delaunay_triangulation():
    """An independent check of the oracle: with a radius that covers everything, the Gabriel graph of points in general position is a
    subgraph of their Delaunay triangulation.  General position is a fact of this seed."""
    from scipy.spatial import Delaunay

    xy = np.random.default_rng(7).uniform(0, 200, (400, 2))
    g = GR.CellGraph(*G.gabriel(xy, 1000.0))
    mine = {tuple(e) for e in GR.edge_list(g).tolist()}
    tri = Delaunay(xy).simplices
    dt = {tuple(sorted((int(t[a]), int(t[b])))) for t in tri for a, b in ((0, 1), (1, 2), (0, 2))}
    assert len(mine) == 747 and len(dt) == 1181 and mine <= dt
    G.assert_same(GR.gabriel_host(xy, 1000.0), g, "one cell of 400")


def test_coincident_piles_are_joined_to_everybody():
    """Piles of 200 and 100 coincident points, 3 apart, r = 5: nobody blocks (every dot is 0 or 9), every row holds all 299 others, the
    own pile first (d2 = 0), each by j."""
    xy, r = G._piles(200, 100)
    got = GR.gabriel_host(xy, r)
    assert int(got.indptr[-1]) == 300 * 299 and (GR.degree(got) == 299).all()
    G.assert_same(got, G.piles_graph(200, 100), "piles")
    assert got.indices[:3].tolist() == [1, 2, 3] and got.indices[199:202].tolist() == [200, 201, 202]


def test_the_open_disc():
    """A point on the circle does not block; one strictly inside does; both diagonals of a square survive."""
    sq = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]])
    assert GR.edge_list(GR.gabriel_host(sq, 10.0)).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    on = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 1.0]])                      # (1, 1) lies ON the circle over (0, 0) - (2, 0)
    assert GR.edge_list(GR.gabriel_host(on, 10.0)).tolist() == [[0, 1], [0, 2], [1, 2]]
    inside = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 0.5]])
    assert GR.edge_list(GR.gabriel_host(inside, 10.0)).tolist() == [[0, 2], [1, 2]]
    assert GR.edge_list(GR.gabriel_host(inside, 1.5)).tolist() == [[0, 2], [1, 2]]          # 0 - 1 is longer than r: no edge, blocker or not
    for xy in (sq, on, inside):
        G.assert_same(GR.gabriel_host(xy, 10.0), G.gabriel(xy, 10.0))


# -- 2: the helpers, on a graph made by hand ---------------------------------------------------------------------
HAND_XY = np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 4.0], [10.0, 10.0]])
HAND = GR.CellGraph(np.array([0, 2, 4, 6, 6], np.int64), np.array([1, 2, 0, 2, 1, 0], np.int32))         # a triangle and an isolated point


def test_helpers_on_a_hand_made_graph(tmp_path):
    assert GR.degree(HAND).tolist() == [2, 2, 2, 0] and GR.degree(HAND).dtype == np.int32
    el = GR.edge_list(HAND)
    assert el.tolist() == [[0, 1], [0, 2], [1, 2]] and el.dtype == np.int32
    ei = GR.edge_index(HAND)
    assert ei.dtype == np.int64 and ei.tolist() == [[0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 1, 0]]
    assert GR.lengths(HAND_XY, HAND).tolist() == [3.0, 5.0, 3.0, 4.0, 4.0, 5.0]
    te = GR.type_edges(HAND, np.array([0, 1, 1, 2], np.int32), 3)
    assert te.dtype == np.int64 and te.tolist() == [[0, 2, 0], [2, 2, 0], [0, 0, 0]] and (te == te.T).all()
    assert GR.type_edges(HAND, np.array([0, 1, 1, 0], np.int32), None).shape == (2, 2)
    with pytest.raises(ValueError):
        GR.type_edges(HAND, np.array([0, 1, 1], np.int32), 3)
    with pytest.raises(TypeError):
        GR.type_edges(HAND, None, 3)
    empty = GR.CellGraph(np.zeros(3, np.int64), np.zeros(0, np.int32))
    assert GR.edge_list(empty).shape == (0, 2) and GR.edge_index(empty).shape == (2, 0) and GR.lengths(HAND_XY[:2], empty).shape == (0,)
    GR.save(tmp_path / "g.npz", [7, 9, 11, 40], HAND)
    with np.load(tmp_path / "g.npz") as z:                           # no pickle
        assert sorted(z.files) == ["indices", "indptr", "labels"] and z["indptr"].dtype == np.int64 and z["indices"].dtype == np.int32
    labels, g = GR.load(tmp_path / "g.npz")
    assert labels == [7, 9, 11, 40] and isinstance(g, GR.CellGraph)
    G.assert_same(g, HAND)
    # the hand-made graph is what the definition gives for its points at r = 6
    G.assert_same(GR.gabriel_host(HAND_XY, 6.0), GR.CellGraph(HAND.indptr, np.array([1, 2, 0, 2, 1, 0], np.int32)))


def test_python_refusals():
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    with pytest.raises(ValueError):
        GR.gabriel_host(np.array([[0.0, np.nan], [1.0, 1.0]]), 1.0)
    with pytest.raises(TypeError):
        GR.gabriel_host(xy.astype(np.float32), 1.0)
    with pytest.raises(ValueError):
        GR.gabriel_host(xy, 0.0)
    with pytest.raises(TypeError):
        GR.gabriel_host(xy, "3")
    with pytest.raises(ValueError):
        GR.gabriel(xy, 1.0, device="cpu")                            # a device that is no GPU


def test_e_at_two_to_the_31_is_refused(monkeypatch):
    monkeypatch.setattr(GR, "MAX_E", 5)
    with pytest.raises(ValueError, match="reach 2\\^31"):
        GR.gabriel_host(HAND_XY, 6.0)                                # six directed edges


# -- 3: the "graph" key of the neighbours argument -----------------------------------------------------------------
def _stub(typed=True):
    """40 nuclei of 3 types on a 64 x 96 image, as `post_proc.process` shapes its entries; labels not contiguous."""
    rng = np.random.default_rng(11)
    info = {}
    for i in range(40):
        x, y = int(rng.integers(3, 92)), int(rng.integers(3, 60))
        box = np.array([[x - 2, y - 2], [x + 2, y - 2], [x + 2, y + 2], [x - 2, y + 2]], np.int32)
        t = int(rng.integers(0, 3))
        info[3 * i + 1] = {"bbox": np.array([[y - 2, x - 2], [y + 3, x + 3]]), "centroid": np.array([x + 0.25 * (i % 3), y + 0.5]), "contour": box,
                           "type_prob": 0.5 + 0.01 * i if typed else None, "type": t if typed else None}
    return info


def test_resolve():
    assert NB.resolve(None) is None and NB.resolve({"radius": 14, "k": 3}) == (14.0, 3)
    assert NB.resolve({"radius": 14.0, "k": 3, "graph": "gabriel"}) == (14.0, 3, "gabriel")
    for bad in ("delaunay", True, None, "Gabriel", 1, ["gabriel"]):
        with pytest.raises(ValueError):
            NB.resolve({"radius": 14.0, "k": 3, "graph": bad})
    with pytest.raises(ValueError):
        NB.resolve({"radius": 14.0, "graph": "gabriel"})
    with pytest.raises(ValueError):
        NB.resolve({"radius": 14.0, "k": 3, "graphs": "gabriel"})
    with pytest.raises(ValueError):
        NB.resolve({"radius": 0.0, "k": 3, "graph": "gabriel"})
    assert P.ARGS == ("neighbours", "clusters", "density", "ripley", "regions")
    assert P.resolve_specs(neighbours={"radius": 14.0, "k": 3, "graph": "gabriel"}).neighbours == (14.0, 3, "gabriel")
    assert P.resolve_specs(neighbours={"radius": 14.0, "k": 3}).neighbours == (14.0, 3)


def test_a_bad_graph_is_refused_before_any_work(monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(NB, "query", no_work)
    monkeypatch.setattr(GR, "gabriel", no_work)
    with pytest.raises(ValueError):
        NB.annotate(_stub(), 14.0, 3, 3, graph="delaunay")
    with pytest.raises(ValueError):
        NB.annotate({}, 14.0, 3, 3, graph=True)


def test_annotate_adds_exactly_the_two_keys():
    info = _stub()
    plain = NB.annotate(copy.deepcopy(info), 14.0, 3, 3)
    same = NB.annotate(copy.deepcopy(info), 14.0, 3, 3, graph=None)
    got = NB.annotate(copy.deepcopy(info), 14.0, 3, 3, graph="gabriel")
    labels, g = GR.of_info(info, 14.0)
    assert labels == list(info) and int(g.indptr[-1]) > 40
    _, xy, _ = P.from_info(info, None)
    dist = GR.lengths(xy, g)
    for i, lab in enumerate(labels):
        assert list(same[lab]) == list(plain[lab]) and same[lab]["neighbours"] == plain[lab]["neighbours"]
        nb = got[lab]["neighbours"]
        assert list(nb) == list(plain[lab]["neighbours"]) + ["graph", "graph_dist"]
        assert {k: nb[k] for k in plain[lab]["neighbours"]} == plain[lab]["neighbours"]
        row = slice(int(g.indptr[i]), int(g.indptr[i + 1]))
        assert nb["graph"] == [labels[j] for j in g.indices[row]] and nb["graph_dist"] == dist[row].tolist()
        assert all(type(v) is int for v in nb["graph"]) and all(type(v) is float for v in nb["graph_dist"])
        assert nb["graph_dist"] == sorted(nb["graph_dist"]) and all(d <= 14.0 for d in nb["graph_dist"])
        assert all(lab in got[other]["neighbours"]["graph"] for other in nb["graph"])            # symmetric
        if nb["knn"]:
            assert nb["graph"][0] == nb["knn"][0] and nb["graph_dist"][0] == nb["knn_dist"][0]
        assert json.loads(json.dumps(nb)) == nb
    untyped = NB.annotate(_stub(False), 14.0, 3, None, graph="gabriel")
    assert [e["neighbours"]["graph"] for e in untyped.values()] == [e["neighbours"]["graph"] for e in got.values()]
    assert NB.annotate({}, 14.0, 3, 3, graph="gabriel") == {}
    assert GR.of_info({}, 14.0)[0] == [] and GR.of_info({}, 14.0)[1].indptr.tolist() == [0]
    # points.annotate passes the key on
    specs = P.resolve_specs(neighbours={"radius": 14.0, "k": 3, "graph": "gabriel"})
    via = P.annotate(copy.deepcopy(info), specs, 3, None)
    assert all(via[lab]["neighbours"] == got[lab]["neighbours"] for lab in info)
    off = P.annotate(copy.deepcopy(info), P.resolve_specs(neighbours={"radius": 14.0, "k": 3}), 3, None)
    assert all(off[lab]["neighbours"] == plain[lab]["neighbours"] for lab in info)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs + [""])


@pytest.mark.parametrize("which", ["tile", "wsi"])
def test_managers_write_the_graph(which, tmp_path):
    """Both managers with the GPU call replaced by a stub that annotates as `process_images` / `WsiInference` do: the json gains the
    two keys and nothing else on disk changes."""
    from hover_net_amd import infer_manager as im

    inp = tmp_path / "in"
    inp.mkdir()
    np.save(inp / "a.npy", np.random.default_rng(1).integers(30, 120, (64, 96, 3), dtype=np.uint8))
    spec = [None]

    def stub():
        return P.annotate(_stub(), P.resolve_specs(neighbours=spec[0]), 3, None)

    method = {"model_args": {"nr_types": 3, "mode": "fast"}, "model_path": None}
    if which == "tile":
        mgr = im.InferManager(method, process_fn=lambda images: [(np.zeros(i.shape[:2], np.int32), stub()) for i in images])
        run, done, json_at = mgr.process_file_list, ["a"], "json/a.json"
    else:
        mgr = im.WsiManager(method, wsi_fn=lambda slide, mask: (None, stub()))
        run, done, json_at = mgr.process_wsi_list, {"a": "done"}, "a.json"
    runs = {"plain": {"radius": 14.0, "k": 3}, "graph": {"radius": 14.0, "k": 3, "graph": "gabriel"}}
    for key, nb in runs.items():
        spec[0] = nb
        assert run({"input_dir": str(inp), "output_dir": str(tmp_path / key), "neighbours": dict(nb)}) == done
    assert _tree(tmp_path / "plain") == _tree(tmp_path / "graph")
    for rel in _tree(tmp_path / "plain"):
        if rel != json_at and os.path.isfile(tmp_path / "plain" / rel):
            assert (tmp_path / "plain" / rel).read_bytes() == (tmp_path / "graph" / rel).read_bytes(), rel
    doc = json.loads((tmp_path / "graph" / json_at).read_text())
    want = NB.annotate(_stub(), 14.0, 3, 3, graph="gabriel")
    assert len(doc["nuc"]) == 40 and sum(len(e["neighbours"]["graph"]) for e in doc["nuc"].values()) > 40
    for k, e in doc["nuc"].items():
        assert e["neighbours"]["graph"] == want[int(k)]["neighbours"]["graph"] and e["neighbours"]["graph_dist"] == want[int(k)]["neighbours"]["graph_dist"]
        del e["neighbours"]["graph"], e["neighbours"]["graph_dist"]
    assert json.dumps(doc) == (tmp_path / "plain" / json_at).read_text()         # without the key the json is today's, byte for byte
    for bad in ("delaunay", True, None):
        with pytest.raises(ValueError):
            run({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "neighbours": {"radius": 14.0, "k": 3, "graph": bad}})
        assert not (tmp_path / "bad").exists()                           # refused before any file is touched


# -- 4: the C side's refusals --------------------------------------------------------------------------------------
def _op(fill):
    """A well-formed GRAPH op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    at = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.x.h = PL.OP_NBR_GRAPH, ncy, ncx, n
    op.w, op.x2.base, op.x2.sn = at(1), at(2), NB.workspace_bytes(n, ncy * ncx)
    if fill:
        op._rsv, op.y.base, op.y.sn, op.y2.base = 1, at(5), 4000, at(6)
    else:
        op._rsv, op.y.base, op.y2.base, op.stride = 0, at(5), at(6), 16
    return op


# one entry per refusal that include/hvn.h lists for NBR_GRAPH: (fill, field, value, status, a word of its text)
GRAPH_REFUSALS = [(0, "_rsv", 2, -1, b"no mode"), (0, "_rsv", -1, -1, b"no mode"), (0, "y.base", None, -1, b"null degree"), (1, "y.base", None, -1, b"null indices"),
                  (1, "y2.base", None, -1, b"null indptr"), (1, "y.sn", 0, -1, b"fewer than one"), (1, "y.sn", -4, -1, b"fewer than one"),
                  (1, "y.sn", 1 << 31, -4, b"reach 2^31"), (1, "y.sn", 1 << 40, -4, b"reach 2^31"), (0, "stride", 0, -1, b"slots per point"),
                  (0, "stride", 65, -1, b"slots per point"), (0, "stride", -2, -1, b"slots per point"), (0, "y.base", 0x15000002, -1, b"misaligned degree or indices"),
                  (1, "y.base", 0x15000001, -1, b"misaligned degree or indices"), (1, "y2.base", 0x16000004, -1, b"misaligned indptr"),
                  (0, "y2.base", 0x16000002, -1, b"misaligned table")]
SHARED_REFUSALS = [("w", None, -1, b"null"), ("x2.base", None, -1, b"null"), ("w", 0x11000004, -1, b"misaligned"), ("x2.base", 0x12000004, -1, b"misaligned"),
                   ("x.h", 0, -1, b"N = 0"), ("x.h", -5, -1, b"N ="), ("kh", 0, -1, b"grid"), ("kw", -1, -1, b"grid"), ("x.h", (1 << 26) + 1, -4, b"2^26"),
                   ("kh", 4097, -4, b"grid"), ("kw", 4097, -4, b"grid"), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4, b"workspace"), ("x2.sn", 0, -4, b"workspace")]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_op_kind_22_is_in_the_header_the_plan_and_the_sources():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    header = open(L.HEADER).read()
    assert PL.OP_NBR_GRAPH == 22 and "HVN_OP_NBR_GRAPH = 22" in header and " NBR_GRAPH " in header and "hvn_graph.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                      # no new export: the op goes through hvn_run_op
    kernels = open(L.CSRC + "/hvn_kernels.h").read()
    assert "struct NbrGraphArgs" in kernels and "HVN_NBR_GRAPH_LIST_CAP %d " % GR.LIST_CAP in kernels
    assert GR.MAX_E == (1 << 31) - 1 and 1 <= GR.TABLE_WIDTH <= 64


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_GRAPH list: its status and a text of its own that leads with the op's name, decided before
    any launch (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as
    tests/test_margins_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code, word):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_graph:") and word in err and b"unknown op kind" not in err, (rc, err, word)

    for fill, path, value, code, word in GRAPH_REFUSALS + [(f,) + r for f in (0, 1) for r in SHARED_REFUSALS]:
        op = _op(fill)
        _set(op, path, value)
        refused(op, 1, code, word)
    texts = set()
    for fill, path, value, _code, _word in GRAPH_REFUSALS:
        op = _op(fill)
        _set(op, path, value)
        l.hvn_run_op(ctypes.byref(op), 1, None)
        texts.add((path, fill, l.hvn_last_error().split(b" of ")[0][:40]))
    assert len({t[2] for t in texts}) >= 9                           # each kind of refusal has a text of its own
    for fill in (0, 1):
        refused(_op(fill), 2, -1, b"batch")                          # batch must be 1
    op = _op(1)
    op.y.sn, op.x.h = (1 << 31) - 1, 0                               # the largest E passes the op's own checks: the next refusal is the shared one
    refused(op, 1, -1, b"N = 0")
    op = _op(0)
    op.y2.base, op.stride, op.x.h = None, 99, 0                      # no table: `stride` is not read
    refused(op, 1, -1, b"N = 0")
    op = _op(0)
    op.stride, op.x.h = 64, 0                                        # the widest table
    refused(op, 1, -1, b"N = 0")
    zero = L.hvn_op()
    zero.kind = _op(0).kind
    refused(zero, 1, -1, b"null")                                    # an all-zero op is refused by name


def test_c_refusals_leave_the_output_untouched_on_the_host_side():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    buf = np.full(4000, 0x5A5A5A5A, np.int32)
    for fill, path, value in ((0, "_rsv", 3), (1, "y.sn", 0), (1, "y2.base", None), (0, "stride", 0), (0, "x.h", 0), (1, "x2.sn", 8), (1, "kh", 5000)):
        op = _op(fill)
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()

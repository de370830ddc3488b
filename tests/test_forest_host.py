"""The spanning forest and the components of the cell graph on the CPU (hover_net_amd/forest.py): `forest_host` against the scalar Kruskal
of tests/forest_ref.py with ==, the forest's own properties checked directly, scipy's minimum spanning tree on the tie-free cases, the
readers, the "forest" key of the `neighbours` argument through `resolve`, `annotate` and both managers (the GPU call replaced by a
stub), and every refusal that include/hvn.h lists for HVN_OP_NBR_FOREST."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import forest_ref as F
from hover_net_amd import forest as FO
from hover_net_amd import graph as GR
from hover_net_amd import neighbours as NB
from hover_net_amd import points as P


def _stub():
    """40 nuclei of 3 types on a 64 x 96 image, as `post_proc.process` shapes its entries; labels not contiguous."""
    rng = np.random.default_rng(11)
    info = {}
    for i in range(40):
        x, y = int(rng.integers(3, 92)), int(rng.integers(3, 60))
        box = np.array([[x - 2, y - 2], [x + 2, y - 2], [x + 2, y + 2], [x - 2, y + 2]], np.int32)
        info[3 * i + 1] = {"bbox": np.array([[y - 2, x - 2], [y + 3, x + 3]]), "centroid": np.array([x + 0.25 * (i % 3), y + 0.5]), "contour": box,
                           "type_prob": 0.5 + 0.01 * i, "type": int(rng.integers(0, 3))}
    return info


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs + [""])


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


# -- 1: host == oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.NAMES)
def test_host_equals_oracle(name):
    (xy, g), want = F.case(name)
    F.assert_case_facts(name, xy, g, want)
    got = FO.forest_host(xy, g)
    assert isinstance(got, FO.Forest) and got._fields == ("component", "edges")
    F.assert_same(got, want, name)
    F.assert_case_facts(name, xy, g, got)
    F.assert_same(FO.forest(xy, g), want, name)


def _find(parent, a):
    while parent[a] != a:
        a = parent[a]
    return a


@pytest.mark.parametrize("name", F.NAMES)
def test_the_forest_is_an_acyclic_part_of_the_graph_that_spans_it(name):
    (xy, g), _ = F.case(name)
    f = FO.forest_host(xy, g)
    n = xy.shape[0]
    assert f.edges.shape[0] == n - FO.n_components(f)
    assert {tuple(e) for e in f.edges.tolist()} <= {tuple(e) for e in GR.edge_list(g).tolist()}
    parent = list(range(n))
    for i, j in f.edges.tolist():                                 # acyclic: every edge joins two trees
        a, b = _find(parent, i), _find(parent, j)
        assert a != b, (name, i, j)
        parent[max(a, b)] = min(a, b)
    assert [_find(parent, i) for i in range(n)] == f.component.tolist()      # and the trees are the graph's components, named by their
    i, j = GR.edge_index(g)                                                  # smallest position
    assert (f.component[i] == f.component[j]).all()


def test_every_other_edge_is_closed_by_smaller_forest_edges():
    """The cycle property, directly: the ends of an edge outside the forest are connected by forest edges of strictly smaller key."""
    (xy, g), _ = F.case("random")
    f = FO.forest_host(xy, g)
    n = xy.shape[0]
    key = lambda e: (float(P.d2_of(xy[e[0], 0], xy[e[0], 1], xy[e[1], 0], xy[e[1], 1])), e[0], e[1])  # noqa: E731
    mine = {tuple(e) for e in f.edges.tolist()}
    events = sorted([(key(e), 0, e) for e in mine] + [(key(tuple(e)), 1, tuple(e)) for e in GR.edge_list(g).tolist() if tuple(e) not in mine])
    parent, closed = list(range(n)), 0
    for _key, other, (i, j) in events:                            # ascending key: a forest edge unites, another edge must find its ends united
        a, b = _find(parent, i), _find(parent, j)
        if other:
            assert a == b, (i, j)
            closed += 1
        else:
            parent[max(a, b)] = min(a, b)
    assert closed == 3919 - 1999


@pytest.mark.parametrize("name", ["random", "untyped", "dense1100"])
def test_scipy_gives_the_same_tree_where_no_d2_ties_or_vanishes(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import minimum_spanning_tree

    (xy, g), want = F.case(name)
    assert F.tied_d2(xy, g) == 0
    i, j = GR.edge_index(g)
    d2 = P.d2_of(xy[i, 0], xy[i, 1], xy[j, 0], xy[j, 1])
    assert (d2 > 0).all()
    n = xy.shape[0]
    t = minimum_spanning_tree(sp.csr_matrix((d2, (i, j)), shape=(n, n))).tocoo()
    theirs = sorted((int(min(a, b)), int(max(a, b))) for a, b in zip(t.row, t.col))
    assert theirs == [tuple(e) for e in want[1].tolist()]


# -- 2: check_graph ----------------------------------------------------------------------------------------------
HAND_XY = np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 4.0], [10.0, 10.0], [10.0, 12.0]])
HAND = GR.CellGraph(np.array([0, 2, 4, 6, 7, 8], np.int64), np.array([1, 2, 0, 2, 1, 0, 4, 3], np.int32))     # a triangle and a pair
HAND_FOREST = FO.Forest(np.array([0, 0, 0, 3, 3], np.int32), np.array([[0, 1], [1, 2], [3, 4]], np.int32))


def test_check_graph_refuses_what_the_definition_does_not_admit():
    ptr, idx = FO.check_graph(HAND, 5)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32
    i64, i32 = lambda *v: np.array(v, np.int64), lambda *v: np.array(v, np.int32)  # noqa: E731
    bad = {"asymmetric": (i64(0, 1, 1, 1), i32(1)), "self-loop": (i64(0, 1, 1), i32(0)), "twice": (i64(0, 2, 4), i32(1, 1, 0, 0)),
           "out of range": (i64(0, 1, 2), i32(1, 2)), "negative": (i64(0, 1, 2), i32(1, -1)), "indptr dtype": (np.array([0, 1, 2], np.int32), i32(1, 0)),
           "indices dtype": (i64(0, 1, 2), np.array([1, 0], np.int64)), "indptr shape": (i64(0, 1, 2, 2), i32(1, 0)), "indices shape": (i64(0, 1, 2), i32(1, 0).reshape(1, 2)),
           "indptr end": (i64(0, 1, 1), i32(1, 0)), "indptr start": (i64(1, 1, 2), i32(1, 0)), "indptr falls": (i64(0, 2, 1, 2), i32(1, 0)),
           "a list": ([0, 1, 2], [1, 0])}
    for what, (indptr, indices) in bad.items():
        n = 3 if what in ("asymmetric", "indptr falls") else 2
        with pytest.raises(ValueError):
            FO.check_graph(GR.CellGraph(indptr, indices), n)
        with pytest.raises(ValueError):
            FO.forest_host(np.zeros((n, 2)) + np.arange(n)[:, None], GR.CellGraph(indptr, indices))
    with pytest.raises(ValueError):
        FO.check_graph(HAND, 6)
    with pytest.raises(ValueError):
        FO.forest(HAND_XY, HAND, device="cpu")                    # a device that is no GPU
    with pytest.raises(TypeError):
        FO.forest_host(HAND_XY.astype(np.float32), HAND)
    with pytest.raises(ValueError):
        FO.DeviceForest(HAND_XY, HAND, graph=object())


# -- 3: the readers, on a forest made by hand --------------------------------------------------------------------
def test_readers_on_a_hand_made_forest(tmp_path):
    F.assert_same(FO.forest_host(HAND_XY, HAND), HAND_FOREST)     # 0 - 2 (length 5) closes the triangle and stays out
    f = HAND_FOREST
    assert FO.n_components(f) == 2
    names, sizes = FO.component_sizes(f)
    assert names.tolist() == [0, 3] and sizes.tolist() == [3, 2] and sizes.dtype == np.int64 and names.dtype == np.int32
    deg = FO.tree_degree(5, f)
    assert deg.tolist() == [1, 2, 1, 1, 1] and deg.dtype == np.int32
    t = FO.tree_csr(HAND_XY, 5, f)
    assert isinstance(t, GR.CellGraph) and t.indptr.tolist() == [0, 1, 3, 4, 5, 6] and t.indices.tolist() == [1, 0, 2, 1, 4, 3]
    assert t.indptr.dtype == np.int64 and t.indices.dtype == np.int32
    FO.check_graph(t, 5)
    assert GR.edge_index(t).tolist() == [[0, 1, 1, 2, 3, 4], [1, 0, 2, 1, 4, 3]]
    assert GR.type_edges(t, np.array([0, 1, 1, 2, 2], np.int32), 3).tolist() == [[0, 1, 0], [1, 2, 0], [0, 0, 2]]
    assert FO.lengths(HAND_XY, f).tolist() == [3.0, 4.0, 2.0]
    s = FO.summary(HAND_XY, f)
    length = np.array([3.0, 4.0, 2.0])
    mean, std = length.sum() / 3.0, np.sqrt(((length - length.sum() / 3.0) ** 2).sum() / 3.0)
    assert s == {"edges": 3, "components": 2, "mean": mean, "std": std, "min": 2.0, "max": 4.0, "min_max_ratio": 0.5, "disorder": std / (mean + std)}
    assert mean == 3.0 and abs(std - np.sqrt(2.0 / 3.0)) < 1e-15 and json.loads(json.dumps(s)) == s
    none = FO.Forest(np.arange(3, dtype=np.int32), np.zeros((0, 2), np.int32))
    assert FO.summary(HAND_XY[:3], none) == {"edges": 0, "components": 3, "mean": None, "std": None, "min": None, "max": None, "min_max_ratio": None, "disorder": None}
    assert FO.lengths(HAND_XY[:3], none).shape == (0,) and not FO.tree_degree(3, none).any() and FO.tree_csr(HAND_XY[:3], 3, none).indptr.tolist() == [0, 0, 0, 0]
    pile = FO.Forest(np.zeros(2, np.int32), np.array([[0, 1]], np.int32))            # two coincident points: every length is 0
    s = FO.summary(np.zeros((2, 2)), pile)
    assert (s["mean"], s["std"], s["min"], s["max"], s["min_max_ratio"], s["disorder"]) == (0.0, 0.0, 0.0, 0.0, None, None)
    FO.save(tmp_path / "f.npz", [7, 9, 11, 40, 41], f)
    with np.load(tmp_path / "f.npz") as z:                        # no pickle
        assert sorted(z.files) == ["component", "edges", "labels"] and z["component"].dtype == np.int32 and z["edges"].dtype == np.int32
    labels, back = FO.load(tmp_path / "f.npz")
    assert labels == [7, 9, 11, 40, 41] and isinstance(back, FO.Forest)
    F.assert_same(back, f)
    FO.save(tmp_path / "e.npz", [1, 2, 3], none)
    assert FO.load(tmp_path / "e.npz")[1].edges.shape == (0, 2)


# -- 4: the "forest" key of the neighbours argument ----------------------------------------------------------------
SPEC = {"radius": 14.0, "k": 3, "graph": "gabriel", "forest": True}


def test_resolve():
    assert NB.resolve(SPEC) == (14.0, 3, "gabriel", True)
    assert NB.resolve({"radius": 14.0, "k": 3, "graph": "gabriel"}) == (14.0, 3, "gabriel") and NB.resolve({"radius": 14, "k": 3}) == (14.0, 3)
    with pytest.raises(ValueError):
        NB.resolve({"radius": 14.0, "k": 3, "forest": True})     # without "graph"
    for bad in (False, 1, "yes", None, np.True_, [True]):
        with pytest.raises(ValueError):
            NB.resolve(dict(SPEC, forest=bad))
    with pytest.raises(ValueError):
        NB.resolve(dict(SPEC, graph="delaunay"))
    with pytest.raises(ValueError):
        NB.resolve(dict(SPEC, forests=True))
    assert P.resolve_specs(neighbours=SPEC).neighbours == (14.0, 3, "gabriel", True)


def test_a_bad_forest_is_refused_before_any_work(monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(NB, "query", no_work)
    monkeypatch.setattr(GR, "gabriel", no_work)
    monkeypatch.setattr(FO, "of_points", no_work)
    with pytest.raises(ValueError):
        NB.annotate(_stub(), 14.0, 3, 3, forest=True)            # without a graph
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            NB.annotate(_stub(), 14.0, 3, 3, graph="gabriel", forest=bad)
    with pytest.raises(ValueError):
        NB.annotate({}, 14.0, 3, 3, forest=True)


def test_annotate_adds_exactly_the_two_keys(monkeypatch):
    info = _stub()
    with_graph = NB.annotate(copy.deepcopy(info), 14.0, 3, 3, graph="gabriel")
    same = NB.annotate(copy.deepcopy(info), 14.0, 3, 3, graph="gabriel", forest=False)
    assert all(list(same[lab]) == list(with_graph[lab]) and same[lab]["neighbours"] == with_graph[lab]["neighbours"] for lab in info)
    calls = []
    host = GR.gabriel_host
    monkeypatch.setattr(GR, "gabriel_host", lambda *a: calls.append(1) or host(*a))
    got = NB.annotate(copy.deepcopy(info), 14.0, 3, 3, graph="gabriel", forest=True)
    assert calls == [1]                                           # the graph is computed once per call
    labels, g, f = FO.of_info(info, 14.0)
    assert labels == list(info) and 0 < f.edges.shape[0] == 40 - FO.n_components(f)
    mine = {(labels[a], labels[b]) for a, b in f.edges.tolist()}
    seen = set()
    for i, lab in enumerate(labels):
        nb = got[lab]["neighbours"]
        assert list(nb) == list(with_graph[lab]["neighbours"]) + ["component", "tree"]
        assert {k: nb[k] for k in with_graph[lab]["neighbours"]} == with_graph[lab]["neighbours"]
        assert nb["component"] == labels[f.component[i]] and type(nb["component"]) is int and all(type(v) is int for v in nb["tree"])
        assert nb["tree"] == [other for other in nb["graph"] if (min(lab, other), max(lab, other)) in mine]      # a part of "graph", in its order
        assert all(lab in got[other]["neighbours"]["tree"] and got[other]["neighbours"]["component"] == nb["component"] for other in nb["tree"])
        seen |= {(min(lab, other), max(lab, other)) for other in nb["tree"]}
        assert json.loads(json.dumps(nb)) == nb
    assert seen == mine
    assert NB.annotate({}, 14.0, 3, 3, graph="gabriel", forest=True) == {}
    empty = FO.of_info({}, 14.0)
    assert empty[0] == [] and empty[1].indptr.tolist() == [0] and empty[2].component.shape == (0,) and empty[2].edges.shape == (0, 2)
    via = P.annotate(copy.deepcopy(info), P.resolve_specs(neighbours=SPEC), 3, None)          # points.annotate passes the key on
    assert all(via[lab]["neighbours"] == got[lab]["neighbours"] for lab in info)
    off = P.annotate(copy.deepcopy(info), P.resolve_specs(neighbours={"radius": 14.0, "k": 3, "graph": "gabriel"}), 3, None)
    assert all(off[lab]["neighbours"] == with_graph[lab]["neighbours"] for lab in info)


@pytest.mark.parametrize("which", ["tile", "wsi"])
def test_managers_write_the_forest(which, tmp_path):
    """Both managers with the GPU call replaced by a stub that annotates as `process_images` / `WsiInference` do: the json gains the
    two keys and nothing else on disk changes; a bad spec is refused before the output directory exists."""
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
    runs = {"graph": {"radius": 14.0, "k": 3, "graph": "gabriel"}, "forest": SPEC}
    for key, nb in runs.items():
        spec[0] = nb
        assert run({"input_dir": str(inp), "output_dir": str(tmp_path / key), "neighbours": dict(nb)}) == done
    assert _tree(tmp_path / "graph") == _tree(tmp_path / "forest")
    for rel in _tree(tmp_path / "graph"):
        if rel != json_at and os.path.isfile(tmp_path / "graph" / rel):
            skip = 128 if rel.endswith(".mat") else 0             # a .mat file opens with 128 bytes of text that hold the time of writing
            assert (tmp_path / "graph" / rel).read_bytes()[skip:] == (tmp_path / "forest" / rel).read_bytes()[skip:], rel
    doc = json.loads((tmp_path / "forest" / json_at).read_text())
    want = NB.annotate(_stub(), 14.0, 3, 3, graph="gabriel", forest=True)
    assert len(doc["nuc"]) == 40 and sum(len(e["neighbours"]["tree"]) for e in doc["nuc"].values()) > 40
    for k, e in doc["nuc"].items():
        assert e["neighbours"]["tree"] == want[int(k)]["neighbours"]["tree"] and e["neighbours"]["component"] == want[int(k)]["neighbours"]["component"]
        del e["neighbours"]["tree"], e["neighbours"]["component"]
    assert json.dumps(doc) == (tmp_path / "graph" / json_at).read_text()         # without the key the json is the graph run's, byte for byte
    for bad in ({"forest": False}, {"forest": 1}, {"forest": "yes"}):
        with pytest.raises(ValueError):
            run({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "neighbours": dict(SPEC, **bad)})
        assert not (tmp_path / "bad").exists()                           # refused before any file is touched
    with pytest.raises(ValueError):
        run({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "neighbours": {"radius": 14.0, "k": 3, "forest": True}})
    assert not (tmp_path / "bad").exists()


# -- 5: the C side's refusals --------------------------------------------------------------------------------------
def _op():
    """A well-formed FOREST op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    at = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, e = 1000, 4000
    op = L.hvn_op()
    op.kind, op.x.h, op.x.base, op.w = PL.OP_NBR_FOREST, n, at(1), at(2)
    op.res.base, op.res.sn, op.y.base, op.y2.base = at(3), e, at(4), at(5)
    op.x2.base, op.x2.sn = at(6), FO.workspace_bytes(n)
    return op


# one entry per refusal that include/hvn.h lists for NBR_FOREST: (field, value, status, a word of its text)
FOREST_REFUSALS = [("_rsv", 4, -1, b"no phase"), ("_rsv", -1, -1, b"no phase"), ("x.base", None, -1, b"null xy"), ("w", None, -1, b"null indptr"),
                   ("y.base", None, -1, b"null component"), ("x2.base", None, -1, b"null workspace"), ("res.base", None, -1, b"null indices"),
                   ("y2.base", None, -1, b"null tree"), ("x.h", 0, -1, b"N = 0"), ("x.h", -5, -1, b"N = -5"), ("x.h", (1 << 26) + 1, -4, b"2^26"),
                   ("res.sn", -1, -1, b"fewer than none"), ("res.sn", 1 << 31, -4, b"reach 2^31"), ("res.sn", 1 << 40, -4, b"reach 2^31"),
                   ("x2.sn", 28 * 1000 + 255, -4, b"workspace of"), ("x2.sn", 0, -4, b"workspace of"), ("x.base", 0x11000004, -1, b"misaligned xy"),
                   ("w", 0x12000004, -1, b"misaligned indptr"), ("x2.base", 0x16000004, -1, b"misaligned workspace"),
                   ("res.base", 0x13000002, -1, b"misaligned indices"), ("y.base", 0x14000002, -1, b"misaligned component")]


def test_op_kind_23_is_in_the_header_the_plan_and_the_sources():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    header = open(L.HEADER).read()
    assert PL.OP_NBR_FOREST == 23 and "HVN_OP_NBR_FOREST = 23" in header and " NBR_FOREST " in header and "hvn_forest.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                      # no new export: the op goes through hvn_run_op
    kernels = open(L.CSRC + "/hvn_kernels.h").read()
    assert "struct NbrForestArgs" in kernels and FO.MAX_E == (1 << 31) - 1


def test_the_workspace_macro_and_its_python_mirror():
    """HVN_NBR_FOREST_WORKSPACE_BYTES and HVN_NBR_FOREST_ROUNDS_AT, read out of the header as arithmetic, against forest.py's."""
    import re

    from hover_net_amd import lib as L

    kernels = open(L.CSRC + "/hvn_kernels.h").read()
    for macro, mirror in (("HVN_NBR_FOREST_WORKSPACE_BYTES", FO.workspace_bytes), ("HVN_NBR_FOREST_ROUNDS_AT", FO.rounds_at)):
        body = re.search(r"#define %s\(N\) (\([^/\n]*\))" % macro, kernels).group(1).strip()
        for n in (1, 2, 1000, 12345, 1 << 26):
            assert eval(re.sub(r"(\d+)L", r"\1", body), {"N": n}) == mirror(n), (macro, n)
    assert FO.workspace_bytes(1000) == 28 * 1000 + 256 and FO.rounds_at(1000) % 4 == 0 and FO.rounds_at(1000) + 4 <= FO.workspace_bytes(1000)
    rounds = int(re.search(r"#define HVN_NBR_FOREST_MAX_ROUNDS (\d+)", kernels).group(1))
    assert rounds == FO.round_bound(P.MAX_N) == 26 and [FO.round_bound(n) for n in (1, 2, 3, 4, 5, 1000, 1024, 1025)] == [1, 1, 2, 2, 3, 10, 10, 11]


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_FOREST list: its status and a text of its own that leads with the op's name, decided before
    any launch (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as
    tests/test_graph_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code, word):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_forest:") and word in err and b"unknown op kind" not in err, (rc, err, word)

    texts = set()
    for path, value, code, word in FOREST_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 1, code, word)
        texts.add(word[:4] if word.startswith(b"N = ") else word)
    assert len(texts) == 17                                         # each kind of refusal has a text of its own
    refused(_op(), 2, -1, b"batch")                                  # batch must be 1
    op = _op()
    op._rsv, op.stride = 2, 26
    refused(op, 1, -1, b"round 26")
    op._rsv, op.stride = 2, -1
    refused(op, 1, -1, b"round -1")
    op = _op()
    op._rsv, op.stride, op.x.h = 2, 25, 0                            # the last round passes the op's own check: the next refusal is N
    refused(op, 1, -1, b"N = 0")
    op = _op()
    op.stride, op.x.h = 99, 0                                        # `stride` is read in phase 2 only
    refused(op, 1, -1, b"N = 0")
    op = _op()
    op.res.sn, op.x.h = (1 << 31) - 1, 0                             # the largest E
    refused(op, 1, -1, b"N = 0")
    op = _op()
    op.res.base, op.y2.base, op.res.sn, op.x2.sn = None, None, 0, 8  # E = 0 needs neither indices nor tree: the next refusal is the workspace
    refused(op, 1, -4, b"workspace of")
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1, b"null xy")                                 # an all-zero op is refused by name


def test_c_refusals_leave_the_output_untouched_on_the_host_side():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    buf = np.full(4000, 0x5A5A5A5A, np.int32)
    for path, value in (("_rsv", 7), ("res.sn", -3), ("w", None), ("x.h", 0), ("x2.sn", 8), ("y2.base", None)):
        op = _op()
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()

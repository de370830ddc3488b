"""-m gpu: the spanning forest and the components of the cell graph on the device (csrc/hvn_forest.hip: HVN_OP_NBR_FOREST) against the
scalar Kruskal of tests/forest_ref.py with == on component and edges, then the opt-in plumbing (`process`, tile mode, a whole slide)
against `neighbours.annotate(..., graph="gabriel", forest=True)` of the plain result on the host path."""
import copy
import json

import numpy as np
import pytest
import torch

import forest_ref as F
import graph_ref as G
import neighbours_ref as NR
from golden_util import assert_same_info
from gpu_util import _maps, _tile_images, synth_net

pytestmark = pytest.mark.gpu

SPEC = {"radius": 60.0, "k": 3, "graph": "gabriel", "forest": True}


def _fo():
    from hover_net_amd import forest as FO

    return FO


def _gr():
    from hover_net_amd import graph as GR

    return GR


# -- 1: device == oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.NAMES)
def test_device_equals_oracle(name):
    """`ruler1024` merges strictly pairwise: ten rounds join something, in order and shuffled.  `chain1000` hooks one chain 999 deep in
    its first round: the flatten walk.  `tiedline`, `lattice` and `piles` are decided by the position tie-break."""
    FO = _fo()
    (xy, g), want = F.case(name)
    F.assert_case_facts(name, xy, g, want)
    q = FO.DeviceForest(xy, g).run()
    got = q.result()
    assert isinstance(got, FO.Forest)
    F.assert_same(got, want, name)
    F.assert_case_facts(name, xy, g, got)
    assert 0 <= q.rounds <= FO.round_bound(xy.shape[0]) and (q.rounds == 0) == (want[1].shape[0] == 0)
    if name in F.ROUNDS:
        assert q.rounds == F.ROUNDS[name], (name, q.rounds)
    F.assert_same(FO.forest(xy, g, device="cuda"), want, name)


@pytest.mark.parametrize("name", ["random", "slide", "lattice", "widened", "one_point"])
def test_a_forest_on_the_buffers_of_a_device_graph(name):
    """`DeviceForest(graph=q)` reads the DeviceGraph's device xy, indptr and indices as they are -- rows in the order the count pass found
    them -- and gives what the host arrays give."""
    FO, GR = _fo(), _gr()
    (xy, g), want = F.case(name)
    _, r = G.points(name)
    q = GR.DeviceGraph(xy, r).run()
    f = FO.DeviceForest(graph=q)
    assert f.xy is q.xy and f.indptr is q.indptr and f.indices is q.indices and f.e == int(g.indptr[-1])
    F.assert_same(f.run().result(), want, name)
    graph, forest = FO.of_points(xy, r, device="cuda")
    G.assert_same(graph, g, name)
    F.assert_same(forest, want, name)
    with pytest.raises(ValueError):
        FO.DeviceForest(graph=GR.DeviceGraph(xy, r))              # a DeviceGraph that has not run


def test_coincident_piles_with_rows_of_2199():
    """Two coincident piles of 1500 and 700 points, 3 apart, r = 5, every row 2199 long (4.8 million entries, all but 1 050 000 of them
    with d2 = 0): the star at 0 over pile one, the edge (0, 1500), the star at 1500 over pile two -- the closed form, no oracle."""
    FO, GR = _fo(), _gr()
    a, b = 1500, 700
    xy, r = G._piles(a, b)
    q = GR.DeviceGraph(xy, r).run()
    assert q.e == (a + b) * (a + b - 1)
    f = FO.DeviceForest(graph=q).run()
    got = f.result()
    want = sorted([[0, j] for j in range(1, a + 1)] + [[a, j] for j in range(a + 1, a + b)])
    assert got.edges.dtype == np.int32 and got.edges.tolist() == want and not got.component.any() and got.component.dtype == np.int32
    assert f.rounds == 2


def test_same_bits_twice_in_reversed_order_and_in_every_form():
    """No output may depend on atomic arrival or on the order of the positions: the random case twice, with its positions reversed
    (mapped back), with one readback per round instead of the device's own early exit, and without the read in front of the atomics."""
    FO, GR = _fo(), _gr()
    (xy, g), want = F.case("random")
    first, second = FO.forest_device(xy, g), FO.forest_device(xy, g)
    F.assert_same(first, want)
    F.assert_same(second, first)
    n = xy.shape[0]
    rxy = np.ascontiguousarray(xy[::-1])
    deg = np.diff(g.indptr)[::-1]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    rows = [n - 1 - g.indices[g.indptr[n - 1 - i]:g.indptr[n - i]] for i in range(n)]
    rev = FO.forest_device(rxy, GR.CellGraph(indptr, np.concatenate(rows).astype(np.int32)))
    back = np.sort(n - 1 - rev.edges.astype(np.int64), 1)
    assert back[np.lexsort((back[:, 1], back[:, 0]))].tolist() == want[1].tolist()         # no tied d2 here: the same edges
    assert not rev.component.any()                                # one component, named by its smallest position, which is now 0
    q = FO.DeviceForest(xy, g).run_with_readbacks()
    F.assert_same(q.result(), want, "one readback per round")
    assert q.rounds == F.ROUNDS["random"] and q.hooks(q.rounds - 1) > 0 and q.hooks(q.rounds) == 0
    q = FO.DeviceForest(xy, g, no_filter=True).run()
    F.assert_same(q.result(), want, "no read before the atomics")


def test_a_symmetric_graph_that_is_not_gabriel():
    """Any symmetric graph is admitted: the symmetrised 5-nearest graph of the random case, 5970 edges with degrees up to 10, connected."""
    from hover_net_amd import neighbours as NB

    FO, GR = _fo(), _gr()
    (xy, _types, _r, _k, _t), res = NR.case("random")
    e = NB.edges(res["knn"]).astype(np.int64)
    rows, cols = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    o = np.lexsort((cols, rows))
    n = xy.shape[0]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    g = GR.CellGraph(indptr, cols[o].astype(np.int32))
    want = F.kruskal(xy, g)
    assert e.shape[0] == 5970 and int(np.diff(indptr).max()) == 10 and want[1].shape[0] == 1999 and not want[0].any()
    F.assert_same(FO.forest_device(xy, g), want, "knn graph")
    F.assert_same(FO.forest_host(xy, g), want, "knn graph, host")


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from hover_net_amd import lib as L
    from hover_net_amd import post_proc as PP

    FO, GR = _fo(), _gr()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(L, "lib", no_launch)
    monkeypatch.setattr(PP, "process_batch_device", no_launch)
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    pair = GR.CellGraph(np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32))
    with pytest.raises(ValueError):
        FO.forest_device(np.array([[0.0, np.nan], [1.0, 1.0]]), pair)
    with pytest.raises(TypeError):
        FO.forest_device(xy.astype(np.float32), pair)
    with pytest.raises(ValueError):
        FO.forest_device(xy, GR.CellGraph(np.array([0, 1, 1], np.int64), np.array([1], np.int32)))          # not symmetric
    with pytest.raises(ValueError):
        FO.forest_device(xy, pair, device="cpu")
    for bad in ({"forest": False}, {"forest": 1}, {"graph": "delaunay"}):
        with pytest.raises(ValueError):
            PP.process(np.zeros((20, 24, 3), np.float32), neighbours=dict({"radius": 5.0, "k": 2, "graph": "gabriel", "forest": True}, **bad))
    with pytest.raises(ValueError):
        PP.process(np.zeros((20, 24, 3), np.float32), neighbours={"radius": 5.0, "k": 2, "forest": True})


# -- 2: the public path --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return synth_net()


def _assert_annotated(info1, info0, nr_types):
    """info1 = info0 + "neighbours", and that entry is `annotate(..., graph="gabriel", forest=True)` of the plain dict on the HOST path;
    -> the number of tree links."""
    from hover_net_amd import neighbours as NB

    assert_same_info(info1, info0)
    want = NB.annotate(copy.deepcopy(info0), SPEC["radius"], SPEC["k"], nr_types, device=None, graph="gabriel", forest=True)
    graph = NB.annotate(copy.deepcopy(info0), SPEC["radius"], SPEC["k"], nr_types, device=None, graph="gabriel")
    links = 0
    for lab, e in info1.items():
        assert set(e) == set(info0[lab]) | {"neighbours"}, lab
        assert e["neighbours"] == want[lab]["neighbours"], lab
        assert list(e["neighbours"]) == list(graph[lab]["neighbours"]) + ["component", "tree"]
        assert json.loads(json.dumps(e["neighbours"])) == e["neighbours"]
        assert set(e["neighbours"]["tree"]) <= set(e["neighbours"]["graph"]) and e["neighbours"]["component"] in info1
        assert all(lab in info1[other]["neighbours"]["tree"] for other in e["neighbours"]["tree"])        # both ends list the edge
        links += len(e["neighbours"]["tree"])
    assert links == 2 * (len(info1) - len({e["neighbours"]["component"] for e in info1.values()}))         # F = N - components
    return links


def test_process_with_forest():
    from hover_net_amd import post_proc as PP

    pred = _maps(300, 340, 91)
    inst0, info0 = PP.process(pred, nr_types=5, return_centroids=True)
    inst1, info1 = PP.process(pred, nr_types=5, neighbours=SPEC)
    np.testing.assert_array_equal(inst1, inst0)
    assert len(info1) > 20 and _assert_annotated(info1, info0, 5) > 20


def test_tile_mode_with_forest(net):
    from hover_net_amd import infer_tile

    images = _tile_images()
    plain = infer_tile.process_images(images, net, nr_types=5, batch_size=8)
    got = infer_tile.process_images(images, net, nr_types=5, batch_size=8, neighbours=SPEC, return_centroids=False)
    entries = 0
    for (inst0, info0), (inst1, info1) in zip(plain, got):
        np.testing.assert_array_equal(inst1, inst0)
        _assert_annotated(info1, info0, 5)
        entries += len(info1)
    assert entries > 0


def test_wsi_forest_crosses_tile_seams(net):
    from hover_net_amd import infer_wsi

    maps = torch.from_numpy(_maps(900, 1000, 92)).to("cuda")
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    inst0, info0 = infer_wsi.WsiInference(net, **kw).stitch_instances(maps)
    inst1, info1 = infer_wsi.WsiInference(net, neighbours=SPEC, **kw).stitch_instances(maps)
    np.testing.assert_array_equal(inst1, inst0)
    assert len(info1) > 100 and _assert_annotated(info1, info0, 5) > 100
    tile = {lab: (int(e["centroid"][1]) // 512, int(e["centroid"][0]) // 512) for lab, e in info1.items()}
    across = sum(1 for lab, e in info1.items() for other in e["neighbours"]["tree"] if tile[other] != tile[lab])
    assert across >= 1

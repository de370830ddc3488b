"""-m gpu: DBSCAN on the device (csrc/hvn_clusters.hip: HVN_OP_NBR_GRID + HVN_OP_NBR_CLUSTER) against the O(N^2) oracle
tests/clusters_ref.py with == on both arrays, then the opt-in plumbing (`process`, tile mode, whole slides, the managers) against
`clusters.annotate` of the plain result on the host path."""
import copy
import json

import numpy as np
import pytest
import torch

import clusters_ref as R
from golden_util import assert_same_info
from gpu_util import _maps, _tile_images, synth_net

pytestmark = pytest.mark.gpu

# on the fixtures below (131 nuclei in 300 x 340, 923 in 900 x 1000, 10 in a 270 tile) these give several clusters with cores, borders and
# noise each; the counts asserted with them were taken from the oracle on those dicts
SPEC = {"radius": 30.0, "min_pts": 4}
TYPED_SPEC = {"radius": 30.0, "min_pts": 3, "types": [1, 2, 4]}
TILE_SPEC = {"radius": 80.0, "min_pts": 3}


def _cl():
    from hover_net_amd import clusters as CL

    return CL


# -- 1: device == oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_oracle(name):
    """Every case of tests/clusters_ref.py.  `snake` is a chain of 4078 points: the deep trees of the union-find; `crowded_all` hooks
    3000 cores of ONE cell onto one root; `widened` has a grid of 2^22 cells for 520 points; `bridge` holds a border point at equal
    d2 from cores of two clusters."""
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = _cl().cluster_device(*args)
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    R.assert_same(_cl().cluster(*args, device="cuda"), want, name)


@pytest.mark.parametrize("name", ["random", "typed", "snake", "slide", "bridge", "crowded_fine"])
def test_same_bits_twice_and_in_reversed_order(name):
    """The order of the points inside a cell and the shape of the union-find trees depend on atomic arrival; no output may.  The
    reversed input is held to the oracle of the reversed input: roots are smallest POSITIONS, so labels are not simply mirrored."""
    (xy, types, r, m, of), want = R.case(name)
    CL = _cl()
    first, second = CL.cluster_device(xy, types, r, m, of), CL.cluster_device(xy, types, r, m, of)
    R.assert_same(first, want, name)
    R.assert_same(second, first, name)
    rxy = np.ascontiguousarray(xy[::-1])
    rtypes = None if types is None else np.ascontiguousarray(types[::-1])
    R.assert_same(CL.cluster_device(rxy, rtypes, r, m, of), R.cluster(rxy, rtypes, r, m, of), name)


@pytest.mark.parametrize("name", ["random", "typed", "snake"])
def test_the_op_initialises_the_second_workspace(name):
    """0xFF bytes in the second workspace before the op (parent = -1, minpos = -1, degree = -1 everywhere): the op writes every word
    it reads, so the result is the oracle's.  The grid workspace is NBR_GRID's, filled as always."""
    args, want = R.case(name)
    q = _cl().DeviceClusters(*args)
    q.run_grid()
    q.ws2.fill_(0xFF)
    q.label.fill_(-7)
    q.degree.fill_(-7)
    q.run_op()
    R.assert_same(q.result(), want, name)
    q.run_op()                                  # and again on its own leftovers
    R.assert_same(q.result(), want, name)


def test_a_type_outside_the_mask_range_is_unselected():
    """Below the Python layer (which refuses such types): the device tensor of types is overwritten before the ops run.  With a mask
    other than -1 a type outside [0, 16) is unselected; with -1 every point takes part whatever its type."""
    (xy, types, r, m, of), _ = R.case("typed")
    CL = _cl()
    bad = types.copy()
    bad[::7] = 16 + 1                                # bit 1 of the mask is set: 17 must not alias type 1
    bad[3::11] = -1
    bad[5::13] = 33                                  # 33 % 32 == 1
    q = CL.DeviceClusters(xy, types, r, m, of)
    q.types.copy_(torch.from_numpy(bad))
    q.run_grid()
    q.run_op()
    R.assert_same(q.result(), R.cluster(xy, bad, r, m, of), "masked")
    q = CL.DeviceClusters(xy, types, r, m, None)
    q.types.copy_(torch.from_numpy(bad))
    q.run_grid()
    q.run_op()
    R.assert_same(q.result(), R.cluster(xy, None, r, m, None), "every point")


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from hover_net_amd import lib as L
    from hover_net_amd import post_proc as PP

    CL = _cl()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(L, "lib", no_launch)
    monkeypatch.setattr(PP, "process_batch_device", no_launch)
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    with pytest.raises(ValueError):
        CL.cluster_device(np.array([[0.0, np.nan], [1.0, 1.0]]), None, 1.0, 1)
    with pytest.raises(TypeError):
        CL.cluster_device(xy.astype(np.float32), None, 1.0, 1)
    with pytest.raises(ValueError):
        CL.cluster_device(xy, np.array([0, 16], np.int32), 1.0, 1)
    with pytest.raises(ValueError):
        CL.cluster_device(xy, None, 0.0, 1)
    with pytest.raises(ValueError):
        CL.cluster_device(xy, None, 1.0, 0)
    with pytest.raises(ValueError):
        CL.cluster_device(xy, None, 1.0, (1 << 26) + 1)
    with pytest.raises(TypeError):
        CL.cluster_device(xy, None, 1.0, 2.0)
    with pytest.raises(ValueError):
        CL.cluster_device(xy, None, 1.0, 1, of_types=(1,))               # of_types without types
    with pytest.raises(ValueError):
        CL.cluster_device(xy, np.array([0, 1], np.int32), 1.0, 1, of_types=())
    with pytest.raises(ValueError):
        CL.cluster_device(xy, None, 1.0, 1, device="cpu")
    with pytest.raises(ValueError):
        PP.process(np.zeros((20, 24, 3), np.float32), clusters={"radius": 5.0})
    with pytest.raises(ValueError):
        PP.process(np.zeros((20, 24, 3), np.float32), clusters={"radius": -5.0, "min_pts": 2})
    with pytest.raises(ValueError):
        PP.process(np.zeros((20, 24, 3), np.float32), nr_types=None, clusters={"radius": 5.0, "min_pts": 2, "types": [1]})


# -- 2: the public path --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return synth_net()


def _assert_annotated(info1, info0, nr_types, spec=SPEC):
    """info1 = info0 + "cluster", and that entry is `annotate` of the plain dict on the HOST path; -> (clusters, cores, borders, noise)."""
    assert_same_info(info1, info0)
    assert all("cluster" not in e for e in info0.values())
    want = _cl().annotate(copy.deepcopy(info0), spec["radius"], spec["min_pts"], nr_types, spec.get("types"), device=None)
    for lab, e in info1.items():
        assert set(e) == set(info0[lab]) | {"cluster"}, lab
        assert e["cluster"] == want[lab]["cluster"], lab
        assert json.loads(json.dumps(e["cluster"])) == e["cluster"]
    c = [e["cluster"] for e in info1.values()]
    return (len({e["id"] for e in c if e["id"] is not None}), sum(e["core"] for e in c), sum(e["id"] is not None and not e["core"] for e in c),
            sum(e["id"] is None and e["degree"] > 0 for e in c))


def test_process_with_clusters():
    from hover_net_amd import post_proc as PP

    pred = _maps(300, 340, 91)
    inst0, info0 = PP.process(pred, nr_types=5, return_centroids=True)
    inst1, info1 = PP.process(pred, nr_types=5, clusters=SPEC)                           # implies the dict
    np.testing.assert_array_equal(inst1, inst0)
    assert len(info1) == 131 and _assert_annotated(info1, info0, 5) == (9, 77, 41, 13)
    _, info3 = PP.process(pred, nr_types=5, clusters=TYPED_SPEC)
    assert _assert_annotated(info3, info0, 5, TYPED_SPEC) == (11, 61, 20, 16)
    assert sum(e["cluster"]["degree"] == 0 for e in info3.values()) == 34                  # unselected nuclei
    inst2, info2 = PP.process(pred[..., 1:], nr_types=None, clusters=SPEC)                 # no type branch
    _, plain2 = PP.process(pred[..., 1:], nr_types=None, return_centroids=True)
    assert min(_assert_annotated(info2, plain2, None)) >= 1
    # together with neighbours= both entries arrive, each as on its own
    _, both = PP.process(pred, nr_types=5, clusters=SPEC, neighbours={"radius": 60.0, "k": 3})
    assert all(e["cluster"] == info1[lab]["cluster"] and "neighbours" in e for lab, e in both.items())


def test_tile_mode_with_clusters(net):
    from hover_net_amd import infer_tile

    images = _tile_images()
    plain = infer_tile.process_images(images, net, nr_types=5, batch_size=8)
    got = infer_tile.process_images(images, net, nr_types=5, batch_size=8, clusters=TILE_SPEC, return_centroids=False)
    counts = []
    for (inst0, info0), (inst1, info1) in zip(plain, got):
        np.testing.assert_array_equal(inst1, inst0)
        counts.append(_assert_annotated(info1, info0, 5, TILE_SPEC))
    assert counts[0][0] >= 1 and counts[0][1] >= TILE_SPEC["min_pts"]          # the first image holds a cluster (these nuclei come from the network)


def test_process_file_list_clusters(net, tmp_path):
    from hover_net_amd import infer_manager, infer_tile

    images = _tile_images()
    inp = tmp_path / "in"
    inp.mkdir()
    for name, img in zip("ab", images):
        np.save(inp / (name + ".npy"), img)
    want = infer_tile.process_images(images, net, nr_types=5, batch_size=8, clusters=TILE_SPEC)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    text = {}
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "batch_size": 8}
        if flag:
            args["clusters"] = dict(TILE_SPEC)
        assert mgr.process_file_list(args) == ["a", "b"]
        for name, (_inst, info) in zip("ab", want):
            text[flag, name] = open(out / "json" / (name + ".json")).read()
            nuc = json.loads(text[flag, name])["nuc"]
            assert sorted(int(k) for k in nuc) == sorted(info)
            for k, e in nuc.items():
                if flag:
                    assert e["cluster"] == info[int(k)]["cluster"]
                else:
                    assert set(e) == {"bbox", "centroid", "contour", "type_prob", "type"}
    # without the key the json is what it is today: the flagged one minus the new entry, byte for byte
    for name in "ab":
        doc = json.loads(text[True, name])
        for e in doc["nuc"].values():
            del e["cluster"]
        assert json.dumps(doc) == text[False, name]
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "clusters": {"radius": 5.0}})
    assert not (tmp_path / "bad").exists()


def test_wsi_clusters_cross_tile_seams(net):
    from hover_net_amd import infer_wsi

    maps = torch.from_numpy(_maps(900, 1000, 92)).to("cuda")
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    inst0, info0 = infer_wsi.WsiInference(net, **kw).stitch_instances(maps)
    inst1, info1 = infer_wsi.WsiInference(net, clusters=SPEC, **kw).stitch_instances(maps)
    np.testing.assert_array_equal(inst1, inst0)
    assert len(info1) == 923 and _assert_annotated(info1, info0, 5) == (76, 449, 250, 224)
    tile = {lab: (int(e["centroid"][1]) // 512, int(e["centroid"][0]) // 512) for lab, e in info1.items()}
    across = sum(1 for lab, e in info1.items() if e["cluster"]["id"] is not None and tile[e["cluster"]["id"]] != tile[lab])
    assert across >= 1                                # a cluster's root nucleus lies in another tile than one of its members
    seam = [e for e in info1.values() if e["cluster"]["id"] is not None and min(abs(e["centroid"][0] - 512), abs(e["centroid"][1] - 512)) < 15]
    assert len(seam) >= 1                             # clustered nuclei within half a radius of a tile seam


def test_wsi_manager_clusters(net, tmp_path, monkeypatch):
    """The manager's key down to the json; stage 1 is replaced by a structured prediction map, as tests/test_gpu_neighbours.py does."""
    from PIL import Image

    from hover_net_amd import infer_manager, infer_wsi
    from hover_net_amd.synth import synth_tiles

    maps = torch.from_numpy(_maps(300, 340, 91)).to("cuda")
    monkeypatch.setattr(infer_wsi.WsiInference, "raw_prediction", lambda self, slide, mask, as_slab=False: infer_wsi.SlabMap(maps, 0))
    inp = tmp_path / "in"
    inp.mkdir()
    np.save(inp / "s.npy", synth_tiles(1, 340, seed=95)[0][:300])
    msk = tmp_path / "msk"
    msk.mkdir()
    Image.fromarray(np.full((10, 11), 255, np.uint8)).save(msk / "s.png")      # all tissue
    mgr = infer_manager.WsiManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    text = {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "input_mask_dir": str(msk), "batch_size": 8, "tile_shape": 512, "chunk_shape": 1000,
                "ambiguous_size": 64}
        if flag:
            args["clusters"] = dict(TYPED_SPEC)
        assert mgr.process_wsi_list(args) == {"s": "done"}
        text[flag] = open(out / "s.json").read()
    doc = json.loads(text[True])
    assert len(doc["nuc"]) > 20
    plain = {int(k): {"centroid": np.array(e["centroid"]), "type": e["type"]} for k, e in json.loads(text[False])["nuc"].items()}
    want = _cl().annotate(plain, TYPED_SPEC["radius"], TYPED_SPEC["min_pts"], 5, TYPED_SPEC["types"], device=None)
    for k, e in doc["nuc"].items():
        assert e["cluster"] == want[int(k)]["cluster"], k
        del e["cluster"]
    assert json.dumps(doc) == text[False]

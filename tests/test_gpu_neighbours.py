"""-m gpu: the neighbour search on the device (csrc/hvn_neighbours.hip: HVN_OP_NBR_GRID + HVN_OP_NBR_QUERY) against the O(N^2) oracle
tests/neighbours_ref.py with == on all three arrays, then the opt-in plumbing (`process`, tile mode, whole slides, the managers) against
`neighbours.annotate` of the plain result on the host path."""
import copy
import json

import numpy as np
import pytest
import torch

import neighbours_ref as R
from golden_util import assert_same_info
from gpu_util import _maps, _tile_images, synth_net

pytestmark = pytest.mark.gpu

SPEC = {"radius": 60.0, "k": 3}


def _nb():
    from hover_net_amd import neighbours as NB

    return NB


# -- 1: device == oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_oracle(name):
    """Cases 1-8 of the issue.  `crowded` holds 3000 points in ONE cell: three staging tiles of 1024 candidates per grid row and
    twelve workgroups of 256 queries; `widened` has a grid of 2^22 cells for 520 points (the scan's 1024 blocks all run)."""
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = _nb().query_device(*args)
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    R.assert_same(_nb().query(*args, device="cuda"), want, name)


def test_same_bits_twice_and_in_reversed_order():
    """The order of the points inside a cell depends on atomic arrival; no output may.  The random case has no two equal distances
    in a neighbourhood, so reversing the input reverses the positions and nothing else."""
    (xy, types, r, k, t), want = R.case("random")
    NB = _nb()
    first, second = NB.query_device(xy, types, r, k, t), NB.query_device(xy, types, r, k, t)
    R.assert_same(first, want)
    R.assert_same(second, first)
    n = xy.shape[0]
    rev = NB.query_device(np.ascontiguousarray(xy[::-1]), np.ascontiguousarray(types[::-1]), r, k, t)
    back = {"count": rev["count"][::-1]}
    for name in ("knn", "nearest_of_type"):
        back[name] = np.where(rev[name] >= 0, n - 1 - rev[name], -1)[::-1].astype(np.int32)
    R.assert_same(back, want)


def test_a_type_outside_the_columns_counts_nowhere_and_stays_in_knn():
    """Below the Python layer (which refuses such types): the device tensor of types is overwritten before the ops run."""
    (xy, types, r, k, t), want = R.case("random")
    NB = _nb()
    bad = types.copy()
    bad[::7] = 9
    bad[3::11] = -1
    q = NB.DeviceQuery(xy, types, r, k, t)
    q.types.copy_(torch.from_numpy(bad))
    q.run_grid()
    q.run_op()
    got = q.result()
    outside = (bad < 0) | (bad >= t)
    wide = R.query(xy, np.where(outside, t, bad), r, k, t + 1)      # the oracle with one more column for them
    assert (got["knn"] == want["knn"]).all()
    assert (got["count"] == wide["count"][:, :t]).all() and (got["nearest_of_type"] == wide["nearest_of_type"][:, :t]).all()
    assert wide["count"][:, t].sum() > 0


def test_coordinates_that_are_not_finite_stay_inside_the_grid():
    """Below the Python layer (which refuses them): NaN, +-inf and +-1e300 overwrite five rows of the device copy of xy.  Their cells
    are clamped into the grid; they are nobody's neighbour (their d2 is NaN or inf); every other row is what the oracle gives without
    them."""
    (xy, types, r, k, t), _ = R.case("untyped")
    NB = _nb()
    n = xy.shape[0]
    rows = [5, 50, 120, 200, 299]
    poisoned = xy.copy()
    for i, v in zip(rows, (np.nan, np.inf, -np.inf, 1.0e300, -1.0e300)):
        poisoned[i, i % 2] = v
    q = NB.DeviceQuery(xy, types, r, k, t)
    q.xy.copy_(torch.from_numpy(poisoned))
    q.run_grid()
    q.run_op()
    got = q.result()
    keep = np.setdiff1d(np.arange(n), rows)
    want = R.query(xy[keep], None, r, k, t)
    back = lambda a: np.where(a >= 0, keep[np.where(a >= 0, a, 0)], -1)  # noqa: E731
    assert (got["count"][keep] == want["count"]).all()
    assert (got["knn"][keep] == back(want["knn"])).all() and (got["nearest_of_type"][keep] == back(want["nearest_of_type"])).all()
    assert not got["count"][rows].any() and (got["knn"][rows] == -1).all()


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from hover_net_amd import lib as L
    from hover_net_amd import post_proc as PP

    NB = _nb()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(L, "lib", no_launch)
    monkeypatch.setattr(PP, "process_batch_device", no_launch)
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    with pytest.raises(ValueError):
        NB.query_device(np.array([[0.0, np.nan], [1.0, 1.0]]), None, 1.0, 1)
    with pytest.raises(TypeError):
        NB.query_device(xy.astype(np.float32), None, 1.0, 1)
    with pytest.raises(ValueError):
        NB.query_device(xy, np.array([0, 5], np.int32), 1.0, 1, 5)
    with pytest.raises(ValueError):
        NB.query_device(xy, None, 0.0, 1)
    with pytest.raises(ValueError):
        NB.query_device(xy, None, 1.0, 17)
    with pytest.raises(ValueError):
        NB.query_device(xy, None, 1.0, 1, device="cpu")
    with pytest.raises(ValueError):
        PP.process(np.zeros((20, 24, 3), np.float32), neighbours={"radius": 5.0})
    with pytest.raises(ValueError):
        PP.process(np.zeros((20, 24, 3), np.float32), neighbours={"radius": -5.0, "k": 2})


# -- 2: the public path --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return synth_net()


def _assert_annotated(info1, info0, nr_types, spec=SPEC):
    """info1 = info0 + "neighbours", and that entry is `annotate` of the plain dict on the HOST path; -> the number of knn links."""
    assert_same_info(info1, info0)
    assert all("neighbours" not in e for e in info0.values())
    want = _nb().annotate(copy.deepcopy(info0), spec["radius"], spec["k"], nr_types, device=None)
    links = 0
    for lab, e in info1.items():
        assert set(e) == set(info0[lab]) | {"neighbours"}, lab
        assert e["neighbours"] == want[lab]["neighbours"], lab
        assert json.loads(json.dumps(e["neighbours"])) == e["neighbours"]
        links += len(e["neighbours"]["knn"])
    return links


def test_process_with_neighbours():
    from hover_net_amd import post_proc as PP

    pred = _maps(300, 340, 91)
    inst0, info0 = PP.process(pred, nr_types=5, return_centroids=True)
    inst1, info1 = PP.process(pred, nr_types=5, neighbours=SPEC)                         # implies the dict
    np.testing.assert_array_equal(inst1, inst0)
    assert len(info1) > 20 and _assert_annotated(info1, info0, 5) > 20
    inst2, info2 = PP.process(pred[..., 1:], nr_types=None, neighbours=SPEC)               # no type branch: one column
    _, plain2 = PP.process(pred[..., 1:], nr_types=None, return_centroids=True)
    assert _assert_annotated(info2, plain2, None) > 20
    assert all(len(e["neighbours"]["count"]) == 1 and e["type"] is None for e in info2.values())


def test_tile_mode_with_neighbours(net):
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


def test_process_file_list_neighbours(net, tmp_path):
    from hover_net_amd import infer_manager, infer_tile

    images = _tile_images()
    inp = tmp_path / "in"
    inp.mkdir()
    for name, img in zip("ab", images):
        np.save(inp / (name + ".npy"), img)
    want = infer_tile.process_images(images, net, nr_types=5, batch_size=8, neighbours=SPEC)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    text = {}
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "batch_size": 8}
        if flag:
            args["neighbours"] = dict(SPEC)
        assert mgr.process_file_list(args) == ["a", "b"]
        for name, (_inst, info) in zip("ab", want):
            text[flag, name] = open(out / "json" / (name + ".json")).read()
            nuc = json.loads(text[flag, name])["nuc"]
            assert sorted(int(k) for k in nuc) == sorted(info)
            for k, e in nuc.items():
                if flag:
                    assert e["neighbours"] == info[int(k)]["neighbours"]
                else:
                    assert set(e) == {"bbox", "centroid", "contour", "type_prob", "type"}
    # without the key the json is what it is today: the flagged one minus the new entry, byte for byte
    for name in "ab":
        doc = json.loads(text[True, name])
        for e in doc["nuc"].values():
            del e["neighbours"]
        assert json.dumps(doc) == text[False, name]
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "neighbours": {"radius": 5.0}})
    assert not (tmp_path / "bad").exists()


def test_wsi_neighbours_cross_tile_seams(net):
    from hover_net_amd import infer_wsi

    maps = torch.from_numpy(_maps(900, 1000, 92)).to("cuda")
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    inst0, info0 = infer_wsi.WsiInference(net, **kw).stitch_instances(maps)
    inst1, info1 = infer_wsi.WsiInference(net, neighbours=SPEC, **kw).stitch_instances(maps)
    np.testing.assert_array_equal(inst1, inst0)
    assert len(info1) > 100 and _assert_annotated(info1, info0, 5) > 100
    tile = {lab: (int(e["centroid"][1]) // 512, int(e["centroid"][0]) // 512) for lab, e in info1.items()}
    across = sum(1 for lab, e in info1.items() for other in e["neighbours"]["knn"] if tile[other] != tile[lab])
    assert across >= 1


def test_wsi_manager_neighbours(net, tmp_path, monkeypatch):
    """The manager's key down to the json; stage 1 is replaced by a structured prediction map, as tests/test_gpu_features.py does."""
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
            args["neighbours"] = dict(SPEC)
        assert mgr.process_wsi_list(args) == {"s": "done"}
        text[flag] = open(out / "s.json").read()
    doc = json.loads(text[True])
    assert len(doc["nuc"]) > 20
    plain = {int(k): {"centroid": np.array(e["centroid"]), "type": e["type"]} for k, e in json.loads(text[False])["nuc"].items()}
    want = _nb().annotate(plain, SPEC["radius"], SPEC["k"], 5, device=None)
    for k, e in doc["nuc"].items():
        assert e["neighbours"] == want[int(k)]["neighbours"], k
        del e["neighbours"]
    assert json.dumps(doc) == text[False]

"""-m gpu: nuclei in annotated regions on the device (csrc/hvn_regions.hip: HVN_OP_NBR_GRID + HVN_OP_NBR_REGIONS) against the all-edges
oracle tests/regions_ref.py and the host path with ==, then the opt-in plumbing (whole slides, the two managers) against
`regions.of_info` of the plain result on the host path.  Integers only: no tolerance anywhere."""
import json

import numpy as np
import pytest
import torch

import regions_ref as R
from gpu_util import _maps, _tile_images, synth_net

pytestmark = pytest.mark.gpu


def _rg():
    from hover_net_amd import regions as RG

    return RG


# -- 1: device == host == oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_host_and_oracle(name):
    """Every case of tests/regions_ref.py.  `long_ring` walks one list of eight staging tiles with region boundaries inside a tile, at
    a tile's end and at a tile's start; `tall_edge` has some 1700 rows for 400 points, so a workgroup walks many rows; `far_outside` has
    edges in the clamped end rows; `degenerate` launches nothing; `many_regions` and `sixteen_types` are the caps."""
    args, want = R.case(name)
    RG = _rg()
    got = RG.regions_device(*args[:4], cell=args[4])
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    assert got.names == args[2].names and (got.area == args[2].area).all()
    R.assert_same(RG.regions_host(*args), want, name)
    R.assert_same(RG.regions(*args[:4], device="cuda", cell=args[4]), want, name)


@pytest.mark.parametrize("name,cell", [("tessellation", 0.75), ("tessellation", 1.0e5), ("sixteen_types", 1.5), ("long_ring", 3.0), ("hole", 1.0e5)])
def test_the_cell_side_changes_nothing(name, cell):
    """Many rows per workgroup, and one row for all (the brute-force form): the same integers."""
    (xy, types, rs, t, _), want = R.case(name)
    R.assert_same(_rg().regions_device(xy, types, rs, t, cell=cell), want, name)


def test_the_degenerate_case_launches_nothing(monkeypatch):
    from hover_net_amd import lib as L

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    args, want = R.case("degenerate")
    R.assert_same(_rg().regions_device(*args[:4]), want, "degenerate")
    with pytest.raises(ValueError, match="no edge"):
        _rg().DeviceRegions(*args[:4])


@pytest.mark.parametrize("name", ["triangle_257", "hole", "overlap", "tessellation", "long_ring", "sixteen_types"])
def test_same_bits_twice_and_in_reversed_order(name):
    """The order of the points inside a cell depends on atomic arrival, and so does the order of the adds; the results may not, and
    with the points reversed first / hits are the reversed arrays."""
    (xy, types, rs, t, cell), want = R.case(name)
    RG = _rg()
    first, second = RG.regions_device(xy, types, rs, t, cell=cell), RG.regions_device(xy, types, rs, t, cell=cell)
    R.assert_same(first, want, name)
    R.assert_same(second, first[:3], name)
    rxy = np.ascontiguousarray(xy[::-1])
    rtypes = None if types is None else np.ascontiguousarray(types[::-1])
    R.assert_same(RG.regions_device(rxy, rtypes, rs, t, cell=cell), (want[0][::-1], want[1][::-1], want[2]), name)


@pytest.mark.parametrize("name", ["triangle_1", "triangle_257", "hole", "far_outside", "many_regions"])
def test_the_op_writes_every_element(name):
    """`out` holds -7 everywhere before the op: the result is still the oracle's (points in no region and bins that no point reaches
    included), and so is the result of the op run again on its own output."""
    args, want = R.case(name)
    q = _rg().DeviceRegions(*args[:4], cell=args[4])
    q.run_grid()
    q.out.fill_(-7)
    q.run_op()
    R.assert_same(q.result(), want, name)
    q.run_op()
    R.assert_same(q.result(), want, name)


@pytest.mark.parametrize("name", ["overlap", "sixteen_types"])
def test_a_type_outside_the_range_is_counted_nowhere(name):
    """Below the Python layer (which refuses such types): the device tensor of types is overwritten before the ops run.  17 must not
    alias type 1, 33 neither, -1 no column at all; with T = 4 a type in [4, 16) neither.  first / hits do not look at types."""
    (xy, types, rs, t, cell), want = R.case(name)
    bad = types.copy()
    bad[::7] = 16
    bad[1::7] = 17
    bad[3::11] = -1
    bad[5::13] = 33
    if t < 16:
        bad[2::17] = 12
    q = _rg().DeviceRegions(xy, types, rs, t, cell=cell)
    q.types.copy_(torch.from_numpy(bad))
    q.run_grid()
    q.run_op()
    got = q.result()
    expect = R.regions(xy, bad, rs.polygons, t)
    inside = (bad >= 0) & (bad < t)
    assert int(expect[2].sum()) < int(want[2].sum()) and 0 < int(inside.sum()) < bad.shape[0]
    R.assert_same(got, (want[0], want[1], expect[2]), name)
    assert int(got.count.sum()) == int(got.hits[inside].sum())


# -- 2: scale -----------------------------------------------------------------------------------------------------
def _slide_points(n, side, seed):
    """Slide-like centroids: 70 % uniform, 30 % in Gaussian clumps of 200 (sigma 40 px), five types."""
    rng = np.random.default_rng(seed)
    nu = n * 7 // 10
    centres = rng.random(((n - nu) // 200, 2)) * side
    clumps = np.repeat(centres, 200, 0) + rng.normal(0.0, 40.0, ((n - nu) // 200 * 200, 2))
    xy = np.concatenate([rng.random((n - clumps.shape[0], 2)) * side, np.clip(clumps, 0.0, side - 1.0)])
    return np.ascontiguousarray(xy[rng.permutation(n)]), rng.integers(0, 5, n).astype(np.int32)


def _blobs(n_regions, n_vertices, side, seed):
    """Irregular star-shaped regions: the radius of vertex k is a base radius times a smooth random factor in [0.6, 1.4]."""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n_vertices) / n_vertices
    regs = []
    for _ in range(n_regions):
        cx, cy = rng.random(2) * side
        base = side * (0.02 + 0.08 * rng.random())
        f = 1.0 + sum(0.4 / 3 * np.sin((h + 2) * a + rng.random() * 6.28) for h in range(3))
        regs.append([[np.stack([cx + base * f * np.cos(a), cy + base * f * np.sin(a)], 1)]])
    return regs


def test_device_equals_host_path_at_slide_size():
    """200 000 points over 16384 x 16384 px against 50 irregular regions of 200 vertices: too many tests for the oracle, so the device
    is held to `regions_host`, which tests/test_regions_host.py holds to the oracle."""
    RG = _rg()
    xy, types = _slide_points(200000, 16384.0, 44)
    rs = RG.RegionSet.from_polygons(_blobs(50, 200, 16384.0, 45))
    host = RG.regions_host(xy, types, rs, 5)
    dev = RG.regions_device(xy, types, rs, 5)
    R.assert_same(dev, host[:3], "slide")
    assert rs.edges.shape[0] > 9900 and int(host.hits.sum()) > 20000 and host.hits.max() >= 2 and int((host.count > 0).sum()) > 200
    assert RG.cell_side(xy, rs)[1].ncy > 500


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from hover_net_amd import infer_wsi
    from hover_net_amd import lib as L

    RG = _rg()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(L, "lib", no_launch)
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    rs = RG.RegionSet.from_polygons([[[R.TRIANGLE]]])
    for args, exc in (((np.array([[0.0, np.nan], [1.0, 1.0]]), None, rs), ValueError), ((xy.astype(np.float32), None, rs), TypeError),
                      ((xy, np.array([0, 16], np.int32), rs), ValueError), ((xy, None, [[[R.TRIANGLE]]]), TypeError), ((xy, None, rs, 17), ValueError)):
        with pytest.raises(exc):
            RG.regions_device(*args)
    with pytest.raises(ValueError):
        RG.regions_device(xy, None, rs, device="cpu")
    with pytest.raises(ValueError):
        infer_wsi.WsiInference(None, regions={"region": rs})
    with pytest.raises(TypeError):
        infer_wsi.WsiInference(None, regions={"regions": 5})


# -- 3: the plumbing ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return synth_net()


def _annotation(h, w):
    """Three regions over an image of h x w: a blob across the middle (hence across a tile seam of a slide), a frame with a hole around
    most of the image, and a corner triangle; as the GeoJSON a user would export."""
    a = 2.0 * np.pi * np.arange(60) / 60
    blob = np.stack([0.5 * w + 0.3 * w * (1.0 + 0.25 * np.sin(3 * a)) * np.cos(a), 0.5 * h + 0.3 * h * (1.0 + 0.25 * np.cos(5 * a)) * np.sin(a)], 1)
    feats = [("tumour", [blob.tolist() + [blob[0].tolist()]]),
             ("frame", [[[0.05 * w, 0.05 * h], [0.95 * w, 0.05 * h], [0.95 * w, 0.95 * h], [0.05 * w, 0.95 * h], [0.05 * w, 0.05 * h]],
                        [[0.4 * w, 0.4 * h], [0.6 * w, 0.4 * h], [0.6 * w, 0.6 * h], [0.4 * w, 0.6 * h], [0.4 * w, 0.4 * h]]]),
             ("corner", [[[0.0, 0.0], [0.3 * w, 0.0], [0.0, 0.3 * h], [0.0, 0.0]]])]
    return {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"name": n}, "geometry": {"type": "Polygon", "coordinates": c}} for n, c in feats]}


def _assert_counts(rc, info, geo, nr_types, scale=1.0):
    """rc is `of_info` of the dict (without its "region" keys) on the HOST path, field by field."""
    RG = _rg()
    rs = RG.RegionSet.from_geojson(geo, scale)
    want = RG.of_info({lab: {k: v for k, v in e.items() if k != "region"} for lab, e in info.items()}, rs, nr_types, device=None)
    assert isinstance(rc, RG.RegionCounts) and list(rc.names) == rs.names == ["tumour", "frame", "corner"] and (np.asarray(rc.area) == rs.area).all()
    R.assert_same(rc, want[:3], "plumbing")
    return want


def _load(path):
    with np.load(path) as z:
        assert sorted(z.files) == ["area", "count", "first", "hits", "names"]
        return _rg().RegionCounts(z["first"], z["hits"], z["count"], z["names"].tolist(), z["area"])


def test_wsi_regions_cross_tile_seams(net):
    """The small synthetic slide of tests/test_gpu_ripley.py (923 nuclei in 900 x 1000, tiles of 512): the regions are tested once
    against the merged dict, so a region that lies across the seam x = 512 counts its nuclei on both sides."""
    from golden_util import assert_same_info
    from hover_net_amd import infer_wsi

    geo = _annotation(900, 1000)
    maps = torch.from_numpy(_maps(900, 1000, 92)).to("cuda")
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    plain = infer_wsi.WsiInference(net, **kw)
    inst0, info0 = plain.stitch_instances(maps)
    assert plain.regions is None and plain.points.regions is None and not any("region" in e for e in info0.values())
    wsi = infer_wsi.WsiInference(net, regions={"regions": geo}, **kw)
    assert wsi.regions is None                                   # nothing before the first slide
    inst1, info1 = wsi.stitch_instances(maps)
    np.testing.assert_array_equal(inst1, inst0)
    assert len(info1) == 923 and all(set(e) == set(info0[lab]) | {"region"} for lab, e in info1.items())
    assert_same_info({lab: {k: v for k, v in e.items() if k != "region"} for lab, e in info1.items()}, info0)
    rc = _assert_counts(wsi.regions, info1, geo, 5)
    assert [e["region"] for e in info1.values()] == rc.first.tolist() and all(type(e["region"]) is int for e in info1.values())
    xs = np.array([e["centroid"][0] for e in info1.values()])
    tumour = (rc.first == 0)
    assert int((tumour & (xs < 512)).sum()) > 20 and int((tumour & (xs >= 512)).sum()) > 20 and rc.hits.max() >= 2 and (rc.count.sum(1) > 0).all()


def test_process_file_list_regions(net, tmp_path):
    from hover_net_amd import infer_manager, infer_tile

    images = _tile_images()
    inp, ann = tmp_path / "in", tmp_path / "ann"
    inp.mkdir()
    ann.mkdir()
    for name, img in zip("ab", images):
        np.save(inp / (name + ".npy"), img)
    geo = _annotation(*images[0].shape[:2])
    doubled = json.loads(json.dumps(geo))
    for f in doubled["features"]:
        f["geometry"]["coordinates"] = [[[2.0 * x, 2.0 * y] for x, y in ring] for ring in f["geometry"]["coordinates"]]
    (ann / "a.geojson").write_text(json.dumps(doubled))              # level-0 pixels at twice the processed size; none for b
    want = infer_tile.process_images(images, net, nr_types=5, batch_size=8)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    text = {}
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "batch_size": 8}
        if flag:
            args["regions"] = {"dir": str(ann), "scale": 0.5}
        assert mgr.process_file_list(args) == ["a", "b"]
        assert (out / "regions").exists() == flag                # absent: no regions/ directory
        for name in "ab":
            text[flag, name] = open(out / "json" / (name + ".json")).read()
    assert text[True, "b"] == text[False, "b"] and not (tmp_path / "out1" / "regions" / "b.npz").exists()     # no file for b: as without the argument
    rc = _assert_counts(_load(tmp_path / "out1" / "regions" / "a.npz"), want[0][1], doubled, 5, scale=0.5)
    assert rc.count.shape == (3, 5) and int(rc.count[0].sum()) > 0 and int(rc.hits.sum()) > 0
    on, off = json.loads(text[True, "a"])["nuc"], json.loads(text[False, "a"])["nuc"]
    assert [e["region"] for e in on.values()] == rc.first.tolist()
    assert {k: {f: v for f, v in e.items() if f != "region"} for k, e in on.items()} == off
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "regions": {"regions": str(ann)}})
    assert not (tmp_path / "bad").exists()


def test_wsi_manager_regions(net, tmp_path, monkeypatch):
    """The manager's key down to regions/<name>.npz; stage 1 is replaced by a structured prediction map, as tests/test_gpu_ripley.py
    does."""
    from PIL import Image

    from hover_net_amd import infer_manager, infer_wsi
    from hover_net_amd.synth import synth_tiles

    maps = torch.from_numpy(_maps(300, 340, 91)).to("cuda")
    monkeypatch.setattr(infer_wsi.WsiInference, "raw_prediction", lambda self, slide, mask, as_slab=False: infer_wsi.SlabMap(maps, 0))
    inp, msk, ann = tmp_path / "in", tmp_path / "msk", tmp_path / "ann"
    for d in (inp, msk, ann):
        d.mkdir()
    np.save(inp / "s.npy", synth_tiles(1, 340, seed=95)[0][:300])
    Image.fromarray(np.full((10, 11), 255, np.uint8)).save(msk / "s.png")      # all tissue
    geo = _annotation(300, 340)
    (ann / "s.geojson").write_text(json.dumps(geo))
    mgr = infer_manager.WsiManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    text = {}
    for flag, d in ((False, None), (True, ann), (True, tmp_path / "nowhere")):
        out = tmp_path / ("out%d%s" % (flag, "" if d in (None, ann) else "x"))
        args = {"input_dir": str(inp), "output_dir": str(out), "input_mask_dir": str(msk), "batch_size": 8, "tile_shape": 512, "chunk_shape": 1000,
                "ambiguous_size": 64}
        if flag:
            args["regions"] = {"dir": str(d)}
        assert mgr.process_wsi_list(args) == {"s": "done"}
        assert (out / "regions").exists() == flag
        text[out.name] = open(out / "s.json").read()
    assert text["out1x"] == text["out0"] and not (tmp_path / "out1x" / "regions" / "s.npz").exists()       # a missing file: byte-identical json, nothing written
    off, on = json.loads(text["out0"])["nuc"], json.loads(text["out1"])["nuc"]
    assert len(off) > 20 and {k: {f: v for f, v in e.items() if f != "region"} for k, e in on.items()} == off
    info = {int(k): {"centroid": np.array(e["centroid"]), "type": e["type"]} for k, e in off.items()}
    rc = _assert_counts(_load(tmp_path / "out1" / "regions" / "s.npz"), info, geo, 5)
    assert rc.count.shape == (3, 5) and [e["region"] for e in on.values()] == rc.first.tolist() and int(rc.hits.sum()) > 10
    with pytest.raises(ValueError):
        mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "regions": {"dir": str(ann), "scale": -1.0}})
    assert not (tmp_path / "bad").exists()

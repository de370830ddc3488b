"""-m gpu: density maps on the device (csrc/hvn_density.hip: HVN_OP_NBR_GRID + HVN_OP_NBR_DENSITY) against the all-pairs oracle
tests/density_ref.py with == on the integer raster, then the opt-in plumbing (whole slides, the two managers) against
`density.of_info` of the plain result on the host path.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import density_ref as R
from gpu_util import _maps, _tile_images, synth_net

pytestmark = pytest.mark.gpu

SLIDE_SPEC = {"radius": 40.0, "step": 16}
TILE_SPEC = {"radius": 60.0, "step": 8}


def _dn():
    from hover_net_amd import density as DN

    return DN


# -- 1: device == oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_oracle(name):
    """Every case of tests/density_ref.py.  `coarse` has blocks of nodes that span 80 grid rows, most of them skipped; `crowded` stages
    five tiles of one run; `outside` has nodes whose cells are clamped from far away; `widened` a grid of 2^22 cells for 520 points;
    `nine_types` runs the 16-column kernel with seven unused columns."""
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = _dn().density_device(*args)
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    R.assert_same(_dn().density(*args, device="cuda"), want, name)


@pytest.mark.parametrize("name", ["lattice", "outside", "fine", "coarse", "crowded", "ragged", "inexact_step", "sixteen_types"])
def test_same_bits_twice_and_in_reversed_order(name):
    """The order of the points inside a cell depends on atomic arrival; the raster may not, and it does not depend on the order of
    the points either: the reversed input gives the SAME array."""
    (xy, types, r, raster, t), want = R.case(name)
    DN = _dn()
    first, second = DN.density_device(xy, types, r, raster, t), DN.density_device(xy, types, r, raster, t)
    R.assert_same(first, want, name)
    R.assert_same(second, first, name)
    rxy = np.ascontiguousarray(xy[::-1])
    rtypes = None if types is None else np.ascontiguousarray(types[::-1])
    R.assert_same(DN.density_device(rxy, rtypes, r, raster, t), first, name)


@pytest.mark.parametrize("name", ["lattice", "outside", "coarse", "ragged", "nine_types"])
def test_the_op_writes_every_element(name):
    """`count` holds -7 everywhere before the op: the result is still the oracle's (nodes without any candidate included), and so is
    the result of the op run again on its own output."""
    args, want = R.case(name)
    q = _dn().DeviceDensity(*args)
    q.run_grid()
    q.count.fill_(-7)
    q.run_op()
    R.assert_same(q.result(), want, name)
    q.run_op()
    R.assert_same(q.result(), want, name)


@pytest.mark.parametrize("name", ["nine_types", "sixteen_types"])
def test_a_type_outside_the_range_is_counted_in_no_channel(name):
    """Below the Python layer (which refuses such types): the device tensor of types is overwritten before the ops run.  17 must not
    alias type 1, 33 neither (33 % 32 == 1), -1 no column at all; with T = 9 the kernel holds 16 columns, and a type in [9, 16) is
    counted in a column that is never stored."""
    (xy, types, r, raster, t), want = R.case(name)
    bad = types.copy()
    bad[::7] = 16
    bad[1::7] = 17
    bad[3::11] = -1
    bad[5::13] = 33
    if t < 16:
        bad[2::17] = 12
    q = _dn().DeviceDensity(xy, types, r, raster, t)
    q.types.copy_(torch.from_numpy(bad))
    q.run_grid()
    q.run_op()
    got = q.result()
    expect = R.density(xy, bad, r, raster, t)
    R.assert_same(got, expect, name)
    inside = (bad >= 0) & (bad < t)
    assert int(expect.sum()) < int(want.sum()) and 0 < int(inside.sum()) < bad.shape[0]
    R.assert_same(got, R.density(xy[inside], bad[inside], r, raster, t), name)       # as if those points were not there


def _slide_points(n, side, seed):
    """Slide-like centroids: 70 % uniform, 30 % in Gaussian clumps of 200 (sigma 40 px), five types."""
    rng = np.random.default_rng(seed)
    nu = n * 7 // 10
    centres = rng.random(((n - nu) // 200, 2)) * side
    clumps = np.repeat(centres, 200, 0) + rng.normal(0.0, 40.0, ((n - nu) // 200 * 200, 2))
    xy = np.concatenate([rng.random((n - clumps.shape[0], 2)) * side, np.clip(clumps, 0.0, side - 1.0)])
    return np.ascontiguousarray(xy[rng.permutation(n)]), rng.integers(0, 5, n).astype(np.int32)


def test_device_equals_host_path_at_slide_size():
    """200 000 points over 16384 x 16384 px, the pipeline raster at step 64 (256 x 256 nodes), r = 150, five types: too many pairs for
    the oracle, so the device is held to `density_host`, which tests/test_density_host.py holds to the oracle."""
    DN = _dn()
    xy, types = _slide_points(200000, 16384.0, 41)
    raster = DN.raster_of((16384, 16384), 64)
    assert (raster.W, raster.H, raster.ox, raster.s) == (256, 256, 31.5, 64.0)
    host = DN.density_host(xy, types, 150.0, raster, 5)
    dev = DN.density_device(xy, types, 150.0, raster, 5)
    R.assert_same(dev, host, "slide")
    assert int(host.sum()) > 2500000 and (host.reshape(5, -1).sum(1) > 400000).all()


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from hover_net_amd import infer_wsi
    from hover_net_amd import lib as L

    DN = _dn()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(L, "lib", no_launch)
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    ok = (0.0, 0.0, 1.0, 4, 3)
    with pytest.raises(ValueError):
        DN.density_device(np.array([[0.0, np.nan], [1.0, 1.0]]), None, 1.0, ok)
    with pytest.raises(TypeError):
        DN.density_device(xy.astype(np.float32), None, 1.0, ok)
    with pytest.raises(ValueError):
        DN.density_device(xy, np.array([0, 16], np.int32), 1.0, ok)
    with pytest.raises(ValueError):
        DN.density_device(xy, None, 0.0, ok)
    with pytest.raises(ValueError):
        DN.density_device(xy, None, 1.0, (0.0, 0.0, 0.0, 4, 3))
    with pytest.raises(ValueError):
        DN.density_device(xy, None, 1.0, (0.0, 0.0, 1.0, 16385, 3))
    with pytest.raises(ValueError):
        DN.density_device(xy, None, 1.0, (0.0, 0.0, 1.0, 16384, 16384), nr_types=2)
    with pytest.raises(ValueError):
        DN.density_device(xy, None, 1.0, (np.inf, 0.0, 1.0, 4, 3))
    with pytest.raises(TypeError):
        DN.density_device(xy, None, 1.0, (0.0, 0.0, 1.0, 4.5, 3))
    with pytest.raises(ValueError):
        DN.density_device(xy, None, 1.0, ok, device="cpu")
    with pytest.raises(ValueError):
        DN.of_info({1: {"centroid": [1.0, 1.0], "type": 0}}, (20, 24), -5.0, 4, 5, device="cuda")
    with pytest.raises(ValueError):
        infer_wsi.WsiInference(None, density={"radius": 5.0})
    with pytest.raises(TypeError):
        infer_wsi.WsiInference(None, density={"radius": 5.0, "step": 2.5})


# -- 2: the plumbing -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return synth_net()


def _assert_map(dm, info, size_hw, spec, nr_types):
    """dm is `of_info` of the dict on the HOST path, field by field."""
    DN = _dn()
    want = DN.of_info(info, size_hw, spec["radius"], spec["step"], nr_types, device=None)
    assert isinstance(dm, DN.DensityMap) and dm.origin == want.origin and dm.step == want.step == spec["step"] and dm.radius == want.radius == spec["radius"]
    R.assert_same(dm.count, want.count, "plumbing")
    return want


def test_wsi_density_crosses_tile_seams(net):
    """The small synthetic slide of tests/test_gpu_clusters.py (923 nuclei in 900 x 1000, tiles of 512): the map is made once from the
    merged dict, so a node near a seam counts nuclei of both tiles."""
    from golden_util import assert_same_info
    from hover_net_amd import infer_wsi

    maps = torch.from_numpy(_maps(900, 1000, 92)).to("cuda")
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    plain = infer_wsi.WsiInference(net, **kw)
    inst0, info0 = plain.stitch_instances(maps)
    assert plain.density is None and plain.points.density is None
    wsi = infer_wsi.WsiInference(net, density=SLIDE_SPEC, **kw)
    assert wsi.density is None                                   # nothing before the first slide
    inst1, info1 = wsi.stitch_instances(maps)
    np.testing.assert_array_equal(inst1, inst0)                  # the return value is unchanged
    assert_same_info(info1, info0)
    assert len(info1) == 923 and all(set(e) == set(info0[lab]) for lab, e in info1.items())
    dm = _assert_map(wsi.density, info1, (900, 1000), SLIDE_SPEC, 5)
    assert dm.count.shape == (5, 57, 63) and int(dm.count.sum()) > 923
    # a node whose disc crosses the seam x = 512 and holds nuclei on both sides of it
    xy = np.array([e["centroid"] for e in info1.values()], np.float64).reshape(-1, 2)
    step, r, (ox, oy) = dm.step, dm.radius, dm.origin
    found = 0
    for v in range(dm.count.shape[1]):
        for u in (31, 32):                                       # nodes at x = 503.5 and 519.5: within r of the seam
            d2 = (xy[:, 0] - (ox + u * step)) ** 2 + (xy[:, 1] - (oy + v * step)) ** 2
            left, right = int(((d2 <= r * r) & (xy[:, 0] < 512)).sum()), int(((d2 <= r * r) & (xy[:, 0] >= 512)).sum())
            if left and right:
                assert int(wsi.density.count[:, v, u].sum()) == left + right
                found += 1
    assert found >= 1


def test_process_file_list_density(net, tmp_path):
    from hover_net_amd import infer_manager, infer_tile

    images = _tile_images()
    inp = tmp_path / "in"
    inp.mkdir()
    for name, img in zip("ab", images):
        np.save(inp / (name + ".npy"), img)
    want = infer_tile.process_images(images, net, nr_types=5, batch_size=8)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    text = {}
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "batch_size": 8}
        if flag:
            args["density"] = dict(TILE_SPEC)
        assert mgr.process_file_list(args) == ["a", "b"]
        assert (out / "density").exists() == flag                # absent: no density/ directory
        for name, img, (_inst, info) in zip("ab", images, want):
            text[flag, name] = open(out / "json" / (name + ".json")).read()
            if flag:
                with np.load(out / "density" / (name + ".npz")) as z:
                    assert sorted(z.files) == ["count", "origin", "radius", "step"]
                    got = _dn().DensityMap(z["count"], tuple(z["origin"].tolist()), int(z["step"]), float(z["radius"]))
                dm = _assert_map(got, info, img.shape[:2], TILE_SPEC, 5)
                assert dm.count.shape == (5, -(-img.shape[0] // 8), -(-img.shape[1] // 8))
    assert int(_dn().of_info(want[0][1], images[0].shape[:2], 60.0, 8, 5).count.sum()) > 0       # the first image holds nuclei
    for name in "ab":
        assert text[True, name] == text[False, name]             # json/ is byte-identical with and without the argument
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "density": {"radius": 5.0}})
    with pytest.raises(TypeError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "density": {"radius": 5.0, "step": 1.5}})
    assert not (tmp_path / "bad").exists()


def test_wsi_manager_density(net, tmp_path, monkeypatch):
    """The manager's key down to density/<name>.npz; stage 1 is replaced by a structured prediction map, as tests/test_gpu_clusters.py
    does."""
    import json

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
            args["density"] = dict(SLIDE_SPEC)
        assert mgr.process_wsi_list(args) == {"s": "done"}
        assert (out / "density").exists() == flag
        text[flag] = open(out / "s.json").read()
    assert text[True] == text[False]                             # the json is byte-identical with and without the argument
    nuc = json.loads(text[False])["nuc"]
    assert len(nuc) > 20
    info = {int(k): {"centroid": np.array(e["centroid"]), "type": e["type"]} for k, e in nuc.items()}
    with np.load(tmp_path / "out1" / "density" / "s.npz") as z:
        got = _dn().DensityMap(z["count"], tuple(z["origin"].tolist()), int(z["step"]), float(z["radius"]))
    dm = _assert_map(got, info, (300, 340), SLIDE_SPEC, 5)
    assert dm.count.shape == (5, 19, 22) and int(dm.count.sum()) > len(nuc)
    with pytest.raises(ValueError):
        mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "density": {"step": 4}})
    assert not (tmp_path / "bad").exists()

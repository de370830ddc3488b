"""-m gpu: typed pair counts on the device (csrc/hvn_pairs.hip: HVN_OP_NBR_GRID + HVN_OP_NBR_PAIRS) against the all-pairs oracle
tests/ripley_ref.py and the host path with ==, the 64-bit sums against a closed form, then the opt-in plumbing (whole slides, the two
managers) against `ripley.of_info` of the plain result on the host path.  Integers only: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import ripley_ref as R
from gpu_util import _maps, _tile_images, synth_net

pytestmark = pytest.mark.gpu

SLIDE_SPEC = {"radii": [8.0, 16.0, 24.0, 40.0]}
TILE_SPEC = {"radii": [10.0, 20.0, 30.0], "window": (20.0, 20.0, 200.0, 220.0)}


def _rp():
    from hover_net_amd import ripley as RP

    return RP


# -- 1: device == host == oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_host_and_oracle(name):
    """Every case of tests/ripley_ref.py.  `crowded` stages five tiles of one run and puts every add on one bin; `widened` has a grid of
    2^22 cells for 520 points; `edge` and `outside` have lanes with m_i < R (two LDS adds per pair); `sixteen_types` fills the 4096 bins
    of the cap."""
    args, want = R.case(name)
    RP = _rp()
    got = RP.pairs_device(*args)
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    R.assert_same(RP.pairs_host(*args), want, name)
    R.assert_same(RP.pairs(*args, device="cuda"), want, name)


@pytest.mark.parametrize("name", ["lattice", "edge", "outside", "r32", "sixteen_types", "crowded"])
def test_same_bits_twice_and_in_reversed_order(name):
    """The order of the points inside a cell depends on atomic arrival, and so does the order of the adds; the sums may not, and they
    do not depend on the order of the points either."""
    (xy, types, radii, window, t), want = R.case(name)
    RP = _rp()
    first, second = RP.pairs_device(xy, types, radii, window, t), RP.pairs_device(xy, types, radii, window, t)
    R.assert_same(first, want, name)
    R.assert_same(second, first[:4], name)
    rxy = np.ascontiguousarray(xy[::-1])
    rtypes = None if types is None else np.ascontiguousarray(types[::-1])
    R.assert_same(RP.pairs_device(rxy, rtypes, radii, window, t), first[:4], name)


@pytest.mark.parametrize("name", ["lattice", "one_point", "outside", "nine_types"])
def test_the_op_writes_every_element(name):
    """`acc` holds -7 everywhere before the op: the result is still the oracle's (bins that no pair reaches included), and so is the
    result of the op run again on its own output."""
    args, want = R.case(name)
    q = _rp().DeviceRipley(*args)
    q.run_grid()
    q.acc.fill_(-7)
    q.run_op()
    R.assert_same(q.result(), want, name)
    q.run_op()
    R.assert_same(q.result(), want, name)


@pytest.mark.parametrize("name", ["nine_types", "sixteen_types"])
def test_a_type_outside_the_range_lands_in_no_bin(name):
    """Below the Python layer (which refuses such types): the device tensor of types is overwritten before the ops run.  17 must not
    alias type 1, 33 neither, -1 no row at all, as i or as j; with T = 9 a type in [9, 16) neither."""
    (xy, types, radii, window, t), want = R.case(name)
    bad = types.copy()
    bad[::7] = 16
    bad[1::7] = 17
    bad[3::11] = -1
    bad[5::13] = 33
    if t < 16:
        bad[2::17] = 12
    q = _rp().DeviceRipley(xy, types, radii, window, t)
    q.types.copy_(torch.from_numpy(bad))
    q.run_grid()
    q.run_op()
    got = q.result()
    expect = R.pairs(xy, bad, radii, window, t)
    inside = (bad >= 0) & (bad < t)
    assert int(expect[0].sum()) < int(want[0].sum()) and 0 < int(inside.sum()) < bad.shape[0]
    for g, w in zip(got[:2], expect[:2]):                       # n and n_in are the host's, from the types the Python layer was given
        assert g.dtype == np.int64 and (g == w).all(), name
    alone = R.pairs(xy[inside], bad[inside], radii, window, t)  # as if those points were not there
    assert (got.pairs == alone[0]).all() and (got.pairs_in == alone[1]).all()


# -- 2: 64-bit accumulation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 2])
def test_coincident_points_pass_2_to_the_32(nt):
    """70 000 points on one spot: N (N - 1) = 4 899 930 000 ordered pairs, all with d2 = 0 and hence in bin 0, above 2^32 -- held to
    the closed form only (`pairs_host` is not run: 5 10^9 candidate tests).  A workgroup walks 69 staging tiles here, so its LDS
    histogram is flushed twice on the way.  With two types alternating, type a has 35 000 points: 35 000 x 34 999 pairs (a, a) and
    35 000^2 pairs (a, b).  The window puts the spot 3 inside: in at r = 2, out at r = 5."""
    n = 70000
    assert n * (n - 1) == 4899930000 > 2 ** 32
    xy = np.tile([[40.0, 3.0]], (n, 1))
    types = None if nt == 1 else (np.arange(n) % 2).astype(np.int32)
    got = _rp().pairs_device(xy, types, (2.0, 5.0), (0.0, 0.0, 100.0, 50.0), None if nt == 1 else 2)
    half = n // 2
    want = np.array([[n * (n - 1)]]) if nt == 1 else np.array([[half * (half - 1), half * half], [half * half, half * (half - 1)]])
    assert got.pairs.dtype == np.int64 and (got.pairs == want[:, :, None]).all(), got.pairs.tolist()
    assert (got.pairs_in[:, :, 0] == want).all() and not got.pairs_in[:, :, 1].any(), got.pairs_in.tolist()
    assert got.n.tolist() == [n // nt] * nt and got.n_in.tolist() == [[n // nt, 0]] * nt


# -- 3: scale -----------------------------------------------------------------------------------------------------
def _slide_points(n, side, seed):
    """Slide-like centroids: 70 % uniform, 30 % in Gaussian clumps of 200 (sigma 40 px), five types."""
    rng = np.random.default_rng(seed)
    nu = n * 7 // 10
    centres = rng.random(((n - nu) // 200, 2)) * side
    clumps = np.repeat(centres, 200, 0) + rng.normal(0.0, 40.0, ((n - nu) // 200 * 200, 2))
    xy = np.concatenate([rng.random((n - clumps.shape[0], 2)) * side, np.clip(clumps, 0.0, side - 1.0)])
    return np.ascontiguousarray(xy[rng.permutation(n)]), rng.integers(0, 5, n).astype(np.int32)


def test_device_equals_host_path_at_slide_size():
    """200 000 points over 16384 x 16384 px, 16 radii up to 100 px, five types, the window of the image: too many pairs for the oracle,
    so the device is held to `pairs_host`, which tests/test_ripley_host.py holds to the oracle."""
    RP = _rp()
    xy, types = _slide_points(200000, 16384.0, 43)
    radii = [6.25 * (k + 1) for k in range(16)]
    window = RP.window_of((16384, 16384))
    host = RP.pairs_host(xy, types, radii, window, 5)
    dev = RP.pairs_device(xy, types, radii, window, 5)
    R.assert_same(dev, host[:4], "slide")
    assert int(host.pairs[:, :, -1].sum()) > 4000000 and (host.pairs[:, :, -1] > 100000).all()
    assert 0 < int(host.pairs_in[:, :, -1].sum()) < int(host.pairs[:, :, -1].sum()) and (host.n_in[:, -1] < host.n).all()


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from hover_net_amd import infer_wsi
    from hover_net_amd import lib as L

    RP = _rp()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(L, "lib", no_launch)
    xy = np.array([[0.0, 0.0], [1.0, 1.0]])
    ok = (0.0, 0.0, 4.0, 3.0)
    for args, exc in (((np.array([[0.0, np.nan], [1.0, 1.0]]), None, (1.0,), ok), ValueError), ((xy.astype(np.float32), None, (1.0,), ok), TypeError),
                      ((xy, np.array([0, 16], np.int32), (1.0,), ok), ValueError), ((xy, None, (), ok), ValueError), ((xy, None, (2.0, 1.0), ok), ValueError),
                      ((xy, None, (1.0,), (0.0, 0.0, 0.0, 3.0)), ValueError), ((xy, None, 1.0, ok), TypeError), ((xy, None, (1.0,), (0.0, 0.0, 4.0)), TypeError)):
        with pytest.raises(exc):
            RP.pairs_device(*args)
    with pytest.raises(ValueError):
        RP.pairs_device(xy, None, (1.0,), ok, device="cpu")
    with pytest.raises(ValueError):
        infer_wsi.WsiInference(None, ripley={"radius": 5.0})
    with pytest.raises(TypeError):
        infer_wsi.WsiInference(None, ripley={"radii": [5.0, "6"]})


# -- 4: the plumbing ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return synth_net()


def _assert_counts(pc, info, size_hw, spec, nr_types):
    """pc is `of_info` of the dict on the HOST path, field by field."""
    RP = _rp()
    want = RP.of_info(info, size_hw, spec["radii"], nr_types, device=None, window=spec.get("window"))
    assert isinstance(pc, RP.PairCounts) and tuple(pc.window) == tuple(want.window) and list(pc.radii) == list(want.radii) == list(spec["radii"])
    R.assert_same(pc, want[:4], "plumbing")
    return want


def _load(path):
    with np.load(path) as z:
        assert sorted(z.files) == ["n", "n_in", "pairs", "pairs_in", "radii", "window"]
        return _rp().PairCounts(z["pairs"], z["pairs_in"], z["n"], z["n_in"], z["radii"], tuple(z["window"].tolist()))


def test_wsi_ripley_crosses_tile_seams(net):
    """The small synthetic slide of tests/test_gpu_clusters.py (923 nuclei in 900 x 1000, tiles of 512): the counts are made once from
    the merged dict, so a pair whose nuclei lie either side of the seam x = 512 is counted."""
    from golden_util import assert_same_info
    from hover_net_amd import infer_wsi

    RP = _rp()
    maps = torch.from_numpy(_maps(900, 1000, 92)).to("cuda")
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    plain = infer_wsi.WsiInference(net, **kw)
    inst0, info0 = plain.stitch_instances(maps)
    assert plain.ripley is None and plain.points.ripley is None
    wsi = infer_wsi.WsiInference(net, ripley=SLIDE_SPEC, **kw)
    assert wsi.ripley is None                                    # nothing before the first slide
    inst1, info1 = wsi.stitch_instances(maps)
    np.testing.assert_array_equal(inst1, inst0)                  # the return value is unchanged
    assert_same_info(info1, info0)
    assert len(info1) == 923 and all(set(e) == set(info0[lab]) for lab, e in info1.items())
    pc = _assert_counts(wsi.ripley, info1, (900, 1000), SLIDE_SPEC, 5)
    assert tuple(pc.window) == (-0.5, -0.5, 999.5, 899.5) and int(pc.n.sum()) == 923 and int(pc.pairs[:, :, -1].sum()) > 923
    # pairs across the seam: the counts of the whole exceed those of the two sides taken alone by exactly the pairs that cross it
    xy = np.array([e["centroid"] for e in info1.values()], np.float64).reshape(-1, 2)
    dx, dy = xy[None, :, 0] - xy[:, None, 0], xy[None, :, 1] - xy[:, None, 1]
    left = xy[:, 0] < 512
    crossing = int((((dx * dx) + (dy * dy) <= 40.0 * 40.0) & (left[:, None] != left[None, :])).sum())
    sides = [RP.of_info({lab: e for lab, e in info1.items() if (e["centroid"][0] < 512) == side}, (900, 1000), SLIDE_SPEC["radii"], 5) for side in (True, False)]
    assert crossing >= 2 and int(wsi.ripley.pairs[:, :, -1].sum()) == sum(int(s.pairs[:, :, -1].sum()) for s in sides) + crossing


def test_process_file_list_ripley(net, tmp_path):
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
            args["ripley"] = dict(TILE_SPEC)
        assert mgr.process_file_list(args) == ["a", "b"]
        assert (out / "ripley").exists() == flag                 # absent: no ripley/ directory
        for name, img, (_inst, info) in zip("ab", images, want):
            text[flag, name] = open(out / "json" / (name + ".json")).read()
            if flag:
                pc = _assert_counts(_load(out / "ripley" / (name + ".npz")), info, img.shape[:2], TILE_SPEC, 5)
                assert pc.pairs.shape == (5, 5, 3) and tuple(pc.window) == TILE_SPEC["window"]
    assert int(_rp().of_info(want[0][1], images[0].shape[:2], TILE_SPEC["radii"], 5).pairs.sum()) > 0        # the first image holds pairs
    for name in "ab":
        assert text[True, name] == text[False, name]             # json/ is byte-identical with and without the argument
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "ripley": {"radius": 5.0}})
    with pytest.raises(TypeError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "ripley": {"radii": 5.0}})
    assert not (tmp_path / "bad").exists()


def test_wsi_manager_ripley(net, tmp_path, monkeypatch):
    """The manager's key down to ripley/<name>.npz; stage 1 is replaced by a structured prediction map, as tests/test_gpu_clusters.py
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
            args["ripley"] = dict(SLIDE_SPEC)
        assert mgr.process_wsi_list(args) == {"s": "done"}
        assert (out / "ripley").exists() == flag
        text[flag] = open(out / "s.json").read()
    assert text[True] == text[False]                             # the json is byte-identical with and without the argument
    nuc = json.loads(text[False])["nuc"]
    assert len(nuc) > 20
    info = {int(k): {"centroid": np.array(e["centroid"]), "type": e["type"]} for k, e in nuc.items()}
    pc = _assert_counts(_load(tmp_path / "out1" / "ripley" / "s.npz"), info, (300, 340), SLIDE_SPEC, 5)
    assert pc.pairs.shape == (5, 5, 4) and int(pc.n.sum()) == len(nuc) and int(pc.pairs[:, :, -1].sum()) > 0
    with pytest.raises(ValueError):
        mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "ripley": {"radii": []}})
    assert not (tmp_path / "bad").exists()

"""-m gpu: the random-labelling test on the device (csrc/hvn_pairs_sim.hip: HVN_OP_NBR_GRID + HVN_OP_NBR_PAIRS + HVN_OP_NBR_PAIRS_SIM per
batch) against the oracle tests/ripley_sims_ref.py and the host path with ==, across batch seams, the 64-bit sums against a closed form,
then the opt-in plumbing (whole slides, the two managers) against `ripley.of_info` on the host path.  Integers only: no tolerance."""
import numpy as np
import pytest
import torch

import ripley_ref as R
import ripley_sims_ref as SR
from gpu_util import _maps, _tile_images, synth_net

pytestmark = pytest.mark.gpu

SLIDE_SPEC = {"radii": [8.0, 16.0, 24.0, 40.0], "sims": 9, "seed": 1}
TILE_SPEC = {"radii": [10.0, 20.0, 30.0], "window": (20.0, 20.0, 200.0, 220.0), "sims": 9, "seed": 1}
OLD_KEYS = ["n", "n_in", "pairs", "pairs_in", "radii", "window"]


def _rp():
    from hover_net_amd import ripley as RP

    return RP


def _assert_equal(got, want, what):
    """Two LabelSims, field by field."""
    R.assert_same(got.observed, want.observed[:4], what)
    SR.assert_same(got, (want.pairs_in, want.n_in), what)
    assert got.seed == want.seed


# -- 1: device == host == oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_host_and_oracle(name):
    """Every case of tests/ripley_ref.py at S = 5, one batch.  `crowded` stages five tiles of one run with every add on one bin per
    simulation; `edge` and `outside` have lanes with m_i < R (two LDS adds per pair and simulation); `sixteen_types` fills the 4096 bins
    of the cap, where the LDS holds 8 simulations."""
    args, want = SR.case(name, 5)
    _, obs = R.case(name)
    RP = _rp()
    got = RP.sims_device(*args, sims=5)
    assert isinstance(got, RP.LabelSims) and got.seed == 0
    R.assert_same(got.observed, obs, name)
    SR.assert_same(got, want, name)
    SR.assert_same(RP.sims_host(*args, sims=5), want, name)
    SR.assert_same(RP.sims(*args, sims=5, device="cuda"), want, name)


@pytest.mark.parametrize("sb", [1, 3])
@pytest.mark.parametrize("name", list(R.CASES))
def test_batch_seams(name, sb, monkeypatch):
    """S = 7 in batches of 1 (SB = 1, seven launches) and of 3 (3 + 3 + 1: the last batch is short, and a label word holds three
    simulations and a padding byte)."""
    args, want = SR.case(name, 7)
    RP = _rp()
    monkeypatch.setattr(RP, "_BATCH", sb)
    q = RP.DeviceRipleySims(*args, sims=7)
    assert q.sb == sb and q.batches == (7 + sb - 1) // sb
    SR.assert_same(q.run().result(), want, name)


@pytest.mark.parametrize("n", [1, 2, 65, 257, 1025])
def test_small_and_odd_sizes(n):
    """N = 1 (b = 2: three of four values lie outside [0, N)), 2, and one past a wave, a workgroup and a power of two; four types."""
    rng = np.random.default_rng(100 + n)
    xy = rng.random((n, 2)) * 30.0
    types = rng.integers(0, 4, n).astype(np.int32)
    radii, window = (1.0, 2.5, 4.0), (1.0, 1.0, 29.0, 29.0)
    got = _rp().sims_device(xy, types, radii, window, 4, sims=5, seed=n)
    SR.assert_same(got, SR.sims(xy, types, radii, window, 4, 5, n), "n = %d" % n)
    R.assert_same(got.observed, R.pairs(xy, types, radii, window, 4), "n = %d" % n)
    assert n < 65 or int(got.pairs_in.sum()) > 0


def test_sixteen_types_in_batches_of_eight(monkeypatch):
    """4096 bins: asked for batches of 32, the LDS holds 8 simulations, so S = 11 is a full batch and a short one; held to the host
    path."""
    args, _ = R.case("sixteen_types")
    RP = _rp()
    monkeypatch.setattr(RP, "_BATCH", 32)
    q = RP.DeviceRipleySims(*args, sims=11, seed=3)
    assert q.sb == 8 and q.batches == 2
    _assert_equal(q.run().result(), RP.sims_host(*args, sims=11, seed=3), "sixteen_types")


@pytest.mark.parametrize("name", ["edge", "untyped"])
def test_the_largest_batch(name, monkeypatch):
    """SB = 32, eight label words per point, then a batch of one: S = 33."""
    args, _ = R.case(name)
    RP = _rp()
    monkeypatch.setattr(RP, "_BATCH", 32)
    q = RP.DeviceRipleySims(*args, sims=33, seed=4)
    assert q.sb == 32 and q.batches == 2
    _assert_equal(q.run().result(), RP.sims_host(*args, sims=33, seed=4), name)


@pytest.mark.parametrize("name", ["lattice", "one_point", "outside", "nine_types"])
def test_the_op_writes_every_element(name):
    """`out` holds -7 everywhere before the ops: the result is still the oracle's, and so is that of every batch run again on its own
    output."""
    args, want = SR.case(name, 7)
    RP = _rp()
    q = RP.DeviceRipleySims(*args, sims=7)
    assert q.batches == 1
    q.run_grid()
    q.out.fill_(-7)
    q.acc.fill_(-7)
    q.labels.fill_(0x01010101)
    q.run_observed()
    q.run_op(0)
    SR.assert_same(q.result(), want, name)
    q.run_op(0)
    SR.assert_same(q.result(), want, name)


@pytest.mark.parametrize("name", ["lattice", "edge", "r32", "crowded"])
def test_same_bits_twice(name):
    """The order of the points inside a cell depends on atomic arrival, and so does the order of the adds; the sums may not."""
    args, want = SR.case(name, 5)
    RP = _rp()
    first, second = RP.sims_device(*args, sims=5), RP.sims_device(*args, sims=5)
    SR.assert_same(first, want, name)
    _assert_equal(second, first, name)


@pytest.mark.parametrize("name", ["nine_types", "sixteen_types"])
def test_a_type_outside_the_range_lands_in_no_bin(name):
    """Below the Python layer (which refuses such types): the device tensor of types is overwritten before the ops run.  17 must not
    alias type 1, 33 neither, -1 no row at all, as i or as j, wherever the permutation puts them; with T = 9 a type in [9, 16) neither.
    cnt comes from the device too, so n_in is the oracle's on those labels."""
    (xy, types, radii, window, t), _ = R.case(name)
    bad = types.copy()
    bad[::7] = 16
    bad[1::7] = 17
    bad[3::11] = -1
    bad[5::13] = 33
    if t < 16:
        bad[2::17] = 12
    q = _rp().DeviceRipleySims(xy, types, radii, window, t, sims=4, seed=8)
    q.types.copy_(torch.from_numpy(bad))
    got = q.run().result()
    expect = SR.sims(xy, bad, radii, window, t, 4, 8)
    assert int(expect[0].sum()) < int(_rp().sims_host(xy, types, radii, window, t, sims=4, seed=8).pairs_in.sum())
    SR.assert_same(got, expect, name)


# -- 2: 64-bit accumulation ---------------------------------------------------------------------------------------
def test_coincident_points_pass_the_flush():
    """70 000 points of two alternating types on one spot, S = 2: every ordered pair has d2 = 0, so the counts do not depend on the
    labelling and every simulation equals the closed form: 35 000 x 34 999 pairs (a, a) and 35 000^2 pairs (a, b) at r = 2, where the
    spot is inside the window, and none at r = 5, where it is not.  A workgroup walks 69 staging tiles here, so the two planes of its LDS
    histogram are flushed twice on the way: each count is more than a hundred times the 2^23 that a word of it may hold."""
    n, h = 70000, 35000
    xy = np.tile([[40.0, 3.0]], (n, 1))
    types = (np.arange(n) % 2).astype(np.int32)
    got = _rp().sims_device(xy, types, (2.0, 5.0), (0.0, 0.0, 100.0, 50.0), 2, sims=2)
    want = np.array([[h * (h - 1), h * h], [h * h, h * (h - 1)]])
    assert got.pairs_in.dtype == np.int64 and got.pairs_in.shape == (2, 2, 2, 2)
    for s in range(2):
        assert (got.pairs_in[s, :, :, 0] == want).all() and not got.pairs_in[s, :, :, 1].any(), got.pairs_in[s].tolist()
        assert got.n_in[s].tolist() == [[h, 0], [h, 0]]
    assert (got.observed.pairs_in[:, :, 0] == want).all() and h * (h - 1) > 100 * 2 ** 23


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
    """50 000 points over 8192 x 8192 px (the density of tests/test_gpu_ripley.py's slide), 16 radii up to 100 px, five types, S = 4:
    too many pairs for the oracle, so the device is held to `sims_host`, which tests/test_ripley_sims_host.py holds to the oracle."""
    RP = _rp()
    xy, types = _slide_points(50000, 8192.0, 43)
    radii = [6.25 * (k + 1) for k in range(16)]
    window = RP.window_of((8192, 8192))
    host = RP.sims_host(xy, types, radii, window, 5, sims=4, seed=6)
    _assert_equal(RP.sims_device(xy, types, radii, window, 5, sims=4, seed=6), host, "slide")
    assert int(host.pairs_in[0, :, :, -1].sum()) > 500000 and (host.pairs_in[:, :, :, -1] > 10000).all()
    assert len({a.tobytes() for a in host.pairs_in}) == 4 and (host.n_in[:, :, -1] < host.observed.n[None]).all()


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from hover_net_amd import infer_wsi
    from hover_net_amd import lib as L

    RP = _rp()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(L, "lib", no_launch)
    xy, ok = np.array([[0.0, 0.0], [1.0, 1.0]]), (0.0, 0.0, 4.0, 3.0)
    for kw, exc in ((dict(sims=0), ValueError), (dict(sims=10000), ValueError), (dict(sims=3, seed=-1), ValueError), (dict(sims=3.0), TypeError), (dict(), TypeError)):
        with pytest.raises(exc):
            RP.sims_device(xy, None, (1.0,), ok, **kw)
    with pytest.raises(ValueError):
        RP.sims_device(xy, None, (1.0,), ok, sims=3, device="cpu")
    with pytest.raises(ValueError):
        infer_wsi.WsiInference(None, ripley={"radii": [5.0], "seed": 3})
    with pytest.raises(TypeError):
        infer_wsi.WsiInference(None, ripley={"radii": [5.0], "sims": "9"})


# -- 4: the plumbing ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return synth_net()


def _assert_sims(ls, info, size_hw, spec, nr_types):
    """ls is `of_info` of the dict on the HOST path, field by field."""
    RP = _rp()
    want = RP.of_info(info, size_hw, spec["radii"], nr_types, device=None, window=spec.get("window"), sims=spec["sims"], seed=spec["seed"])
    assert isinstance(ls, RP.LabelSims) and ls.pairs_in.shape[0] == spec["sims"] and list(ls.observed.radii) == list(spec["radii"])
    _assert_equal(ls, want, "plumbing")
    return want


def _load(path):
    RP = _rp()
    with np.load(path) as z:
        assert sorted(z.files) == sorted(OLD_KEYS + ["seed", "sim_n_in", "sim_pairs_in"])
        return RP.LabelSims(RP.PairCounts(z["pairs"], z["pairs_in"], z["n"], z["n_in"], z["radii"], tuple(z["window"].tolist())), z["sim_pairs_in"], z["sim_n_in"],
                            int(z["seed"]))


def test_wsi_ripley_sims(net):
    """The small synthetic slide of tests/test_gpu_ripley.py: `self.ripley` is the LabelSims of the merged dict, and without "sims" the
    PairCounts it was before, equal to the observed part."""
    from hover_net_amd import infer_wsi

    RP = _rp()
    maps = torch.from_numpy(_maps(900, 1000, 92)).to("cuda")
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    plain = infer_wsi.WsiInference(net, ripley={"radii": SLIDE_SPEC["radii"]}, **kw)
    plain.stitch_instances(maps)
    wsi = infer_wsi.WsiInference(net, ripley=SLIDE_SPEC, **kw)
    assert wsi.ripley is None and wsi.points.ripley == (tuple(SLIDE_SPEC["radii"]), None, 9, 1)
    _inst, info = wsi.stitch_instances(maps)
    want = _assert_sims(wsi.ripley, info, (900, 1000), SLIDE_SPEC, 5)
    assert isinstance(plain.ripley, RP.PairCounts) and len(info) == 923
    R.assert_same(plain.ripley, want.observed[:4], "without sims")
    assert len({a.tobytes() for a in want.pairs_in}) == 9


def test_process_file_list_ripley_sims(net, tmp_path):
    from hover_net_amd import infer_manager, infer_tile

    images = _tile_images()
    inp = tmp_path / "in"
    inp.mkdir()
    for name, img in zip("ab", images):
        np.save(inp / (name + ".npy"), img)
    want = infer_tile.process_images(images, net, nr_types=5, batch_size=8)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        spec = dict(TILE_SPEC) if flag else {k: v for k, v in TILE_SPEC.items() if k not in ("sims", "seed")}
        assert mgr.process_file_list({"input_dir": str(inp), "output_dir": str(out), "batch_size": 8, "ripley": spec}) == ["a", "b"]
    for name, img, (_inst, info) in zip("ab", images, want):
        ls = _assert_sims(_load(tmp_path / "out1" / "ripley" / (name + ".npz")), info, img.shape[:2], TILE_SPEC, 5)
        with np.load(tmp_path / "out0" / "ripley" / (name + ".npz")) as z:          # without "sims": exactly the six old keys, equal arrays
            assert sorted(z.files) == OLD_KEYS
            assert all((z[k] == np.asarray(getattr(ls.observed, k))).all() for k in OLD_KEYS)
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "ripley": {"radii": [5.0], "sims": 0}})
    assert not (tmp_path / "bad").exists()


def test_wsi_manager_ripley_sims(net, tmp_path, monkeypatch):
    """The manager's key down to ripley/<name>.npz; stage 1 is replaced by a structured prediction map, as tests/test_gpu_ripley.py
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
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        spec = dict(SLIDE_SPEC) if flag else {"radii": SLIDE_SPEC["radii"]}
        args = {"input_dir": str(inp), "output_dir": str(out), "input_mask_dir": str(msk), "batch_size": 8, "tile_shape": 512, "chunk_shape": 1000,
                "ambiguous_size": 64, "ripley": spec}
        assert mgr.process_wsi_list(args) == {"s": "done"}
    assert open(tmp_path / "out1" / "s.json").read() == open(tmp_path / "out0" / "s.json").read()
    nuc = json.loads(open(tmp_path / "out1" / "s.json").read())["nuc"]
    info = {int(k): {"centroid": np.array(e["centroid"]), "type": e["type"]} for k, e in nuc.items()}
    ls = _assert_sims(_load(tmp_path / "out1" / "ripley" / "s.npz"), info, (300, 340), SLIDE_SPEC, 5)
    assert len(nuc) > 20 and ls.pairs_in.shape == (9, 5, 5, 4)
    with np.load(tmp_path / "out0" / "ripley" / "s.npz") as z:
        assert sorted(z.files) == OLD_KEYS and all((z[k] == np.asarray(getattr(ls.observed, k))).all() for k in OLD_KEYS)

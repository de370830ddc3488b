"""-m gpu: test-time augmentation on the device (csrc/hvn_tta.hip, Engine.run_tta) against the numpy oracle tests/tta_ref.py.

Contracts: HVN_OP_VIEW equals numpy; the hv channels of HVN_OP_TTA equal the same fp32 sum bit for bit; the np channel
and the type probabilities stay within four times the float32 oracle's own error against float64 (the factor is for the device's
expf), never above 1e-5; one view (0,) gives PREDMAP's np and hv bits; `run_tta` is the plain network pass per view."""
import ctypes

import numpy as np
import pytest
import torch

import tta_ref as R

pytestmark = pytest.mark.gpu
OP_PREDMAP, OP_VIEW, OP_TTA = 5, 9, 10
SETS = {"d4": tuple(range(8)), "rot": (0, 1, 2, 3), "flips": (0, 4, 6, 2)}


def _run(op, n):
    from hover_net_amd import lib as L

    rc = L.lib().hvn_run_op(ctypes.addressof(op), n, L.stream_ptr("cuda"))
    return rc, L.lib().hvn_last_error()


def _view_op(x, y, k, h=None, w=None):
    from hover_net_amd import lib as L

    op = L.hvn_op()
    op.kind, op._rsv = OP_VIEW, k
    op.x.base, op.y.base = x.data_ptr(), y.data_ptr()
    for v in (op.x, op.y):
        v.h, v.w, v.c = (x.shape[1] if h is None else h), (x.shape[2] if w is None else w), 3
    return op


# ---- VIEW ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(35, 35), (19, 35)])
def test_view_equals_numpy(shape):
    """35 is odd and more than one 32-wide tile; 19 x 35 runs the views that do not transpose on a non-square patch.  The output
    lies inside a larger buffer whose other bytes must stay untouched."""
    h, w = shape
    n = 3
    a = np.random.default_rng(11).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    x = torch.from_numpy(a).to("cuda")
    for k in range(8):
        if k & 1 and h != w:
            continue
        guard = torch.full((n * h * w * 3 + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        y = guard[256:256 + n * h * w * 3].view(n, h, w, 3) if not k & 1 else guard[256:256 + n * h * w * 3].view(n, w, h, 3)
        rc, err = _run(_view_op(x, y, k, h, w), n)
        assert rc == 0, err
        want = np.stack([R.view(s, k) for s in a])
        assert (y.cpu().numpy() == want).all(), k
        g = guard.cpu().numpy()
        assert (g[:256] == 0xA5).all() and (g[-256:] == 0xA5).all(), k


def test_view_refusals():
    x = torch.zeros((2, 20, 20, 3), dtype=torch.uint8, device="cuda")
    y = torch.zeros_like(x)
    assert _run(_view_op(x, y, 3), 2)[0] == 0
    for k in (8, -1, 12):
        rc, err = _run(_view_op(x, y, k), 2)
        assert rc == -1 and b"view" in err
    assert _run(_view_op(x, y, 1, 20, 18), 2)[0] == -1          # a quarter turn of a non-square patch
    assert _run(_view_op(x, y, 3, 18, 20), 2)[0] == -1
    assert _run(_view_op(x, y, 2, 20, 18), 2)[0] == 0           # a half turn of one is fine
    op = _view_op(x, y, 0)
    op.y.h = 19
    assert _run(op, 2)[0] == -1                                 # different extents
    op = _view_op(x, y, 0)
    op.y.c = 4
    assert _run(op, 2)[0] == -1
    assert _run(_view_op(x, x, 0), 2)[0] == -1                  # in place
    op = _view_op(x, y, 0)
    op.x_dtype = 1
    assert _run(op, 2)[0] == -1                                 # float input: HoVerNet.forward's contract gets no TTA
    op = _view_op(x, y, 0)
    op.y.base = None
    assert _run(op, 2)[0] == -1


# ---- TTA on given logits ---------------------------------------------------------------------
def _tta_op(lg, acc, y, k, first, last, K, T, h, w):
    from hover_net_amd import lib as L

    op = L.hvn_op()
    op.kind, op._rsv, op.kh, op.kw, op.stride, op.cout = OP_TTA, k, int(first), int(last), K, T
    op.x.base, op.res.base = lg["np"].data_ptr(), lg["hv"].data_ptr()
    op.w = lg["tp"].data_ptr() if T else None
    op.y2.base = None if acc is None else acc.data_ptr()
    op.y.base = None if y is None else y.data_ptr()
    op.y.h, op.y.w, op.y.c = h, w, 4 if T else 3
    return op


def _reduce_device(per_view, views, T, n, h, w):
    """HVN_OP_TTA over device logits, one call per view in order -> (y [n,h,w,3|4], acc [n,h,w,3+T]) numpy."""
    acc = torch.full((n, h, w, 3 + T), float("nan"), dtype=torch.float32, device="cuda")
    y = torch.full((n, h, w, 4 if T else 3), float("nan"), dtype=torch.float32, device="cuda")
    for i, (lg, k) in enumerate(zip(per_view, views)):
        rc, err = _run(_tta_op(lg, acc, y, k, i == 0, i == len(views) - 1, len(views), T, h, w), n)
        assert rc == 0, err
    return y.cpu().numpy(), acc.cpu().numpy()


def _random_logits(views, T, n, h, w, seed):
    rng = np.random.default_rng(seed)
    per = []
    for k in views:
        hv_, wv_ = (w, h) if k & 1 else (h, w)
        d = {"np": (3 * rng.standard_normal((n, 2, hv_, wv_))).astype(np.float32), "hv": (3 * rng.standard_normal((n, 2, hv_, wv_))).astype(np.float32)}
        if T:
            d["tp"] = (3 * rng.standard_normal((n, T, hv_, wv_))).astype(np.float32)
        per.append(d)
    return per


def _check_against_oracle(y, acc, per, views, T, what):
    """The checks of one reduction: hv bit-equal to the fp32 oracle; np and the type probabilities within 4 x the fp32 oracle's own
    error against float64 (<= 1e-5); the type where the float64 top-two gap is at least 1e-4."""
    r32, r64 = R.reduce_f32(per, views), R.reduce_f64(per, views)
    c0 = 1 if T else 0
    assert (y[..., c0 + 1:c0 + 3] == r32["hv"]).all(), what
    assert (acc[..., 1:3] == r32["acc_hv"]).all(), what
    own = np.abs(r32["np"] - r64["np"]).max()
    got = np.abs(y[..., c0].astype(np.float64) - r64["np"]).max()
    if T:
        own = max(own, np.abs(r32["tp"] - r64["tp"]).max())
        got = max(got, np.abs(acc[..., 3:].astype(np.float64) / len(views) - r64["tp"]).max())
    bound = min(4.0 * own, 1e-5)
    print("%s: device error vs float64 %.3g, float32 oracle's own %.3g, bound %.3g" % (what, got, own, bound))
    assert got <= bound, (what, got, bound)
    if T:
        sure = R.top2_gap(r64["tp"]) >= 1e-4
        assert (~sure).mean() < 0.01, what
        assert (y[..., 0][sure] == r64["type"][sure]).all(), what
        assert ((y[..., 0] >= 0) & (y[..., 0] < T) & (y[..., 0] == np.round(y[..., 0]))).all()


CASES = [(33, 33, v) for v in ("d4", "rot", "flips", (5,), (3, 6, 1))] + [(19, 35, "flips")]


@pytest.mark.parametrize("T", [5, 0])
@pytest.mark.parametrize("h,w,views", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_tta_on_given_logits(h, w, views, T):
    n = 3
    ids = SETS.get(views, views)
    per = _random_logits(ids, T, n, h, w, seed=100 + 8 * len(ids) + T)
    dev = [{b: torch.from_numpy(a).to("cuda") for b, a in d.items()} for d in per]
    y, acc = _reduce_device(dev, ids, T, n, h, w)
    assert np.isfinite(y).all() and np.isfinite(acc).all()      # every element of both buffers was written
    _check_against_oracle(y, acc, per, ids, T, "%dx%d %s T=%d" % (h, w, views, T))


@pytest.mark.parametrize("T", [5, 0])
def test_single_identity_view_is_predmap(T):
    """(0,): the np and hv channels are PREDMAP's bits; the type (argmax of the probabilities, not of the logits) differs only on
    near-ties, below the project's own figure of 2e-3."""
    from hover_net_amd import lib as L

    n, h, w = 3, 33, 33
    per = _random_logits((0,), T, n, h, w, seed=7)
    dev = [{b: torch.from_numpy(a).to("cuda") for b, a in d.items()} for d in per]
    y, _ = _reduce_device(dev, (0,), T, n, h, w)
    pm = torch.full((n, h, w, 4 if T else 3), float("nan"), dtype=torch.float32, device="cuda")
    op = L.hvn_op()
    op.kind, op.cout = OP_PREDMAP, T
    op.x.base, op.res.base, op.w = dev[0]["np"].data_ptr(), dev[0]["hv"].data_ptr(), (dev[0]["tp"].data_ptr() if T else None)
    op.y.base = pm.data_ptr()
    op.y.h, op.y.w, op.y.c = h, w, 4 if T else 3
    rc, err = _run(op, n)
    assert rc == 0, err
    pm = pm.cpu().numpy()
    c0 = 1 if T else 0
    assert (y[..., c0:].view(np.uint32) == pm[..., c0:].view(np.uint32)).all()
    if T:
        assert (y[..., 0] != pm[..., 0]).mean() < 2e-3


def test_tta_refusals():
    n, h, w, T = 2, 12, 12, 5
    lg = {"np": torch.zeros((n, 2, h, w), device="cuda"), "hv": torch.zeros((n, 2, h, w), device="cuda"), "tp": torch.zeros((n, T, h, w), device="cuda")}
    acc = torch.zeros((n, h, w, 3 + T), device="cuda")
    ybuf = torch.zeros((n * h * w * 4 + 4,), device="cuda")
    y = ybuf[:n * h * w * 4]
    assert _run(_tta_op(lg, acc, y, 0, True, True, 1, T, h, w), n)[0] == 0
    assert _run(_tta_op(lg, acc, None, 3, True, False, 0, T, h, w), n)[0] == 0        # not the last view: neither y nor K is read
    for k in (8, -1):
        rc, err = _run(_tta_op(lg, acc, y, k, True, True, 1, T, h, w), n)
        assert rc == -1 and b"tta" in err
    assert _run(_tta_op(lg, acc, y, 1, True, True, 1, T, 12, 10), n)[0] == -1         # a quarter turn of a non-square map
    assert _run(_tta_op(lg, acc, y, 2, True, True, 1, T, 12, 10), n)[0] == 0
    assert _run(_tta_op(lg, None, y, 0, True, True, 1, T, h, w), n)[0] == -1          # no accumulator
    assert _run(_tta_op(lg, acc, None, 0, True, True, 1, T, h, w), n)[0] == -1        # a last view without an output
    assert _run(_tta_op(lg, acc, y, 0, True, True, 0, T, h, w), n)[0] == -1           # K < 1
    assert _run(_tta_op(lg, acc, y, 0, True, True, -3, T, h, w), n)[0] == -1
    assert _run(_tta_op(lg, acc, ybuf[1:], 0, True, True, 1, T, h, w), n)[0] == -1    # y misaligned for the float4 store
    op = _tta_op(lg, acc, y, 0, True, True, 1, T, h, w)
    op.w = None
    assert _run(op, n)[0] == -1                                                       # types declared, no type logits
    # kind 99 stays refused
    op.kind = 99
    assert _run(op, n)[0] == -1


# ---- engine plumbing -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    """One model, three tiles, and -- made once, left unchanged -- the logits of eight plain `Engine.run` calls on host-made views."""
    from hover_net_amd import net_desc
    from hover_net_amd.synth import synth_state_dict, synth_tiles

    net = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    net.load_state_dict(synth_state_dict("original", 5, seed=21), strict=True)
    net = net.to("cuda").eval()
    net.max_batch = 16
    tiles = synth_tiles(3, 270, seed=22)
    eng = net.engine(3)
    assert getattr(eng, "_tta_acc", None) is None              # nothing allocated before the first TTA run
    per = []
    for k in range(8):
        v = np.ascontiguousarray(np.stack([R.view(t, k) for t in tiles]))
        logits, _ = eng.run(torch.from_numpy(v).to("cuda"))
        per.append({b: t.clone() for b, t in logits.items()})
    return net, tiles, per


def test_infer_step_tta_is_the_plain_pass_per_view(rig):
    from hover_net_amd import run_desc

    net, tiles, per = rig
    t = torch.from_numpy(tiles)
    before = run_desc.infer_step_device(t, net).clone()
    got = run_desc.infer_step_device(t, net, tta="d4").clone()
    want, _ = _reduce_device(per, tuple(range(8)), 5, 3, 80, 80)
    assert (got.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    assert net.engine(3)._tta_acc is not None
    # the plain step afterwards: the bits it returned before
    assert torch.equal(run_desc.infer_step_device(t, net), before)
    assert not torch.equal(got, before)
    # the host form and a tuple of ids
    flips = run_desc.infer_step(t, net, tta=(0, 4, 6, 2))
    want_f, _ = _reduce_device([per[k] for k in (0, 4, 6, 2)], (0, 4, 6, 2), 5, 3, 80, 80)
    assert isinstance(flips, np.ndarray) and (flips.view(np.uint32) == want_f.view(np.uint32)).all()


def test_run_tta_argument_checks(rig):
    net, tiles, _ = rig
    eng = net.engine(3)
    with pytest.raises(ValueError):
        eng.run_tta(torch.from_numpy(tiles).to("cuda"), "d8")
    with pytest.raises(TypeError):
        eng.run_tta(torch.zeros((1, 3, 270, 270), device="cuda"), "d4")
    with pytest.raises(ValueError):
        eng.run_tta(torch.zeros((1, 256, 256, 3), dtype=torch.uint8, device="cuda"), "d4")


@pytest.mark.parametrize("g", [1, 5])
def test_d4_average_is_equivariant(rig, g):
    """tta="d4" on view_g(tiles) against view_g of the tta="d4" result (hv vectors times M_g).  D4 is closed and the network is
    deterministic and batch-invariant, so both sides sum the SAME eight per-view terms, in another order: two fp32 sums of K terms
    differ by at most 2 (K - 1) 2^-24 sum|t_k| (each is within (K - 1) 2^-24 sum|t_k| of the exact sum), and the division by K keeps
    that relative size exactly (K = 8 is a power of two): per element 2 (K - 1) 2^-24 sum_k |t_k| / K."""
    from hover_net_amd import run_desc

    net, tiles, per = rig
    K = 8
    host = [{b: t.cpu().numpy() for b, t in d.items()} for d in per]
    r32, r64 = R.reduce_f32(host, tuple(range(8))), R.reduce_f64(host, tuple(range(8)))
    base = run_desc.infer_step_device(torch.from_numpy(tiles), net, tta="d4").cpu().numpy()
    vt = np.ascontiguousarray(np.stack([R.view(t, g) for t in tiles]))
    got = run_desc.infer_step_device(torch.from_numpy(vt), net, tta="d4").cpu().numpy()
    mag_np = sum(np.abs(t[0]) for t in r32["terms"])
    mag_hv = sum(np.abs(t[1]) for t in r32["terms"])
    bound = 2.0 * (K - 1) * 2.0 ** -24 * np.concatenate([mag_np[..., None], mag_hv], -1).astype(np.float64) / K
    want = np.stack([np.concatenate([R.view(s[..., 1:2], g), R.field_view(s[..., 2:], g)], -1) for s in base])
    absM = np.abs(R.M(g))
    bound_g = np.stack([np.concatenate([R.view(s[..., :1], g), R.view(s[..., 1:], g) @ absM.T.astype(np.float64)], -1) for s in bound])
    err = np.abs(got[..., 1:].astype(np.float64) - want.astype(np.float64))
    print("view %d: largest error / bound = %.3f" % (g, (err / np.maximum(bound_g, 1e-300)).max()))
    assert (err <= bound_g).all(), (g, (err / np.maximum(bound_g, 1e-300)).max())
    sure = np.stack([R.view(s, g) for s in (R.top2_gap(r64["tp"]) >= 1e-4)])
    assert (~sure).mean() < 0.05
    want_type = np.stack([R.view(s, g) for s in base[..., 0]])
    assert (got[..., 0][sure] == want_type[sure]).all()


def test_process_images_with_tta(rig):
    from hover_net_amd import infer_tile
    from hover_net_amd.synth import synth_tiles

    net, _, _ = rig
    images = [np.ascontiguousarray(synth_tiles(1, 340, seed=31 + i)[0][:300, :340]) for i in range(2)]
    plain = infer_tile.process_images(images, net, nr_types=5, batch_size=4, return_raw=True)
    aug = infer_tile.process_images(images, net, nr_types=5, batch_size=4, return_raw=True, tta="flips")
    assert len(aug) == len(plain) == 2
    for (inst0, info0, raw0), (inst1, info1, raw1) in zip(plain, aug):
        assert inst1.shape == inst0.shape == (300, 340) and inst1.dtype == inst0.dtype
        assert raw1.shape == raw0.shape == (300, 340, 4) and raw1.dtype == np.float32
        assert isinstance(info1, dict) and type(info1) is type(info0)
        for e in info1.values():
            assert set(e) == {"bbox", "centroid", "contour", "type_prob", "type"}
        assert not np.array_equal(raw1, raw0)                   # the augmentation reached the maps


def test_wsi_inference_with_tta(rig, monkeypatch):
    """WsiInference(tta="flips").run: the stage-1 map it hands to stage 2 holds the TTA'd patches, and the instance map is
    `stitch_instances` over that map."""
    from hover_net_amd import infer_wsi, run_desc

    net, _, _ = rig
    rng = np.random.default_rng(82)
    slide = infer_wsi.ArraySlide(rng.integers(0, 256, (1100, 1300, 3), dtype=np.uint8))
    kw = dict(nr_types=5, batch_size=16, chunk_shape=800, tile_shape=512, ambiguous_size=64)
    wsi = infer_wsi.WsiInference(net, tta="flips", **kw)
    seen = {}
    stage2 = wsi.stitch_instances
    monkeypatch.setattr(wsi, "stitch_instances", lambda pm, *a, **k: (seen.update(map=pm), stage2(pm, *a, **k))[1])
    inst, info = wsi.run(slide, np.ones((34, 40), np.uint8))
    pred = seen["map"].t
    assert tuple(pred.shape) == (1100, 1300, 4)
    _, patch = infer_wsi.get_chunk_patch_info(np.array([1100, 1300]), np.array([800, 800]), np.array([270, 270]), np.array([80, 80]))
    inside = [k for k in range(patch.shape[0]) if (patch[k, 0, 1] <= np.array([1100, 1300])).all()]
    for k in (inside[0], inside[len(inside) // 2], inside[-1]):
        y, x = patch[k, 0, 0]
        tile = torch.from_numpy(slide.array[y:y + 270, x:x + 270][None])
        one = run_desc.infer_step(tile, net, tta="flips")[0]
        got = pred[y + 95:y + 175, x + 95:x + 175].cpu().numpy()
        assert np.array_equal(got[..., 1:], one[..., 1:])           # same kernels, same order; batch position does not matter
        assert not np.array_equal(got[..., 1:], run_desc.infer_step(tile, net)[0][..., 1:])
    inst_ref, info_ref = infer_wsi.WsiInference(net, **kw).stitch_instances(pred)
    np.testing.assert_array_equal(inst, inst_ref)
    assert sorted(info) == sorted(info_ref)


def test_tile_pipeline_with_tta(rig):
    from hover_net_amd import post_proc, run_desc
    from hover_net_amd.pipeline import TilePipeline

    net, tiles, _ = rig
    t = torch.from_numpy(tiles)
    pipe = TilePipeline(net, nr_types=5, tta="flips")
    inst = pipe.submit(t)[0]
    pipe.wait()
    want = post_proc.process_batch_device(run_desc.infer_step_device(t, net, tta="flips"), 5)[0]
    assert torch.equal(inst.cpu(), want.cpu())


def test_run_args_tta_reaches_the_raw_map(rig, tmp_path):
    """`run_args["tta"]` of the tile-mode run loop: the saved raw map is the TTA'd step's, stitched."""
    import scipy.io as sio

    from hover_net_amd import infer_manager, infer_tile
    from hover_net_amd.synth import synth_tiles

    net, _, _ = rig
    inp = tmp_path / "in"
    inp.mkdir()
    img = np.ascontiguousarray(synth_tiles(1, 300, seed=41)[0][:283, :300])
    np.save(inp / "a.npy", img)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    out = str(tmp_path / "out")
    assert mgr.process_file_list({"input_dir": str(inp), "output_dir": out, "batch_size": 8, "save_raw_map": True, "tta": "rot"}) == ["a"]
    want = infer_tile.process_images([img], net, nr_types=5, batch_size=8, return_raw=True, tta=(0, 1, 2, 3))[0][2]
    assert np.array_equal(sio.loadmat(out + "/mat/a.mat")["raw_map"], want)

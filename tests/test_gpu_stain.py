"""-m gpu: Macenko stain normalisation on the device (csrc/hvn_stain.hip, hover_net_amd/stain.py).

Contracts: HVN_OP_STAIN_HIST + HVN_OP_STAIN_COMPACT equal np.unique(return_counts=True) exactly; HVN_OP_STAIN_APPLY equals
stain.apply_host bit for bit; the device fit equals the host fit bit for bit; `stain_norm=` of process_images / WsiInference / the
run loop equals the plain call on the image normalised on the host."""
import ctypes

import numpy as np
import pytest
import torch

import stain_ref as R

pytestmark = pytest.mark.gpu
OP_HIST, OP_COMPACT, OP_APPLY = 11, 12, 13
GUARD = 64      # guard rows of 8 bytes on either side of the list


def _run(op, n):
    from hover_net_amd import lib as L

    rc = L.lib().hvn_run_op(ctypes.addressof(op), n, L.stream_ptr("cuda"))
    return rc, L.lib().hvn_last_error()


def _image(v, t):
    """hvn_view of a uint8 device tensor [n, h, w, 3] (rows / samples may be strided); returns n."""
    n, h, w, _ = t.shape
    assert t.stride(3) == 1 and t.stride(2) == 3
    v.base, v.h, v.w, v.c, v.sn, v.sy = t.data_ptr(), h, w, 3, t.stride(0), t.stride(1)
    return n


@pytest.fixture(scope="module")
def table():
    """The 2^24 bins (clear; every test leaves them clear), COMPACT's workspace and status."""
    return {"bins": torch.zeros(1 << 24, dtype=torch.int32, device="cuda"), "ws": torch.empty(65536, dtype=torch.uint8, device="cuda"),
            "status": torch.empty(2, dtype=torch.int64, device="cuda")}


def _hist(table, x, mask=None):
    from hover_net_amd import lib as L

    op = L.hvn_op()
    op.kind = OP_HIST
    n = _image(op.x, x)
    if mask is not None:
        op.res.base = mask.data_ptr()
    op.y.base = table["bins"].data_ptr()
    rc, err = _run(op, n)
    assert rc == 0, err


def _compact(table, cap, clear=True):
    """-> (pairs uint32 [min(n, cap), 2], status); checks the guard rows and what the rows past the written ones hold."""
    from hover_net_amd import lib as L

    buf = torch.full((cap + 2 * GUARD, 2), -1515870811, dtype=torch.int32, device="cuda")        # 0xA5A5A5A5
    table["status"].fill_(-7)
    op = L.hvn_op()
    op.kind, op._rsv = OP_COMPACT, int(clear)
    op.x.base, op.y.base, op.y.h = table["bins"].data_ptr(), buf[GUARD:].data_ptr(), cap
    op.y2.base, op.x2.base = table["status"].data_ptr(), table["ws"].data_ptr()
    rc, err = _run(op, 1)
    assert rc == 0, err
    status = table["status"].cpu().numpy()
    b = buf.cpu().numpy()
    assert (b[:GUARD] == -1515870811).all() and (b[GUARD + cap:] == -1515870811).all()
    n = min(int(status[0]), cap)
    assert (b[GUARD + n:GUARD + cap] == -1515870811).all()           # nothing past the last pair
    if clear:
        assert int(table["bins"].count_nonzero()) == 0
    return b[GUARD:GUARD + n].view(np.uint32), status


def _unique(a, mask=None):
    key = (a[..., 0].astype(np.uint32) << 16) | (a[..., 1].astype(np.uint32) << 8) | a[..., 2]
    key = key.reshape(-1) if mask is None else key[mask != 0]
    return np.unique(key, return_counts=True)


def _check_list(pairs, status, a, mask=None):
    keys, counts = _unique(a, mask)
    assert status[0] == len(keys) and status[1] == counts.sum()
    assert (np.diff(pairs[:, 0].astype(np.int64)) > 0).all()
    assert np.array_equal(pairs[:, 0], keys) and np.array_equal(pairs[:, 1], counts)


# ---- HIST + COMPACT ----------------------------------------------------------------------------
def test_hist_odd_extents(table):
    """1 x 37 x 53: one folded row of 1961 pixels, 490 groups of four and a tail of one; then the same bytes from an odd address
    (the byte form)."""
    a = R.he_image(37, 53, 5)[None]
    x = torch.from_numpy(a).to("cuda")
    _hist(table, x)
    _check_list(*_compact(table, 37 * 53), a)
    raw = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
    y = raw[1:1 + a.size].view(1, 37, 53, 3)
    y.copy_(x)
    assert y.data_ptr() % 4 == 1
    _hist(table, y)
    _check_list(*_compact(table, 37 * 53), a)


@pytest.mark.parametrize("x0", [8, 7])
@pytest.mark.parametrize("masked", [False, True])
def test_hist_window_of_a_larger_buffer(table, x0, masked):
    """3 x 40 x 64 inside [3][48][80][3]: row stride 240 > 192; x0 = 8 starts every row on a dword, x0 = 7 on none."""
    rng = np.random.default_rng(17)
    big = rng.integers(0, 256, (3, 48, 80, 3), dtype=np.uint8)
    big[:, 4:44, x0:x0 + 64] = np.stack([R.he_image(40, 64, 20 + i) for i in range(3)])
    big[:, 10:20, x0 + 5:x0 + 50] = (233, 231, 235)                       # a run of equal neighbours
    dev = torch.from_numpy(big).to("cuda")
    win = dev[:, 4:44, x0:x0 + 64]
    assert win.stride(1) == 240 and not win.is_contiguous()
    mask = (rng.random((3, 40, 64)) < 0.5).astype(np.uint8) * 3 if masked else None
    _hist(table, win, None if mask is None else torch.from_numpy(mask).to("cuda"))
    _check_list(*_compact(table, 3 * 40 * 64), big[:, 4:44, x0:x0 + 64], mask)


def test_hist_hot_bin(table):
    """300 x 300 of one colour plus five others: 90 000 pixels, six bins, more than one workgroup."""
    a = np.full((1, 300, 300, 3), (244, 243, 246), np.uint8)
    rng = np.random.default_rng(2)
    others = np.array([(0, 0, 0), (255, 255, 255), (244, 243, 245), (1, 2, 3), (200, 100, 50)], np.uint8)
    for k, c in enumerate(others):
        ys, xs = rng.integers(0, 300, 40 * (k + 1)), rng.integers(0, 300, 40 * (k + 1))
        a[0, ys, xs] = c
    _hist(table, torch.from_numpy(a).to("cuda"))
    pairs, status = _compact(table, 16)
    assert status[0] == 6 and status[1] == 90000
    _check_list(pairs, status, a)


def test_two_calls_add_into_one_table(table):
    a, b = R.he_image(45, 70, 8)[None], R.he_image(33, 41, 9)[None]
    _hist(table, torch.from_numpy(a).to("cuda"))
    _hist(table, torch.from_numpy(b).to("cuda"))
    both = np.concatenate([a.reshape(-1, 3), b.reshape(-1, 3)])
    # without the clearing flag the table stays: a second COMPACT gives the same list
    first, st1 = _compact(table, both.shape[0], clear=False)
    again, st2 = _compact(table, both.shape[0], clear=True)
    _check_list(first, st1, both)
    assert np.array_equal(first, again) and np.array_equal(st1, st2)


def test_list_capacity(table):
    """cap = 10 on an image of more colours: the first 10 pairs, the status holds the true number."""
    a = R.he_image(37, 53, 5)[None]
    keys, counts = _unique(a)
    assert len(keys) > 100
    _hist(table, torch.from_numpy(a).to("cuda"))
    pairs, status = _compact(table, 10)
    assert status[0] == len(keys) and status[1] == 37 * 53
    assert pairs.shape == (10, 2) and np.array_equal(pairs[:, 0], keys[:10]) and np.array_equal(pairs[:, 1], counts[:10])


# ---- APPLY ---------------------------------------------------------------------------------------
def _apply_op(x, y, tab):
    from hover_net_amd import lib as L

    op = L.hvn_op()
    op.kind = OP_APPLY
    n = _image(op.x, x)
    _image(op.y, y)
    op.w = tab.data_ptr()
    return op, n


def _extreme_tables():
    """Entries that overflow 255, +inf and 0 (0 * inf -> NaN -> 255), and tiny ones."""
    rng = np.random.default_rng(6)
    t = np.exp(rng.normal(0, 1.5, (3, 3, 256)))
    t[0, 0, ::7] = np.inf
    t[0, 1, ::5] = 0.0
    t[1, 2, ::3] = 1e-300
    t[2, 0, ::11] = 1e300
    t[2, 1, 100:] = np.inf
    return t


@pytest.fixture(scope="module")
def real_tables():
    from hover_net_amd import stain

    return stain.tables(stain.fit(R.he_image(96, 96, 1)))


@pytest.mark.parametrize("which", ["fit", "extreme"])
@pytest.mark.parametrize("case", ["dense", "strided", "odd_address"])
def test_apply_equals_apply_host(real_tables, which, case):
    from hover_net_amd import stain

    tab = real_tables if which == "fit" else _extreme_tables()
    tab_dev = torch.from_numpy(tab).to("cuda")
    rng = np.random.default_rng(12)
    if case == "strided":           # 2 x 19 x 35 inside [2][25][45][3]
        big = rng.integers(0, 256, (2, 25, 45, 3), dtype=np.uint8)
        a = big[:, 3:22, 6:41]
        xdev = torch.from_numpy(big).to("cuda")
        x = xdev[:, 3:22, 6:41]
        ybig = torch.full((2, 25, 45, 3), 0xA5, dtype=torch.uint8, device="cuda")
        y = ybig[:, 3:22, 6:41]
    else:
        a = R.he_image(37, 53, 5)[None]
        a = np.where(rng.random(a.shape) < 0.3, rng.integers(0, 256, a.shape, dtype=np.uint8), a).astype(np.uint8)
        off = 1 if case == "odd_address" else 0
        xraw = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
        x = xraw[off:off + a.size].view(a.shape)
        x.copy_(torch.from_numpy(a))
        ybig = torch.full((a.size + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        y = ybig[256 + off:256 + off + a.size].view(a.shape)
    want = stain.apply_host(a, tab)
    op, n = _apply_op(x, y, tab_dev)
    rc, err = _run(op, n)
    assert rc == 0, err
    assert np.array_equal(y.cpu().numpy(), want)
    # the bytes around the output stayed
    g = ybig.cpu().numpy().copy()
    if case == "strided":
        g[:, 3:22, 6:41] = 0xA5
    else:
        g[256 + off:256 + off + a.size] = 0xA5
    assert (g == 0xA5).all()
    # in place
    op, n = _apply_op(x, x, tab_dev)
    rc, err = _run(op, n)
    assert rc == 0, err
    assert np.array_equal(x.cpu().numpy(), want)
    if case == "strided":
        rest = xdev.cpu().numpy()
        rest[:, 3:22, 6:41] = big[:, 3:22, 6:41]
        assert np.array_equal(rest, big)
    # and the Python form
    assert np.array_equal(stain.apply_device(torch.from_numpy(np.ascontiguousarray(a)).to("cuda"), tab).cpu().numpy(), want)


# ---- the fit ---------------------------------------------------------------------------------------
def test_device_fit_equals_host_fit():
    from hover_net_amd import stain

    a = R.he_image(270, 270, 2)
    host = stain.fit(a)
    dev = stain.fit(torch.from_numpy(a).to("cuda"))
    assert np.array_equal(dev.he, host.he) and np.array_equal(dev.max_c, host.max_c) and (dev.kept, dev.pixels) == (host.kept, host.pixels)
    shuffled = a[np.random.default_rng(1).permutation(270)]
    again = stain.fit(torch.from_numpy(shuffled).to("cuda"))
    assert np.array_equal(again.he, host.he) and np.array_equal(again.max_c, host.max_c)
    mask = (np.random.default_rng(2).random((270, 270)) < 0.7).astype(np.uint8)
    hm, dm = stain.fit(a, mask), stain.fit(torch.from_numpy(a).to("cuda"), torch.from_numpy(mask).to("cuda"))
    assert np.array_equal(dm.he, hm.he) and np.array_equal(dm.max_c, hm.max_c) and dm.pixels == hm.pixels == int(mask.sum())
    k, c = stain.colour_counts_device(torch.from_numpy(a).to("cuda"))
    k2, c2 = stain.colour_counts_host(a)
    assert k.dtype == k2.dtype and np.array_equal(k, k2) and np.array_equal(c, c2)


# ---- refusals ----------------------------------------------------------------------------------
def test_stain_refusals(table, real_tables):
    from hover_net_amd import lib as L

    tab = torch.zeros(9 * 256 + 1, dtype=torch.float64, device="cuda")
    tab[:9 * 256] = torch.from_numpy(real_tables).reshape(-1).to("cuda")
    xbuf = torch.zeros((2, 24, 20, 3), dtype=torch.uint8, device="cuda")
    x, y = xbuf[:, :20], torch.full((2, 20, 20, 3), 0xA5, dtype=torch.uint8, device="cuda")

    def refused(op, n, name, code=-1):
        rc, err = _run(op, n)
        assert rc == code and err.startswith(name + b":"), (rc, err)

    def apply(**kw):
        op, _ = _apply_op(x, y, tab)
        for k, v in kw.items():
            obj, f = (op, k) if "." not in k else (getattr(op, k.split(".")[0]), k.split(".")[1])
            setattr(obj, f, v)
        return op

    assert _run(apply(), 2)[0] == 0
    assert (y.cpu().numpy() != 0xA5).any()
    y.fill_(0xA5)
    refused(apply(**{"y.base": x.data_ptr() + 60}), 2, b"stain_apply")             # y starts one row into x: partial overlap
    refused(apply(**{"y.base": x.data_ptr(), "y.sy": 60, "y.sn": 1200}), 2, b"stain_apply")       # x's base with other strides
    refused(apply(w=tab.data_ptr() + 4), 2, b"stain_apply")                        # misaligned tables
    refused(apply(w=None), 2, b"stain_apply")
    refused(apply(**{"y.base": None}), 2, b"stain_apply")
    refused(apply(**{"x.c": 4}), 2, b"stain_apply")
    refused(apply(**{"y.h": 19}), 2, b"stain_apply")
    refused(apply(x_dtype=1), 2, b"stain_apply")
    refused(apply(**{"x.sy": 59}), 2, b"stain_apply")
    refused(apply(**{"x.sn": 60 * 19}), 2, b"stain_apply")
    refused(apply(), 65536, b"stain_apply")
    assert (y.cpu().numpy() == 0xA5).all() and int(xbuf.count_nonzero()) == 0       # nothing was launched

    def hist(**kw):
        op = L.hvn_op()
        op.kind = OP_HIST
        _image(op.x, x)
        op.y.base = table["bins"].data_ptr()
        for k, v in kw.items():
            obj, f = (op, k) if "." not in k else (getattr(op, k.split(".")[0]), k.split(".")[1])
            setattr(obj, f, v)
        return op

    refused(hist(**{"y.base": table["bins"].data_ptr() + 2}), 2, b"stain_hist")
    refused(hist(**{"y.base": None}), 2, b"stain_hist")
    refused(hist(**{"x.base": None}), 2, b"stain_hist")
    refused(hist(**{"x.c": 1}), 2, b"stain_hist")
    refused(hist(x_dtype=1), 2, b"stain_hist")
    refused(hist(**{"x.sy": 10}), 2, b"stain_hist")
    refused(hist(**{"x.h": 1 << 15, "x.w": (1 << 15) + 1, "x.sy": 0, "x.sn": 0}), 1, b"stain_hist", -4)
    refused(hist(), 65536, b"stain_hist")
    assert int(table["bins"].count_nonzero()) == 0

    lst = torch.full((34, 2), -1, dtype=torch.int32, device="cuda")

    def compact(**kw):
        op = L.hvn_op()
        op.kind = OP_COMPACT
        op.x.base, op.y.base, op.y.h = table["bins"].data_ptr(), lst[1:].data_ptr(), 32
        op.y2.base, op.x2.base = table["status"].data_ptr(), table["ws"].data_ptr()
        for k, v in kw.items():
            setattr(getattr(op, k.split(".")[0]), k.split(".")[1], v)
        return op

    table["status"].fill_(-7)
    refused(compact(), 2, b"stain_compact")                                         # batch must be 1
    refused(compact(**{"y.base": lst.data_ptr() + 4}), 1, b"stain_compact")
    refused(compact(**{"y2.base": table["status"].data_ptr() + 4}), 1, b"stain_compact")
    refused(compact(**{"x2.base": table["ws"].data_ptr() + 4}), 1, b"stain_compact")
    refused(compact(**{"x.base": table["bins"].data_ptr() + 4}), 1, b"stain_compact")
    refused(compact(**{"x.base": None}), 1, b"stain_compact")
    refused(compact(**{"y.h": 0}), 1, b"stain_compact", -4)
    refused(compact(**{"y.h": (1 << 24) + 1}), 1, b"stain_compact", -4)
    assert (lst.cpu().numpy() == -1).all() and (table["status"].cpu().numpy() == -7).all()
    rc, err = _run(compact(), 1)
    assert rc == 0, err
    assert (table["status"].cpu().numpy() == 0).all() and (lst.cpu().numpy() == -1).all()      # an empty table: no pair


# ---- plumbing ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from hover_net_amd import net_desc
    from hover_net_amd.synth import synth_state_dict

    net = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    net.load_state_dict(synth_state_dict("original", 5, seed=21), strict=True)
    net = net.to("cuda").eval()
    net.max_batch = 16
    return net


def _norm(img, mask=None, src=None):
    """Host fit (of `src`, default the image itself, under `mask`) + apply_host."""
    from hover_net_amd import stain

    return stain.apply_host(img, stain.tables(stain.fit(img if src is None else src, mask)))


def _same_info(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert sorted(a[k]) == sorted(b[k])
        for f in a[k]:
            assert np.array_equal(np.asarray(a[k][f]), np.asarray(b[k][f])), (k, f)


def _same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0])
        _same_info(g[1], w[1])
        assert np.array_equal(g[2].view(np.uint32), w[2].view(np.uint32))


def test_process_images_with_stain_norm(net):
    from hover_net_amd import infer_tile

    a = R.he_image(300, 340, 31)
    b = R.he_image(300, 340, 32, he=((0.55, 0.76, 0.35), (0.15, 0.93, 0.25)), strength=(0.7, 1.3))
    white = np.full((300, 340, 3), 255, np.uint8)
    kw = dict(nr_types=5, batch_size=4, return_raw=True)
    plain = infer_tile.process_images([a, b, white], net, **kw)
    with pytest.warns(UserWarning, match="stain normalisation skipped") as rec:
        got = infer_tile.process_images([a, b, white], net, stain_norm="macenko", **kw)
    assert len([r for r in rec if "stain normalisation skipped" in str(r.message)]) == 1
    want = infer_tile.process_images([_norm(a), _norm(b), white], net, **kw)
    _same_results(got, want)
    _same_results(got[2:], plain[2:])                       # the white image passed through
    assert not np.array_equal(got[0][2], plain[0][2]) and not np.array_equal(got[1][2], plain[1][2])
    # a StainFit of a target image is a target
    from hover_net_amd import stain

    target = stain.fit(b)
    got_t = infer_tile.process_images([a], net, stain_norm=target, **kw)
    want_t = infer_tile.process_images([stain.apply_host(a, stain.tables(stain.fit(a), target))], net, **kw)
    _same_results(got_t, want_t)


@pytest.mark.parametrize("tta", [None, "flips"])
def test_wsi_inference_with_stain_norm(net, tta, monkeypatch):
    from hover_net_amd import infer_wsi, stain

    tile = R.he_image(300, 340, 33)
    arr = np.ascontiguousarray(np.tile(tile, (4, 4, 1))[:1100, :1300])
    slide = infer_wsi.ArraySlide(arr)
    mask = np.ones((34, 40), np.uint8)
    mask[:6, :9] = 0
    mask[20:, 30:] = 0
    kw = dict(nr_types=5, batch_size=16, chunk_shape=800, tile_shape=512, ambiguous_size=64)
    if tta:
        kw["tta"] = tta
    thumb = slide.thumbnail(8)
    th, tw = thumb.shape[:2]
    tmask = np.array([[mask[(y * 34) // th, (x * 40) // tw] for x in range(tw)] for y in range(th)], np.uint8)
    assert 0 < tmask.sum() < tmask.size
    maps = []

    def run(slide_, **more):
        """(inst, info) of WsiInference.run, with the stage-1 map it handed to stage 2 appended to `maps`."""
        wsi = infer_wsi.WsiInference(net, **kw, **more)
        stage2 = wsi.stitch_instances
        monkeypatch.setattr(wsi, "stitch_instances", lambda pm, *a, **k: (maps.append(pm.t.clone()), stage2(pm, *a, **k))[1])
        return wsi.run(slide_, mask)

    inst, info = run(slide, stain_norm="macenko")
    inst_w, info_w = run(infer_wsi.ArraySlide(_norm(arr, tmask, src=thumb)))
    assert tuple(maps[0].shape) == (1100, 1300, 4) and torch.equal(maps[0].view(torch.int32), maps[1].view(torch.int32))
    assert np.array_equal(inst, inst_w)
    _same_info(info, info_w)
    assert np.array_equal(stain.thumbnail_mask((th, tw), mask), tmask)
    if tta is None:
        run(slide)
        assert not torch.equal(maps[0], maps[2])                # the normalisation reached the network


def test_run_args_stain_norm_reaches_the_raw_map(net, tmp_path):
    import scipy.io as sio

    from hover_net_amd import infer_manager, infer_tile

    inp = tmp_path / "in"
    inp.mkdir()
    img = R.he_image(283, 300, 41)
    np.save(inp / "a.npy", img)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    bad = str(tmp_path / "bad")
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": bad, "batch_size": 8, "stain_norm": "reinhard"})
    assert not (tmp_path / "bad").exists()
    with pytest.raises(ValueError):
        infer_manager.WsiManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net).process_wsi_list(
            {"input_dir": str(inp), "output_dir": bad, "stain_norm": "reinhard"})
    assert not (tmp_path / "bad").exists()
    out = str(tmp_path / "out")
    assert mgr.process_file_list({"input_dir": str(inp), "output_dir": out, "batch_size": 8, "save_raw_map": True, "stain_norm": "macenko"}) == ["a"]
    want = infer_tile.process_images([_norm(img)], net, nr_types=5, batch_size=8, return_raw=True)[0][2]
    raw = sio.loadmat(out + "/mat/a.mat")["raw_map"]
    assert np.array_equal(raw, want)
    assert not np.array_equal(raw, infer_tile.process_images([img], net, nr_types=5, batch_size=8, return_raw=True)[0][2])

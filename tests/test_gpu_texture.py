"""-m gpu: the per-nucleus texture pass (csrc/hvn_texture.hip, HVN_OP_INST_TEXTURE) against the per-pixel oracle tests/texture_ref.py,
from the op (`PostProc.texture`) up through `process_batch_device`, `process`, tile mode and the manager.  The device fields are
integers: everything is compared with ==, both scales and both accumulation forms; the float features are `texture.derive` of the
oracle's integers."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import texture_ref as R
from golden_util import assert_same_info

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "proc_*.npz")))
IDS = [os.path.basename(p)[5:-4] for p in CASES]
SCALES = ["range", "fixed"]


def _pp():
    from hover_net_amd import post_proc as PP

    return PP._pp(torch.device("cuda"))


def _table(inst_dev, max_inst):
    """hvn_instance_table with a free choice of max_inst -> device records [n, max_inst, sizeof(rec)]."""
    from hover_net_amd import lib as L

    n, h, w = inst_dev.shape
    ws = torch.empty(max(1, L.lib().hvn_instance_table_workspace_bytes(n, max_inst, 0)), dtype=torch.uint8, device="cuda")
    rec = torch.empty((n, max_inst, ctypes.sizeof(L.hvn_inst_rec)), dtype=torch.uint8, device="cuda")
    counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    L.check(L.lib().hvn_instance_table(inst_dev.data_ptr(), None, n, h, w, 0, 0, rec.data_ptr(), counts.data_ptr(), max_inst, ws.data_ptr(),
                                       ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "hvn_instance_table")
    return rec


def _host(t, n, m):
    from hover_net_amd import texture as TX

    return t.cpu().numpy().view(TX.TEX_DTYPE).reshape(n, m)


def _check(maps, image, max_inst=None, scales=SCALES):
    """The device fields of every slot of every map == the oracle's, both forms, and seen == area; -> (records, {scale: slots}) on the host."""
    from hover_net_amd import post_proc as PP

    maps = np.ascontiguousarray(maps, np.int32)
    maps = maps[None] if maps.ndim == 2 else maps
    image = image[None] if image.ndim == 3 else image
    max_inst = max(int(maps.max()), 1) if max_inst is None else max_inst
    n = maps.shape[0]
    inst = torch.from_numpy(maps).to("cuda")
    img = torch.from_numpy(np.ascontiguousarray(image)).to("cuda")
    rec = _table(inst, max_inst)
    rec_h = rec.cpu().numpy().view(PP._REC_DTYPE).reshape(n, max_inst)
    out = {}
    for scale in scales:
        want = [R.map_sums(maps[i], image[i], max_inst, scale) for i in range(n)]
        for form in (0, 1):
            tex = _pp().texture(inst, rec, img, scale, form=form)
            assert tex.shape == (n, max_inst, 1104) and tex.dtype == torch.uint8
            got = _host(tex, n, max_inst)
            for i in range(n):
                R.assert_equal(got[i], want[i], "map %d, %s, form %d" % (i, scale, form))
                assert got[i]["seen"].tolist() == rec_h[i]["area"].tolist()
        out[scale] = got
    return rec_h, out


# -- 1: integer fields ------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.SIZES)
def test_map_sizes(h, w):
    _check(R.sized_map(h, w), R.image((h, w), 5))


def test_three_maps_with_different_content_in_one_call():
    maps = R.three_maps()
    _check(maps, R.image(maps.shape, 9))


@pytest.mark.parametrize("name", R.SHAPES)
def test_hand_shapes(name):
    m = R.shape(name)
    _, got = _check(m, R.image(m.shape, 3))
    if name in R.ONLY:
        for scale in SCALES:
            for j in range(got[scale].shape[1]):
                assert [d for d in range(4) if got[scale]["glcm"][0, j, d].any()] == list(R.ONLY[name]), (name, scale, j)


@pytest.mark.parametrize("width", [61, 62, 63, 64, 65, 124, 125, 129])
def test_strip_boundaries(width):
    """A strip owns 62 columns: 62 | 63 and 124 | 125 are where the number of strips changes; 64, 65 and 129 are the word sizes a
    one-word-per-row form would break at.  Dense noise, so every strip boundary cuts through pairs of all four directions."""
    m = R.strip_case(width)
    rec_h, _ = _check(m, R.image(m.shape, width))
    assert int(rec_h[0]["cmax"][0] - rec_h[0]["cmin"][0]) == width


# -- 2: contention and range ------------------------------------------------------------------------------
def _square():
    m = np.zeros((64, 66), np.int32)
    m[2:62, 3:63] = 1                                  # 60 x 60
    return m


def test_constant_colour_lands_in_one_word():
    m = _square()
    img = np.zeros(m.shape + (3,), np.uint8)
    img[:] = (120, 60, 200)
    _, got = _check(m, img)
    for scale in SCALES:
        g = got[scale]["glcm"][0, 0]
        assert [int(np.count_nonzero(g[d])) for d in range(4)] == [1, 1, 1, 1] and int(g[0].sum()) == 60 * 59 and int(g[1].sum()) == 59 * 59


def test_random_image_hits_every_word():
    m = _square()
    grey = np.random.default_rng(17).integers(0, 256, m.shape + (1,), dtype=np.uint8)
    _, got = _check(m, np.repeat(grey, 3, axis=2))         # R = G = B = v has grey value v: the levels are uniform, 55 pairs per word
    for scale in SCALES:
        assert got[scale]["glcm"][0, 0].all() and got[scale]["hist"][0, 0].all()


def test_grey_values_span_0_to_255():
    m = _square()
    img = R.image(m.shape, 18)
    img[10, 10], img[40, 33] = (0, 0, 0), (255, 255, 255)
    _, got = _check(m, img)
    assert got["range"]["lo"][0, 0] == 0 and got["range"]["hi"][0, 0] == 255
    assert got["range"].tobytes() == got["fixed"].tobytes()             # the two scales coincide


def test_counts_pass_65535():
    """One label over 300 x 300: a word packed into 16 bits would wrap."""
    m = np.ones((300, 300), np.int32)
    img = np.zeros(m.shape + (3,), np.uint8)
    img[:, :150] = 40
    img[:, 150:] = 50                                      # one level with 40 under both scales
    img[::7, ::5] = 200
    _, got = _check(m, img)
    for scale in SCALES:
        assert int(got[scale]["glcm"][0, 0].max()) > 65535 and int(got[scale]["hist"][0, 0].max()) > 65535


# -- 3: tables ----------------------------------------------------------------------------------------------
def test_max_inst_smaller_than_the_largest_label():
    m = R.blobs(40, 50, seed=11, sigma=1.5)
    assert m.max() > 6
    _, got = _check(m, R.smooth_image(m.shape, 1), max_inst=4)        # labels 5.. are background to everyone
    assert got["range"].shape == (1, 4)


def test_stale_table_stays_inside_the_map_and_shows_in_seen():
    """A table whose boxes do not belong to the map (shifted, partly outside) on a VALID map: the call returns OK, the bbox is
    clamped to the map by construction, `seen` counts the label inside the clamped box and differs from `area`."""
    from hover_net_amd import post_proc as PP

    m = R.blobs(48, 60, seed=21)
    img = R.image(m.shape, 4)
    max_inst = int(m.max())
    inst = torch.from_numpy(m[None]).to("cuda")
    rec_h = _table(inst, max_inst).cpu().numpy().view(PP._REC_DTYPE).reshape(max_inst).copy()
    for k, d in (("rmin", 7), ("rmax", 7), ("cmin", -9), ("cmax", -9)):
        rec_h[k][rec_h["area"] > 0] += d
    stale = torch.from_numpy(rec_h.view(np.uint8).reshape(1, max_inst, -1)).to("cuda")
    boxes = [tuple(int(rec_h[k][j]) for k in ("area", "rmin", "rmax", "cmin", "cmax")) for j in range(max_inst)]
    img_dev = torch.from_numpy(img[None]).to("cuda")
    for scale in SCALES:
        got = _host(_pp().texture(inst, stale, img_dev, scale), 1, max_inst)[0]
        torch.cuda.synchronize()
        R.assert_equal(got, R.map_sums(m, img, max_inst, scale, boxes), scale)
        want = [int(np.count_nonzero(m[max(r0, 0):min(r1, 48), max(c0, 0):min(c1, 60)] == j + 1)) if a > 0 else 0
                for j, (a, r0, r1, c0, c1) in enumerate(boxes)]
        assert got["seen"].tolist() == want and (got["seen"] != rec_h["area"]).any()


def test_all_background_map_is_all_zero_words():
    m = np.zeros((20, 30), np.int32)
    inst = torch.from_numpy(m[None]).to("cuda")
    rec = _table(inst, 5)
    tex = _pp().texture(inst, rec, torch.from_numpy(R.image((1, 20, 30), 2)).to("cuda"))
    assert tex.shape == (1, 5, 1104) and not tex.any()


def test_every_word_is_overwritten_and_two_runs_agree():
    """The op writes into a tensor pre-filled with 0xFF bytes: nothing of the fill survives, and a second run gives the same bytes."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    m = R.blobs(67, 131, seed=2, q=0.7)
    max_inst = int(m.max()) + 3                            # empty slots too
    inst = torch.from_numpy(m[None]).to("cuda")
    img = torch.from_numpy(R.smooth_image(m.shape, 3)[None]).to("cuda")
    rec = _table(inst, max_inst)
    for mode in (0, 1):
        runs = []
        for _ in range(2):
            out = torch.full((1, max_inst, 1104), 0xFF, dtype=torch.uint8, device="cuda")
            op = L.hvn_op()
            op.kind, op.cout, op._rsv = PL.OP_INST_TEXTURE, max_inst, mode
            op.x.base, op.x.h, op.x.w, op.x.c = img.data_ptr(), 67, 131, 3
            op.res.base, op.w, op.y.base = inst.data_ptr(), rec.data_ptr(), out.data_ptr()
            L.call("hvn_run_op", ctypes.addressof(op), 1, L.stream_ptr(torch.device("cuda")))
            runs.append(out.cpu().numpy())
        assert runs[0].tobytes() == runs[1].tobytes()
        got = _host(torch.from_numpy(runs[0]), 1, max_inst)[0]
        R.assert_equal(got, R.map_sums(m, img[0].cpu().numpy(), max_inst, SCALES[mode]), mode)     # no 0xFF word can pass this
        assert got["seen"].sum() > 0 and not got[-3:].view(np.int32).any()


def test_c_abi_refuses_without_touching_the_output():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    inst = torch.zeros((1, 8, 8), dtype=torch.int32, device="cuda")
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    rec = _table(inst, 2)
    out = torch.full((1, 2, 1104), 0x5A, dtype=torch.uint8, device="cuda")

    def op_with(**kw):
        op = L.hvn_op()
        op.kind, op.cout = PL.OP_INST_TEXTURE, 2
        op.x.base, op.x.h, op.x.w, op.x.c = img.data_ptr(), 8, 8, 3
        op.res.base, op.w, op.y.base = inst.data_ptr(), rec.data_ptr(), out.data_ptr()
        for k, v in kw.items():
            setattr(op, k, v)
        return op

    s = L.stream_ptr(torch.device("cuda"))
    for kw, code in (({"_rsv": 2}, -1), ({"cout": 0}, -1), ({"w": None}, -1), ({"stride": 5}, -1), ({"x_dtype": 1}, -1)):
        op = op_with(**kw)
        assert L.lib().hvn_run_op(ctypes.byref(op), 1, s) == code and L.lib().hvn_last_error().startswith(b"inst_texture:")
    torch.cuda.synchronize()
    assert (out == 0x5A).all()
    op = op_with()
    assert L.lib().hvn_run_op(ctypes.byref(op), 1, s) == 0
    torch.cuda.synchronize()
    assert not out.any()


# -- 4: the public path -------------------------------------------------------------------------------------
def _want_texture(inst_map, image, scale):
    """{label: texture dict} of every label of a host label map: `derive` of the oracle's integers."""
    from hover_net_amd import texture as TX

    max_inst = max(int(inst_map.max()), 1)
    s = R.map_sums(inst_map, image, max_inst, scale)
    tex = np.zeros(max_inst, TX.TEX_DTYPE)
    for k in R.INT_FIELDS:
        tex[k] = s[k]
    dicts = TX.to_dicts(TX.derive(tex))
    return {j + 1: dicts[j] for j in range(max_inst) if s["seen"][j] > 0}


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_goldens_batched_and_process(path):
    from hover_net_amd import post_proc as PP

    z = np.load(path)
    nt = None if int(z["nr_types"]) < 0 else int(z["nr_types"])
    pred = torch.from_numpy(z["pred"]).to("cuda")
    img = R.image(z["pred"].shape[:3], 31)
    img_dev = torch.from_numpy(img).to("cuda")
    plain = PP.process_batch_device(pred, nt, True)
    out = PP.process_batch_device(pred, nt, True, return_texture="range", image=img_dev)
    assert len(plain) == 3 and len(out) == 4
    for a, b in zip(plain, out):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(out[0].cpu().numpy(), z["inst"])
    n, max_inst = out[1].shape[:2]
    got = _host(out[3], n, max_inst)
    used = max(int(z["inst"].max()), 1)
    assert not got[:, used:].view(np.int32).any()
    for i in range(n):
        R.assert_equal(got[i, :used], R.map_sums(z["inst"][i], img[i], used, "range"), i)
    # features first, texture LAST
    feats = PP.process_batch_device(pred, nt, True, return_features=True, image=img_dev)
    both = PP.process_batch_device(pred, nt, True, return_contours=True, return_features=True, return_texture="fixed", image=img_dev)
    assert len(both) == 8 and torch.equal(both[6], feats[3]) and both[7].shape == out[3].shape
    fixed = _host(both[7], n, max_inst)
    R.assert_equal(fixed[0, :used], R.map_sums(z["inst"][0], img[0], used, "fixed"), "fixed")
    for i in (0, n - 1):
        inst0, info0 = PP.process(z["pred"][i], nr_types=nt, return_centroids=True)
        inst1, info1 = PP.process(z["pred"][i], nr_types=nt, texture=True, image=img[i])            # implies the dict; True = "range"
        np.testing.assert_array_equal(inst1, inst0)
        assert_same_info(info1, info0)
        assert all("texture" not in e and "features" not in e for e in info0.values())
        want = _want_texture(inst0, img[i], "range")
        assert len(info1) > 0
        for lab, e in info1.items():
            assert e["texture"] == want[lab], (i, lab)
            assert "features" not in e
    inst2, info2 = PP.process(z["pred"][0], nr_types=nt, features=True, texture="fixed", image=img[0])
    want = _want_texture(inst2, img[0], "fixed")
    assert all(e["texture"] == want[lab] and len(e["features"]["mean_rgb"]) == 3 for lab, e in info2.items())


@pytest.fixture(scope="module")
def net():
    from hover_net_amd import net_desc
    from hover_net_amd.synth import synth_state_dict

    model = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    model.load_state_dict(synth_state_dict("original", 5, seed=51), strict=True)
    return model.to("cuda").eval()


def _tile_images():
    from hover_net_amd.synth import synth_tiles

    return [synth_tiles(1, 270, seed=52)[0], synth_tiles(1, 270, seed=53)[0][:170, :121]]       # 170 x 121: no multiple of the 80-px step


@pytest.fixture(scope="module")
def tile_results(net):
    """The two synthetic tiles through tile mode once, shared: plain, with features only, with features and "fixed" texture."""
    from hover_net_amd import infer_tile

    images = _tile_images()
    return (images, infer_tile.process_images(images, net, nr_types=5, batch_size=8),
            infer_tile.process_images(images, net, nr_types=5, batch_size=8, return_features=True),
            infer_tile.process_images(images, net, nr_types=5, batch_size=8, return_features=True, return_texture="fixed"))


def test_tile_mode_features_and_texture(tile_results):
    images, plain, feats, got = tile_results
    entries = 0
    for img, (inst0, info0), (_, info_f), (inst1, info1) in zip(images, plain, feats, got):
        np.testing.assert_array_equal(inst1, inst0)
        assert_same_info(info1, info0)
        want = _want_texture(inst1, img, "fixed")
        for lab, e in info1.items():
            assert e["texture"] == want[lab], lab
            assert e["features"] == info_f[lab]["features"]
        assert all("texture" not in e for e in info_f.values())
        entries += len(info1)
    assert entries > 0


def test_process_file_list_save_texture(net, tile_results, tmp_path):
    from hover_net_amd import infer_manager

    images, plain, _, _ = tile_results
    inp = tmp_path / "in"
    inp.mkdir()
    for name, img in zip("ab", images):
        np.save(inp / (name + ".npy"), img)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "batch_size": 8}
        if flag:
            args["save_texture"] = True
        assert mgr.process_file_list(args) == ["a", "b"]
        for name, img, (inst, info) in zip("ab", images, plain):
            nuc = json.load(open(out / "json" / (name + ".json")))["nuc"]
            assert sorted(int(k) for k in nuc) == sorted(info)
            want = _want_texture(inst, img, "range")
            for k, e in nuc.items():
                if flag:
                    assert e["texture"] == want[int(k)] and set(e) == {"bbox", "centroid", "contour", "type_prob", "type", "texture"}
                else:
                    assert set(e) == {"bbox", "centroid", "contour", "type_prob", "type"}

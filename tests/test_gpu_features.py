"""-m gpu: the per-nucleus feature pass (csrc/hvn_features.hip) against the numpy / scipy oracle tests/features_ref.py, from the C ABI
(`PostProc.features`) up through `process_batch_device`, `process`, tile mode, the managers and the whole-slide stitch.  The device
fields are integers: everything is compared with ==; the float features are `features.derive` of the oracle's integers."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import features_ref as R
from golden_util import assert_same_info

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "proc_*.npz")))
IDS = [os.path.basename(p)[5:-4] for p in CASES]


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


def _host(rec, feat):
    from hover_net_amd import features as F
    from hover_net_amd import post_proc as PP

    n, m = rec.shape[:2]
    return rec.cpu().numpy().view(PP._REC_DTYPE).reshape(n, m), feat.cpu().numpy().view(F.FEAT_DTYPE).reshape(n, m)


def _assert_sums(got, want, what):
    for k in R.INT_FIELDS:
        assert got[k].tolist() == want[k].tolist(), (what, k)


def _check(maps, image=None, max_inst=None):
    """The device fields of every slot of every map == the oracle's, and seen == area; -> (records, features) on the host."""
    maps = np.ascontiguousarray(maps, np.int32)
    maps = maps[None] if maps.ndim == 2 else maps
    image = None if image is None else (image[None] if image.ndim == 3 else image)
    max_inst = max(int(maps.max()), 1) if max_inst is None else max_inst
    inst = torch.from_numpy(maps).to("cuda")
    rec = _table(inst, max_inst)
    feat = _pp().features(inst, rec, None if image is None else torch.from_numpy(np.ascontiguousarray(image)).to("cuda"))
    assert feat.shape == (maps.shape[0], max_inst, 88) and feat.dtype == torch.uint8
    rec_h, feat_h = _host(rec, feat)
    for i in range(maps.shape[0]):
        _assert_sums(feat_h[i], R.map_sums(maps[i], max_inst, None if image is None else image[i]), "map %d" % i)
        assert feat_h[i]["seen"].tolist() == rec_h[i]["area"].tolist()
        if image is None:
            assert not feat_h[i]["csum"].any() and not feat_h[i]["csq"].any()
    return rec_h, feat_h


def _blobs(h, w, seed, sigma=2.0, q=0.55):
    """A label map of random blobs: the 4-connected components of a thresholded smooth field (holes, ragged borders, edge contact)."""
    rng = np.random.default_rng(seed)
    field = ndimage.gaussian_filter(rng.normal(size=(h, w)), sigma, mode="constant")
    return ndimage.label(field > np.quantile(field, q))[0].astype(np.int32)


def _image(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)


# -- 1: integer fields ------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (64, 64), (67, 131)])
@pytest.mark.parametrize("with_image", [False, True])
def test_map_sizes(h, w, with_image):
    maps = np.ones((1, 1), np.int32) if (h, w) == (1, 1) else _blobs(h, w, seed=h * w, sigma=1.0 if h < 8 else 2.0)
    assert maps.max() >= 1
    _check(maps, _image((h, w), 5) if with_image else None)


def test_three_maps_with_different_content_in_one_call():
    maps = np.stack([_blobs(67, 131, seed=s, q=q) for s, q in ((1, 0.5), (2, 0.7), (3, 0.3))])
    assert len({int(m.max()) for m in maps}) == 3
    _check(maps, _image(maps.shape, 9))


def _shape(name):
    m = np.zeros((24, 40), np.int32)
    if name == "all_four_edges":
        m[:, 17] = 1
        m[11, :] = 1
        m[5:20, 10:30] = 1
    elif name == "single_pixel":
        m[7, 9] = 1
    elif name == "corner_pixels":
        m[0, 0] = 1
        m[23, 39] = 2
    elif name == "hline":
        m[6, 4:30] = 1
    elif name == "vline":
        m[2:22, 13] = 1
    elif name == "diagonal":
        for k in range(20):
            m[2 + k, 5 + k] = 1
        for k in range(15):
            m[20 - k, 22 + k] = 2           # the other diagonal
    elif name == "ring_with_a_label_in_its_hole":
        m[3:20, 5:30] = 1
        m[7:16, 10:25] = 0
        m[9:14, 13:22] = 2
        m[11, 16] = 0                      # and a hole in that one
    elif name == "shared_long_edge":
        m[4:12, 3:36] = 1
        m[12:20, 3:36] = 2
        m[4:20, 36:39] = 3                 # and a vertical one
    elif name == "two_pieces":
        m[2:8, 3:12] = 1
        m[14:22, 25:38] = 1
        m[10:13, 14:20] = 2                # another label inside the first one's bbox
    elif name == "checkerboard":
        yy, xx = np.mgrid[0:24, 0:40]
        m[(yy + xx) % 2 == 0] = 1          # every pixel a border pixel with diagonal neighbours only
    elif name == "full_map":
        m[:] = 1
    else:
        raise KeyError(name)
    return m


SHAPES = ["all_four_edges", "single_pixel", "corner_pixels", "hline", "vline", "diagonal", "ring_with_a_label_in_its_hole",
          "shared_long_edge", "two_pieces", "checkerboard", "full_map"]


@pytest.mark.parametrize("name", SHAPES)
def test_hand_shapes(name):
    m = _shape(name)
    _check(m, _image(m.shape, 3))
    _check(m)


@pytest.mark.parametrize("width", [59, 60, 61, 64, 65, 120, 121, 129])
def test_wide_bboxes(width):
    """A strip owns 60 columns: 60 | 61 and 120 | 121 are where the number of strips changes; 64, 65 and 129 are the word sizes a
    one-word-per-row form would break at.  Dense noise, so every strip boundary cuts through border pixels."""
    rng = np.random.default_rng(width)
    m = np.zeros((14, width + 7), np.int32)
    m[2:13, 3:3 + width] = rng.random((11, width)) < 0.7
    m[2:13, 3] = 1
    m[2:13, 3 + width - 1] = 1             # the bbox is exactly `width` columns
    m[m == 0] = (rng.random(m.shape) < 0.3)[m == 0] * 2      # a second label in the gaps and around
    rec_h, _ = _check(m, _image(m.shape, width))
    assert int(rec_h[0]["cmax"][0] - rec_h[0]["cmin"][0]) == width


def test_max_inst_smaller_than_the_largest_label():
    m = _blobs(40, 50, seed=11, sigma=1.5)
    assert m.max() > 6
    _, feat_h = _check(m, _image(m.shape, 1), max_inst=4)     # labels 5.. are background to everyone
    assert feat_h.shape == (1, 4)


def test_random_uint8_image_reaches_255_squared():
    m = np.zeros((30, 30), np.int32)
    m[2:28, 2:28] = 1
    img = _image(m.shape, 17)
    img[5:9, 5:9] = 255
    _, feat_h = _check(m, img)
    assert int(feat_h[0]["csq"][0].max()) > 255 * 255 * 16
    _, none_h = _check(m, None)
    for k in ("sxx", "syy", "sxy", "seen", "per"):
        assert none_h[k].tolist() == feat_h[k].tolist()


# -- 2: same-map and stale tables --------------------------------------------------------------------------
def test_stale_table_stays_inside_the_map_and_shows_in_seen():
    """A table whose boxes do not belong to the map (shifted, partly outside) on a VALID map: the call returns OK, the bbox is
    clamped to the map by construction, `seen` counts the label inside the clamped box and differs from `area`."""
    from hover_net_amd import features as F
    from hover_net_amd import post_proc as PP

    m = _blobs(48, 60, seed=21)
    max_inst = int(m.max())
    inst = torch.from_numpy(m[None]).to("cuda")
    rec = _table(inst, max_inst)
    rec_h = rec.cpu().numpy().view(PP._REC_DTYPE).reshape(max_inst).copy()
    for k, d in (("rmin", 7), ("rmax", 7), ("cmin", -9), ("cmax", -9)):
        rec_h[k][rec_h["area"] > 0] += d
    stale = torch.from_numpy(rec_h.view(np.uint8).reshape(1, max_inst, -1)).to("cuda")
    feat = _pp().features(inst, stale).cpu().numpy().view(F.FEAT_DTYPE).reshape(max_inst)
    torch.cuda.synchronize()
    want = []
    for j in range(max_inst):
        r0, r1 = max(int(rec_h["rmin"][j]), 0), min(int(rec_h["rmax"][j]), 48)
        c0, c1 = max(int(rec_h["cmin"][j]), 0), min(int(rec_h["cmax"][j]), 60)
        want.append(int(np.count_nonzero(m[r0:r1, c0:c1] == j + 1)) if rec_h["area"][j] > 0 and r0 < r1 and c0 < c1 else 0)
    assert feat["seen"].tolist() == want
    assert (feat["seen"] != rec_h["area"]).any()


# -- 3: golden maps through the public path ----------------------------------------------------------------
def _want_features(inst_map, image, with_colour):
    """{label: features dict} of every label of a host label map: `derive` of the oracle's integers."""
    from hover_net_amd import features as F
    from hover_net_amd import post_proc as PP

    max_inst = max(int(inst_map.max()), 1)
    t, s = R.table(inst_map, max_inst), R.map_sums(inst_map, max_inst, image)
    rec = np.zeros(max_inst, PP._REC_DTYPE)
    for k in t:
        rec[k] = t[k]
    feat = np.zeros(max_inst, F.FEAT_DTYPE)
    for k in R.INT_FIELDS:
        feat[k] = s[k]
    dicts = F.to_dicts(F.derive(rec, feat, with_colour))
    return {j + 1: dicts[j] for j in range(max_inst) if rec["area"][j] > 0}


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_goldens_batched_and_process(path):
    from hover_net_amd import features as F
    from hover_net_amd import post_proc as PP

    z = np.load(path)
    nt = None if int(z["nr_types"]) < 0 else int(z["nr_types"])
    pred = torch.from_numpy(z["pred"]).to("cuda")
    img = _image(z["pred"].shape[:3], 31)
    plain = PP.process_batch_device(pred, nt, True)
    out = PP.process_batch_device(pred, nt, True, return_features=True, image=torch.from_numpy(img).to("cuda"))
    assert len(plain) == 3 and len(out) == 4
    for a, b in zip(plain, out):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(out[0].cpu().numpy(), z["inst"])
    rec_h, feat_h = _host(out[1], out[3])
    for i in range(pred.shape[0]):
        _assert_sums(feat_h[i], R.map_sums(z["inst"][i], rec_h.shape[1], img[i]), i)
        assert feat_h[i]["seen"].tolist() == rec_h[i]["area"].tolist()
    # contours first, features LAST; no image -> shape features only
    both = PP.process_batch_device(pred, nt, True, return_contours=True, return_features=True)
    assert len(both) == 7 and both[6].shape == out[3].shape
    shape_only = both[6].cpu().numpy().view(F.FEAT_DTYPE).reshape(feat_h.shape)
    assert not shape_only["csum"].any() and shape_only["per"].tolist() == feat_h["per"].tolist()
    for i in (0, pred.shape[0] - 1):
        inst0, info0 = PP.process(z["pred"][i], nr_types=nt, return_centroids=True)
        inst1, info1 = PP.process(z["pred"][i], nr_types=nt, return_centroids=True, features=True, image=img[i])
        np.testing.assert_array_equal(inst1, inst0)
        assert_same_info(info1, info0)
        assert all("features" not in e for e in info0.values())
        want = _want_features(inst0, img[i], True)
        for lab, e in info1.items():
            assert e["features"] == want[lab], (i, lab)
        inst2, info2 = PP.process(z["pred"][i], nr_types=nt, features=True)             # implies the dict; no colour entries
        np.testing.assert_array_equal(inst2, inst0)
        want = _want_features(inst0, None, False)
        assert list(info2) == list(info0) and all(info2[lab]["features"] == want[lab] for lab in info2)


# -- 4: negative -------------------------------------------------------------------------------------------
def test_bad_image_raises_before_any_launch(monkeypatch):
    from hover_net_amd import post_proc as PP

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    pred = torch.zeros((2, 20, 24, 3), dtype=torch.float32, device="cuda")
    inst = torch.zeros((2, 20, 24), dtype=torch.int32, device="cuda")
    rec = _table(inst, 3)
    good = torch.zeros((2, 20, 24, 3), dtype=torch.uint8, device="cuda")
    pp = _pp()
    monkeypatch.setattr(PP.PostProc, "separate", no_launch)
    monkeypatch.setattr(PP.L, "lib", no_launch)
    with pytest.raises(TypeError):
        PP.process_batch_device(pred, None, True, return_features=True, image=good.float())
    with pytest.raises(ValueError):
        PP.process_batch_device(pred, None, True, return_features=True, image=good[:, :, :23])
    with pytest.raises(ValueError):
        PP.process_batch_device(pred, None, True, return_features=True, image=good[:1])
    with pytest.raises(ValueError):
        PP.process_batch_device(pred, None, True, return_features=True, image=good.cpu())
    with pytest.raises(ValueError):
        PP.process_batch_device(pred, None, True, image=good)                         # an image nobody reads
    with pytest.raises(TypeError):
        pp.features(inst, rec, good.to(torch.int32))
    with pytest.raises(ValueError):
        pp.features(inst, rec, good[..., :2])
    with pytest.raises(TypeError):
        PP.process(np.zeros((20, 24, 3), np.float32), features=True, image=np.zeros((20, 24, 3), np.float32))
    with pytest.raises(ValueError):
        PP.process(np.zeros((20, 24, 3), np.float32), features=True, image=np.zeros((24, 20, 3), np.uint8))


def test_c_abi_refuses_bad_arguments():
    from hover_net_amd import lib as L

    inst = torch.zeros((1, 8, 8), dtype=torch.int32, device="cuda")
    rec = _table(inst, 2)
    feat = torch.zeros((1, 2, 88), dtype=torch.uint8, device="cuda")
    f = L.lib().hvn_instance_features
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lib().hvn_instance_features_workspace_bytes(1, 8, 8, 2) == 0
    assert f(inst.data_ptr(), None, 1, 8, 8, rec.data_ptr(), 2, feat.data_ptr(), None, 0, s) == 0
    assert f(None, None, 1, 8, 8, rec.data_ptr(), 2, feat.data_ptr(), None, 0, s) == -1
    assert f(inst.data_ptr(), None, 1, 8, 8, None, 2, feat.data_ptr(), None, 0, s) == -1
    assert f(inst.data_ptr(), None, 1, 8, 8, rec.data_ptr(), 2, None, None, 0, s) == -1
    assert f(inst.data_ptr(), None, 0, 8, 8, rec.data_ptr(), 2, feat.data_ptr(), None, 0, s) == -1
    assert f(inst.data_ptr(), None, 1, 8, 8, rec.data_ptr(), 0, feat.data_ptr(), None, 0, s) == -1
    assert f(inst.data_ptr(), None, 1, 8, 8, rec.data_ptr(), 2, feat.data_ptr() + 4, None, 0, s) == -1
    assert f(inst.data_ptr(), None, 65536, 8, 8, rec.data_ptr(), 65536, feat.data_ptr(), None, 0, s) == -4
    torch.cuda.synchronize()
    assert not feat.any()


# -- 5: tile mode, the managers, whole slides --------------------------------------------------------------
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


def test_tile_mode_features_with_colour(net):
    from hover_net_amd import infer_tile

    images = _tile_images()
    plain = infer_tile.process_images(images, net, nr_types=5, batch_size=8)
    got = infer_tile.process_images(images, net, nr_types=5, batch_size=8, return_features=True)
    raw = infer_tile.process_images(images, net, nr_types=5, batch_size=8, return_raw=True, return_features=True)
    entries = 0
    for img, (inst0, info0), (inst1, info1), with_raw in zip(images, plain, got, raw):
        np.testing.assert_array_equal(inst1, inst0)
        assert_same_info(info1, info0)
        want = _want_features(inst1, img, True)
        for lab, e in info1.items():
            assert e["features"] == want[lab], lab
            assert len(e["features"]["mean_rgb"]) == 3
        entries += len(info1)
        assert len(with_raw) == 3 and with_raw[2].shape == img.shape[:2] + (4,) and with_raw[2].dtype == np.float32
        assert {k: v["features"] for k, v in with_raw[1].items()} == {k: v["features"] for k, v in info1.items()}
    assert entries > 0


def test_process_file_list_save_features(net, tmp_path):
    from hover_net_amd import infer_manager, infer_tile

    images = _tile_images()
    inp = tmp_path / "in"
    inp.mkdir()
    for name, img in zip("ab", images):
        np.save(inp / (name + ".npy"), img)
    want = infer_tile.process_images(images, net, nr_types=5, batch_size=8, return_features=True)
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    for flag in (True, False):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "batch_size": 8}
        if flag:
            args["save_features"] = True
        assert mgr.process_file_list(args) == ["a", "b"]
        for name, (_inst, info) in zip("ab", want):
            nuc = json.load(open(out / "json" / (name + ".json")))["nuc"]
            assert sorted(int(k) for k in nuc) == sorted(info)
            for k, e in nuc.items():
                if flag:
                    assert e["features"] == info[int(k)]["features"]
                else:
                    assert set(e) == {"bbox", "centroid", "contour", "type_prob", "type"}


def _wsi_maps(h, w, seed):
    from hover_net_amd.synth import synth_pred_maps

    return torch.from_numpy(synth_pred_maps(1, h, w, 5, seed=seed, k_lo=4, k_hi=12)[0][0]).to("cuda")


def test_wsi_smaller_than_one_tile(net):
    from hover_net_amd import infer_wsi

    maps = _wsi_maps(300, 340, 91)
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    inst0, info0 = infer_wsi.WsiInference(net, **kw).stitch_instances(maps)
    wsi = infer_wsi.WsiInference(net, features=True, **kw)
    inst1, info1 = wsi.stitch_instances(maps)
    assert any("feat" in s for ring in wsi._slots.values() for s in ring["slots"])      # the bytes came through the pinned slots
    np.testing.assert_array_equal(inst1, inst0)
    assert_same_info(info1, info0)
    assert len(info1) > 20 and all("features" not in e for e in info0.values())
    want = _want_features(inst1, None, False)
    for lab, e in info1.items():
        assert e["features"] == want[lab], lab
        assert "mean_rgb" not in e["features"]


def test_wsi_two_by_two_tiles(net, monkeypatch):
    from hover_net_amd import infer_wsi

    maps = _wsi_maps(900, 1000, 92)
    kw = dict(nr_types=5, batch_size=8, tile_shape=512, ambiguous_size=64)
    inst0, info0 = infer_wsi.WsiInference(net, **kw).stitch_instances(maps)
    inst1, info1 = infer_wsi.WsiInference(net, features=True, **kw).stitch_instances(maps)
    np.testing.assert_array_equal(inst1, inst0)
    assert_same_info(info1, info0)                      # ids, bbox, centroid, contour, type
    assert len(info1) > 100
    for lab, e in info1.items():
        f = e["features"]
        box = (e["bbox"][1][0] - e["bbox"][0][0]) * (e["bbox"][1][1] - e["bbox"][0][1])
        assert 0 < f["area"] <= box and f["extent"] == f["area"] / box, lab
        assert f["perimeter"] >= 0 and f["major_axis_length"] >= f["minor_axis_length"] >= 0
    # the host merger carries the entries the same way
    monkeypatch.setenv("HVN_WSI_HOST_MERGE", "1")
    inst2, info2 = infer_wsi.WsiInference(net, features=True, **kw).stitch_instances(maps)
    np.testing.assert_array_equal(inst2, inst0)
    assert {k: v["features"] for k, v in info2.items()} == {k: v["features"] for k, v in info1.items()}


def test_wsi_manager_save_features(net, tmp_path, monkeypatch):
    """The manager's switch down to the json.  Stage 1 is not what this is about (and seeded noise through the synthetic network
    leaves a 300 x 340 slide without a nucleus), so it is replaced by a structured prediction map."""
    from PIL import Image

    from hover_net_amd import infer_manager, infer_wsi
    from hover_net_amd.synth import synth_tiles

    maps = _wsi_maps(300, 340, 91)
    monkeypatch.setattr(infer_wsi.WsiInference, "raw_prediction", lambda self, slide, mask, as_slab=False: infer_wsi.SlabMap(maps, 0))
    inp = tmp_path / "in"
    inp.mkdir()
    np.save(inp / "s.npy", synth_tiles(1, 340, seed=95)[0][:300])
    msk = tmp_path / "msk"
    msk.mkdir()
    Image.fromarray(np.full((10, 11), 255, np.uint8)).save(msk / "s.png")      # all tissue
    mgr = infer_manager.WsiManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    nuc = {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out), "input_mask_dir": str(msk), "batch_size": 8, "tile_shape": 512, "chunk_shape": 1000,
                "ambiguous_size": 64}
        if flag:
            args["save_features"] = True
        assert mgr.process_wsi_list(args) == {"s": "done"}
        nuc[flag] = json.load(open(out / "s.json"))["nuc"]
    assert list(nuc[True]) == list(nuc[False]) and len(nuc[True]) > 20
    for k, e in nuc[True].items():
        assert {x: e[x] for x in e if x != "features"} == nuc[False][k]
        assert set(e["features"]) == {"area", "vxx", "vyy", "vxy", "major_axis_length", "minor_axis_length", "eccentricity", "orientation",
                                      "perimeter", "equivalent_diameter", "extent", "circularity"}

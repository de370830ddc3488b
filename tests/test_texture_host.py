"""The per-nucleus texture on the CPU (hover_net_amd/texture.py): `sums_host` against the per-pixel loops of tests/texture_ref.py with ==,
the identities of the co-occurrence counts, `derive` against the oracle's centred float formulas, the degenerate nuclei by hand, the
header facts, every refusal that include/hvn.h lists for HVN_OP_INST_TEXTURE, and the Python-side refusals before any launch."""
import ctypes
import json
import math
import re

import numpy as np
import pytest
import torch

import texture_ref as R
from hover_net_amd import texture as TX

SCALES = ["range", "fixed"]


def _rec(inst, max_inst=None, boxes=None):
    """`post_proc._REC_DTYPE` records of one map, from the oracle's boxes."""
    from hover_net_amd import post_proc as PP

    max_inst = max(int(np.asarray(inst).max()), 1) if max_inst is None else max_inst
    boxes = R.boxes_of(inst, max_inst) if boxes is None else boxes
    rec = np.zeros(max_inst, PP._REC_DTYPE)
    for j, (area, rmin, rmax, cmin, cmax) in enumerate(boxes):
        rec[j]["label"], rec[j]["area"], rec[j]["rmin"], rec[j]["rmax"], rec[j]["cmin"], rec[j]["cmax"] = j + 1, area, rmin, rmax, cmin, cmax
    return rec


def _check(inst, image, scale, max_inst=None):
    rec = _rec(inst, max_inst)
    got = TX.sums_host(inst, rec, image, scale)
    assert got.dtype == TX.TEX_DTYPE and got.shape == rec.shape
    R.assert_equal(got, R.map_sums(inst, image, rec.shape[0], scale), scale)
    assert got["seen"].tolist() == rec["area"].tolist() and not got["reserved"].any()
    return got


# -- 1: host == oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("h,w", R.SIZES)
def test_map_sizes(h, w, scale):
    _check(R.sized_map(h, w), R.image((h, w), 5), scale)


@pytest.mark.parametrize("scale", SCALES)
def test_three_maps_in_one_call(scale):
    maps = R.three_maps()
    img = R.image(maps.shape, 9)
    max_inst = int(maps.max())
    rec = np.stack([_rec(m, max_inst) for m in maps])
    got = TX.sums_host(maps, rec, img, scale)
    assert got.shape == (3, max_inst)
    for i in range(3):
        R.assert_equal(got[i], R.map_sums(maps[i], img[i], max_inst, scale), i)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", R.SHAPES)
def test_hand_shapes(name, scale):
    m = R.shape(name)
    got = _check(m, R.image(m.shape, 3), scale)
    if name in R.ONLY:
        for j in range(got.shape[0]):
            assert [d for d in range(4) if got["glcm"][j, d].any()] == list(R.ONLY[name]), (name, j)


def test_smooth_image_and_max_inst_below_the_largest_label():
    m = R.blobs(40, 50, seed=11, sigma=1.5)
    assert m.max() > 6
    for scale in SCALES:
        assert _check(m, R.smooth_image(m.shape, 2), scale, max_inst=4).shape == (4,)


def test_stale_table_is_clamped_and_shows_in_seen():
    m = R.blobs(48, 60, seed=21)
    img = R.image(m.shape, 4)
    max_inst = int(m.max())
    boxes = [(a, r0 + 7, r1 + 7, c0 - 9, c1 - 9) if a else (a, r0, r1, c0, c1) for a, r0, r1, c0, c1 in R.boxes_of(m, max_inst)]
    rec = _rec(m, max_inst, boxes)
    for scale in SCALES:
        got = TX.sums_host(m, rec, img, scale)
        R.assert_equal(got, R.map_sums(m, img, max_inst, scale, boxes), scale)
        want = [int(np.count_nonzero(m[max(r0, 0):min(r1, 48), max(c0, 0):min(c1, 60)] == j + 1)) if a else 0 for j, (a, r0, r1, c0, c1) in enumerate(boxes)]
        assert got["seen"].tolist() == want and (got["seen"] != rec["area"]).any()
        empty = got[got["seen"] == 0]
        assert len(empty) and not empty.view(np.int32).any()             # a box that finds nothing is 276 zero words


# -- 2: identities -------------------------------------------------------------------------------------------
def _pairs(mask, dx, dy):
    h, w = mask.shape
    src = mask[0:h - dy, (1 if dx < 0 else 0):(w - 1 if dx > 0 else w)]
    dst = mask[dy:h, (1 if dx > 0 else 0):(w - 1 if dx < 0 else w)]
    return int(np.count_nonzero(src & dst))


@pytest.mark.parametrize("scale", SCALES)
def test_identities(scale):
    m = R.blobs(64, 64, seed=7)
    img = R.smooth_image(m.shape, 8)
    got = TX.sums_host(m, _rec(m), img, scale)
    assert got["hist"].sum(axis=1).tolist() == got["seen"].tolist()
    for j in range(got.shape[0]):
        mask = m == j + 1
        assert _pairs(mask, 1, 0) == int(np.count_nonzero(mask[:, :-1] & mask[:, 1:]))
        for d, (dx, dy) in enumerate(R.OFFSETS):
            assert int(got["glcm"][j, d].sum()) == _pairs(mask, dx, dy), (j, d)
    # a transposed map swaps d = 0 with d = 2 (and keeps (a, b): the upper / left pixel stays the first)
    mt, it = np.ascontiguousarray(m.T), np.ascontiguousarray(img.transpose(1, 0, 2))
    tr = TX.sums_host(mt, _rec(mt, got.shape[0]), it, scale)
    assert tr["glcm"][:, 0].tolist() == got["glcm"][:, 2].tolist() and tr["glcm"][:, 2].tolist() == got["glcm"][:, 0].tolist()
    assert tr["glcm"][:, 1].tolist() == got["glcm"][:, 1].tolist() and tr["hist"].tolist() == got["hist"].tolist()
    # a left-right flip swaps d = 1 with d = 3 and transposes d = 0
    mf, jf = np.ascontiguousarray(m[:, ::-1]), np.ascontiguousarray(img[:, ::-1])
    fl = TX.sums_host(mf, _rec(mf, got.shape[0]), jf, scale)
    assert fl["glcm"][:, 1].tolist() == got["glcm"][:, 3].tolist() and fl["glcm"][:, 3].tolist() == got["glcm"][:, 1].tolist()
    assert fl["glcm"][:, 0].tolist() == got["glcm"][:, 0].transpose(0, 2, 1).tolist() and fl["glcm"][:, 2].tolist() == got["glcm"][:, 2].tolist()


def test_a_horizontal_ramp_is_strictly_upper_triangular():
    """Grey rises with x, so the right neighbour's level is never lower: a swapped (a, b) would fill the lower triangle."""
    m = np.zeros((12, 70), np.int32)
    m[2:10, 3:67] = 1
    img = np.zeros(m.shape + (3,), np.uint8)
    img[:] = (np.arange(70) * 3 + 20).astype(np.uint8)[None, :, None]
    for scale in SCALES:
        got = _check(m, img, scale)
        c = got["glcm"][0, 0]
        assert np.triu(c, 1).sum() > 0 and not np.tril(c, -1).any()
        assert not np.tril(got["glcm"][0, 1], -1).any() and not np.triu(got["glcm"][0, 3], 1).any()     # (1, 1) rises too, (-1, 1) falls


# -- 3: derive -----------------------------------------------------------------------------------------------
def _assert_derived(inst, image, scale):
    got = TX.sums_host(inst, _rec(inst), image, scale)
    d = TX.derive(got)
    want = R.map_sums(inst, image, got.shape[0], scale)
    checked = 0
    for j in range(got.shape[0]):
        if got["seen"][j] == 0:
            assert not any(d[k][j] for k in d.dtype.names)
            continue
        ref = R.float_features({"glcm": want["glcm"][j]})
        ref.update(R.grey_features(R.mask_values(inst, image, j + 1), want["hist"][j]))
        for k in R.GLCM_FIELDS + R.GREY_FIELDS:
            np.testing.assert_allclose(d[k][j], ref[k], rtol=1e-9, atol=1e-9, err_msg="%s slot %d" % (k, j))
        checked += 1
    return checked


@pytest.mark.parametrize("scale", SCALES)
def test_derive_against_the_centred_floats(scale):
    n = _assert_derived(R.blobs(67, 131, seed=3), R.smooth_image((67, 131), 6), scale)
    n += _assert_derived(R.blobs(64, 64, seed=5), R.image((64, 64), 7), scale)
    m = np.zeros((130, 130), np.int32)
    m[1:129, 1:129] = 1                                                   # 128 px across
    n += _assert_derived(m, R.smooth_image(m.shape, 12), scale)
    assert n > 30


def test_derive_of_big_counts_takes_the_exact_path():
    """Counts near 2^31 make N^2 pass 2^62: the Python-int path gives what scaled-down counts give."""
    small = np.zeros(1, TX.TEX_DTYPE)
    small["seen"], small["gsum"], small["hi"] = 4, [[400, 40400, 4120000, 424040000]], 101
    small["lo"] = 99
    small["hist"][0, :2] = [3, 1]
    small["glcm"][0, 0, :2, :2] = [[5, 3], [1, 2]]
    big = small.copy()
    big["glcm"] = small["glcm"] * (1 << 27)
    a, b = TX.derive(small), TX.derive(big)
    for k in R.GLCM_FIELDS:
        np.testing.assert_allclose(b[k], a[k], rtol=1e-15, atol=0)


def test_to_dicts_is_plain_json():
    m = R.blobs(40, 50, seed=11, sigma=1.5)
    dicts = TX.to_dicts(TX.derive(TX.sums_host(m, _rec(m), R.image(m.shape, 1))))
    assert len(dicts) == int(m.max()) and set(dicts[0]) == set(R.GLCM_FIELDS + R.GREY_FIELDS)
    assert all(type(v) is float for e in dicts for v in e.values())
    assert json.loads(json.dumps(dicts)) == dicts
    by_bytes = TX.derive(TX.sums_host(m, _rec(m), R.image(m.shape, 1)).view(np.uint8).reshape(-1, 1104))
    assert TX.to_dicts(by_bytes) == dicts


# -- 4: degenerate nuclei by hand ----------------------------------------------------------------------------
def _one(m, img, scale="range"):
    got = TX.sums_host(m, _rec(m), img, scale)
    return got[0], TX.to_dicts(TX.derive(got))[0]


def test_single_pixel():
    m = R.shape("single_pixel")
    img = np.zeros(m.shape + (3,), np.uint8)
    img[7, 9] = (200, 100, 50)
    g = (77 * 200 + 150 * 100 + 29 * 50 + 128) >> 8
    for scale in SCALES:
        s, d = _one(m, img, scale)
        assert s["seen"] == 1 and s["lo"] == s["hi"] == g and s["gsum"].tolist() == [g, g ** 2, g ** 3, g ** 4] and not s["glcm"].any()
        assert s["hist"].tolist() == [1 if q == (0 if scale == "range" else g >> 5) else 0 for q in range(8)]
        assert [d[k] for k in R.GLCM_FIELDS] == [0.0] * 7                 # no direction has pairs
        assert d["grey_mean"] == g and d["grey_min"] == d["grey_max"] == g
        assert d["grey_std"] == d["grey_skewness"] == d["grey_kurtosis"] == d["grey_entropy"] == 0.0


def test_flat_nucleus():
    m = np.zeros((10, 12), np.int32)
    m[2:8, 3:9] = 1
    img = np.full(m.shape + (3,), 90, np.uint8)                            # grey 90 everywhere: span = 1, every level 0
    s, d = _one(m, img)
    assert s["lo"] == s["hi"] == 90 and s["hist"].tolist() == [36, 0, 0, 0, 0, 0, 0, 0]
    assert [int(s["glcm"][k, 0, 0]) for k in range(4)] == [30, 25, 30, 25] and int(s["glcm"].sum()) == 110
    assert d["correlation"] == 1.0 and d["entropy"] == 0.0 and d["contrast"] == 0.0 and d["dissimilarity"] == 0.0
    assert d["homogeneity"] == 1.0 and d["asm"] == 1.0 and d["energy"] == 1.0
    assert d["grey_mean"] == 90.0 and d["grey_std"] == 0.0 and d["grey_skewness"] == 0.0 and d["grey_kurtosis"] == 0.0 and d["grey_entropy"] == 0.0
    s, d = _one(m, img, "fixed")
    assert s["hist"].tolist() == [0, 0, 36, 0, 0, 0, 0, 0] and int(s["glcm"][0, 2, 2]) == 30 and d["correlation"] == 1.0 and d["entropy"] == 0.0


def test_two_level_image_by_hand():
    """A 2 x 4 nucleus, left half grey 10, right half grey 20: levels 0 and 7 under "range" (span 11, (10 * 8) // 11 = 7), level 0
    for both under "fixed"."""
    m = np.zeros((4, 6), np.int32)
    m[1:3, 1:5] = 1
    img = np.zeros(m.shape + (3,), np.uint8)
    img[:, :3] = 10
    img[:, 3:] = 20                                                        # grey(v, v, v) = (256 v + 128) >> 8 = v
    s, d = _one(m, img)
    hi_level = (10 * 8) // 11
    assert hi_level == 7 and s["lo"] == 10 and s["hi"] == 20 and s["hist"].tolist() == [4, 0, 0, 0, 0, 0, 0, 4]
    want = np.zeros((4, 8, 8), np.int64)
    want[0, 0, 0], want[0, 0, 7], want[0, 7, 7] = 2, 2, 2                  # per row: (0,0) (0,7) (7,7)
    want[1, 0, 0], want[1, 0, 7], want[1, 7, 7] = 1, 1, 1                  # one row of diagonals
    want[2, 0, 0], want[2, 7, 7] = 2, 2
    want[3, 0, 0], want[3, 7, 0], want[3, 7, 7] = 1, 1, 1
    assert s["glcm"].tolist() == want.tolist()
    assert s["gsum"].tolist() == [120, 4 * 100 + 4 * 400, 4 * 1000 + 4 * 8000, 4 * 10000 + 4 * 160000]
    # d = 0: S = [[4, 2], [2, 4]] on levels {0, 7}, N = 12; d = 1 and 3: S = [[2, 1], [1, 2]], N = 6; d = 2: S = diag(4, 4), N = 8
    contrast = (49 * 4 / 12 + 49 * 2 / 6 + 0 + 49 * 2 / 6) / 4
    np.testing.assert_allclose(d["contrast"], contrast, rtol=1e-12)
    np.testing.assert_allclose(d["dissimilarity"], (7 * 4 / 12 + 7 * 2 / 6 + 0 + 7 * 2 / 6) / 4, rtol=1e-12)
    np.testing.assert_allclose(d["homogeneity"], ((8 + 4 / 50) / 12 + (4 + 2 / 50) / 6 + 1 + (4 + 2 / 50) / 6) / 4, rtol=1e-12)
    np.testing.assert_allclose(d["asm"], (40 / 144 + 10 / 36 + 32 / 64 + 10 / 36) / 4, rtol=1e-12)
    # correlation of a symmetric two-point distribution with P(equal) = p: 2 p - 1
    np.testing.assert_allclose(d["correlation"], ((2 * 8 / 12 - 1) + (2 * 4 / 6 - 1) + 1 + (2 * 4 / 6 - 1)) / 4, rtol=1e-12)
    h3 = -(2 * (1 / 3) * math.log2(1 / 3) + 2 * (1 / 6) * math.log2(1 / 6))
    np.testing.assert_allclose(d["entropy"], (h3 + h3 + 1.0 + h3) / 4, rtol=1e-12)
    assert d["grey_mean"] == 15.0 and d["grey_std"] == 5.0 and d["grey_skewness"] == 0.0 and d["grey_kurtosis"] == 1.0 and d["grey_entropy"] == 1.0
    assert d["grey_min"] == 10.0 and d["grey_max"] == 20.0
    s, d = _one(m, img, "fixed")
    assert s["lo"] == 10 and s["hi"] == 20 and s["hist"].tolist() == [8, 0, 0, 0, 0, 0, 0, 0]      # the extremes are stored in both modes
    assert d["grey_min"] == 10.0 and d["grey_max"] == 20.0 and d["correlation"] == 1.0 and d["entropy"] == 0.0


def test_the_level_division_by_multiplication_is_exact():
    """csrc/hvn_texture.hip forms ((g - lo) * 8) / span as (n * ceil(2^20 / span)) >> 20: exact for every n and span it can meet."""
    n = np.arange(0, 2041, dtype=np.int64)
    for span in range(1, 257):
        magic = ((1 << 20) + span - 1) // span
        assert ((n * magic) >> 20).tolist() == (n // span).tolist(), span


# -- 5: the header facts ----------------------------------------------------------------------------------------
def test_op_kind_24_is_in_the_header_the_plan_and_the_sources():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    header = open(L.HEADER).read()
    assert PL.OP_INST_TEXTURE == 24 and "HVN_OP_INST_TEXTURE = 24" in header and " INST_TEXTURE " in header and "hvn_texture.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                       # no new export: the op goes through hvn_run_op
    words = int(re.search(r"#define HVN_TEX_WORDS (\d+)", header).group(1))
    levels = int(re.search(r"#define HVN_TEX_LEVELS (\d+)", header).group(1))
    assert words == 276 == TX.TEX_DTYPE.itemsize // 4 == TX.WORDS and levels == 8 == TX.LEVELS and words == 12 + levels + 4 * levels * levels
    assert [TX.TEX_DTYPE.fields[k][1] // 4 for k in ("gsum", "seen", "lo", "hi", "reserved", "hist", "glcm")] == [0, 8, 9, 10, 11, 12, 20]
    assert "struct InstTextureArgs" in open(L.CSRC + "/hvn_kernels.h").read()


# -- 6: the C side's refusals -------------------------------------------------------------------------------------
def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def _op():
    """A well-formed INST_TEXTURE op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    at = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    op = L.hvn_op()
    op.kind, op.cout = PL.OP_INST_TEXTURE, 100
    op.x.base, op.x.h, op.x.w, op.x.c = at(1), 64, 80, 3
    op.res.base, op.w, op.y.base = at(2), at(3), at(4)
    return op


# one entry per refusal that include/hvn.h lists for INST_TEXTURE: (field, value, status, a word of its text)
TEXTURE_REFUSALS = [("x.base", None, -1, b"null image"), ("res.base", None, -1, b"null inst"), ("w", None, -1, b"null records"),
                    ("y.base", None, -1, b"null output"), ("x.h", 0, -1, b"< 1"), ("x.w", -3, -1, b"< 1"), ("cout", 0, -1, b"< 1"),
                    ("x.h", 1 << 30, -1, b"h * w >= 2^31"), ("x.c", 4, -1, b"not c = 3 uint8"), ("x_dtype", 1, -1, b"not c = 3 uint8"),
                    ("x.sy", 3 * 80 + 16, -1, b"not dense"), ("x.sx", 4, -1, b"not dense"), ("x.sn", 8, -1, b"not dense"),
                    ("_rsv", 2, -1, b"no scale mode"), ("_rsv", -1, -1, b"no scale mode"), ("stride", 2, -1, b"no accumulation form"),
                    ("y.base", 0x14000004, -1, b"misaligned output or records"), ("w", 0x13000004, -1, b"misaligned output or records"),
                    ("res.base", 0x12000002, -1, b"misaligned inst"), ("cout", 1 << 30, -4, b"n * max_inst >= 2^31")]


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's INST_TEXTURE list: its status and a text of its own that leads with the op's name, decided before
    any launch (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as
    tests/test_forest_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code, word, lead=b"inst_texture:"):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(lead) and word in err and b"unknown op kind" not in err, (rc, err, word)

    texts = set()
    for path, value, code, word in TEXTURE_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 2 if code == -4 else 1, code, word)
        texts.add(word)
    assert len(texts) == 13                                           # each kind of refusal has a text of its own
    refused(_op(), 0, -1, b"bad arguments", lead=b"run_op:")          # n < 1 is hvn_run_op's own refusal
    op = _op()
    op.x.sy, op.x.sx, op.x.sn, op._rsv, op.stride, op.y.base = 3 * 80, 3, 3 * 80 * 64, 1, 1, None   # the dense strides spelled out pass
    refused(op, 3, -1, b"null output")
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1, b"null image")                               # an all-zero op is refused by name


def test_c_refusals_leave_the_output_untouched_on_the_host_side():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    buf = np.full(276 * 100, 0x5A5A5A5A, np.int32)
    for path, value in (("x.base", None), ("_rsv", 7), ("x.c", 1), ("cout", -1), ("x.h", 0), ("res.base", 0x12000001)):
        op = _op()
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()


# -- 7: the Python side's refusals, before any launch ---------------------------------------------------------------
def test_python_refusals_before_any_launch(monkeypatch, tmp_path):
    from hover_net_amd import infer_manager, infer_tile
    from hover_net_amd import post_proc as PP

    def no_launch(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(PP.L, "lib", no_launch)
    monkeypatch.setattr(PP.L, "require_gpu", no_launch)
    pred = np.zeros((20, 24, 3), np.float32)
    good = np.zeros((20, 24, 3), np.uint8)
    with pytest.raises(ValueError, match="needs the image"):
        PP.process(pred, texture=True)                                                   # texture without an image
    with pytest.raises(ValueError, match="needs the image"):
        PP.process_batch_device(torch.zeros((1, 20, 24, 3)), None, True, return_texture="range")
    with pytest.raises(TypeError):
        PP.process(pred, texture="fixed", image=good.astype(np.float32))                # a wrong dtype
    with pytest.raises(ValueError, match="does not match"):
        PP.process(pred, texture="fixed", image=good[:, :23])                           # a wrong shape
    with pytest.raises(TypeError):
        PP.process_batch_device(torch.zeros((1, 20, 24, 3)), None, True, return_texture="range", image=torch.zeros((1, 20, 24, 3)))
    with pytest.raises(ValueError, match="does not match"):
        PP.process_batch_device(torch.zeros((1, 20, 24, 3)), None, True, return_texture="range", image=torch.zeros((1, 20, 23, 3), dtype=torch.uint8))
    for bad in ("wide", 1, False, b"range"):
        with pytest.raises(ValueError, match="scale"):
            PP.process(pred, texture=bad, image=good)                                   # a bad scale
        with pytest.raises(ValueError, match="scale"):
            PP.process_batch_device(torch.zeros((1, 20, 24, 3)), None, True, return_texture=bad, image=torch.zeros((1, 20, 24, 3), dtype=torch.uint8))
        with pytest.raises(ValueError, match="scale"):
            infer_tile.process_images([good], None, return_texture=bad)
        with pytest.raises(ValueError, match="scale"):
            TX.sums_host(np.zeros((2, 2), np.int32), np.zeros(1, PP._REC_DTYPE), np.zeros((2, 2, 3), np.uint8), bad)
    with pytest.raises(ValueError, match="only used with"):
        PP.process(pred, image=good)                                                     # an image nobody reads is still refused
    method = {"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}
    (tmp_path / "in").mkdir()
    np.save(tmp_path / "in" / "a.npy", np.zeros((30, 30, 3), np.uint8))
    mgr = infer_manager.InferManager(method, process_fn=no_launch)
    with pytest.raises(ValueError, match="scale"):
        mgr.process_file_list({"input_dir": str(tmp_path / "in"), "output_dir": str(tmp_path / "out_tile"), "save_texture": "wide"})
    assert not (tmp_path / "out_tile").exists()
    wsi = infer_manager.WsiManager(method, wsi_fn=no_launch)
    for value in (True, "range", "fixed"):
        with pytest.raises(ValueError, match="prediction map"):
            wsi.process_wsi_list({"input_dir": str(tmp_path / "in"), "output_dir": str(tmp_path / "out_wsi"), "save_texture": value})
        assert not (tmp_path / "out_wsi").exists()                                       # refused before any file is touched

"""Host half of the per-nucleus features: hover_net_amd/features.py (`derive`, `to_dicts`) against the independent oracle
tests/features_ref.py.  No GPU."""
import json
import math

import numpy as np
import pytest

import features_ref as R
from hover_net_amd import features as F
from hover_net_amd import io_utils, post_proc


def _rec_feat(inst, image=None):
    """Structured record + feature arrays (the device's layout) of every label of `inst`, made by the oracle."""
    max_inst = int(inst.max())
    t, s = R.table(inst, max_inst), R.map_sums(inst, max_inst, image)
    rec = np.zeros(max_inst, post_proc._REC_DTYPE)
    rec["label"] = np.arange(1, max_inst + 1)
    for k in ("area", "rmin", "rmax", "cmin", "cmax", "sum_x", "sum_y"):
        rec[k] = t[k]
    feat = np.zeros(max_inst, F.FEAT_DTYPE)
    for k in R.INT_FIELDS:
        feat[k] = s[k]
    return rec, feat


def _blob(rng, size):
    """A random blob up to `size` px across: a thresholded smooth field plus salt noise (holes, ragged borders, several pieces)."""
    from scipy import ndimage

    field = ndimage.gaussian_filter(rng.normal(size=(size, size)), size / 8.0)
    mask = field > np.quantile(field, rng.uniform(0.3, 0.8))
    mask ^= rng.random((size, size)) < 0.02
    if not mask.any():
        mask[size // 2, size // 2] = True
    return mask


def test_oracle_convolution_classes_equal_the_pixel_loop():
    rng = np.random.default_rng(7)
    for k in range(200):
        mask = rng.random((12, 12)) < rng.uniform(0.1, 0.95)
        assert R.perimeter_classes(mask).tolist() == R.perimeter_classes_loop(mask).tolist(), k


@pytest.mark.parametrize("a,b", [(3, 7), (7, 3), (5, 5), (1, 9), (9, 1), (2, 2)])
def test_rectangle(a, b):
    """a rows x b columns."""
    inst = np.zeros((a + 4, b + 6), np.int32)
    inst[2:2 + a, 3:3 + b] = 1
    d = F.derive(*_rec_feat(inst))[0]
    assert d["vxx"] == pytest.approx((b * b - 1) / 12.0, rel=1e-15, abs=0)
    assert d["vyy"] == pytest.approx((a * a - 1) / 12.0, rel=1e-15, abs=0)
    assert d["vxy"] == 0.0 and d["area"] == a * b and d["extent"] == 1.0
    if b > a:
        assert d["orientation"] == 0.0
    elif a > b:
        assert d["orientation"] == pytest.approx(math.pi / 2, rel=1e-15)
    else:
        assert d["eccentricity"] == 0.0 and d["orientation"] == 0.0
    assert d["major_axis_length"] == pytest.approx(4 * math.sqrt((max(a, b) ** 2 - 1) / 12.0), rel=1e-14)
    assert d["minor_axis_length"] == pytest.approx(4 * math.sqrt((min(a, b) ** 2 - 1) / 12.0), rel=1e-14, abs=0)


def test_single_pixel_has_no_nan():
    inst = np.zeros((3, 3), np.int32)
    inst[1, 1] = 1
    img = np.full((3, 3, 3), 200, np.uint8)
    d = F.derive(*_rec_feat(inst, img), with_colour=True)[0]
    for k in d.dtype.names:
        assert np.all(np.isfinite(d[k])), k
    assert d["perimeter"] == 0 and d["circularity"] == 0 and d["major_axis_length"] == 0 and d["minor_axis_length"] == 0
    assert d["eccentricity"] == 0 and d["orientation"] == 0 and d["area"] == 1 and d["extent"] == 1
    assert d["mean_rgb"].tolist() == [200.0] * 3 and d["std_rgb"].tolist() == [0.0] * 3


def test_absent_slot_is_all_zero():
    inst = np.zeros((4, 4), np.int32)
    inst[1, 1:3] = 2                       # label 1 absent
    d = F.derive(*_rec_feat(inst))
    assert all(d[0][k] == 0 for k in d.dtype.names) and d[1]["area"] == 2


def test_big_integers_take_the_exact_path():
    """A numerator beyond int64 (S * sxx ~ 2^70) must not wrap: a 2^20-pixel-wide, 1-row label by its closed form."""
    n = 1 << 20
    rec = np.zeros(1, post_proc._REC_DTYPE)
    rec["label"], rec["area"], rec["rmin"], rec["rmax"], rec["cmin"], rec["cmax"] = 1, n, 0, 1, 0, n
    rec["sum_x"] = n * (n - 1) // 2
    feat = np.zeros(1, F.FEAT_DTYPE)
    feat["sxx"] = (n - 1) * n * (2 * n - 1) // 6
    feat["per"] = (n, 0, 0)
    d = F.derive(rec, feat)[0]
    assert d["vxx"] == pytest.approx((n * n - 1) / 12.0, rel=1e-15) and d["vyy"] == 0 and d["orientation"] == 0
    assert d["eccentricity"] == 1.0


@pytest.mark.parametrize("size", [9, 33, 128])
def test_derive_agrees_with_the_float_oracle(size):
    """rtol = atol = 1e-9: on blobs <= 128 px across the integer numerator is < 2^53 (exact in float64 too) and the oracle's centred
    sums carry a few float64 roundings; 1e-9 is that bound with room, not a measured figure.  The orientation is an AXIS: it is
    compared modulo pi (vxy = -1e-17 instead of 0 moves atan2 from +pi to -pi; the axis is the same)."""
    rng = np.random.default_rng(size)
    for k in range(12):
        mask = _blob(rng, size)
        inst = np.zeros((size + 3, size + 5), np.int32)
        inst[1:1 + size, 2:2 + size][mask] = 1
        img = rng.integers(0, 256, inst.shape + (3,), dtype=np.uint8)
        got = F.derive(*_rec_feat(inst, img), with_colour=True)[0]
        want = R.float_features(inst, 1, img)
        for name in got.dtype.names:
            if name == "orientation":
                if want["eccentricity"] < 1e-3:
                    continue                      # a (nearly) isotropic blob has no axis
                diff = (got[name] - want[name] + math.pi / 2) % math.pi - math.pi / 2
                assert abs(diff) <= 1e-9 + 1e-9 * abs(want[name]), (k, name, got[name], want[name])
            else:
                np.testing.assert_allclose(got[name], want[name], rtol=1e-9, atol=1e-9, err_msg="%d %s" % (k, name))


def test_to_dicts_round_trips_through_save_json(tmp_path):
    rng = np.random.default_rng(3)
    inst = np.zeros((40, 50), np.int32)
    inst[3:20, 4:21][_blob(rng, 17)] = 1
    inst[25:38, 10:45][rng.random((13, 35)) < 0.6] = 2
    img = rng.integers(0, 256, inst.shape + (3,), dtype=np.uint8)
    rec, feat = _rec_feat(inst, img)
    info = post_proc.records_to_dict(rec, None, feat_host=feat, with_colour=True)
    assert sorted(info) == [1, 2]
    dicts = F.to_dicts(F.derive(rec, feat, True))
    for lab in (1, 2):
        assert info[lab]["features"] == dicts[lab - 1]
        assert all(type(v) in (float, list) for v in dicts[lab - 1].values())
    path = tmp_path / "out.json"
    io_utils.save_json(str(path), info, mag=40)
    back = json.load(open(path))["nuc"]
    for lab in (1, 2):
        assert back[str(lab)]["features"] == info[lab]["features"]            # repr round trip of float64 is exact
        assert set(back[str(lab)]) == {"bbox", "centroid", "contour", "type_prob", "type", "features"}
    # without feat_host the entries are what they always were
    assert all("features" not in v for v in post_proc.records_to_dict(rec, None).values())


def test_feature_bytes_travel_with_the_item_arrays():
    """What a remote rank sends to rank 0: the item's four arrays plus the feature bytes, packed, unpacked and assembled there."""
    from hover_net_amd import infer_tile as T

    rng = np.random.default_rng(5)
    inst = np.zeros((40, 50), np.int32)
    inst[3:20, 4:21][_blob(rng, 17)] = 1
    inst[25:38, 10:45][rng.random((13, 35)) < 0.8] = 2
    rec, feat = _rec_feat(inst)
    arrs = T.result_to_arrays(inst, rec, None) + [feat.view(np.uint8).reshape(feat.shape[0], -1)]
    back = T.unpack_arrays(T.pack_arrays(arrs))
    assert len(back) == 5 and back[4].shape == (2, F.FEAT_DTYPE.itemsize)
    inst_b, info = T.arrays_to_result(back[:4], None, shift_xy=(100, 200), feat_b=back[4])
    plain = T.arrays_to_result(back[:4], None, shift_xy=(100, 200))[1]
    want = F.to_dicts(F.derive(rec, feat))
    assert np.array_equal(inst_b, inst) and sorted(info) == sorted(plain)
    for lab, e in info.items():
        assert e["features"] == want[lab - 1]                      # the tile origin does not touch them
        assert e["bbox"].tolist() == plain[lab]["bbox"].tolist() and "features" not in plain[lab]

"""Per-nucleus morphometric features from the integer sums of `hvn_instance_features` (include/hvn.h, csrc/hvn_features.hip).

Host side, numpy only, importable without a GPU.  The device pass delivers exact integers per record slot (second moments about
the bbox origin, border-pixel class counts, colour sums); `derive` turns them into the regionprops-style numbers users compute
from an instance map.  With S = area, Sx = sum_x, Sy = sum_y of the record (all about the bbox origin):

    vxx = (S sxx - Sx^2) / S^2, vyy, vxy likewise          (population (co)variances; the numerator in exact integers)
    l1, l2 = (vxx + vyy) / 2 +- sqrt(((vxx - vyy) / 2)^2 + vxy^2)
    major_axis_length = 4 sqrt(l1),  minor_axis_length = 4 sqrt(max(l2, 0))
    eccentricity = sqrt(1 - l2 / l1)                        (0 when l1 == 0)
    orientation = atan2(2 vxy, vxx - vyy) / 2               (the major axis from +x, y DOWN, in (-pi/2, pi/2]; 0 when both are 0)
    perimeter = per0 + per1 sqrt(2) + per2 (1 + sqrt(2)) / 2   (scikit-image's 4-neighbourhood estimator)
    equivalent_diameter = sqrt(4 S / pi),  extent = S / bbox area,  circularity = 4 pi S / perimeter^2  (0 when perimeter == 0)
    mean_rgb = csum / S,  std_rgb = sqrt((S csq - csum^2) / S^2) (population; only with an image)
"""
import numpy as np

from . import lib as L

FEAT_DTYPE = np.dtype(L.hvn_inst_feat)

SHAPE_FIELDS = ("area", "vxx", "vyy", "vxy", "major_axis_length", "minor_axis_length", "eccentricity", "orientation", "perimeter",
                "equivalent_diameter", "extent", "circularity")
_SQRT2 = float(np.sqrt(2.0))


def out_dtype(with_colour):
    fields = [(k, "<f8") for k in SHAPE_FIELDS]
    if with_colour:
        fields += [("mean_rgb", "<f8", (3,)), ("std_rgb", "<f8", (3,))]
    return np.dtype(fields)


def _central(s, a, b, c):
    """The integer s * a - b * c, element-wise and exact: int64 where every product provably fits, Python ints otherwise."""
    s, a, b, c = (np.asarray(v, np.int64) for v in (s, a, b, c))

    def top(v):
        return int(np.abs(v).max()) if v.size else 0

    if top(s) * top(a) < 2 ** 62 and top(b) * top(c) < 2 ** 62:
        return s * a - b * c
    return s.astype(object) * a.astype(object) - b.astype(object) * c.astype(object)


def _ratio(num, den):
    """num / den in float64 (Python's int / int is correctly rounded for the big-integer form)."""
    if num.dtype == object:
        return np.array([int(n) / int(d) for n, d in zip(num.reshape(-1), np.broadcast_to(den, num.shape).reshape(-1))],
                        np.float64).reshape(num.shape)
    return num.astype(np.float64) / den.astype(np.float64)


def derive(rec, feat, with_colour=False):
    """rec: structured array of `post_proc._REC_DTYPE` records, feat: the FEAT_DTYPE slots parallel to it -> float64 structured
    array (`out_dtype(with_colour)`), one row per slot.  A slot with area 0 is all zeros."""
    rec, feat = np.asarray(rec).reshape(-1), np.asarray(feat).reshape(-1)
    if rec.shape != feat.shape:
        raise ValueError("records %s and features %s are not parallel" % (rec.shape, feat.shape))
    out = np.zeros(rec.shape, out_dtype(with_colour))
    ok = rec["area"] > 0
    if not ok.any():
        return out
    r, f = rec[ok], feat[ok]
    s = r["area"].astype(np.int64)
    sx, sy = np.rint(r["sum_x"]).astype(np.int64), np.rint(r["sum_y"]).astype(np.int64)
    den = s * s                         # area is an int32: the square fits
    nxx, nyy, nxy = _central(s, f["sxx"], sx, sx), _central(s, f["syy"], sy, sy), _central(s, f["sxy"], sx, sy)
    vxx, vyy, vxy = (_ratio(n, den) for n in (nxx, nyy, nxy))
    half, root = (vxx + vyy) / 2, np.sqrt(((vxx - vyy) / 2) ** 2 + vxy ** 2)
    l1, l2 = half + root, half - root
    sf = s.astype(np.float64)
    o = np.zeros(r.shape, out.dtype)
    o["area"], o["vxx"], o["vyy"], o["vxy"] = sf, vxx, vyy, vxy
    o["major_axis_length"] = 4 * np.sqrt(np.maximum(l1, 0))
    o["minor_axis_length"] = 4 * np.sqrt(np.maximum(l2, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        o["eccentricity"] = np.where(l1 > 0, np.sqrt(np.maximum(1 - l2 / np.where(l1 > 0, l1, 1), 0)), 0.0)
    o["orientation"] = 0.5 * np.arctan2(2 * vxy, vxx - vyy)     # arctan2(0, 0) = 0
    per = f["per"].astype(np.float64)
    o["perimeter"] = per[:, 0] + per[:, 1] * _SQRT2 + per[:, 2] * ((1 + _SQRT2) / 2)
    o["equivalent_diameter"] = np.sqrt(4 * sf / np.pi)
    box = (r["rmax"].astype(np.int64) - r["rmin"]) * (r["cmax"].astype(np.int64) - r["cmin"])
    o["extent"] = sf / np.maximum(box, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        o["circularity"] = np.where(o["perimeter"] > 0, 4 * np.pi * sf / np.where(o["perimeter"] > 0, o["perimeter"], 1) ** 2, 0.0)
    if with_colour:
        o["mean_rgb"] = f["csum"] / sf[:, None]
        s3 = np.repeat(s[:, None], 3, 1)
        var_n = _central(s3, f["csq"], f["csum"], f["csum"])
        o["std_rgb"] = np.sqrt(np.maximum(_ratio(var_n, s3 * s3), 0))
    out[ok] = o
    return out


def to_dicts(derived):
    """`derive`'s rows -> one dict of plain Python floats (lists for the colour triples) per row: JSON-serialisable as it is."""
    names = derived.dtype.names
    cols = {k: derived[k].tolist() for k in names}
    return [{k: cols[k][i] for k in names} for i in range(derived.shape[0])]

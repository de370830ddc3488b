"""Oracle for the per-nucleus features (numpy / scipy only, independent of hover_net_amd/features.py and of the kernel).

Integer part: the sums of include/hvn.h's hvn_inst_feat per label, from `np.nonzero(mask)`; the border by binary erosion with the
cross element, the perimeter codes by scikit-image's `[[10,2,10],[2,1,2],[10,2,10]]` convolution of the border image.
Float part: the features from CENTRED float64 coordinates (not from the integer formula of features.py)."""
import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)
KERNEL = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
# code -> class (scikit-image's perimeter weights 1, sqrt(2), (1 + sqrt(2)) / 2)
CLASS_OF_CODE = {5: 0, 7: 0, 15: 0, 17: 0, 25: 0, 27: 0, 21: 1, 33: 1, 13: 2, 23: 2}

INT_FIELDS = ("sxx", "syy", "sxy", "seen", "per", "csum", "csq")


def perimeter_classes(mask):
    """mask: bool [h,w] (outside = background) -> int [3] class counts."""
    mask = np.asarray(mask, bool)
    border = mask & ~ndimage.binary_erosion(mask, CROSS, border_value=0)
    codes = ndimage.convolve(border.astype(np.int64), KERNEL, mode="constant", cval=0)
    per = np.zeros(3, np.int64)
    for code, cls in CLASS_OF_CODE.items():
        per[cls] += int(np.count_nonzero(border & (codes == code)))
    return per


def perimeter_classes_loop(mask):
    """The same classes by a plain per-pixel loop over (n4, nd): the issue's restatement of the estimator."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape

    def at(a, y, x):
        return bool(a[y, x]) if 0 <= y < h and 0 <= x < w else False

    border = np.zeros_like(mask)
    for y in range(h):
        for x in range(w):
            if mask[y, x]:
                border[y, x] = not (at(mask, y - 1, x) and at(mask, y + 1, x) and at(mask, y, x - 1) and at(mask, y, x + 1))
    cls0 = {(2, 0), (3, 0), (2, 1), (3, 1), (2, 2), (3, 2)}
    cls1 = {(0, 2), (1, 3)}
    cls2 = {(1, 1), (1, 2)}
    per = np.zeros(3, np.int64)
    for y in range(h):
        for x in range(w):
            if not border[y, x]:
                continue
            n4 = at(border, y - 1, x) + at(border, y + 1, x) + at(border, y, x - 1) + at(border, y, x + 1)
            nd = at(border, y - 1, x - 1) + at(border, y - 1, x + 1) + at(border, y + 1, x - 1) + at(border, y + 1, x + 1)
            for k, group in enumerate((cls0, cls1, cls2)):
                per[k] += (n4, nd) in group
    return per


def label_sums(inst, label, rmin, cmin, image=None):
    """The integer fields of one label of `inst` (int [h,w]) about the bbox origin (rmin, cmin) -> dict."""
    mask = np.asarray(inst) == label
    ys, xs = np.nonzero(mask)
    dy, dx = ys.astype(np.int64) - int(rmin), xs.astype(np.int64) - int(cmin)
    # the estimator on the label's own bounding box: outside it there is only background (border_value=0 / cval=0 say the same)
    crop = mask[ys.min():ys.max() + 1, xs.min():xs.max() + 1] if ys.size else mask
    out = {"sxx": int((dx * dx).sum()), "syy": int((dy * dy).sum()), "sxy": int((dx * dy).sum()), "seen": int(ys.size),
           "per": perimeter_classes(crop), "csum": np.zeros(3, np.int64), "csq": np.zeros(3, np.int64)}
    if image is not None:
        px = np.asarray(image)[ys, xs].astype(np.int64)
        out["csum"], out["csq"] = px.sum(0), (px * px).sum(0)
    return out


def table(inst, max_inst):
    """The fields of hvn_instance_table the features build on, for labels 1..max_inst of one map -> dict of arrays [max_inst]."""
    inst = np.asarray(inst)
    rec = {k: np.zeros(max_inst, np.int64) for k in ("area", "rmin", "rmax", "cmin", "cmax", "sum_x", "sum_y")}
    for lab in range(1, max_inst + 1):
        ys, xs = np.nonzero(inst == lab)
        if ys.size == 0:
            rec["rmin"][lab - 1], rec["cmin"][lab - 1] = 0x7FFFFFFF, 0x7FFFFFFF      # the device table's empty slot
            continue
        j = lab - 1
        rec["area"][j] = ys.size
        rec["rmin"][j], rec["rmax"][j], rec["cmin"][j], rec["cmax"][j] = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
        rec["sum_x"][j], rec["sum_y"][j] = (xs - xs.min()).sum(), (ys - ys.min()).sum()
    return rec


def map_sums(inst, max_inst, image=None):
    """-> dict of integer arrays, slot j = label j + 1 of `inst`; an absent label is all zeros."""
    inst = np.asarray(inst)
    out = {"sxx": np.zeros(max_inst, np.int64), "syy": np.zeros(max_inst, np.int64), "sxy": np.zeros(max_inst, np.int64),
           "seen": np.zeros(max_inst, np.int64), "per": np.zeros((max_inst, 3), np.int64), "csum": np.zeros((max_inst, 3), np.int64),
           "csq": np.zeros((max_inst, 3), np.int64)}
    for lab in np.unique(inst):
        if lab <= 0 or lab > max_inst:
            continue
        ys, xs = np.nonzero(inst == lab)
        one = label_sums(inst, lab, ys.min(), xs.min(), image)
        for k in out:
            out[k][lab - 1] = one[k]
    return out


def float_features(inst, label, image=None):
    """Float features of one label from centred float64 coordinates -> dict (orientation: major axis from +x, y down)."""
    mask = np.asarray(inst) == label
    ys, xs = np.nonzero(mask)
    s = float(ys.size)
    x, y = xs.astype(np.float64), ys.astype(np.float64)
    xc, yc = x - x.mean(), y - y.mean()
    vxx, vyy, vxy = float((xc * xc).mean()), float((yc * yc).mean()), float((xc * yc).mean())
    ev = np.linalg.eigvalsh(np.array([[vxx, vxy], [vxy, vyy]]))
    l1, l2 = float(ev[1]), float(ev[0])
    per = perimeter_classes(mask).astype(np.float64)
    perimeter = float(per[0] + per[1] * np.sqrt(2.0) + per[2] * (1 + np.sqrt(2.0)) / 2)
    box = float((ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1))
    out = {"area": s, "vxx": vxx, "vyy": vyy, "vxy": vxy,
           "major_axis_length": 4 * np.sqrt(max(l1, 0.0)), "minor_axis_length": 4 * np.sqrt(max(l2, 0.0)),
           "eccentricity": float(np.sqrt(max(1 - l2 / l1, 0.0))) if l1 > 0 else 0.0,
           "orientation": 0.5 * float(np.arctan2(2 * vxy, vxx - vyy)),
           "perimeter": perimeter, "equivalent_diameter": float(np.sqrt(4 * s / np.pi)), "extent": s / box,
           "circularity": 4 * np.pi * s / perimeter ** 2 if perimeter > 0 else 0.0}
    if image is not None:
        px = np.asarray(image)[ys, xs].astype(np.float64)
        out["mean_rgb"] = px.mean(0)
        out["std_rgb"] = px.std(0)
    return out

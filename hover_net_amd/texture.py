"""Per-nucleus chromatin texture: the grey-level co-occurrence counts of HVN_OP_INST_TEXTURE (include/hvn.h, csrc/hvn_texture.hip,
DESIGN.md 4.27) -- the definition of the integers, their host form, and the float features derived from them.  Opt-in everywhere.
Host side, numpy only, importable without a GPU.

Inputs per map: `inst` int32 [H, W], the record table (`post_proc._REC_DTYPE` slots, slot j describes label j + 1) and `image` uint8
[H, W, 3] RGB, which is required.  As in the feature pass (features.py) the mask of a label is inst == label INSIDE the record's bbox
clamped to the map; any label map is valid (several pieces, holes, other labels inside the bbox, stale tables).

    grey value   g = (77 R + 150 G + 29 B + 128) >> 8                      in 0..255
    level        q = ((g - lo) * 8) // span,  span = hi - lo + 1            in 0..7 (LEVELS = 8)
    scale        "range" (the default): lo, hi = the smallest and largest grey value of that nucleus's mask, which makes the texture
                 invariant to staining intensity (H&E nuclei occupy only three or four of the fixed levels);
                 "fixed": lo = 0, hi = 255, so q = g >> 5
    offsets      (dx, dy), distance 1, y down:  d = 0: (1, 0),  1: (1, 1),  2: (0, 1),  3: (-1, 1)
    glcm[d][a][b] = the number of mask pixels p of level a whose neighbour p + offset_d is also a mask pixel of the same label and
                 has level b.  The pairs are ORDERED and not symmetrised: every unordered pixel pair is counted exactly once, at its
                 upper or left pixel.

A slot is HVN_TEX_WORDS = 276 int32 words (1104 bytes), mirrored by TEX_DTYPE:

    words 0..7    gsum   int64 [4]: the sums of g, g^2, g^3, g^4 over the mask (255^4 * (2^31 - 1) < 2^63: they fit)
    word  8       seen   mask pixels found; differs from the record's area for a stale table, as in the feature pass
    words 9, 10   lo, hi the nucleus's OWN smallest and largest grey value, whatever the scale: `scale` decides only whether the level
                         formula uses them or 0 and 255 (both 0 when seen == 0)
    word  11      reserved, always 0
    words 12..19  hist   [8]: mask pixels per level
    words 20..275 glcm   [4][8][8]

A slot with area <= 0, an empty clamped bbox or no mask pixel inside it is 276 zero words.  `sums_host` implements this definition;
the device returns the same integers, and tests/texture_ref.py (per-pixel Python loops) is the independent oracle of both.

`derive` makes the float features.  Per direction d with n_d = sum(glcm[d]) > 0, S = C + C^T (C = glcm[d]), N = 2 n_d, m_a = sum_b
S[a][b], M = sum_a a m_a; every numerator that is an integer is formed as an exact integer and divided once:

    contrast      = sum (a - b)^2 S / N
    dissimilarity = sum |a - b| S / N
    homogeneity   = (sum over k = 0..7 ascending of T_k / (1 + k^2)) / N,  T_k = the sum of S over |a - b| = k
    asm           = sum S^2 / N^2,   energy = sqrt(asm)
    correlation   = (N sum a b S - M^2) / (N sum a^2 m_a - M^2), and 1.0 when the denominator is 0
    entropy       = -sum P log2 P over P = S / N > 0, in row-major order

Each reported value is the mean over the directions that have pairs, taken in the order d = 0..3, and 0.0 when no direction has
pairs (a single pixel).  First-order values, from gsum = (g1, g2, g3, g4) and S = seen with exact integer central numerators:

    grey_mean = g1 / S,  grey_std = sqrt(m2), m2 = (S g2 - g1^2) / S^2 (population)
    grey_skewness = m3 / m2^1.5, m3 = (S^2 g3 - 3 S g1 g2 + 2 g1^3) / S^3
    grey_kurtosis = m4 / m2^2,   m4 = (S^3 g4 - 4 S^2 g1 g3 + 6 S g1^2 g2 - 3 g1^4) / S^4   (not the excess; both 0 when m2 == 0)
    grey_min, grey_max = lo, hi of the slot;  grey_entropy = -sum p log2 p over p = hist / S > 0, levels ascending
"""
import math

import numpy as np

LEVELS = 8
WORDS = 12 + LEVELS + 4 * LEVELS * LEVELS          # HVN_TEX_WORDS of include/hvn.h
TEX_DTYPE = np.dtype([("gsum", "<i8", (4,)), ("seen", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("reserved", "<i4"),
                      ("hist", "<i4", (LEVELS,)), ("glcm", "<i4", (4, LEVELS, LEVELS))])
OFFSETS = ((1, 0), (1, 1), (0, 1), (-1, 1))        # (dx, dy) of d = 0..3, y down
SCALES = {"range": 0, "fixed": 1}                  # the op's scale mode

GLCM_FIELDS = ("contrast", "dissimilarity", "homogeneity", "asm", "energy", "correlation", "entropy")
GREY_FIELDS = ("grey_mean", "grey_std", "grey_skewness", "grey_kurtosis", "grey_min", "grey_max", "grey_entropy")
OUT_DTYPE = np.dtype([(k, "<f8") for k in GLCM_FIELDS + GREY_FIELDS])


def check_scale(scale):
    """The `scale` / `texture` argument of the public entry points -> "range" | "fixed" (True means "range"); ValueError otherwise."""
    if scale is True:
        return "range"
    if not isinstance(scale, str) or scale not in SCALES:
        raise ValueError('texture scale must be "range" or "fixed" (or True: "range"), got %r' % (scale,))
    return scale


def grey(image):
    """uint8 [..., 3] RGB -> int32 [...]: (77 R + 150 G + 29 B + 128) >> 8."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim < 1 or image.shape[-1] != 3:
        raise ValueError("image must be uint8 [..., 3], got %s %s" % (image.dtype, image.shape))
    i = image.astype(np.int32)
    return (77 * i[..., 0] + 150 * i[..., 1] + 29 * i[..., 2] + 128) >> 8


def _map_sums(inst, rec, g, fixed, out):
    h, w = inst.shape
    for j in range(rec.shape[0]):
        r0, r1 = max(int(rec["rmin"][j]), 0), min(int(rec["rmax"][j]), h)
        c0, c1 = max(int(rec["cmin"][j]), 0), min(int(rec["cmax"][j]), w)
        if rec["area"][j] <= 0 or r0 >= r1 or c0 >= c1:
            continue
        mask = inst[r0:r1, c0:c1] == j + 1
        seen = int(mask.sum())
        if seen == 0:
            continue
        gc = g[r0:r1, c0:c1].astype(np.int64)
        gm = gc[mask]
        o = out[j]
        o["gsum"] = [int(gm.sum()), int((gm ** 2).sum()), int((gm ** 3).sum()), int((gm ** 4).sum())]
        o["seen"], o["lo"], o["hi"] = seen, int(gm.min()), int(gm.max())
        lo, hi = (0, 255) if fixed else (int(o["lo"]), int(o["hi"]))
        q = ((gc - lo) * LEVELS) // (hi - lo + 1)
        o["hist"] = np.bincount(q[mask], minlength=LEVELS)
        hh, ww = mask.shape
        for d, (dx, dy) in enumerate(OFFSETS):
            ys, yd = slice(0, hh - dy), slice(dy, hh)
            xs, xd = (slice(0, ww - 1), slice(1, ww)) if dx == 1 else (slice(0, ww), slice(0, ww)) if dx == 0 else (slice(1, ww), slice(0, ww - 1))
            both = mask[ys, xs] & mask[yd, xd]
            o["glcm"][d] = np.bincount(q[ys, xs][both] * LEVELS + q[yd, xd][both], minlength=LEVELS * LEVELS).reshape(LEVELS, LEVELS)


def sums_host(inst, rec, image, scale="range"):
    """The definition above on the host.  inst: int32 [H, W] or [N, H, W]; rec: `post_proc._REC_DTYPE` records [max_inst] or
    [N, max_inst]; image: uint8 [H, W, 3] or [N, H, W, 3] -> TEX_DTYPE array of rec's shape."""
    fixed = SCALES[check_scale(scale)] == 1
    inst, rec = np.asarray(inst), np.asarray(rec)
    if image is None:
        raise ValueError("texture needs the image")
    g = grey(image)
    if inst.ndim not in (2, 3) or g.shape != inst.shape or rec.ndim != inst.ndim - 1 or (inst.ndim == 3 and rec.shape[0] != inst.shape[0]):
        raise ValueError("inst %s, records %s and image %s do not belong together" % (inst.shape, rec.shape, np.shape(image)))
    out = np.zeros(rec.shape, TEX_DTYPE)
    if inst.ndim == 2:
        _map_sums(inst, rec, g, fixed, out)
    else:
        for i in range(inst.shape[0]):
            _map_sums(inst[i], rec[i], g[i], fixed, out[i])
    return out


def _ints(a, bound):
    """`a` as int64 where `bound` (on the magnitude of everything formed from it below) fits, as Python ints otherwise."""
    return a.astype(np.int64) if bound < 2 ** 62 else a.astype(object)


def _div(num, den):
    """num / den in float64, element-wise; Python's int / int is correctly rounded for the big-integer form."""
    if num.dtype == object or den.dtype == object:
        return np.array([int(n) / int(d) for n, d in zip(num.reshape(-1), np.broadcast_to(den, num.shape).reshape(-1))],
                        np.float64).reshape(num.shape)
    return num.astype(np.float64) / den.astype(np.float64)


def _glcm_features(glcm):
    """glcm: int [K, 4, 8, 8] with K > 0 -> {field: float64 [K]}, the mean over the directions that have pairs."""
    k = glcm.shape[0]
    c = glcm.astype(np.int64)
    n_big = int(c.sum(axis=(2, 3)).max()) * 2
    s = _ints(c + c.transpose(0, 1, 3, 2), 49 * n_big * n_big)         # the largest product below: N * sum a b S <= 49 N^2
    n = s.sum(axis=(2, 3))                                              # [K, 4] = 2 n_d
    has = n > 0
    safe_n = np.where(has, n, 1)
    a = np.arange(LEVELS, dtype=np.int64)
    diff = np.abs(a[:, None] - a[None, :])
    vals = {}
    vals["contrast"] = _div((s * (diff * diff)).sum(axis=(2, 3)), safe_n)
    vals["dissimilarity"] = _div((s * diff).sum(axis=(2, 3)), safe_n)
    hom = np.zeros((k, 4))
    for kk in range(LEVELS):                                            # k ascending
        hom = hom + _div((s * (diff == kk)).sum(axis=(2, 3)), np.full((k, 4), 1 + kk * kk, np.int64))
    vals["homogeneity"] = hom / safe_n.astype(np.float64)
    vals["asm"] = _div((s * s).sum(axis=(2, 3)), safe_n * safe_n)
    vals["energy"] = np.sqrt(vals["asm"])
    m = s.sum(axis=3)                                                   # [K, 4, 8] = m_a
    big_m = (m * a).sum(axis=2)
    num = safe_n * (s * (a[:, None] * a[None, :])).sum(axis=(2, 3)) - big_m * big_m
    den = safe_n * (m * (a * a)).sum(axis=2) - big_m * big_m
    zero = den == 0
    vals["correlation"] = np.where(zero, 1.0, _div(num, np.where(zero, 1, den)))
    p = _div(s, np.broadcast_to(safe_n[:, :, None, None], s.shape))
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0)
    ent = np.zeros((k, 4))
    for i in range(LEVELS):                                             # row-major order
        for j in range(LEVELS):
            ent = ent + term[:, :, i, j]
    vals["entropy"] = -ent + 0.0
    count = has.sum(axis=1)
    out = {}
    for name, v in vals.items():
        tot = np.zeros(k)
        for d in range(4):                                              # d = 0..3
            tot = tot + np.where(has[:, d], v[:, d], 0.0)
        out[name] = np.where(count > 0, tot / np.maximum(count, 1), 0.0)
    return out


def derive(tex):
    """TEX_DTYPE slots (any shape; or their bytes, uint8 [..., 1104]) -> float64 structured array (OUT_DTYPE) of the same shape.  A slot
    without a mask pixel is all zeros."""
    tex = np.asarray(tex)
    if tex.dtype != TEX_DTYPE:
        tex = np.ascontiguousarray(tex).view(TEX_DTYPE).reshape(tex.shape[:-1])
    shape = tex.shape
    tex = tex.reshape(-1)
    out = np.zeros(tex.shape, OUT_DTYPE)
    ok = tex["seen"] > 0
    if not ok.any():
        return out.reshape(shape)
    t = tex[ok]
    o = np.zeros(t.shape, OUT_DTYPE)
    for name, v in _glcm_features(t["glcm"]).items():
        o[name] = v
    for i in range(t.shape[0]):                                         # the central numerators pass 2^63 for ordinary nuclei: Python ints
        s = int(t["seen"][i])
        g1, g2, g3, g4 = (int(v) for v in t["gsum"][i])
        n2 = s * g2 - g1 * g1
        o["grey_mean"][i] = g1 / s
        m2 = n2 / (s * s)
        o["grey_std"][i] = math.sqrt(m2) if n2 > 0 else 0.0
        if n2 > 0:
            m3 = (s * s * g3 - 3 * s * g1 * g2 + 2 * g1 ** 3) / s ** 3
            m4 = (s ** 3 * g4 - 4 * s * s * g1 * g3 + 6 * s * g1 * g1 * g2 - 3 * g1 ** 4) / s ** 4
            o["grey_skewness"][i] = m3 / m2 ** 1.5
            o["grey_kurtosis"][i] = m4 / (m2 * m2)
        ent = 0.0
        for c in t["hist"][i].tolist():                                 # levels ascending
            if c > 0:
                ent += (c / s) * math.log2(c / s)
        o["grey_entropy"][i] = -ent + 0.0
    o["grey_min"], o["grey_max"] = t["lo"], t["hi"]
    out[ok] = o
    return out.reshape(shape)


def to_dicts(derived):
    """`derive`'s rows (one dimension) -> one dict of plain Python floats per row: JSON-serialisable as it is."""
    names = derived.dtype.names
    cols = {k: derived[k].tolist() for k in names}
    return [{k: cols[k][i] for k in names} for i in range(derived.shape[0])]

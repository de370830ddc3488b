"""Macenko stain normalisation (Macenko et al. 2009, with the constants of the common implementations): the definition of the
result, on the host, and the device form that gives the same bytes (csrc/hvn_stain.hip).  Opt-in everywhere.

Constants: Io = 240, beta = 0.15, alpha = 1, HE_REF / MAXC_REF below.  The optical density of a byte is od[v] = -ln((v + 1) / Io):
256 values per channel (`od_table`).

The fit is a function of the colour histogram.  Every statistic of the fit is a function of the multiset of RGB triples, i.e. of
the list (key = r << 16 | g << 8 | b, count) in ascending key order -- `np.unique(keys, return_counts=True)`.  That list comes
from the host (`colour_counts_host`) or, in exact integers, from the device (`colour_counts_device`: HVN_OP_STAIN_HIST adds the
pixels to 2^24 uint32 bins with integer atomics, HVN_OP_STAIN_COMPACT writes the non-empty bins in key order); everything after
it is `fit_from_counts`, float64 numpy on at most a few 10^5 rows, the same code for both: the device fit equals the host fit bit
for bit by construction.  `fit_from_counts(keys, counts)`:

 1. keep the rows whose three od are all >= beta;
 2. the count-weighted mean and covariance of the kept rows (divided by n - 1);
 3. `np.linalg.eigh`, the two leading eigenvectors, each negated if its component sum is negative (LAPACK's sign must not decide
    on which side of the +-pi wrap the angles fall);
 4. phi = arctan2 of the projections; minPhi / maxPhi = the alpha / 100 - alpha percentiles, weighted by count;
 5. the two stain vectors from minPhi and maxPhi; the one with the larger first component goes first (haematoxylin);
 6. the concentrations of ALL rows (not only the kept) through pinv(HE);
 7. max_c = the count-weighted 99th percentile of each concentration.

"Percentile" is `np.percentile`'s linear rule on the expanded multiset, from cumulative counts (`weighted_percentile`): with n
values sorted ascending, pos = (n - 1) * (q / 100), lo = floor(pos), hi = min(lo + 1, n - 1), t = pos - lo, the result is
v_lo + (v_hi - v_lo) t, and v_hi - (v_hi - v_lo)(1 - t) where t >= 0.5 (numpy's two-sided interpolation); v_j is the value of the
first sorted row whose cumulative count exceeds j.  The fit raises `StainFitError` (a ValueError) with fewer than 64 kept pixels,
fewer than 3 distinct kept colours, a non-finite HE, max_c or M, or max_c <= 0.

The apply needs no transcendental per pixel.  With M = HE_target . diag(MAXC_target / max_c) . pinv(HE) (3 x 3, `matrix`), the
normalised channel c is Io exp(-sum_k M[c,k] od[I_k]) = Io prod_k T[c][k][I_k], T[c][k][v] = exp(-M[c][k] od[v]): nine 256-entry
float64 tables made here (`tables`).  The result is DEFINED as

    x = ((Io * T[c][0][r]) * T[c][1][g]) * T[c][2][b]      in float64, multiplied in that order,
    out = (uint8) (x < 255 ? x : 255)                       truncating; NaN and +inf give 255,

which `apply_host` computes in numpy and HVN_OP_STAIN_APPLY on the device (tables in LDS): only IEEE multiplications, so the two
agree bit for bit.  Against the textbook min(255, Io exp(-M od)) the table form differs by at most one level, rarely.
"""
import collections
import ctypes

import numpy as np

IO, BETA, ALPHA = 240.0, 0.15, 1.0
HE_REF = np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]], np.float64)
MAXC_REF = np.array([1.9705, 1.0308], np.float64)
MIN_KEPT, MIN_COLOURS = 64, 3

StainFit = collections.namedtuple("StainFit", "he max_c kept pixels")      # he float64 [3,2], max_c float64 [2], pixel counts
REFERENCE = StainFit(HE_REF, MAXC_REF, 0, 0)


class StainFitError(ValueError):
    pass


def od_table():
    """od[v] = -ln((v + 1) / Io) for the 256 byte values, float64."""
    return -np.log((np.arange(256, dtype=np.float64) + 1.0) / IO)


def resolve(spec):
    """The target a `stain_norm` argument names: None -> None (off), "macenko" -> the reference constants, a `StainFit` (of a
    target image) -> itself.  ValueError otherwise."""
    if spec is None:
        return None
    if isinstance(spec, StainFit):
        return spec
    if isinstance(spec, str) and spec == "macenko":
        return REFERENCE
    raise ValueError('stain_norm=%r: None, "macenko" or a StainFit (the fit of a target image)' % (spec,))


# ---- the colour list ---------------------------------------------------------------------------
def _mask_of(mask, shape):
    if mask is None:
        return None
    if tuple(mask.shape) != tuple(shape):
        raise ValueError("mask %s does not match the image's pixels %s" % (tuple(mask.shape), tuple(shape)))
    return mask


def colour_counts_host(img, mask=None):
    """uint8 [..., 3] -> (keys uint32 ascending, counts int64) of the pixels (where `mask`, same leading shape, is non-zero)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim < 2 or img.shape[-1] != 3:
        raise ValueError("expected a uint8 array [..., 3], got %s %s" % (img.dtype, img.shape))
    key = (img[..., 0].astype(np.uint32) << 16) | (img[..., 1].astype(np.uint32) << 8) | img[..., 2]
    mask = _mask_of(mask, key.shape)
    key = key.reshape(-1) if mask is None else key[np.asarray(mask) != 0]
    keys, counts = np.unique(key, return_counts=True)
    return keys.astype(np.uint32), counts.astype(np.int64)


_STATE = {}      # per device: the 2^24 bins (clear between calls), COMPACT's workspace and status, the list (grown on demand)
_WS_BYTES = 65536


def _image_view(op_view, t):
    """hvn_view of a uint8 device tensor [n, h, w, 3] whose pixels are three contiguous bytes; returns n."""
    n, h, w, c = t.shape
    sn, sy, sx, sc = t.stride()
    if c != 3 or sc != 1 or sx != 3 or h * w > 1 << 30:
        raise ValueError("expected uint8 [.., h, w, 3] with contiguous pixels and h * w <= 2^30, got %s strides %s" % (tuple(t.shape), t.stride()))
    op_view.base, op_view.h, op_view.w, op_view.c = t.data_ptr(), h, w, 3
    op_view.sy, op_view.sn = (sy if h > 1 else 0), (sn if n > 1 else 0)
    return n


def _as_batch(t, what):
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() in (3, 4)):
        raise ValueError("%s: expected a uint8 device tensor [h, w, 3] or [n, h, w, 3]" % what)
    return t if t.dim() == 4 else t.unsqueeze(0)


def colour_counts_device(t, mask=None):
    """`colour_counts_host` of a uint8 device tensor [h, w, 3] or [n, h, w, 3] (rows and samples may be strided), `mask` a uint8
    device tensor of the leading shape.  One bins tensor is kept per device and left clear by every call; the one synchronisation
    is the readback of the status and then of the list."""
    import torch

    from . import lib as L
    from . import plan as PL

    x = _as_batch(t, "colour_counts_device")
    dev = x.device
    pixels = x.shape[0] * x.shape[1] * x.shape[2]
    if pixels >= 1 << 32:
        raise ValueError("colour_counts_device: %d pixels do not fit the uint32 bins" % pixels)
    if x.shape[0] > 65535:
        raise ValueError("colour_counts_device: batch %d above 65535" % x.shape[0])
    with torch.cuda.device(dev):
        st = _STATE.get(dev)
        if st is None:
            st = _STATE[dev] = {"bins": torch.zeros(1 << 24, dtype=torch.int32, device=dev), "ws": torch.empty(_WS_BYTES, dtype=torch.uint8, device=dev),
                                "status": torch.empty(2, dtype=torch.int64, device=dev), "list": None}
        cap = max(1, min(pixels, 1 << 24))
        if st["list"] is None or st["list"].shape[0] < cap:
            st["list"] = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        hist = L.hvn_op()
        hist.kind = PL.OP_STAIN_HIST
        n = _image_view(hist.x, x)
        if mask is not None:
            if not (mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(t.shape[:-1])):
                raise ValueError("colour_counts_device: mask must be a uint8 device tensor of shape %s" % (tuple(t.shape[:-1]),))
            mask = mask.contiguous()
            hist.res.base = mask.data_ptr()
        hist.y.base = st["bins"].data_ptr()
        comp = L.hvn_op()
        comp.kind, comp._rsv = PL.OP_STAIN_COMPACT, 1
        comp.x.base, comp.y.base, comp.y.h = st["bins"].data_ptr(), st["list"].data_ptr(), cap
        comp.y2.base, comp.x2.base = st["status"].data_ptr(), st["ws"].data_ptr()
        sp = L.stream_ptr(dev)
        try:
            L.call("hvn_run_op", ctypes.addressof(hist), n, sp)
            L.call("hvn_run_op", ctypes.addressof(comp), 1, sp)
            n_keys, n_pix = (int(v) for v in st["status"].cpu().numpy())
            pairs = st["list"][:n_keys].cpu().numpy().view(np.uint32)
        except Exception:
            _STATE.pop(dev, None)        # the bins may hold a half-finished image: start from a fresh table
            raise
    assert n_keys <= cap and n_pix <= pixels, (n_keys, cap, n_pix, pixels)
    return np.ascontiguousarray(pairs[:, 0]), pairs[:, 1].astype(np.int64)


# ---- the fit -------------------------------------------------------------------------------------
def weighted_percentile(values, counts, q):
    """`np.percentile(np.repeat(values, counts), q)` (method "linear") from cumulative counts, bit for bit."""
    values, counts = np.asarray(values, np.float64), np.asarray(counts, np.int64)
    order = np.argsort(values, kind="stable")
    v, cum = values[order], np.cumsum(counts[order])
    n = int(cum[-1])
    pos = (n - 1) * (q / 100.0)
    lo = int(np.floor(pos))
    if lo >= n - 1:
        lo = hi = n - 1
    else:
        hi = lo + 1
    t = pos - np.floor(pos)
    a, b = v[np.searchsorted(cum, lo, side="right")], v[np.searchsorted(cum, hi, side="right")]
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def fit_from_counts(keys, counts):
    """The Macenko fit of a colour list (module docstring) -> StainFit."""
    keys, counts = np.asarray(keys).astype(np.int64), np.asarray(counts).astype(np.int64)
    rgb = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1)
    od = od_table()[rgb]
    keep = (od >= BETA).all(1)
    od_k, w_k = od[keep], counts[keep]
    pixels, n = int(counts.sum()), int(w_k.sum())
    if n < MIN_KEPT:
        raise StainFitError("stain fit: %d pixels of optical density >= %g, fewer than %d" % (n, BETA, MIN_KEPT))
    if od_k.shape[0] < MIN_COLOURS:
        raise StainFitError("stain fit: %d distinct stained colours, fewer than %d" % (od_k.shape[0], MIN_COLOURS))
    mu = (od_k * w_k[:, None]).sum(0) / n
    d = od_k - mu
    cov = (d * w_k[:, None]).T @ d / (n - 1)
    with np.errstate(all="ignore"):
        _, evec = np.linalg.eigh(cov)
        e = evec[:, 1:3].copy()
        for j in range(2):
            if e[:, j].sum() < 0:
                e[:, j] = -e[:, j]
        proj = od_k @ e
        phi = np.arctan2(proj[:, 1], proj[:, 0])
        mn, mx = weighted_percentile(phi, w_k, ALPHA), weighted_percentile(phi, w_k, 100.0 - ALPHA)
        v_min = e @ np.array([np.cos(mn), np.sin(mn)])
        v_max = e @ np.array([np.cos(mx), np.sin(mx)])
        he = np.array([v_min, v_max]).T if v_min[0] > v_max[0] else np.array([v_max, v_min]).T
        if not np.isfinite(he).all():
            raise StainFitError("stain fit: the stain vectors are not finite")
        try:
            conc = np.linalg.pinv(he) @ od.T
        except np.linalg.LinAlgError as err:
            raise StainFitError("stain fit: %s" % err) from None
        max_c = np.array([weighted_percentile(conc[0], counts, 99.0), weighted_percentile(conc[1], counts, 99.0)])
    if not np.isfinite(max_c).all() or (max_c <= 0).any():
        raise StainFitError("stain fit: the 99th percentile concentrations %s are not positive and finite" % (max_c,))
    out = StainFit(he, max_c, n, pixels)
    if not np.isfinite(matrix(out)).all():
        raise StainFitError("stain fit: the normalisation matrix is not finite")
    return out


def fit(image, mask=None):
    """StainFit of a uint8 numpy array [..., 3] (host list) or a uint8 device tensor [h, w, 3] / [n, h, w, 3] (device list): the
    same fit bit for bit."""
    if isinstance(image, np.ndarray):
        return fit_from_counts(*colour_counts_host(image, mask))
    return fit_from_counts(*colour_counts_device(image, mask))


def matrix(fit, target=None):
    """M = HE_target . diag(MAXC_target / max_c) . pinv(HE), float64 [3, 3]; `target`: a StainFit, None = the reference constants."""
    target = REFERENCE if target is None else target
    with np.errstate(all="ignore"):
        return np.asarray(target.he, np.float64) @ np.diag(np.asarray(target.max_c, np.float64) / fit.max_c) @ np.linalg.pinv(fit.he)


def tables(fit, target=None):
    """T[c][k][v] = exp(-M[c][k] od[v]), float64 [3, 3, 256]."""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.exp(-matrix(fit, target)[:, :, None] * od_table()[None, None, :]))


# ---- the apply -----------------------------------------------------------------------------------
def _tables_ok(tab):
    tab = np.ascontiguousarray(tab, np.float64)
    if tab.shape != (3, 3, 256):
        raise ValueError("tables must be float64 [3, 3, 256], got %s" % (tab.shape,))
    return tab


def apply_host(img, tab):
    """The definition of the normalised image: uint8 [..., 3] -> uint8 [..., 3]."""
    img, tab = np.asarray(img), _tables_ok(tab)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    out = np.empty(img.shape, np.uint8)
    with np.errstate(all="ignore"):
        for c in range(3):
            x = ((IO * tab[c, 0][r]) * tab[c, 1][g]) * tab[c, 2][b]
            out[..., c] = np.where(x < 255, x, 255.0).astype(np.uint8)
    return out


def tables_device(tab, device):
    import torch

    return torch.from_numpy(_tables_ok(tab)).to(device)


def apply_device(t, tab, out=None):
    """`apply_host` of a uint8 device tensor [h, w, 3] or [n, h, w, 3] (rows and samples may be strided) on the current stream, no
    synchronisation.  `tab`: numpy tables or `tables_device`'s tensor.  out: None = a new contiguous tensor, `t` itself = in
    place, or another tensor of the same shape that does not overlap `t`."""
    import torch

    from . import lib as L
    from . import plan as PL

    x = _as_batch(t, "apply_device")
    if out is None:
        out = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    if tuple(out.shape) != tuple(t.shape) or out.device != t.device:
        raise ValueError("apply_device: out %s on %s does not match the image %s on %s" % (tuple(out.shape), out.device, tuple(t.shape), t.device))
    y = _as_batch(out, "apply_device (out)")
    if x.shape[0] > 65535:
        raise ValueError("apply_device: batch %d above 65535" % x.shape[0])
    with torch.cuda.device(t.device):
        tab_dev = tab if isinstance(tab, torch.Tensor) else tables_device(tab, t.device)
        if not (tab_dev.dtype == torch.float64 and tuple(tab_dev.shape) == (3, 3, 256) and tab_dev.is_contiguous() and tab_dev.device == t.device):
            raise ValueError("apply_device: tables must be a contiguous float64 [3, 3, 256] tensor on %s" % t.device)
        op = L.hvn_op()
        op.kind = PL.OP_STAIN_APPLY
        n = _image_view(op.x, x)
        _image_view(op.y, y)
        op.w = tab_dev.data_ptr()
        L.call("hvn_run_op", ctypes.addressof(op), n, L.stream_ptr(t.device))
    return out


# ---- whole images --------------------------------------------------------------------------------
def tables_or_none(image, target, mask=None):
    """`tables(fit(image, mask), target)`; a degenerate image (StainFitError) gives None with one warning: the caller passes it
    through unnormalised."""
    import warnings

    try:
        return tables(fit(image, mask), target)
    except StainFitError as err:
        warnings.warn("stain normalisation skipped, the image passes through as it is: %s" % err, stacklevel=2)
        return None


def thumbnail_mask(thumb_shape, mask):
    """Which pixels of a [th, tw] thumbnail count under a tissue mask of any scale: pixel (y, x) reads the mask cell
    (floor(y * mask_h / th), floor(x * mask_w / tw)); uint8 [th, tw] of {0, 1}."""
    th, tw = int(thumb_shape[0]), int(thumb_shape[1])
    mask = np.asarray(mask)
    ys = (np.arange(th, dtype=np.int64) * mask.shape[0]) // th
    xs = (np.arange(tw, dtype=np.int64) * mask.shape[1]) // tw
    return (mask[ys][:, xs] != 0).astype(np.uint8)

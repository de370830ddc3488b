"""Tissue mask at 1.25x for whole-slide inference -- the preprocessing of `infer/wsi.py:486-500` (`simple_get_mask`): grey
conversion, Otsu threshold, tissue = dark side, drop objects < 16x16 px (8-connected), fill holes < 128x128 px, dilate with a
radius-16 disk.

The host functions of this module are the default and the definition of the result.  Opt-in, the same bytes come from the GPU
(`simple_get_mask(thumb, device=...)`, `simple_get_mask_device`; csrc/hvn_tissue.hip): grey and its histogram, the threshold
test, both connected-component size filters and the dilation run there, integer only; the Otsu threshold alone stays here, as
float64 arithmetic on the 256 counters the device sends back (`otsu_from_hist`) -- the one synchronisation of the device form.

The two OpenCV calls are restated (OpenCV is not on the box, so they are unpinned against it): `cvtColor(RGB2GRAY)` is the
8-bit fixed-point form (R*4899 + G*9617 + B*1868 + 8192) >> 14, `threshold(THRESH_OTSU)` maximises the between-class
variance over the 256-bin histogram (first maximum wins) and marks pixels > t.  The three skimage.morphology calls are
restated with scipy.ndimage and pinned against skimage 0.18.3 (tests/golden/tissue_mask.npz, oracle/make_golden_tissue.py).
"""
import numpy as np
from scipy import ndimage


def rgb_to_gray(rgb):
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def otsu_from_hist(hist):
    """The Otsu threshold from the 256 counters of a grey plane (any integer or float dtype)."""
    hist = np.asarray(hist).astype(np.float64)
    n = hist.sum()
    p = hist / n
    omega = np.cumsum(p)                       # class-0 probability for threshold t (values <= t)
    mu = np.cumsum(p * np.arange(256))
    mu_t = mu[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma = (mu_t * omega - mu) ** 2 / (omega * (1.0 - omega))
    sigma[~np.isfinite(sigma)] = 0.0
    return int(np.argmax(sigma))


def otsu_threshold(gray):
    return otsu_from_hist(np.bincount(gray.reshape(-1), minlength=256))


def remove_small_objects(mask, min_size, connectivity):
    """skimage.morphology.remove_small_objects on a boolean image (connectivity 1 = 4-, 2 = 8-neighbourhood)."""
    lab, _ = ndimage.label(mask, ndimage.generate_binary_structure(2, connectivity))
    sizes = np.bincount(lab.reshape(-1))
    too_small = sizes < min_size
    too_small[0] = False
    out = mask.copy()
    out[too_small[lab]] = False
    return out


def remove_small_holes(mask, area_threshold):
    """skimage.morphology.remove_small_holes (default connectivity 1): small objects of the complement are filled."""
    return ~remove_small_objects(~mask, area_threshold, 1)


def disk(radius):
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return (xx * xx + yy * yy) <= radius * radius


def simple_get_mask(thumb_rgb, device=None):
    """thumb_rgb: uint8 [h,w,3] thumbnail at 1.25x -> uint8 {0,1} tissue mask (wsi.py:489-500).  `device`: None = the host
    code below; a device = upload, `simple_get_mask_device`, download: the same array."""
    if device is not None:
        import torch

        thumb = torch.from_numpy(np.ascontiguousarray(thumb_rgb[..., :3], dtype=np.uint8)).to(device)
        return simple_get_mask_device(thumb).cpu().numpy()
    gray = rgb_to_gray(thumb_rgb)
    t = otsu_threshold(gray)
    mask = ~(gray > t)                                               # cv2.threshold -> 255 where > t; tissue = (mask == 0)
    mask = remove_small_objects(mask, 16 * 16, 2)
    mask = remove_small_holes(mask, 128 * 128)
    mask = ndimage.binary_dilation(mask, structure=disk(16))
    return mask.astype(np.uint8)


# ----------------------------------------------------------------------------------------------
# the device form (csrc/hvn_tissue.hip): everything on the current stream of the tensor's device
def _plane(t, channels):
    import torch

    shape = tuple(t.shape)
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and len(shape) == 2 + bool(channels) and (not channels or shape[2] == 3)):
        raise ValueError("expected a contiguous uint8 device tensor [h, w%s], got %s %s on %s" % (", 3" if channels else "", t.dtype, shape, t.device))
    return int(shape[0]), int(shape[1])


def gray_hist_device(thumb_dev):
    """uint8 device [h,w,3] -> (grey uint8 device [h,w], its 256 counters int32 device), `rgb_to_gray` and `np.bincount`."""
    import torch

    from . import lib as L

    h, w = _plane(thumb_dev, True)
    with torch.cuda.device(thumb_dev.device):
        gray = torch.empty((h, w), dtype=torch.uint8, device=thumb_dev.device)
        hist = torch.empty(256, dtype=torch.int32, device=thumb_dev.device)        # uint32 counters: a plane has at most 2^30 pixels
        L.call("hvn_tissue_gray_hist", thumb_dev.data_ptr(), h, w, gray.data_ptr(), hist.data_ptr(), L.stream_ptr(thumb_dev.device))
    return gray, hist


def mask_from_gray_device(gray_dev, t, min_obj=16 * 16, max_hole=128 * 128, radius=16, taps=False):
    """The chain after the threshold is known, on a grey plane in HBM: uint8 device [h,w] of {0,1}; with `taps` also the planes
    after the object filter and after the hole filter, `(mask, a, b)`.  No synchronisation."""
    import torch

    from . import lib as L

    h, w = _plane(gray_dev, False)
    dev = gray_dev.device
    with torch.cuda.device(dev):
        need = int(L.lib().hvn_tissue_mask_workspace_bytes(h, w))
        ws = L.grown(None, max(need, 1), dev)
        out = [torch.empty((h, w), dtype=torch.uint8, device=dev) for _ in range(3 if taps else 1)]
        L.call("hvn_tissue_mask", gray_dev.data_ptr(), h, w, int(t), int(min_obj), int(max_hole), int(radius), out[0].data_ptr(),
               out[1].data_ptr() if taps else None, out[2].data_ptr() if taps else None, ws.data_ptr(), need, L.stream_ptr(dev))
    return tuple(out) if taps else out[0]


def simple_get_mask_device(thumb_dev, taps=False):
    """`simple_get_mask` of a uint8 device tensor [h,w,3]: uint8 device [h,w] of {0,1} (with `taps`: `(mask, a, b)`), enqueued on
    the current stream.  Its one synchronisation is the readback of the 256 histogram counters for the Otsu threshold."""
    gray, hist = gray_hist_device(thumb_dev)
    t = otsu_from_hist(hist.cpu().numpy())
    return mask_from_gray_device(gray, t, taps=taps)

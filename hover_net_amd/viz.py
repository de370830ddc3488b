"""Overlay writer of the tile manager (`misc/viz_utils.py:94-125` `visualize_instances_dict`): contours of every instance in
its type colour (or a random colour without a type table) and an optional centroid dot, drawn into a copy of the image.
Host glue behind the hot path; numpy only (cv2 is absent from this image), so the line rasterisation follows
`cv2.drawContours(thickness=2)` in intent -- closed polygon through the contour vertices, 2 px wide -- not bit for bit.

The host functions below are the default and the DEFINITION of the result.  Opt-in, the same pixels are drawn on the GPU
(csrc/hvn_overlay.hip, `hvn_draw_overlay`): `draw_overlay_device` on flat device arrays, `overlay_from_records` straight from
`post_proc.process_batch_device(..., return_contours=True)`, and `visualize_instances_dict(..., device="cuda")` for a dict."""
import colorsys
import random
import struct
import zlib

import numpy as np


def random_colors(n, bright=True):
    """misc/viz_utils.py:22-33: n equally spaced hues, shuffled (python `random`: not reproducible by design)."""
    brightness = 1.0 if bright else 0.7
    colors = [colorsys.hsv_to_rgb(i / n, 1, brightness) for i in range(n)]
    random.shuffle(colors)
    return colors


def _segment_pixels(p0, p1):
    """Integer pixels of the straight segment p0 -> p1 (both inclusive), one per step along the major axis."""
    n = int(max(abs(p1[0] - p0[0]), abs(p1[1] - p0[1])))
    if n == 0:
        return np.array([[p0[0], p0[1]]], np.int64)
    t = np.arange(n + 1, dtype=np.float64) / n
    xs = np.floor(p0[0] + (p1[0] - p0[0]) * t + 0.5).astype(np.int64)
    ys = np.floor(p0[1] + (p1[1] - p0[1]) * t + 0.5).astype(np.int64)
    return np.stack([xs, ys], 1)


def draw_contour(img, contour, colour, thickness=2):
    """Closed polyline through `contour` (int [K,2] as (x, y)) into `img` (uint8 [H,W,3], modified in place)."""
    h, w = img.shape[:2]
    contour = np.asarray(contour, np.int64).reshape(-1, 2)
    if contour.shape[0] == 0:
        return img
    pts = [_segment_pixels(contour[i], contour[(i + 1) % contour.shape[0]]) for i in range(contour.shape[0])]
    pts = np.concatenate(pts, 0)
    lo, hi = -((thickness - 1) // 2), thickness // 2          # thickness 2 -> offsets {0, +1}; 3 -> {-1, 0, +1}
    offs = np.array([(dx, dy) for dy in range(lo, hi + 1) for dx in range(lo, hi + 1)], np.int64)
    allp = (pts[:, None, :] + offs[None]).reshape(-1, 2)
    ok = (allp[:, 0] >= 0) & (allp[:, 0] < w) & (allp[:, 1] >= 0) & (allp[:, 1] < h)
    allp = allp[ok]
    img[allp[:, 1], allp[:, 0]] = np.asarray(colour, np.uint8)
    return img


def draw_centroid_dot(img, centre, radius=3, colour=(255, 0, 0)):
    """Filled disc (`cv2.circle(..., 3, (255, 0, 0), -1)`, misc/viz_utils.py:121-124)."""
    h, w = img.shape[:2]
    cx, cy = int(centre[0]), int(centre[1])
    ys, xs = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    keep = xs * xs + ys * ys <= radius * radius
    px, py = xs[keep] + cx, ys[keep] + cy
    ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
    img[py[ok], px[ok]] = np.asarray(colour, np.uint8)
    return img


def _resolve_colours(inst_dict, type_colour):
    """The colour of every entry, chosen the way misc/viz_utils.py:100-113 does (one `random_colors` call, consumed or not)."""
    rng_colours = (np.array(random_colors(len(inst_dict))) * 255).astype(np.uint8) if len(inst_dict) else np.zeros((0, 3), np.uint8)
    out = []
    for idx, (_inst_id, info) in enumerate(inst_dict.items()):
        if "type" in info and type_colour is not None and info["type"] in type_colour:
            out.append(type_colour[info["type"]][1])
        else:
            out.append(rng_colours[idx].tolist())
    return out


def visualize_instances_dict(input_image, inst_dict, draw_dot=False, type_colour=None, line_thickness=2, *, device=None):  # noqa: A002
    """Same signature as misc/viz_utils.py:94-96.  `type_colour`: {type_id: (name, (r, g, b))}.
    `device` (keyword only): None draws on the host; a torch device draws the same pixels there (`draw_overlay_device`) --
    the colours are resolved on the host first, consuming python's `random` stream identically."""
    if device is not None:
        return _visualize_on_device(input_image, inst_dict, draw_dot, type_colour, line_thickness, device)
    overlay = np.array(input_image, copy=True)
    for (_inst_id, info), colour in zip(inst_dict.items(), _resolve_colours(inst_dict, type_colour)):
        if info.get("contour") is not None:
            draw_contour(overlay, info["contour"], colour, line_thickness)
        if draw_dot:
            draw_centroid_dot(overlay, info["centroid"])
    return overlay


# ---- the device route ------------------------------------------------------------------------------
_I32 = np.iinfo(np.int32)


def flatten_instances(inst_dict, colours):
    """dict -> `hvn_draw_overlay`'s flat host arrays, one slot per entry in dict order: (pts int32 [P,2] of (x, y),
    offs int64 [len+1], rgba uint8 [len,4] with draw flag 1, centres int32 [len,2]).  A `None` (or empty) contour owns no points;
    its slot still draws its dot.  Contours are converted the way `draw_contour` does (int64, reshape(-1, 2)), centres the way
    `draw_centroid_dot` does (`int()`: truncation); a contour vertex beyond int32 raises ValueError, a centre is clamped (it is
    outside every image either way)."""
    n = len(inst_dict)
    chunks, offs = [], np.zeros(n + 1, np.int64)
    rgba = np.zeros((n, 4), np.uint8)
    centres = np.zeros((n, 2), np.int32)
    for i, ((_inst_id, info), colour) in enumerate(zip(inst_dict.items(), colours)):
        c = np.zeros((0, 2), np.int64) if info.get("contour") is None else np.asarray(info["contour"], np.int64).reshape(-1, 2)
        if c.size and (c.min() < _I32.min or c.max() > _I32.max):
            raise ValueError("contour vertex outside the int32 range")
        chunks.append(c.astype(np.int32))
        offs[i + 1] = offs[i] + c.shape[0]
        rgba[i, :3] = np.asarray(colour, np.uint8)
        rgba[i, 3] = 1
        centres[i] = [min(max(int(info["centroid"][k]), _I32.min), _I32.max) for k in (0, 1)]
    pts = np.concatenate(chunks, 0) if chunks else np.zeros((0, 2), np.int32)
    return np.ascontiguousarray(pts, np.int32), offs, rgba, centres


def unflatten_instances(pts, offs, rgba, centres):
    """Inverse of `flatten_instances`, as a list in slot order: (contour int32 [K,2], (r, g, b), (cx, cy))."""
    return [(pts[int(offs[i]):int(offs[i + 1])], tuple(int(v) for v in rgba[i, :3]), (int(centres[i, 0]), int(centres[i, 1])))
            for i in range(len(offs) - 1)]


def _check_draw_args(thickness, dot_radius):
    if int(thickness) != thickness or not 1 <= thickness <= 7:
        raise ValueError("thickness must be an integer in 1..7, got %r" % (thickness,))
    if int(dot_radius) != dot_radius or not 0 <= dot_radius <= 15:
        raise ValueError("dot_radius must be an integer in 0..15, got %r" % (dot_radius,))


_WORKSPACE = {}


def draw_overlay_device(images, pts, offs, rgba, centres=None, *, thickness=2, dot_radius=3, dot_colour=(255, 0, 0), out=None,
                        return_status=False):
    """`hvn_draw_overlay` on the current stream, no host sync: device tensors in, uint8 device tensor [n,h,w,3] out.
    images uint8 [n,h,w,3]; pts int32 [P,2] of (x, y); offs int64 [n*slots+1] and rgba uint8 [n*slots,4] (r, g, b, draw flag) in
    `PostProc.contours`' (image, slot) layout; centres int32 [n*slots,2] or None (no dots).  `out` may be `images` (in place).
    return_status=True -> (overlay, status int32 [4] on the device = (slots with a bad offs range -- they draw nothing --,
    the first of them or -1, 0, 0))."""
    import ctypes

    import torch

    _check_draw_args(thickness, dot_radius)
    if not (torch.is_tensor(images) and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[-1] == 3 and images.is_cuda
            and images.numel()):
        raise ValueError("images must be a non-empty uint8 device tensor [n, h, w, 3]")
    n, h, w, _ = images.shape
    if offs.dtype != torch.int64 or offs.dim() != 1 or offs.numel() < 2 or (offs.numel() - 1) % n:
        raise ValueError("offs must be int64 [n * slots + 1] with slots >= 1")
    m = offs.numel() - 1
    if pts.dtype != torch.int32 or pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError("pts must be int32 [P, 2]")
    if rgba.dtype != torch.uint8 or tuple(rgba.shape) != (m, 4):
        raise ValueError("rgba must be uint8 [n * slots, 4]")
    if centres is not None and (centres.dtype != torch.int32 or tuple(centres.shape) != (m, 2)):
        raise ValueError("centres must be int32 [n * slots, 2]")
    if out is not None and (out.dtype != torch.uint8 or out.shape != images.shape or not out.is_contiguous() or out.data_ptr() % 4):
        raise ValueError("out must be a contiguous, 4-byte aligned uint8 tensor of the images' shape")
    from . import lib as L

    L.require_gpu()
    dev = images.device
    if not images.is_contiguous() or images.data_ptr() % 4:
        images = images.clone(memory_format=torch.contiguous_format)
    pts, offs, rgba = pts.contiguous(), offs.contiguous(), rgba.contiguous()
    centres = None if centres is None else centres.contiguous()
    if out is None:
        out = torch.empty_like(images)
    ws = _WORKSPACE[str(dev)] = L.grown(_WORKSPACE.get(str(dev)), L.lib().hvn_overlay_workspace_bytes(n, h, w), dev)
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    dot = (ctypes.c_uint8 * 3)(*[int(v) for v in dot_colour])
    with torch.cuda.device(dev):
        L.call("hvn_draw_overlay", images.data_ptr(), out.data_ptr(), n, h, w, pts.data_ptr() if pts.shape[0] else None, pts.shape[0],
               offs.data_ptr(), m // n, rgba.data_ptr(), None if centres is None else centres.data_ptr(),
               int(thickness), int(dot_radius), dot, status.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr(dev))
    return (out, status) if return_status else out


def overlay_from_records(images, rec, pts, offs, type_colours, *, draw_dot=False, thickness=2):
    """The device-resident route from `post_proc.process_batch_device(..., nr_types, True, return_contours=True)`: images uint8
    [n,h,w,3] on the device, rec / pts / offs as returned there, type_colours [nr_types,3] (the colour of type id t in row t; every
    type id of the records must have a row) -> the overlays `visualize_instances_dict(image, records_to_dict(...), type_colour=...)`
    draws, as a uint8 device tensor.  A record draws when area > 0 and its contour has at least 3 points (`records_to_dict`'s
    rule); centres are int(centroid).  Torch ops and one library call on the current stream, no host sync."""
    import torch

    n, max_inst = rec.shape[0], rec.shape[1]
    rec = rec.contiguous()
    i32 = rec.view(torch.int32)                                      # label, area, rmin, rmax, cmin, cmax, -, -, -, -, type, type_count
    f64 = rec.view(torch.float64)                                    # -, -, -, sum_x, sum_y, -
    area = i32[..., 1].reshape(-1)
    draw = (area > 0) & ((offs[1:] - offs[:-1]) >= 3)
    table = torch.as_tensor(np.asarray(type_colours), device=rec.device).to(torch.uint8).reshape(-1, 3)
    colour = table[i32[..., 10].reshape(-1).long().clamp_(0, table.shape[0] - 1)]
    rgba = torch.cat([colour, draw.to(torch.uint8)[:, None]], 1).contiguous()
    centres = None
    if draw_dot:
        a = torch.where(draw, area, torch.ones_like(area)).double()
        cx = f64[..., 3].reshape(-1) / a + i32[..., 4].reshape(-1).double()
        cy = f64[..., 4].reshape(-1) / a + i32[..., 2].reshape(-1).double()
        centres = torch.where(draw[:, None], torch.stack([cx, cy], 1), torch.zeros((), dtype=torch.float64, device=rec.device)).trunc().to(torch.int32)
    assert rgba.shape[0] == n * max_inst
    return draw_overlay_device(images, pts, offs, rgba, centres, thickness=thickness)


def _visualize_on_device(input_image, inst_dict, draw_dot, type_colour, line_thickness, device):
    import torch

    _check_draw_args(line_thickness, 3)
    img = np.asarray(input_image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("the device overlay needs a uint8 [H, W, 3] image, got %s %s" % (img.dtype, img.shape))
    flat = flatten_instances(inst_dict, _resolve_colours(inst_dict, type_colour))
    if not len(inst_dict):
        return np.array(img, copy=True)
    dev = torch.device(device)
    pts, offs, rgba, centres = (torch.from_numpy(a).to(dev) for a in flat)
    out = draw_overlay_device(torch.from_numpy(np.ascontiguousarray(img)[None]).to(dev), pts, offs, rgba, centres if draw_dot else None,
                              thickness=int(line_thickness))
    return out[0].cpu().numpy()


# ---- the run loop's picture (models/hovernet/run_desc.py:201-256 viz_step_output) -------------------------------------------------
# matplotlib's "jet" as its published segment points (x, y below, y above), per channel
_JET = (((0.0, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.0, 0.5, 0.5)),
        ((0.0, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.64, 1, 1), (0.91, 0, 0), (1.0, 0, 0)),
        ((0.0, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.0, 0, 0)))
_JET_LUT = None
MAX_TYPES = 16      # the kernel's cap on nr_types


def jet_lut():
    """uint8 [256,3] = `(plt.get_cmap("jet")(np.arange(256))[:, :3] * 255).astype("uint8")` without matplotlib: the linear
    interpolation of a 256-entry segmented colormap (gamma 1) between `_JET`'s points, in float64, truncated like the reference does."""
    global _JET_LUT
    if _JET_LUT is None:
        n = 256
        xind = (n - 1) * np.linspace(0, 1, n)
        lut = np.empty((n, 3), np.float64)
        for ch, data in enumerate(_JET):
            d = np.array(data, np.float64)
            x, y0, y1 = d[:, 0] * (n - 1), d[:, 1], d[:, 2]
            ind = np.searchsorted(x, xind)[1:-1]
            dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
            lut[:, ch] = np.clip(np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0.0, 1.0)
        _JET_LUT = (lut * 255).astype(np.uint8)
        _JET_LUT.setflags(write=False)
    return _JET_LUT


def colorize(ch, vmin, vmax):
    """The reference's `colorize` (run_desc.py:218-229) as float32 arithmetic and a table: clamp to [vmin, vmax], (v - vmin) /
    float32(vmax - vmin) -- the reference's `+ 1.0e-16` vanishes in double for every range it uses --, times 256, truncated, 256 ->
    255, looked up in `jet_lut()`; NaN -> (0, 0, 0).  uint8 [..., 3] of `np.squeeze(ch)`'s shape.  This is the definition the
    device kernel (csrc/hvn_viz.hip) is held to."""
    v = np.squeeze(np.asarray(ch).astype(np.float32))
    bad = np.isnan(v)
    v = np.where(v > vmax, np.float32(vmax), v)
    v = np.where(v < vmin, np.float32(vmin), v)
    with np.errstate(invalid="ignore"):
        t = ((v - np.float32(vmin)) / np.float32(float(vmax - vmin) + 1.0e-16)) * np.float32(256.0)
        k = np.minimum(np.where(bad, np.float32(0), t).astype(np.int64), 255)
    out = np.array(jet_lut()[k])        # a copy also for a map that squeezes to one value
    out[bad] = 0
    return out


_LUT_DEV = {}


def strip_device(img, pred, np_map, hv_map, tp_map, sel, out=None, n_blocks=None, nr_types=None):
    """`hvn_viz_strip` (include/hvn.h) on the current stream of `img`'s device, no host sync unless `sel` is a device tensor (then
    one, to check it): the picture `run_desc.viz_step_output` draws, as a uint8 device tensor [n_blocks * 2h, ncol * w, 3].
    img uint8 [n,ih,iw,3]; pred float32 [n,h,w,3] = (p_nuc, h, v), or [n,h,w,4] = (type, p_nuc, h, v) with `nr_types`; np_map int32
    [n,h,w]; hv_map float32 [n,h,w,2]; tp_map int32 [n,h,w] or None (no TP column); all contiguous device tensors.  sel: pairs
    (sample in the batch, block of the strip), int [n_sel,2] as a host sequence / array, or an int32 device tensor; a pair out of
    range raises ValueError before anything is launched.  Every pair draws its block (two pairs naming one block race); the other
    blocks keep what `out` holds (a new `out` is zeroed).  n_blocks defaults to out's, else to n_sel."""
    import torch

    from . import lib as L

    nt = 0 if nr_types is None else int(nr_types)
    if nr_types is not None and not 0 < nt <= MAX_TYPES:
        raise ValueError("nr_types must be None or in [1, %d]" % MAX_TYPES)

    def dev_tensor(t, dtype, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.device == img.device):
            raise ValueError("%s must be a contiguous %s tensor on the image's device" % (what, dtype))

    if not (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 4 and img.shape[-1] == 3 and img.is_contiguous()
            and img.numel()):
        raise ValueError("img must be a non-empty contiguous uint8 device tensor [n, ih, iw, 3]")
    dev = img.device
    n, ih, iw, _ = (int(v) for v in img.shape)
    dev_tensor(pred, torch.float32, "pred")
    if pred.dim() != 4 or int(pred.shape[0]) != n or int(pred.shape[3]) != (4 if nt else 3) or not pred.numel():
        raise ValueError("pred must be [n, h, w, %d] (nr_types = %r), got %s" % (4 if nt else 3, nr_types, tuple(pred.shape)))
    h, w, c = (int(v) for v in pred.shape[1:])
    if ih < h or iw < w:
        raise ValueError("the image (%d x %d) is smaller than the maps (%d x %d)" % (ih, iw, h, w))
    dev_tensor(np_map, torch.int32, "np_map")
    dev_tensor(hv_map, torch.float32, "hv_map")
    if tuple(np_map.shape) != (n, h, w) or tuple(hv_map.shape) != (n, h, w, 2):
        raise ValueError("np_map must be [n, h, w] and hv_map [n, h, w, 2]")
    if tp_map is not None:
        dev_tensor(tp_map, torch.int32, "tp_map")
        if tuple(tp_map.shape) != (n, h, w):
            raise ValueError("tp_map must be [n, h, w]")
    ncol = 5 if nt and tp_map is not None else 4
    if torch.is_tensor(sel) and sel.is_cuda:
        dev_tensor(sel, torch.int32, "sel")
        sel_dev, sel_host = sel, sel.cpu().numpy()
    else:
        sel_host = np.asarray(sel.cpu() if torch.is_tensor(sel) else sel, np.int64).reshape(-1, 2)
        sel_dev = None
    sel_host = sel_host.reshape(-1, 2)
    n_sel = int(sel_host.shape[0])
    if out is not None:
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev and out.dim() == 3
                and int(out.shape[0]) % (2 * h) == 0 and int(out.shape[0]) > 0 and tuple(out.shape[1:]) == (ncol * w, 3)):
            raise ValueError("out must be a contiguous uint8 device tensor [n_blocks * %d, %d, 3]" % (2 * h, ncol * w))
        if n_blocks is not None and int(n_blocks) != int(out.shape[0]) // (2 * h):
            raise ValueError("n_blocks = %d, but out holds %d blocks" % (n_blocks, int(out.shape[0]) // (2 * h)))
        n_blocks = int(out.shape[0]) // (2 * h)
    n_blocks = n_sel if n_blocks is None else int(n_blocks)
    if n_blocks < 1 and n_sel == 0:
        return torch.zeros((0, ncol * w, 3), dtype=torch.uint8, device=dev)
    if n_blocks < 1:
        raise ValueError("n_blocks must be at least 1")
    if n_sel and ((sel_host[:, 0] < 0) | (sel_host[:, 0] >= n) | (sel_host[:, 1] < 0) | (sel_host[:, 1] >= n_blocks)).any():
        raise ValueError("sel: a pair names a sample outside [0, %d) or a block outside [0, %d)" % (n, n_blocks))
    if out is None:
        out = torch.zeros((n_blocks * 2 * h, ncol * w, 3), dtype=torch.uint8, device=dev)
    if n_sel == 0:
        return out
    L.require_gpu()
    if sel_dev is None:
        sel_dev = torch.from_numpy(np.ascontiguousarray(sel_host, np.int32)).to(dev, non_blocking=True)
    lut = _LUT_DEV.get(str(dev))
    if lut is None:
        lut = _LUT_DEV[str(dev)] = torch.from_numpy(np.array(jet_lut())).to(dev)
    with torch.cuda.device(dev):
        L.call("hvn_viz_strip", img.data_ptr(), n, ih, iw, pred.data_ptr(), c, np_map.data_ptr(), hv_map.data_ptr(),
               None if tp_map is None else tp_map.data_ptr(), h, w, nt, sel_dev.data_ptr(), n_sel, lut.data_ptr(),
               out.data_ptr(), n_blocks, L.stream_ptr(dev))
    return out


def save_png(path, rgb):
    """uint8 [H,W,3] -> PNG.  PIL when present, else a minimal zlib writer (8-bit RGB, filter 0)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    try:
        from PIL import Image

        Image.fromarray(rgb).save(path)
        return
    except ImportError:
        pass
    h, w = rgb.shape[:2]
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))

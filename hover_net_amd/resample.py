"""Resampling a slide to the processing magnification (`proc_mag`) -- the whole-slide resize of `misc/wsi_handler.py:59-99,
167-190` (`cv2.resize` of the WHOLE slide on the host, `INTER_CUBIC` up / `INTER_LINEAR` down, into a cache file) done window by
window instead: a chunk reads the native-resolution box its taps touch, and the box is resampled where the chunk is consumed
(`resize_window_host` on the host, `resize_window_device` = csrc/hvn_resample.hip on the GPU).  No cache file, no whole-slide
resize, and the upload is 1 / f^2 of the resampled bytes.

The arithmetic restates OpenCV's SCALAR 8-bit fixed-point `resize` path with 11 coefficient bits (ONE = 2048): float32 coefficient
tables per axis, rounded to int16; an exact int32 horizontal pass; an integer vertical pass.  OpenCV is not on the box, so the
restatement is UNPINNED against it (as tissue_mask.py's two calls are).  Two known differences from the OpenCV library: its SIMD
cubic vertical pass goes through float32 (this one stays in integers), and it swaps an exact 1/2 `INTER_LINEAR` for `INTER_AREA`
(this one uses the generic formula for every factor).  What IS pinned: the window property (a window of the output depends only on
its own table entries, so chunks and ranks agree with the whole-image resize bit for bit), 1 grey level against the float64
evaluation of the same float32 coefficients, and bit equality of the device kernel with this module (tests/test_resample_host.py,
tests/test_gpu_resample.py).

    f = proc_mag / base_mag;  kind = "cubic" if f > 1 else "linear";  f == 1: no resampling at all.
"""
import functools

import numpy as np

ONE_BITS = 11
ONE = 1 << ONE_BITS          # 2048
CUBIC_A = np.float32(-0.75)


def kind_of(f):
    return "cubic" if f > 1 else "linear"


def out_size(n, f):
    """Round-half-even of n * f in float64."""
    return int(np.rint(float(n) * float(f)))


def _axis(n_src, n_dst, f, kind):
    """(s int32 [n_dst], c float32 [n_dst, taps]): the float32 coefficients before they are rounded to int16."""
    assert kind in ("cubic", "linear"), kind
    f32 = np.float32
    d = np.arange(int(n_dst), dtype=np.float64)
    fx = ((d + 0.5) * (1.0 / float(f)) - 0.5).astype(f32)     # float64 product, rounded once
    s = np.floor(fx).astype(np.int32)
    fx = (fx - s.astype(f32)).astype(f32)
    if kind == "linear":
        low, high = s < 0, s >= int(n_src) - 1
        s = np.where(low, 0, np.where(high, int(n_src) - 1, s)).astype(np.int32)
        fx = np.where(low | high, f32(0), fx).astype(f32)
        c = np.stack([f32(1) - fx, fx], axis=1)
    else:
        A = CUBIC_A
        x, y = fx, f32(1) - fx
        x1 = x + f32(1)
        c0 = ((A * x1 - f32(5) * A) * x1 + f32(8) * A) * x1 - f32(4) * A
        c1 = ((A + f32(2)) * x - (A + f32(3))) * x * x + f32(1)
        c2 = ((A + f32(2)) * y - (A + f32(3))) * y * y + f32(1)
        c3 = f32(1) - c0 - c1 - c2
        c = np.stack([c0, c1, c2, c3], axis=1)
    assert c.dtype == np.float32
    return s, c


def axis_table(n_src, n_dst, f, kind):
    """(ofs int32 [n_dst], coef int16 [n_dst, taps]), taps = 4 (cubic) | 2 (linear).  Tap k of entry d reads source index
    clamp(ofs[d] + k - (taps == 4), 0, n_src - 1) (`tap_index`)."""
    s, c = _axis(n_src, n_dst, f, kind)
    return s, np.rint(c * np.float32(ONE)).astype(np.int16)


def tap_index(ofs, n_src, taps):
    """int64 [n, taps]: the source index of every tap, clamped against the FULL source axis."""
    k = np.arange(taps, dtype=np.int64) - (1 if taps == 4 else 0)
    return np.clip(ofs.astype(np.int64)[:, None] + k[None, :], 0, int(n_src) - 1)


@functools.lru_cache(maxsize=8)
def _full_tables(H, W, f, kind):
    """Both full-axis tables of one slide, kept between the chunk reads of a run (shared: callers slice them and never write)."""
    return axis_table(W, out_size(W, f), f, kind) + axis_table(H, out_size(H, f), f, kind)


def _tables(full_shape, f, kind):
    return _full_tables(int(full_shape[0]), int(full_shape[1]), float(f), kind or kind_of(f))


def _passes(src, xi, xc, yi, yc):
    """src uint8 [sh, sw, 3]; xi [w, taps] / yi [h, taps]: tap indices INTO src; xc / yc int16 [., taps] -> uint8 [h, w, 3]."""
    taps = xc.shape[1]
    src = np.asarray(src)[..., :3]
    xc32, yc32 = xc.astype(np.int32), yc.astype(np.int32)
    hor = np.zeros((src.shape[0], xi.shape[0], 3), np.int32)               # horizontal pass: exact int32
    for k in range(taps):
        hor += src[:, xi[:, k], :].astype(np.int32) * xc32[:, k][None, :, None]
    out = np.empty((yi.shape[0], xi.shape[0], 3), np.uint8)
    for r0 in range(0, yi.shape[0], 256):                                  # strips bound the temporaries, not the arithmetic
        r1 = min(r0 + 256, yi.shape[0])
        if taps == 4:
            v = np.zeros((r1 - r0, xi.shape[0], 3), np.int32)
            for k in range(4):
                v += hor[yi[r0:r1, k]] * yc32[r0:r1, k][:, None, None]
            out[r0:r1] = np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
        else:
            a = (yc32[r0:r1, 0][:, None, None] * (hor[yi[r0:r1, 0]] >> 4)) >> 16
            b = (yc32[r0:r1, 1][:, None, None] * (hor[yi[r0:r1, 1]] >> 4)) >> 16
            out[r0:r1] = ((a + b + 2) >> 2).astype(np.uint8)
    return out


def window_tables(full_shape, f, y0, x0, h, w, kind=None):
    """(xofs, xcoef, yofs, ycoef) of the output window [y0, y0 + h) x [x0, x0 + w): the window's entries of the full tables,
    ofs in FULL-source coordinates."""
    xo, xc, yo, yc = _tables(full_shape, f, kind)
    y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    assert 0 <= y0 and 0 <= x0 and h > 0 and w > 0 and y0 + h <= yo.shape[0] and x0 + w <= xo.shape[0], \
        ((y0, x0, h, w), (yo.shape[0], xo.shape[0]))
    return xo[x0:x0 + w], xc[x0:x0 + w], yo[y0:y0 + h], yc[y0:y0 + h]


def _box(full_shape, xo, xc, yo, yc):
    yi = tap_index(yo, full_shape[0], yc.shape[1])
    xi = tap_index(xo, full_shape[1], xc.shape[1])
    sy0, sx0 = int(yi.min()), int(xi.min())
    return yi, xi, (sy0, sx0, int(yi.max()) - sy0 + 1, int(xi.max()) - sx0 + 1)


def tables_box(full_shape, tables):
    """(sy0, sx0, sh, sw) covering every clamped tap of `window_tables`' result."""
    return _box(full_shape, *tables)[2]


def source_window(full_shape, f, y0, x0, h, w, kind=None):
    """(sy0, sx0, sh, sw): the source box covering every clamped tap of the output window."""
    if f == 1 and kind is None:
        return int(y0), int(x0), int(h), int(w)
    return _box(full_shape, *window_tables(full_shape, f, y0, x0, h, w, kind))[2]


def resize_window_host(read_rows, full_shape, f, y0, x0, h, w, kind=None):
    """uint8 [h, w, 3]: the window [y0, y0 + h) x [x0, x0 + w) of `resize_host` of the full source, from the source box its taps
    touch alone.  read_rows: `(sy0, sx0, sh, sw) -> uint8 [sh, sw, 3]`, or the full source as an array."""
    if not callable(read_rows):
        full = read_rows
        read_rows = lambda sy, sx, sh, sw: full[sy:sy + sh, sx:sx + sw]  # noqa: E731
    if f == 1 and kind is None:
        return np.array(np.asarray(read_rows(int(y0), int(x0), int(h), int(w)))[..., :3])
    xo, xc, yo, yc = window_tables(full_shape, f, y0, x0, h, w, kind)
    yi, xi, (sy0, sx0, sh, sw) = _box(full_shape, xo, xc, yo, yc)
    src = np.asarray(read_rows(sy0, sx0, sh, sw))
    assert src.shape[:2] == (sh, sw) and src.dtype == np.uint8, (src.shape, src.dtype, (sh, sw))
    return _passes(src, xi - sx0, xc, yi - sy0, yc)


def resize_host(img, f, kind=None):
    """uint8 [H, W, 3] -> uint8 [out_size(H, f), out_size(W, f), 3].  kind=None: by the factor, and f == 1 is a copy; a given
    kind runs the arithmetic for any factor."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] >= 3, (img.dtype, img.shape)
    H, W = img.shape[:2]
    return resize_window_host(img, (H, W), f, 0, 0, out_size(H, f), out_size(W, f), kind)


def resize_float64(img, f, kind=None):
    """floor(x + 0.5) clipped of the float64 evaluation of the same float32 coefficients: what the fixed-point passes
    approximate (the tests bound the difference by 1 grey level)."""
    img = np.asarray(img)[..., :3]
    H, W = img.shape[:2]
    kind = kind or kind_of(f)
    ys, yc = _axis(H, out_size(H, f), f, kind)
    xs, xc = _axis(W, out_size(W, f), f, kind)
    yi, xi = tap_index(ys, H, yc.shape[1]), tap_index(xs, W, xc.shape[1])
    src = img.astype(np.float64)
    hor = sum(src[:, xi[:, k], :] * xc[:, k].astype(np.float64)[None, :, None] for k in range(xc.shape[1]))
    v = sum(hor[yi[:, k]] * yc[:, k].astype(np.float64)[:, None, None] for k in range(yc.shape[1]))
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


# ----------------------------------------------------------------------------------------------
def resize_window_device(src_dev, src_origin, full_shape, f, y0, x0, h, w, kind=None, out=None, tables=None):
    """src_dev: uint8 device tensor [sh, sw, 3], the box of the full source [full_shape] whose top-left is src_origin = (sy0, sx0)
    (rows may be strided: stride(0) >= 3 * sw) -> uint8 device tensor [h, w, 3] = the window [y0, y0 + h) x [x0, x0 + w) of the
    resampled source, bit-equal to `resize_window_host` (hvn_resize_window on the current stream; `out` = write into this
    contiguous tensor; `tables` = the window's `window_tables`, when the caller has made them already).  The coefficient tables are made here on the host and uploaded: the device does integer arithmetic only.
    A box that does not hold every clamped tap of the window is refused BEFORE the launch (lib.HvnError, `out` untouched): the
    tables live on the device, so the launcher cannot see their end values; it checks the box against the full source."""
    import torch

    from . import lib as L

    L.require_gpu()
    assert src_dev.dtype == torch.uint8 and src_dev.is_cuda and src_dev.dim() == 3 and src_dev.shape[2] == 3
    if src_dev.stride(2) != 1 or src_dev.stride(1) != 3:
        src_dev = src_dev.contiguous()
    sy0, sx0 = int(src_origin[0]), int(src_origin[1])
    sh, sw = int(src_dev.shape[0]), int(src_dev.shape[1])
    h, w = int(h), int(w)
    xo, xc, yo, yc = tables if tables is not None else window_tables(full_shape, f, y0, x0, h, w, kind)
    assert xo.shape[0] == w and yo.shape[0] == h, ((yo.shape[0], xo.shape[0]), (h, w))
    _yi, _xi, (by0, bx0, bh, bw) = _box(full_shape, xo, xc, yo, yc)
    if by0 < sy0 or bx0 < sx0 or by0 + bh > sy0 + sh or bx0 + bw > sx0 + sw:
        raise L.HvnError("hvn_resize_window refused (%d): the uploaded box rows [%d, %d) x columns [%d, %d) lacks a tap of the window "
                         "(taps reach rows [%d, %d) x columns [%d, %d))" % (-1, sy0, sy0 + sh, sx0, sx0 + sw, by0, by0 + bh, bx0, bx0 + bw))
    dev = src_dev.device
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (h, w, 3) and out.device == dev
    tabs = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xo, xc, yo, yc)]
    L.call("hvn_resize_window", src_dev.data_ptr(), sh, sw, int(src_dev.stride(0)), sy0, sx0, int(full_shape[0]), int(full_shape[1]),
           tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(), int(xc.shape[1]),
           out.data_ptr(), h, w, L.stream_ptr(dev))
    return out

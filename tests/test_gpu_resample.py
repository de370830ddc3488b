"""csrc/hvn_resample.hip against hover_net_amd/resample.py: every comparison is bit equality with the host statement of the
arithmetic.  The kernel's tile is 16 rows x 80 pixels (240 bytes), its LDS holds 36 source rows per row group."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from hover_net_amd import resample as R
from resample_cases import checkerboard, random_image, windows

pytestmark = pytest.mark.gpu
TILE_H, TILE_W = 16, 80


@functools.lru_cache(maxsize=None)
def source(name, h, w):
    return {"random": lambda: random_image(h, w, 11), "checker": lambda: checkerboard(h, w), "checker3": lambda: checkerboard(h, w, 3)}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, h, w, f):
    """The whole-image host resize, computed once per (source, factor) and shared; never written."""
    out = R.resize_host(source(name, h, w), f)
    out.setflags(write=False)
    return out


def device_window(img, f, y0, x0, h, w, box=None, pad=0):
    """The window on the device from the source box `box` (default: exactly source_window's) uploaded alone."""
    sy, sx, sh, sw = box or R.source_window(img.shape[:2], f, y0, x0, h, w)
    if pad:                                                         # rows `pad` pixels longer than the box: src_pitch > 3 * src_w
        wide = torch.from_numpy(np.ascontiguousarray(np.pad(img[sy:sy + sh, sx:sx + sw], ((0, 0), (0, pad), (0, 0)), constant_values=201))).to("cuda")
        src = wide[:, :sw]
        assert src.stride(0) == 3 * (sw + pad)
    else:
        src = torch.from_numpy(np.ascontiguousarray(img[sy:sy + sh, sx:sx + sw])).to("cuda")
    return R.resize_window_device(src, (sy, sx), img.shape[:2], f, y0, x0, h, w).cpu().numpy()


@pytest.mark.parametrize("name", ["random", "checker", "checker3"])
@pytest.mark.parametrize("f", [2.0, 1.6, 40 / 26, 0.625, 0.5])
@pytest.mark.parametrize("shape", [(37, 53), (64, 64)])
def test_full_image(shape, f, name):
    img, want = source(name, *shape), reference(name, *shape, f)
    got = device_window(img, f, 0, 0, want.shape[0], want.shape[1])
    assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("f", [2.0, 1.6, 0.625, 0.5])
def test_windows_from_their_source_box_alone(f):
    """Origin translation and full-source clamping: corners (the bottom-right box ends at the source's edge), an odd interior
    origin, one row, one column, 1 x 1."""
    img, want = source("random", 37, 53), reference("random", 37, 53, f)
    H, W = want.shape[:2]
    for y0, x0, h, w in windows(H, W):
        sy, sx, sh, sw = R.source_window((37, 53), f, y0, x0, h, w)
        if (y0 + h, x0 + w) == (H, W) and f != 0.5:                     # (at 1/2 the last taps of an odd size stop one short of the edge)
            assert (sy + sh, sx + sw) == (37, 53)
        assert np.array_equal(device_window(img, f, y0, x0, h, w), want[y0:y0 + h, x0:x0 + w]), (f, y0, x0, h, w)


@pytest.mark.parametrize("f", [2.0, 0.625])
def test_shapes_around_the_tile_edges(f):
    """tile - 1, tile, tile + 1 rows and columns, from an odd x0 (rows start on an unaligned byte of the source box), widths whose
    3 * w is no multiple of 4 (79, 81: every second output row starts off a dword), and a second tile in each direction."""
    shape = (40, 90) if f > 1 else (120, 280)
    img, want = source("random", *shape), reference("random", *shape, f)
    assert want.shape[0] >= 2 * TILE_H + 3 and want.shape[1] >= 2 * TILE_W + 4
    for h in (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1):
        for w in (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1):
            for y0, x0 in ((0, 0), (1, 3)):
                assert np.array_equal(device_window(img, f, y0, x0, h, w), want[y0:y0 + h, x0:x0 + w]), (f, y0, x0, h, w)


@pytest.mark.parametrize("f", [0.25, 0.2])
def test_small_factors_take_several_row_groups(f):
    """Below 1/2 a 16-row tile needs more source rows (about 64 and 80) than the LDS holds (36): the tile is worked in row groups."""
    img, want = source("random", 200, 470), reference("random", 200, 470, f)
    assert want.shape[0] > 2 * TILE_H and want.shape[1] > TILE_W
    assert np.array_equal(device_window(img, f, 0, 0, want.shape[0], want.shape[1]), want)
    assert np.array_equal(device_window(img, f, 5, 7, 33, 83), want[5:38, 7:90])


def test_single_pixel_and_single_row_windows():
    img, want = source("checker3", 64, 64), reference("checker3", 64, 64, 1.6)
    H, W = want.shape[:2]
    for y0, x0, h, w in [(0, 0, 1, 1), (H - 1, W - 1, 1, 1), (50, 51, 1, 1), (9, 0, 1, W), (H - 1, 1, 1, W - 1), (0, 7, H, 1)]:
        assert np.array_equal(device_window(img, 1.6, y0, x0, h, w), want[y0:y0 + h, x0:x0 + w]), (y0, x0, h, w)


def test_source_pitch_longer_than_a_row():
    img = source("random", 64, 64)
    for f, (y0, x0, h, w) in [(2.0, (3, 5, 40, 90)), (0.5, (1, 1, 20, 30))]:
        want = reference("random", 64, 64, f)
        assert np.array_equal(device_window(img, f, y0, x0, h, w, pad=5), want[y0:y0 + h, x0:x0 + w])
    # a box larger than the window needs: the origin translation is by the box, not by the first tap
    want = reference("random", 64, 64, 2.0)
    assert np.array_equal(device_window(img, 2.0, 30, 31, 20, 21, box=(10, 11, 30, 33)), want[30:50, 31:52])


def test_a_box_that_lacks_a_tap_is_refused_before_the_launch():
    from hover_net_amd import lib as L

    img = source("random", 64, 64)
    sy, sx, sh, sw = R.source_window((64, 64), 2.0, 20, 20, 30, 30)
    out = torch.full((30, 30, 3), 123, dtype=torch.uint8, device="cuda")
    for box in [(sy, sx, sh - 1, sw), (sy + 1, sx, sh - 1, sw), (sy, sx, sh, sw - 1), (sy, sx + 1, sh, sw - 1)]:      # last / first tap row, column
        by, bx, bh, bw = box
        src = torch.from_numpy(np.ascontiguousarray(img[by:by + bh, bx:bx + bw])).to("cuda")
        with pytest.raises(L.HvnError, match="lacks a tap"):
            R.resize_window_device(src, (by, bx), (64, 64), 2.0, 20, 20, 30, 30, out=out)
    # the launcher's own argument checks, through lib.check: a box that leaves the full source, taps that are neither 2 nor 4
    src = torch.from_numpy(np.ascontiguousarray(img[sy:sy + sh, sx:sx + sw])).to("cuda")
    xo, xc, yo, yc = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in R.window_tables((64, 64), 2.0, 20, 20, 30, 30))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(src_y0, full_h, taps):
        return L.lib().hvn_resize_window(src.data_ptr(), sh, sw, 3 * sw, src_y0, sx, full_h, 64, xo.data_ptr(), xc.data_ptr(), yo.data_ptr(),
                                         yc.data_ptr(), taps, out.data_ptr(), 30, 30, stream)

    for args, text in [((sy, sy + sh - 1, 4), "leaves the full source"), ((-1, 64, 4), "leaves the full source"), ((sy, 64, 3), "taps")]:
        with pytest.raises(L.HvnError, match=text):
            L.check(call(*args), "hvn_resize_window")
    torch.cuda.synchronize()
    assert bool((out == 123).all())                                   # nothing was launched
    L.check(call(sy, 64, 4), "hvn_resize_window")                     # and the same call with right arguments draws the window
    assert np.array_equal(out.cpu().numpy(), reference("random", 64, 64, 2.0)[20:50, 20:50])


@pytest.fixture(scope="module")
def net():
    from hover_net_amd import net_desc
    from hover_net_amd.synth import synth_state_dict

    model = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    model.load_state_dict(synth_state_dict("original", 5, seed=81), strict=True)
    return model.to("cuda").eval()


@pytest.mark.parametrize("shape,base_mag,proc_mag", [((450, 505), 20, 40), ((1800, 2020), 40, 20)])
def test_whole_slide_prediction_equals_the_resized_slide(net, shape, base_mag, proc_mag):
    """Chunks of 700 cut the resampled 900 x 1010 slide where a whole-image resize never does: the map predicted from
    `ScaledSlide` (rows uploaded at the base resolution, resampled on the GPU chunk by chunk) is bit-equal to the map predicted
    from the host-resized array."""
    from hover_net_amd import infer_wsi

    a = random_image(shape[0], shape[1], 12)
    wsi = infer_wsi.WsiInference(net, nr_types=5, batch_size=16, chunk_shape=700, tile_shape=512, ambiguous_size=64)
    mask = np.ones((30, 34), np.uint8)
    scaled = infer_wsi.ScaledSlide(infer_wsi.ArraySlide(a), base_mag, proc_mag)
    assert tuple(scaled.shape) == (900, 1010, 3)
    calls = []
    read_device = scaled.read_region_device
    scaled.read_region_device = lambda *args: calls.append(args[:2]) or read_device(*args)
    got = wsi.raw_prediction(scaled, mask)
    assert len(calls) > 1                                             # several chunks, each read through the device resampler
    want = wsi.raw_prediction(infer_wsi.ArraySlide(R.resize_host(a, proc_mag / base_mag)), mask)
    assert tuple(got.shape) == (900, 1010, 4) and torch.equal(got, want)

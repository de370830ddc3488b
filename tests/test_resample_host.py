"""hover_net_amd/resample.py on the host: the fixed-point resize restated (identity at f = 1, the window property that lets chunks
and ranks agree with the whole-image resize, 1 grey level against the float64 evaluation of the same coefficients), the
`ScaledSlide` backend and the manager's `base_mag` run argument."""
import os

import numpy as np
import pytest

from hover_net_amd import resample as R
from resample_cases import checkerboard, random_image, windows

FACTORS = [2.0, 1.6, 0.625, 0.5]


@pytest.mark.parametrize("kind", ["cubic", "linear"])
def test_factor_one_is_the_identity(kind):
    for img in (random_image(37, 53, 1), checkerboard(37, 53)):
        assert np.array_equal(R.resize_host(img, 1.0, kind=kind), img)
    ofs, coef = R.axis_table(53, 53, 1.0, kind)
    assert ofs.dtype == np.int32 and coef.dtype == np.int16 and coef.shape == (53, 4 if kind == "cubic" else 2)
    assert np.array_equal(ofs, np.arange(53)) and np.all(coef[:, 1 if kind == "cubic" else 0] == R.ONE) and np.all(coef.sum(1) == R.ONE)
    img = random_image(9, 11, 2)
    assert R.resize_host(img, 1.0) is not img and np.array_equal(R.resize_host(img, 1.0), img)      # no kind: a copy, no arithmetic
    assert R.source_window((9, 11), 1.0, 2, 3, 4, 5) == (2, 3, 4, 5)


def test_sizes_and_kinds():
    assert [R.out_size(n, f) for n, f in [(37, 2.0), (37, 1.6), (53, 0.625), (37, 0.5), (5, 0.5), (7, 0.5)]] == [74, 59, 33, 18, 2, 4]
    assert R.kind_of(2.0) == "cubic" and R.kind_of(0.5) == "linear" and R.kind_of(40 / 26) == "cubic"
    for f in FACTORS:
        out = R.resize_host(random_image(37, 53, 3), f)
        assert out.dtype == np.uint8 and out.shape == (R.out_size(37, f), R.out_size(53, f), 3)


@pytest.mark.parametrize("f", FACTORS)
def test_window_property(f):
    """A window of the output, computed from the source box its taps touch alone, is that crop of the whole-image resize."""
    img = random_image(37, 53, 4)
    full = R.resize_host(img, f)
    H, W = full.shape[:2]
    for y0, x0, h, w in windows(H, W):
        sy, sx, sh, sw = R.source_window((37, 53), f, y0, x0, h, w)
        assert 0 <= sy and 0 <= sx and sh > 0 and sw > 0 and sy + sh <= 37 and sx + sw <= 53, (y0, x0, h, w)
        reads = []

        def read(by, bx, bh, bw):
            reads.append((by, bx, bh, bw))
            return img[by:by + bh, bx:bx + bw]

        got = R.resize_window_host(read, (37, 53), f, y0, x0, h, w)
        assert reads == [(sy, sx, sh, sw)]                              # one read, of exactly the box source_window names
        assert np.array_equal(got, full[y0:y0 + h, x0:x0 + w]), (f, y0, x0, h, w)
    # an interior window reads far less than the source
    sy, sx, sh, sw = R.source_window((37, 53), f, H // 2, W // 2, 2, 2)
    assert sh <= 2 / f + 5 and sw <= 2 / f + 5


@pytest.mark.parametrize("f", FACTORS + [40 / 26])
def test_within_one_grey_level_of_the_float64_evaluation(f):
    """A sanity check on the restatement (measured on a 37 x 53 prototype: at most 1), not on the kernel."""
    for img in (random_image(37, 53, 5), checkerboard(37, 53), checkerboard(37, 53, 3)):
        got, want = R.resize_host(img, f).astype(np.int32), R.resize_float64(img, f).astype(np.int32)
        assert np.abs(got - want).max() <= 1
    if f > 1:                                                             # cells of 3 drive the cubic past both ends
        raw = R.resize_host(checkerboard(37, 53, 3), f)
        assert raw.min() == 0 and raw.max() == 255


def test_every_tap_clamped_on_a_tiny_source():
    img = random_image(3, 3, 6)
    ofs, coef = R.axis_table(3, 6, 2.0, "cubic")
    idx = R.tap_index(ofs, 3, 4)
    assert idx.min() == 0 and idx.max() == 2 and all(len(set(row)) < 4 for row in idx.tolist())   # every entry repeats a source index
    out = R.resize_host(img, 2.0)
    assert out.shape == (6, 6, 3) and np.abs(out.astype(np.int32) - R.resize_float64(img, 2.0)).max() <= 1
    assert np.array_equal(R.resize_window_host(img, (3, 3), 2.0, 5, 5, 1, 1), out[5:, 5:])
    flat = np.full((3, 3, 3), 77, np.uint8)
    assert np.all(R.resize_host(flat, 2.0) == 77) and np.all(R.resize_host(flat, 0.5) == 77)


def test_scaled_slide_reads_windows_of_the_whole_resize():
    from hover_net_amd import infer_wsi

    a = random_image(40, 50, 7)
    for base_mag, proc_mag in [(20, 40), (40, 20), (26, 40)]:
        f = proc_mag / base_mag
        full = R.resize_host(a, f)
        s = infer_wsi.ScaledSlide(infer_wsi.ArraySlide(a), base_mag, proc_mag)
        assert s.shape == full.shape
        assert np.array_equal(s.read_region((0, 0), (s.shape[1], s.shape[0])), full)
        assert np.array_equal(s.read_region((7, 3), (11, 9)), full[3:12, 7:18])
        assert np.array_equal(s.read_region((s.shape[1] - 4, s.shape[0] - 3), (10, 10)), full[-3:, -4:])    # cut at the edge like an array
    up = infer_wsi.ScaledSlide(infer_wsi.ArraySlide(a), 20, 40)
    assert np.array_equal(up.thumbnail(32), a[::16, ::16]) and np.array_equal(up.thumbnail(1), a)
    down = infer_wsi.ScaledSlide(infer_wsi.ArraySlide(a), 40, 20)
    assert np.array_equal(down.thumbnail(8), a[::16, ::16])


def test_manager_honours_base_mag(tmp_path):
    """`base_mag` 20 with `proc_mag` 40 hands the whole-slide run a slide at twice the file's size whose pixels are the cubic
    resize; a mapping gives the magnification per slide; without `base_mag` the slide is the plain array backend."""
    import json

    from PIL import Image

    from hover_net_amd import infer_manager as im, infer_wsi

    inp, masks = tmp_path / "slides", tmp_path / "masks"
    inp.mkdir()
    masks.mkdir()
    a = random_image(40, 50, 8)
    for name in ("s1", "s2"):
        np.save(inp / (name + ".npy"), a)
        Image.fromarray(np.full((5, 6), 255, np.uint8)).save(masks / (name + ".png"))
    seen = {}

    def wsi_fn(slide, mask):
        seen[len(seen)] = slide
        return None, {}

    mgr = im.WsiManager({"model_args": {"nr_types": None, "mode": "fast"}, "model_path": None}, wsi_fn=wsi_fn)
    args = {"input_dir": str(inp), "input_mask_dir": str(masks), "proc_mag": 40}
    st = mgr.process_wsi_list(dict(args, output_dir=str(tmp_path / "o1"), base_mag=20))
    assert st == {"s1": "done", "s2": "done"}
    slide = seen[0]
    assert isinstance(slide, infer_wsi.ScaledSlide) and tuple(slide.shape) == (80, 100, 3)
    assert np.array_equal(slide.read_region((0, 0), (100, 80)), R.resize_host(a, 2.0))
    assert json.load(open(str(tmp_path / "o1") + "/s1.json"))["mag"] == 40
    seen.clear()
    mgr.process_wsi_list(dict(args, output_dir=str(tmp_path / "o2"), base_mag={"s1": 40, "s2": 80}))
    assert type(seen[0]) is infer_wsi.ArraySlide and tuple(seen[0].shape) == (40, 50, 3)           # already at proc_mag: not wrapped
    assert isinstance(seen[1], infer_wsi.ScaledSlide) and tuple(seen[1].shape) == (20, 25, 3)      # 80 -> 40: the linear kind
    assert np.array_equal(seen[1].read_region((0, 0), (25, 20)), R.resize_host(a, 0.5))
    seen.clear()
    st = mgr.process_wsi_list(dict(args, output_dir=str(tmp_path / "o4"), base_mag={"s1": 20}))      # a mapping that lacks a slide
    assert st == {"s1": "done", "s2": "crash"} and len(seen) == 1 and not os.path.exists(str(tmp_path / "o4") + "/s2.json")
    seen.clear()
    mgr.process_wsi_list(dict(args, output_dir=str(tmp_path / "o3")))
    assert type(seen[0]) is infer_wsi.ArraySlide and tuple(seen[0].shape) == (40, 50, 3)
    assert type(im.open_slide(str(inp / "s1.npy"))) is infer_wsi.ArraySlide
    assert isinstance(im.open_slide(str(inp / "s1.npy"), 20, 40), infer_wsi.ScaledSlide)

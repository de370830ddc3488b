"""The host side of the device tissue mask: the workspace size is host arithmetic, `otsu_from_hist` is `otsu_threshold` from
the counters on, `select_valid_sat` keeps exactly the boxes `select_valid` keeps, and `simple_get_mask` without a device is the
chain of its parts."""
import numpy as np
import pytest
from scipy import ndimage

from hover_net_amd import infer_wsi, lib as L, tissue_mask as TM


def test_workspace_size_is_host_arithmetic():
    lib = L.lib()
    need = lib.hvn_tissue_mask_workspace_bytes(100, 130)                 # host arithmetic only: no device is touched
    assert need >= 100 * 130 * (2 * 4 + 3) and lib.hvn_tissue_mask_workspace_bytes(0, 130) == 0
    assert lib.hvn_tissue_mask_workspace_bytes(1 << 15, (1 << 15) + 1) == 0


@pytest.mark.parametrize("kind", ["random", "bimodal", "constant", "two-valued", "one pixel"])
def test_otsu_from_hist_is_otsu_threshold(kind):
    rng = np.random.default_rng(4)
    g = {"random": rng.integers(0, 256, (90, 70), dtype=np.uint8),
         "bimodal": np.concatenate([rng.normal(60, 10, 5000), rng.normal(190, 15, 8000)]).clip(0, 255).astype(np.uint8),
         "constant": np.full((20, 30), 181, np.uint8),
         "two-valued": np.where(rng.random((40, 45)) < 0.3, 40, 200).astype(np.uint8),
         "one pixel": np.array([[7]], np.uint8)}[kind]
    hist = np.bincount(g.reshape(-1), minlength=256)
    t = TM.otsu_from_hist(hist)
    assert isinstance(t, int) and t == TM.otsu_threshold(g)
    assert TM.otsu_from_hist(hist.astype(np.uint32)) == t and TM.otsu_from_hist(hist.astype(np.int32)) == t
    if kind == "constant":
        assert t == 0                                                    # no finite variance anywhere: the first bin
    if kind == "two-valued":
        assert t == 40                                                   # equal maxima for every t in [40, 200): the first wins


# -- select_valid_sat ---------------------------------------------------------------------------
def _same(info, mask, shape, has_output_info=True, sat=None):
    want = infer_wsi.select_valid(info, mask, shape, has_output_info)
    got = infer_wsi.select_valid_sat(info, mask, shape, has_output_info, sat=sat)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    return got


def _blob_mask(h, w, seed):
    field = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((h, w)), 6.0)
    return (field > np.quantile(field, 0.6)).astype(np.uint8)


def test_select_valid_sat_on_a_slide():
    shape = np.array([9000, 11000])
    mask = _blob_mask(282, 344, 1)
    _, patch = infer_wsi.get_chunk_patch_info(shape, np.array([10000, 10000]), np.array([270, 270]), np.array([80, 80]))
    assert patch.shape[0] == 15096
    got = _same(patch, mask, shape)
    assert 0 < got.shape[0] < patch.shape[0]
    sat = infer_wsi.mask_sat(mask)
    for tiles in infer_wsi.get_tile_info(shape, np.array([2048, 2048]), 128):
        got = _same(tiles, mask, shape, has_output_info=False, sat=sat)
        assert 0 < got.shape[0]
    n_kept = _same(patch, mask, shape).shape[0]
    assert _same(patch, np.zeros_like(mask), shape).shape[0] == 0
    assert _same(patch, np.ones_like(mask), shape).shape[0] > n_kept      # (patches past the slide's edge have an empty slice)
    assert _same(patch, mask * np.uint8(255), shape).shape[0] == n_kept
    assert _same(patch, mask.astype(bool), shape).shape[0] == n_kept


def test_select_valid_sat_edges():
    mask = np.zeros((10, 12), np.uint8)
    mask[9, 11] = 1
    mask[2, 3] = 255
    shape = np.array([100, 120])                                         # ratio 0.1
    boxes = np.array([
        [[90, 110], [200, 300]],      # past the bottom-right edge: clamped, holds (9, 11)
        [[100, 0], [150, 120]],       # starts at the mask's last row + 1: an empty slice
        [[0, 0], [100, 120]],         # the whole mask
        [[25, 35], [45, 45]],         # 2.5 -> 2, 3.5 -> 4, 4.5 -> 4: rows [2, 4) x columns [4, 4): empty
        [[25, 25], [45, 45]],         # rows [2, 4) x columns [2, 4): holds (2, 3)
        [[15, 25], [25, 45]],         # 1.5 -> 2, 2.5 -> 2: rows [2, 2): empty
        [[5, 25], [25, 35]],          # 0.5 -> 0: rows [0, 2): misses (2, 3)
        [[30, 30], [20, 40]],         # reversed rows: empty
        [[0, 0], [0, 0]],
    ], np.int64)
    kept = _same(boxes, mask, shape, has_output_info=False)
    assert [b.tolist() for b in kept] == [boxes[0].tolist(), boxes[2].tolist(), boxes[4].tolist()]
    info = np.stack([boxes - 5, boxes], axis=1)                          # [N, 2, 2, 2]: only the output box is tested
    assert np.array_equal(_same(info, mask, shape)[:, 1], kept)
    _same(boxes[:0], mask, shape, has_output_info=False)                 # no boxes
    _same(info[:0], mask, shape)


def test_select_valid_sat_negative_coordinate_takes_the_slice_semantics(monkeypatch):
    mask = np.zeros((10, 12), np.uint8)
    mask[8, 5] = 1
    shape = np.array([100, 120])
    boxes = np.array([[[-20, 0], [100, 120]],                            # rows [-2, 10) wrap to [8, 10): holds (8, 5)
                      [[-40, 0], [-30, 120]],                            # rows [-4, -3) = row 6: empty of tissue
                      [[0, 0], [50, 50]]], np.int64)
    calls = []
    real = infer_wsi.select_valid
    monkeypatch.setattr(infer_wsi, "select_valid", lambda *a: calls.append(1) or real(*a))
    got = infer_wsi.select_valid_sat(boxes, mask, shape, has_output_info=False)
    assert calls == [1] and np.array_equal(got, real(boxes, mask, shape, False)) and got.shape[0] == 1
    calls.clear()
    infer_wsi.select_valid_sat(boxes[2:], mask, shape, has_output_info=False)
    assert calls == []                                                   # without a negative coordinate the table decides


def test_wsi_inference_lists_use_the_same_boxes():
    """`tile_lists` (now through the summed-area table) against `select_valid` spelt out."""
    class Net:
        mode = "original"

        def parameters(self):
            import torch

            return iter([torch.zeros(1)])

    wsi = infer_wsi.WsiInference(Net(), nr_types=5, tile_shape=512, ambiguous_size=64)
    assert wsi.device_mask is False
    shape, mask = np.array([2100, 2500]), _blob_mask(66, 79, 2)
    lists = wsi.tile_lists(shape, mask)
    for got, t in zip(lists, infer_wsi.get_tile_info(shape, wsi.tile_shape, 64)):
        assert np.array_equal(got, infer_wsi.select_valid(t, mask, shape, has_output_info=False))
    other = np.ones_like(mask)                                           # another mask object: the cached table is not reused
    for got, t in zip(wsi.tile_lists(shape, other), infer_wsi.get_tile_info(shape, wsi.tile_shape, 64)):
        assert np.array_equal(got, t)


def test_simple_get_mask_without_a_device_is_the_chain_of_its_parts():
    from hover_net_amd.synth import synth_thumbnail

    thumb, frac = synth_thumbnail(300, 340, seed=6)
    assert 0.2 < frac < 0.6
    gray = TM.rgb_to_gray(thumb)
    m = ~(gray > TM.otsu_threshold(gray))
    m = TM.remove_small_objects(m, 256, 2)
    m = TM.remove_small_holes(m, 16384)
    m = ndimage.binary_dilation(m, structure=TM.disk(16)).astype(np.uint8)
    assert np.array_equal(TM.simple_get_mask(thumb), m) and np.array_equal(TM.simple_get_mask(thumb, device=None), m)
    assert 0 < int(m.sum()) < m.size


def test_odd_lists_and_edited_masks():
    mask = np.zeros((10, 12), np.uint8)
    mask[2, 3] = 1
    shape = np.array([100, 120])
    boxes = np.array([[[20, 30], [30, 40]], [[50, 50], [60, 60]]], np.int64)
    with pytest.raises(Exception):                                       # a plain box list read as (input, output) pairs fails
        infer_wsi.select_valid(boxes, mask, shape, True)                 # in the loop, and so it does here: the fallback
    with pytest.raises(Exception):
        infer_wsi.select_valid_sat(boxes, mask, shape, True)

    class Net:
        mode = "original"

        def parameters(self):
            import torch

            return iter([torch.zeros(1)])

    with pytest.raises(ValueError, match="device_mask"):
        infer_wsi.WsiInference(Net(), nr_types=5, device_mask=True)
    wsi = infer_wsi.WsiInference(Net(), nr_types=5, tile_shape=512, ambiguous_size=64)
    shape = np.array([2100, 2500])
    mask = np.zeros((66, 79), np.uint8)
    assert wsi.tile_lists(shape, mask)[0].shape[0] == 0
    mask[:] = 1                                                          # the same object, edited in place
    grid = infer_wsi.get_tile_info(shape, wsi.tile_shape, 64)[0]
    assert np.array_equal(wsi.tile_lists(shape, mask)[0], grid)

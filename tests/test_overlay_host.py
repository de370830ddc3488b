"""CPU: the host side of the device overlay route (viz.flatten_instances, the `device=` keyword of visualize_instances_dict and the
argument checks that come before any GPU call)."""
import random

import numpy as np
import pytest
import torch

from hover_net_amd import viz

DICT = {
    9: {"contour": np.array([[2, 2], [2, 10], [12, 10], [12, 2]]), "centroid": [7.9, 6.2], "type": 1},
    3: {"contour": np.array([[5, 5]]), "centroid": np.array([5.0, 5.0]), "type": 0},              # one point
    4: {"contour": [[1, 1], [8, 3]], "centroid": (-0.5, 3.99), "type": 1},                        # two points, a list
    7: {"contour": None, "centroid": [14.2, 1.0], "type": 0},                                     # no contour: only the dot
    1: {"contour": np.array([[[0, 0]], [[19, 0]], [[19, 19]]], np.int32), "centroid": [12.7, 6.1], "type": 2},   # cv2's [K,1,2] form
}
COLOURS = [(1, 2, 3), (4, 5, 6), [7, 8, 9], (10, 11, 12), (13, 14, 15)]


def test_flatten_round_trips_in_dict_order():
    pts, offs, rgba, centres = viz.flatten_instances(DICT, COLOURS)
    assert pts.dtype == np.int32 and offs.dtype == np.int64 and rgba.dtype == np.uint8 and centres.dtype == np.int32
    assert offs.tolist() == [0, 4, 5, 7, 7, 10] and pts.shape == (10, 2) and pts.flags.c_contiguous
    assert rgba[:, 3].tolist() == [1] * 5
    back = viz.unflatten_instances(pts, offs, rgba, centres)
    assert len(back) == len(DICT)
    for (contour, colour, centre), info, want in zip(back, DICT.values(), COLOURS):
        ref = np.zeros((0, 2), np.int64) if info["contour"] is None else np.asarray(info["contour"], np.int64).reshape(-1, 2)
        assert contour.tolist() == ref.tolist() and colour == tuple(want)
        assert centre == (int(info["centroid"][0]), int(info["centroid"][1]))                     # int(): -0.5 -> 0, 3.99 -> 3
    assert back[2][2] == (0, 3) and back[3][0].shape == (0, 2)


def test_flatten_empty_dict_and_bad_vertices():
    pts, offs, rgba, centres = viz.flatten_instances({}, [])
    assert pts.shape == (0, 2) and offs.tolist() == [0] and rgba.shape == (0, 4) and centres.shape == (0, 2)
    with pytest.raises(ValueError, match="int32"):
        viz.flatten_instances({1: {"contour": np.array([[0, 0], [2 ** 31, 0]]), "centroid": [0, 0]}}, [(1, 1, 1)])
    far = viz.flatten_instances({1: {"contour": None, "centroid": [1e30, -1e30]}}, [(1, 1, 1)])[3]
    assert far.tolist() == [[2 ** 31 - 1, -2 ** 31]]


@pytest.mark.parametrize("typed", [True, False])
def test_device_none_is_the_host_writer(typed):
    img = np.random.default_rng(1).integers(0, 256, (20, 20, 3), dtype=np.uint8)
    tc = {0: ("a", (1, 2, 3)), 1: ("b", (200, 100, 0))} if typed else None                      # type 2 falls back to a random colour
    random.seed(5)
    want = viz.visualize_instances_dict(img, DICT, True, tc, 3)
    state = random.getstate()
    random.seed(5)
    got = viz.visualize_instances_dict(img, DICT, True, tc, 3, device=None)
    assert np.array_equal(got, want) and random.getstate() == state
    assert (want != img).any() and got is not img
    with pytest.raises(TypeError):
        viz.visualize_instances_dict(img, DICT, True, tc, 3, "cuda")                             # `device` is keyword only


def test_device_route_checks_its_arguments_before_any_gpu_call(monkeypatch):
    from hover_net_amd import lib as L

    def no_gpu(*a, **kw):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "lib", no_gpu)
    monkeypatch.setattr(L, "require_gpu", no_gpu)
    img = np.zeros((20, 20, 3), np.uint8)
    for thickness in (0, 8, -1, 2.5):
        with pytest.raises(ValueError, match="thickness"):
            viz.visualize_instances_dict(img, DICT, line_thickness=thickness, device="cuda")
    for bad in (img.astype(np.float32), img[..., 0], np.zeros((20, 20, 4), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            viz.visualize_instances_dict(bad, DICT, device="cuda")
    images = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    pts, offs = torch.zeros((0, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    rgba = torch.zeros((1, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="thickness"):
        viz.draw_overlay_device(images, pts, offs, rgba, thickness=8)
    with pytest.raises(ValueError, match="dot_radius"):
        viz.draw_overlay_device(images, pts, offs, rgba, dot_radius=16)
    with pytest.raises(ValueError, match="images"):
        viz.draw_overlay_device(images.float(), pts, offs, rgba)
    with pytest.raises(ValueError, match="images"):
        viz.draw_overlay_device(images, pts, offs, rgba)                                          # a host tensor

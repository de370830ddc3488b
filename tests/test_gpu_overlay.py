"""-m gpu: the device overlay writer (csrc/hvn_overlay.hip) against the host writer `viz.visualize_instances_dict`, from the C ABI
(`viz.draw_overlay_device`) up through `overlay_from_records`, `visualize_instances_dict(device=)` and `InferManager`.  Integer
work: every comparison is np.array_equal on the whole overlay."""
import ctypes
import glob
import os
import random

import numpy as np
import pytest
import torch

from golden_util import golden_dicts
from hover_net_amd import viz

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "proc_*.npz")))
IDS = [os.path.basename(p)[5:-4] for p in CASES]
PALETTE = {t: (str(t), c) for t, c in enumerate([(1, 2, 3), (250, 128, 0), (0, 200, 90), (30, 60, 255), (255, 255, 255), (90, 0, 170)])}


def _image(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _host(images, dicts, draw_dot, thickness):
    return np.stack([viz.visualize_instances_dict(img, d, draw_dot, PALETTE, thickness) for img, d in zip(images, dicts)])


def _flat_batch(dicts, slots=None, pad_front=0):
    """Typed dicts -> one (pts, offs, rgba, centres) for the batch: `slots` per image, the unused ones empty with draw flag 0
    (`pad_front` of them before the image's entries)."""
    slots = slots or max(1, max(len(d) for d in dicts) + pad_front)
    pts, offs, rgba, centres = [], [0], np.zeros((len(dicts) * slots, 4), np.uint8), np.zeros((len(dicts) * slots, 2), np.int32)
    for i, d in enumerate(dicts):
        p, o, c, ctr = viz.flatten_instances(d, [PALETTE[v["type"]][1] for v in d.values()])
        cnt = np.concatenate([np.zeros(pad_front, np.int64), np.diff(o), np.zeros(slots - pad_front - len(d), np.int64)])
        offs += (offs[-1] + np.cumsum(cnt)).tolist()
        pts.append(p)
        rgba[i * slots + pad_front:i * slots + pad_front + len(d)] = c
        centres[i * slots + pad_front:i * slots + pad_front + len(d)] = ctr
    return np.concatenate(pts, 0).astype(np.int32).reshape(-1, 2), np.asarray(offs, np.int64), rgba, centres


def _device(images, flat, draw_dot, thickness, **kw):
    pts, offs, rgba, centres = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in flat)
    out, status = viz.draw_overlay_device(torch.from_numpy(np.ascontiguousarray(images)).to("cuda"), pts, offs, rgba, centres if draw_dot else None,
                                          thickness=thickness, return_status=True, **kw)
    return out.cpu().numpy(), status.cpu().tolist()


def _check(images, dicts, draw_dot=True, thickness=2, **kw):
    """Device == host for a batch of typed dicts, through the flat arrays; -> the overlays."""
    images = np.stack(images)
    want = _host(images, dicts, draw_dot, thickness)
    got, status = _device(images, _flat_batch(dicts, **kw), draw_dot, thickness)
    assert status == [0, -1, 0, 0]
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    return got


def _poly(pts, t, centroid=None):
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    return {"contour": pts, "centroid": pts.mean(0) if centroid is None else np.asarray(centroid, np.float64), "type": t}


# -- 1: one rectangle, every thickness parity; the host test's own two cases ----------------------
@pytest.mark.parametrize("thickness", [1, 2, 3, 4])
def test_rectangle_and_dot(thickness):
    d = {7: _poly([[2, 2], [2, 10], [12, 10], [12, 2]], 1, [7.9, 6.2])}
    out = _check([_image(24, 20)], [d], True, thickness)
    assert out[0, 2, 2].tolist() == [250, 128, 0] and out[0, 6, 7].tolist() == [255, 0, 0]
    _check([_image(24, 20)], [d], False, thickness)


def test_the_host_tests_two_cases():
    img = np.zeros((20, 20, 3), np.uint8)
    d = {7: {"contour": np.array([[2, 2], [2, 10], [12, 10], [12, 2]]), "centroid": [7.0, 6.0], "type": 1}}
    want = viz.visualize_instances_dict(img, d, draw_dot=False, type_colour={1: ("a", (1, 2, 3))}, line_thickness=2)
    got = viz.visualize_instances_dict(img, d, draw_dot=False, type_colour={1: ("a", (1, 2, 3))}, line_thickness=2, device="cuda")
    assert np.array_equal(got, want) and got[3, 3].tolist() == [1, 2, 3] and img.sum() == 0
    d = {1: {"contour": np.array([[-3, 5], [25, 5]]), "centroid": [0.0, 0.0]}}            # x = -3 .. 25 on a 20-wide image, random colour
    random.seed(11)
    want = viz.visualize_instances_dict(img, d, draw_dot=True)
    state = random.getstate()
    random.seed(11)
    got = viz.visualize_instances_dict(img, d, draw_dot=True, device="cuda")
    assert np.array_equal(got, want) and got[5, 10].any() and got[0, 0].tolist() == [255, 0, 0]
    assert random.getstate() == state                                                   # python's random stream consumed identically
    assert np.array_equal(viz.visualize_instances_dict(img, {}, device="cuda"), img)


# -- 2: clipping ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(53, 37), (37, 53)])
@pytest.mark.parametrize("thickness", [1, 2, 5])
def test_clipping_on_all_four_sides(hw, thickness):
    h, w = hw
    d = {1: _poly([[-4, -4], [w + 3, -2], [w + 2, h + 5], [-6, h + 1]], 0, [0, 0]),     # a frame just outside: its stamps reach in
         2: _poly([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], 2, [w - 1, h - 1]),
         3: _poly([[-100000, 5], [100000, 7]], 3, [w // 2, -3]),
         4: _poly([[5, 100000], [9, -100000]], 4, [-3, h // 2]),
         5: _poly([[w + 50, 3]], 5, [w + 2, h + 2]),                                    # one point outside, dot touching the corner
         6: _poly([[w - 1, h - 1]], 5, [w + 40, 7])}
    _check([_image(h, w, 3)], [d], True, thickness)


def test_far_vertices_cost_nothing():
    """A vertex at +-2^30 cannot be rasterised by the host (2^31 steps); on an axis-parallel segment every step is exact, so the
    overlay equals that of the same line cut short just outside the image."""
    h, w = 37, 53
    far = {1: _poly([[-2 ** 30, 7], [2 ** 30, 7]], 1, [3, 3]), 2: _poly([[11, 2 ** 30], [11, -2 ** 30]], 2, [40, 30]),
           3: _poly([[2 ** 30, 2 ** 30], [2 ** 30 + 5, 2 ** 30 - 9], [2 ** 30 - 2, -2 ** 30]], 3, [2 ** 31 - 1, -2 ** 31])}
    near = {1: _poly([[-60, 7], [w + 60, 7]], 1, [3, 3]), 2: _poly([[11, h + 60], [11, -60]], 2, [40, 30])}
    img = _image(h, w, 4)
    got, status = _device(img[None], _flat_batch([far]), True, 3)
    assert status == [0, -1, 0, 0]
    assert np.array_equal(got, _host(img[None], [near], True, 3))


# -- 3: drawing order -----------------------------------------------------------------------------
def test_overlap_order_and_a_switched_off_slot():
    a = _poly([[5, 5], [30, 6], [28, 30], [6, 27]], 0, [18, 5])                          # its dot sits on its own contour
    off = _poly([[0, 0], [39, 39], [39, 0]], 4, [20, 20])
    b = _poly([[18, 4], [22, 32], [36, 20]], 1, [28, 6])                                # its contour runs over a's dot, its dot over a's contour
    c = _poly([[2, 17], [38, 19], [20, 36]], 2, [21, 19])
    img = _image(40, 40, 5)
    want = _host(img[None], [{1: a, 3: b, 4: c}], True, 2)
    flat = _flat_batch([{1: a, 2: off, 3: b, 4: c}])
    flat[2][1, 3] = 0                                                                   # slot 1 draws nothing, neither contour nor dot
    got, status = _device(img[None], flat, True, 2)
    assert status == [0, -1, 0, 0] and np.array_equal(got, want)

    def mask(d, contour=True, dot=True):
        m = np.zeros((40, 40, 3), np.uint8)
        if contour:
            viz.draw_contour(m, d["contour"], (1, 1, 1), 2)
        if dot:
            viz.draw_centroid_dot(m, d["centroid"])
        return m.any(-1)

    later = mask(b, dot=False) & mask(a, contour=False) & ~mask(b, contour=False) & ~mask(c)
    assert later.any() and (got[0][later] == PALETTE[1][1]).all()                       # slot j+1's contour over slot j's dot
    own = mask(a, dot=False) & mask(a, contour=False) & ~mask(b) & ~mask(c)
    assert own.any() and (got[0][own] == (255, 0, 0)).all()                             # a slot's dot over its own contour
    gone = mask(off) & ~mask(a) & ~mask(b) & ~mask(c)
    assert gone.any() and np.array_equal(got[0][gone], img[gone])                       # the switched-off slot left the image alone


# -- 4: general slopes ----------------------------------------------------------------------------
@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_random_polygons(thickness):
    h, w = 61, 97
    rng = np.random.default_rng(17)
    d = {}
    for k in range(200):
        nv = int(rng.integers(1, 9))
        if k % 3 == 0:                                                                  # short segments around a random origin
            o = rng.integers([-30, -30], [w + 30, h + 30])
            v = o + rng.integers(-int(rng.integers(1, 20)), int(rng.integers(1, 20)) + 1, (nv, 2))
        else:                                                                           # lengths up to ~200, all octants
            v = rng.integers([-30, -30], [w + 31, h + 31], (nv, 2))
        d[k + 1] = _poly(v, int(rng.integers(0, 6)), rng.uniform([-5, -5], [w + 5, h + 5]))
    # minor axis on .5 at the middle step (the host gives y = 1, 0, 1), and lengths at which i / n * n is inexact
    for k, v in enumerate([[[40, 20], [42, 21]], [[50, 20], [52, 19]], [[60, 20], [58, 21]], [[3, 3], [52, 20]], [[90, 50], [41, 57]],
                           [[10, 58], [17, 9]], [[-20, 10], [29, 13], [78, 9], [127, 12]], [[0, 60], [93, 0]], [[96, 60], [-11, 5]]]):
        d[1000 + k] = _poly(v, k % 6, [-50, -50])
    lens = {int(abs(c[i] - c[(i + 1) % len(c)]).max()) for c in (v["contour"] for v in d.values()) for i in range(len(c))}
    assert {1, 2, 49} <= lens and max(lens) >= 100
    assert viz._segment_pixels(np.array([0, 0]), np.array([2, 1]))[1].tolist() == [1, 1]
    assert viz._segment_pixels(np.array([0, 0]), np.array([2, -1]))[1].tolist() == [1, 0]
    assert viz._segment_pixels(np.array([0, 0]), np.array([-2, 1]))[1].tolist() == [-1, 1]
    _check([_image(h, w, 6)], [d], True, thickness)


# -- 5: batches, empty slots, nothing to draw -----------------------------------------------------
def _blobs(rng, count, h, w):
    d = {}
    for k in range(count):
        c = rng.uniform([0, 0], [w, h])
        ang = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(3, 12))))
        r = rng.uniform(1, 7, ang.size)
        d[k + 1] = _poly(np.stack([c[0] + r * np.cos(ang), c[1] + r * np.sin(ang)], 1).astype(np.int64), int(rng.integers(0, 6)), c)
    return d


@pytest.mark.parametrize("pad_front", [0, 5])
def test_batch_with_empty_slots(pad_front):
    rng = np.random.default_rng(23)
    dicts = [{}, _blobs(rng, 1, 48, 64), _blobs(rng, 70, 48, 64)]
    images = [_image(48, 64, 30 + i) for i in range(3)]
    out = _check(images, dicts, True, 2, pad_front=pad_front)
    assert np.array_equal(out[0], images[0])                                            # an image without instances is copied
    _check(images, dicts, False, 3, slots=129, pad_front=pad_front)


def test_no_points_at_all():
    images = np.stack([_image(48, 64, 40 + i) for i in range(3)])
    got, status = _device(images, _flat_batch([{}, {}, {}], slots=4), True, 2)
    assert status == [0, -1, 0, 0] and np.array_equal(got, images)
    dots = [{1: {"contour": None, "centroid": [5.5, 7.9], "type": 0}}, {}, {2: {"contour": np.zeros((0, 2)), "centroid": [63, 47], "type": 1}}]
    got, status = _device(images, _flat_batch(dots), True, 2)                         # no contour still draws the dot, as on the host
    assert np.array_equal(got, _host(images, dots, True, 2)) and got[0, 7, 5].tolist() == [255, 0, 0]


def test_300_instances_across_waves_and_workgroups():
    rng = np.random.default_rng(29)
    _check([_image(200, 200, 7)], [_blobs(rng, 300, 200, 200)], True, 2)
    many = {k + 1: _poly(rng.integers(-20, 220, (150, 2)), k, [100, 100]) for k in range(3)}   # more points than one round of a wave
    _check([_image(200, 200, 8)], [many], False, 1)


# -- 6: the reference's process() output ----------------------------------------------------------
@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_goldens(path):
    from hover_net_amd import post_proc as PP

    z = np.load(path)
    nt = None if int(z["nr_types"]) < 0 else int(z["nr_types"])
    n, h, w = z["inst"].shape
    images = np.stack([_image(h, w, 50 + i) for i in range(n)])
    type_colour = PALETTE if nt is not None else {None: ("no label", (9, 200, 30))}
    table = [PALETTE[t][1] for t in range(nt)] if nt is not None else [(9, 200, 30)]
    pred = torch.from_numpy(np.ascontiguousarray(z["pred"], np.float32)).to("cuda")
    inst, rec, _, pts, offs, status = PP.process_batch_device(pred, nt, True, return_contours=True)
    assert status.cpu().tolist() == [0, 0, -1, 0]
    got = viz.overlay_from_records(torch.from_numpy(images).to("cuda"), rec, pts, offs, table, draw_dot=True)
    assert got.is_cuda and got.dtype == torch.uint8
    rec_h = rec.cpu().numpy().view(PP._REC_DTYPE).reshape(n, -1)
    flat = PP.split_contours(pts.cpu().numpy(), offs.cpu().numpy(), n, rec.shape[1])
    drawn = 0
    for i, gold in enumerate(golden_dicts(z)):
        info = PP.records_to_dict(rec_h[i], nt, contours_flat=flat[i])
        assert list(info) == list(gold)
        drawn += len(info)
        want = viz.visualize_instances_dict(images[i], info, draw_dot=True, type_colour=type_colour)
        assert np.array_equal(got[i].cpu().numpy(), want)
        assert np.array_equal(viz.visualize_instances_dict(images[i], gold, draw_dot=True, type_colour=type_colour, device="cuda"), want)
        want = viz.visualize_instances_dict(images[i], gold, draw_dot=False, type_colour=type_colour, line_thickness=3)
        assert np.array_equal(viz.visualize_instances_dict(images[i], gold, False, type_colour, 3, device="cuda"), want)
    assert drawn > 50
    plain = viz.overlay_from_records(torch.from_numpy(images).to("cuda"), rec, pts, offs, table, thickness=1).cpu().numpy()
    assert np.array_equal(plain[0], viz.visualize_instances_dict(images[0], golden_dicts(z)[0], False, type_colour, 1))


# -- 7: in place, bad slots, refusals -------------------------------------------------------------
def test_in_place_gives_the_same_bytes():
    rng = np.random.default_rng(31)
    dicts = [_blobs(rng, 20, 37, 53), _blobs(rng, 9, 37, 53)]
    images = np.stack([_image(37, 53, 60), _image(37, 53, 61)])
    want = _host(images, dicts, True, 2)
    pts, offs, rgba, centres = (torch.from_numpy(a).to("cuda") for a in _flat_batch(dicts))
    buf = torch.from_numpy(images).to("cuda")
    out = viz.draw_overlay_device(buf, pts, offs, rgba, centres, out=buf)
    assert out.data_ptr() == buf.data_ptr() and np.array_equal(buf.cpu().numpy(), want)
    other = torch.empty_like(buf)
    assert viz.draw_overlay_device(torch.from_numpy(images).to("cuda"), pts, offs, rgba, centres, out=other) is other
    assert np.array_equal(other.cpu().numpy(), want)
    green = viz.draw_overlay_device(torch.from_numpy(images).to("cuda"), pts, offs, rgba, centres, dot_radius=5, dot_colour=(0, 255, 0)).cpu().numpy()
    ref = images.copy()
    for i, d in enumerate(dicts):
        for v in d.values():
            viz.draw_contour(ref[i], v["contour"], PALETTE[v["type"]][1], 2)
            viz.draw_centroid_dot(ref[i], v["centroid"], 5, (0, 255, 0))
    assert np.array_equal(green, ref)


def test_a_bad_offs_range_is_counted_and_draws_nothing():
    rng = np.random.default_rng(37)
    d = _blobs(rng, 6, 40, 40)
    img = _image(40, 40, 62)
    pts, offs, rgba, centres = _flat_batch([d])
    for bad, first in ((2, 2), (5, 5)):
        o = offs.copy()
        if bad == 2:
            o[2], o[3] = offs[3], offs[2]                    # slot 2 reversed; slots 1 and 3 now overlap it and stay valid
        else:
            o[6] = len(pts) + 1                              # the last slot leaves the points
        keep = [k for k in range(6) if not (o[k] > o[k + 1] or o[k + 1] > len(pts))]
        want = img.copy()
        for k in keep:
            viz.draw_contour(want, pts[o[k]:o[k + 1]], rgba[k, :3], 2)
            viz.draw_centroid_dot(want, centres[k])
        got, status = _device(img[None], (pts, o, rgba, centres), True, 2)
        assert status == [6 - len(keep), first, 0, 0] and len(keep) < 6
        assert np.array_equal(got[0], want)


def test_refusals_at_the_c_abi():
    from hover_net_amd import lib as L

    n, h, w = 1, 16, 16
    img = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    pts = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    rgba = torch.ones((1, 4), dtype=torch.uint8, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    need = L.lib().hvn_overlay_workspace_bytes(n, h, w)
    assert need >= n * h * w * 4 and L.lib().hvn_overlay_workspace_bytes(0, h, w) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dot = (ctypes.c_uint8 * 3)(255, 0, 0)

    def call(thickness=2, radius=3, ws_bytes=need, slots=1):
        return L.lib().hvn_draw_overlay(img.data_ptr(), img.data_ptr(), n, h, w, pts.data_ptr(), 4, offs.data_ptr(), slots, rgba.data_ptr(), None,
                                        thickness, radius, dot, status.data_ptr(), ws.data_ptr(), ws_bytes, None)

    assert call() == 0
    assert call(ws_bytes=n * h * w * 4 - 1) == -4                                        # HVN_E_SIZE
    assert call(thickness=0) == -4 and call(thickness=8) == -4 and call(radius=-1) == -4 and call(radius=16) == -4
    assert call(slots=2 ** 30) == -4                                                    # 2 * slot + 2 would leave int32
    torch.cuda.synchronize()
    assert img.sum().item() == 4 * 3                                                    # the one accepted call stamped (0, 0) 2 x 2


# -- 8: the tile manager --------------------------------------------------------------------------
def test_infer_manager_device_overlay(tmp_path):
    from PIL import Image

    from hover_net_amd import infer_manager, net_desc
    from hover_net_amd.synth import synth_state_dict, synth_tiles

    net = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    net.load_state_dict(synth_state_dict("original", 5, seed=81), strict=True)
    net = net.to("cuda").eval()
    inp = tmp_path / "in"
    inp.mkdir()
    shapes = {"a": (120, 95), "b": (97, 141)}
    for i, (name, (h, w)) in enumerate(shapes.items()):
        np.save(inp / (name + ".npy"), synth_tiles(1, 160, seed=82 + i)[0][:h, :w])
    mgr = infer_manager.InferManager({"model_args": {"nr_types": 5, "mode": "original"}, "model_path": None}, model=net)
    args = {"input_dir": str(inp), "batch_size": 8, "draw_dot": True, "patch_input_shape": 270, "patch_output_shape": 80}
    assert mgr.process_file_list(dict(args, output_dir=str(tmp_path / "host"))) == ["a", "b"]
    assert mgr.process_file_list(dict(args, output_dir=str(tmp_path / "dev"), device_overlay=True)) == ["a", "b"]
    drawn = 0
    for name, (h, w) in shapes.items():
        want = np.asarray(Image.open(tmp_path / "host" / "overlay" / (name + ".png")))
        got = np.asarray(Image.open(tmp_path / "dev" / "overlay" / (name + ".png")))
        assert want.shape == (h, w, 3) and np.array_equal(got, want)
        drawn += int((want != np.load(inp / (name + ".npy"))).any(-1).sum())
    assert drawn > 0                                                                    # the comparison was not of two plain copies

"""CPU: hover_net_amd/density.py's host path against the all-pairs oracle tests/density_ref.py on every case the GPU tests run, the
derived forms (`of_info`, `resolve`, `total`, `fraction`, `per_area`, `hot_spots`), the Python refusals and the C refusals of
HVN_OP_NBR_DENSITY, which the library decides before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import density_ref as R
from hover_net_amd import density as DN
from hover_net_amd import neighbours as NB


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_equals_oracle(name):
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = DN.density_host(*args)
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    R.assert_same(DN.density(*args, device=None), want, name)


def test_host_path_does_not_depend_on_the_round_size(monkeypatch):
    monkeypatch.setattr(DN, "_PAIRS", 700)           # hundreds of rounds, and single points whose window is worked off in row bands
    for name in ("lattice", "fine", "crowded", "inexact_step", "sixteen_types"):
        args, want = R.case(name)
        R.assert_same(DN.density_host(*args), want, name)


def test_host_path_in_reversed_order():
    for name in ("lattice", "ragged", "nine_types"):
        (xy, types, r, raster, t), want = R.case(name)
        R.assert_same(DN.density_host(np.ascontiguousarray(xy[::-1]), np.ascontiguousarray(types[::-1]), r, raster, t), want, name)


def test_the_window_holds_where_nodes_round_to_one_position():
    """An origin of 2^60 with a step of 1: every node position rounds to ox itself (the spacing of float64 there is 256), so all W nodes
    are the same point and each counts whatever lies within r of it.  A window computed by dividing by the step would miss them."""
    ox = 2.0 ** 60
    xy = np.array([[ox, 0.0], [ox + 256.0, 0.0], [ox - 128.0, 0.0]])
    raster = (ox, 0.0, 1.0, 40, 1)
    assert (DN.nodes(DN.Raster(*raster))[0] == ox).all()
    want = R.density(xy, None, 200.0, raster, 1)
    assert want.reshape(-1).tolist() == [2] * 40
    R.assert_same(DN.density_host(xy, None, 200.0, raster), want)


def test_d2_and_r2_are_those_of_neighbours():
    (xy, _types, r, raster, _t), want = R.case("lattice")
    px, py = DN.nodes(DN.Raster(*raster))
    d2 = NB.d2_of(px[5], py[5], xy[:, 0], xy[:, 1])               # dx = xj - px: the node stands where neighbours.py has point i
    assert NB.r2_of(r) == 25.0 and int((d2 <= 25.0).sum()) == int(want[:, 5, 5].sum()) == 81 and int((d2 == 25.0).sum()) == 12


# -- of_info, resolve, the helpers ---------------------------------------------------------------------------
def _hand_dict(typed=True):
    """Labels neither contiguous nor sorted.  On the step-4 raster of a 10 x 14 image the nodes are at 1.5, 5.5, 9.5, 13.5 (x) and 1.5,
    5.5, 9.5 (y).  40 sits on node (u 1, v 1); 7 is at exactly 2.5 from it; 12 is within 2.5 of node (u 3, v 2); 3 lies in the middle of four nodes, sqrt(8) from each."""
    pts = {40: (5.5, 5.5, 1), 7: (7.0, 7.5, 0), 12: (13.0, 8.0, 1), 3: (3.5, 3.5, 2)}
    return {lab: {"bbox": np.zeros((2, 2), np.int64), "centroid": np.array([x, y]), "contour": None, "type_prob": None,
                  "type": t if typed else None} for lab, (x, y, t) in pts.items()}


def test_of_info_hand_made_dict():
    dm = DN.of_info(_hand_dict(), (10, 14), 2.5, 4, 3)
    assert isinstance(dm, DN.DensityMap) and dm.origin == (1.5, 1.5) and dm.step == 4 and dm.radius == 2.5
    assert dm.count.dtype == np.int32 and dm.count.shape == (3, 3, 4)             # H = ceil(10 / 4), W = ceil(14 / 4)
    want = np.zeros((3, 3, 4), np.int32)
    want[1, 1, 1] = 1                                                             # 40 on its node
    want[0, 1, 1] = 1                                                             # 7 at d2 = 2.25 + 4 = 6.25 = r2 exactly
    want[0, 2, 1] = 1                                                             # 7 from node (5.5, 9.5): 2.25 + 4 again
    want[1, 2, 3] = 1                                                             # 12 from node (13.5, 9.5): 0.25 + 2.25
    assert (dm.count == want).all()
    assert (DN.of_info(_hand_dict(), (10, 14), 2.5, 4, 5).count == np.concatenate([want, np.zeros((2, 3, 4), np.int32)])).all()
    one = DN.of_info(_hand_dict(), (10, 14), 2.5, 1, 3)                           # step 1: origin 0, one node per pixel
    assert one.origin == (0.0, 0.0) and one.count.shape == (3, 10, 14) and one.count[1, 5:7, 5:7].tolist() == [[1, 1], [1, 1]] and one.count[1, 0, 0] == 0


def test_of_info_untyped_and_empty():
    dm = DN.of_info(_hand_dict(typed=False), (10, 14), 2.5, 4, None)
    assert dm.count.shape == (1, 3, 4) and dm.count[0].tolist() == [[0, 0, 0, 0], [0, 2, 0, 0], [0, 1, 0, 1]]
    empty = DN.of_info({}, (10, 14), 2.5, 4, 5)
    assert empty.count.shape == (5, 3, 4) and empty.count.dtype == np.int32 and not empty.count.any() and empty.origin == (1.5, 1.5)
    assert DN.of_info({}, (9, 9), 2.5, 3, None).count.shape == (1, 3, 3)
    with pytest.raises(ValueError):
        DN.of_info(_hand_dict(typed=False), (10, 14), 2.5, 4, 3)                  # nr_types given, entries untyped
    with pytest.raises(ValueError):
        DN.of_info(_hand_dict(), (10, 14), 2.5, 4, 2)                             # a type outside [0, 2)
    with pytest.raises(ValueError):
        DN.of_info(_hand_dict(), (10, 14), 2.5, 0, 3)
    with pytest.raises(ValueError):
        DN.of_info({}, (20000, 14), 2.5, 1, 3)                                    # H above 16384, also for an empty dict


def test_of_info_equals_density_on_a_case_and_save_round_trips(tmp_path):
    (xy, types, r, _raster, t), _ = R.case("ragged")
    labels = [3 * i + 5 for i in range(xy.shape[0])][::-1]
    info = {lab: {"centroid": xy[i], "type": int(types[i])} for i, lab in enumerate(labels)}
    dm = DN.of_info(info, (190, 370), r, 7, t)
    assert dm.count.shape == (t, 28, 53)
    R.assert_same(dm.count, R.density(xy, types, r, (3.0, 3.0, 7.0, 53, 28), t), "of_info")
    DN.save(str(tmp_path / "a.npz"), dm)
    with np.load(tmp_path / "a.npz") as z:
        assert sorted(z.files) == ["count", "origin", "radius", "step"]
        assert (z["count"] == dm.count).all() and z["count"].dtype == np.int32 and z["origin"].tolist() == [3.0, 3.0] and int(z["step"]) == 7 and float(z["radius"]) == r


def test_total_fraction_per_area():
    dm = DN.of_info(_hand_dict(), (10, 14), 2.5, 4, 3)
    tot = DN.total(dm)
    assert tot.dtype == np.int64 and tot.tolist() == [[0, 0, 0, 0], [0, 2, 0, 0], [0, 1, 0, 1]] and (DN.total(dm.count) == tot).all()
    f = DN.fraction(dm, 1)
    assert f.dtype == np.float64 and f[1, 1] == 0.5 and f[2, 1] == 0.0 and f[2, 3] == 1.0
    assert np.isnan(f[tot == 0]).all() and not np.isnan(f[tot > 0]).any()         # NaN exactly where the total is 0
    pa = DN.per_area(dm, 0.25)
    r_mm = 2.5 * 0.25 / 1000.0
    area = np.pi * r_mm * r_mm
    assert pa.shape == dm.count.shape and pa[1, 1, 1] == 1.0 / area and pa[0, 0, 0] == 0.0
    with pytest.raises(ValueError):
        DN.per_area(dm, 0.0)


def test_hot_spots_order_and_suppression():
    plane = np.zeros((6, 8), np.int32)
    plane[2, 3] = 9
    plane[2, 4] = 9                 # a tie with (2, 3): (v, u) order puts (2, 3) first; one node away
    plane[1, 3] = 9                 # a tie that comes FIRST in (v, u) order
    plane[5, 7] = 4
    plane[2, 6] = 7                 # 3 nodes from (1, 3) along u, 1 along v: d2 = 10
    plane[0, 0] = 1
    assert DN.hot_spots(plane, 10, 0).tolist() == [[1, 3, 9], [2, 3, 9], [2, 4, 9], [2, 6, 7], [5, 7, 4], [0, 0, 1]]
    assert DN.hot_spots(plane, 3, 0).tolist() == [[1, 3, 9], [2, 3, 9], [2, 4, 9]]
    assert DN.hot_spots(plane, 10, 1).tolist() == [[1, 3, 9], [2, 4, 9], [2, 6, 7], [5, 7, 4], [0, 0, 1]]    # (2, 3) is 1 from (1, 3); (2, 4) is d2 = 2 > 1
    assert DN.hot_spots(plane, 10, 3).tolist() == [[1, 3, 9], [2, 6, 7], [5, 7, 4], [0, 0, 1]]               # d2 = 10 > 9 keeps (2, 6); (0, 0) is d2 = 10 away too
    assert DN.hot_spots(plane, 10, 4).tolist() == [[1, 3, 9], [5, 7, 4]]                                      # d2 = 10 <= 16 drops (2, 6) and (0, 0); (5, 7): 16 + 16
    out = DN.hot_spots(np.zeros((4, 4), np.int32), 5, 1)
    assert out.shape == (0, 3) and out.dtype == np.int64                                                       # zeros are never accepted
    assert DN.hot_spots(plane, 0, 0).shape == (0, 3)
    with pytest.raises(ValueError):
        DN.hot_spots(plane.astype(np.float64), 3, 1)


def test_resolve():
    assert DN.resolve(None) is None and DN.resolve({"radius": 150, "step": 64}) == (150.0, 64)
    assert DN.resolve({"radius": 2.5, "step": np.int64(1)}) == (2.5, 1)
    for bad in ({"radius": 50}, {"step": 5}, {"radius": 50, "step": 5, "k": 3}, (50, 5), "50", {"radius": 0, "step": 5}, {"radius": -1.0, "step": 5},
                {"radius": np.inf, "step": 5}, {"radius": 5, "step": 0}, {"radius": 5, "step": -2}):
        with pytest.raises(ValueError):
            DN.resolve(bad)
    for bad in ({"radius": 5, "step": 2.0}, {"radius": "5", "step": 2}, {"radius": 5, "step": True}, {"radius": True, "step": 2}, {"radius": 5, "step": "2"}):
        with pytest.raises(TypeError):
            DN.resolve(bad)


# -- refusals ----------------------------------------------------------------------------------------------
GOOD = dict(xy=np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.5]]), types=np.array([0, 1, 1], np.int32), radius=2.0, raster=(0.0, 0.0, 1.0, 4, 3),
            nr_types=None)

# one assertion per bound of the definition; the raster is (ox, oy, s, W, H)
BAD = [("xy", np.zeros((3, 2), np.float32), TypeError), ("xy", [[0.0, 0.0]], TypeError), ("xy", np.zeros((3, 3)), ValueError),
       ("xy", np.zeros((0, 2)), ValueError), ("xy", np.array([[0.0, np.nan], [1.0, 1.0], [2.0, 2.0]]), ValueError),
       ("xy", np.array([[0.0, np.inf], [1.0, 1.0], [2.0, 2.0]]), ValueError), ("xy", np.array([[-1.0e308, 0.0], [1.0e308, 1.0], [2.0, 2.0]]), ValueError),
       ("types", np.array([0, 1, 1], np.int64), TypeError), ("types", np.array([0, 1], np.int32), ValueError), ("types", np.array([0, 16, 1], np.int32), ValueError),
       ("types", np.array([0, -1, 1], np.int32), ValueError), ("nr_types", 1, ValueError), ("nr_types", 17, ValueError), ("nr_types", 2.0, TypeError),
       ("radius", 0.0, ValueError), ("radius", -1.0, ValueError), ("radius", np.nan, ValueError), ("radius", np.inf, ValueError),
       ("radius", 1.0e200, ValueError), ("radius", 1.0e-200, ValueError), ("radius", "2", TypeError), ("radius", True, TypeError),
       ("raster", (np.nan, 0.0, 1.0, 4, 3), ValueError), ("raster", (0.0, np.inf, 1.0, 4, 3), ValueError), ("raster", (0.0, -np.inf, 1.0, 4, 3), ValueError),
       ("raster", (0.0, 0.0, 0.0, 4, 3), ValueError), ("raster", (0.0, 0.0, -1.0, 4, 3), ValueError), ("raster", (0.0, 0.0, np.inf, 4, 3), ValueError),
       ("raster", (0.0, 0.0, np.nan, 4, 3), ValueError), ("raster", (0.0, 0.0, 1.0, 0, 3), ValueError), ("raster", (0.0, 0.0, 1.0, 4, 0), ValueError),
       ("raster", (0.0, 0.0, 1.0, 16385, 3), ValueError), ("raster", (0.0, 0.0, 1.0, 4, 16385), ValueError),
       ("raster", (0.0, 0.0, 1.0, 16384, 8193), ValueError),                      # T = 2: 2 * 8193 * 16384 > 2^28
       ("raster", (1.0e308, 0.0, 1.0e306, 200, 3), ValueError), ("raster", (0.0, -1.0e308, 1.0e308, 4, 3), ValueError),       # the last node overflows
       ("raster", (0.0, 0.0, 1.0, 4.0, 3), TypeError), ("raster", (0.0, 0.0, 1.0, 4, True), TypeError), ("raster", ("0", 0.0, 1.0, 4, 3), TypeError),
       ("raster", (0.0, 0.0, True, 4, 3), TypeError), ("raster", (0.0, 0.0, 1.0, 4), TypeError), ("raster", None, TypeError), ("raster", "abcde", TypeError)]


@pytest.mark.parametrize("field,value,exc", BAD, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BAD)])
def test_python_refusals_precede_any_work(field, value, exc, monkeypatch):
    """Both paths refuse in `_check`: before a window or a grid is chosen and, for the device form, before anything is allocated or
    launched."""
    from hover_net_amd import lib as L

    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(L, "lib", no_work)
    monkeypatch.setattr(L, "call", no_work)
    monkeypatch.setattr(NB, "grid", no_work)
    monkeypatch.setattr(DN, "_window", no_work)
    args = dict(GOOD, **{field: value})
    for fn in (DN.density_host, DN.density_device, DN.density):
        with pytest.raises(exc):
            fn(args["xy"], args["types"], args["radius"], args["raster"], args["nr_types"])


def test_the_bounds_themselves_are_admitted():
    xy = np.array([[0.0, 0.0]])
    assert DN.density_host(xy, None, 1.0, (0.0, 0.0, 1.0, 16384, 1)).shape == (1, 1, 16384)
    assert DN._check(xy, None, 1.0, (0.0, 0.0, 1.0, 16384, 16384), None)[3] == DN.Raster(0.0, 0.0, 1.0, 16384, 16384)      # 2^28 nodes exactly
    assert DN._check(xy, None, 1.0, (0.0, 0.0, 1.0, 4096, 4096), 16)[4] == 16
    assert DN.workspace_bytes is NB.workspace_bytes


def _op():
    """A well-formed DENSITY op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.x.h = PL.OP_NBR_DENSITY, ncy, ncx, n
    op.w, op.x2.base, op.x2.sn = P(1), P(2), NB.workspace_bytes(n, ncy * ncx)
    op.cout, op.bias = 5, P(3)
    op.y.base, op.y.h, op.y.w = P(5), 100, 120
    return op


# one entry per refusal that include/hvn.h lists for NBR_DENSITY: (field, value, status)
DENSITY_REFUSALS = [("y.base", None, -1), ("bias", None, -1), ("y.base", 0x15000002, -1), ("bias", 0x13000004, -1), ("cout", 0, -1), ("cout", 17, -1),
                    ("cout", -3, -1), ("y.h", 0, -1), ("y.w", 0, -1), ("y.h", -4, -1), ("y.w", -1, -1), ("y.h", 16385, -4), ("y.w", 16385, -4),
                    ("y.h", 1 << 30, -4)]
SHARED_REFUSALS = [("w", None, -1), ("x2.base", None, -1), ("w", 0x11000004, -1), ("x2.base", 0x12000004, -1), ("x.h", 0, -1), ("x.h", -5, -1),
                   ("kh", 0, -1), ("kw", -1, -1), ("x.h", (1 << 26) + 1, -4), ("kh", 4097, -4), ("kw", 4097, -4), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4),
                   ("x2.sn", 0, -4)]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_op_kind_17_is_in_the_header_and_the_plan():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    assert PL.OP_NBR_DENSITY == 17 and "HVN_OP_NBR_DENSITY = 17" in open(L.HEADER).read() and "hvn_density.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                      # no new export


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_DENSITY list: its status, a text that leads with the op's name, decided before any launch
    (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as tests/test_clusters_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_density:") and b"unknown op kind" not in err, (rc, err)

    for path, value, code in DENSITY_REFUSALS + SHARED_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 1, code)
    refused(_op(), 2, -1)                                            # batch must be 1
    op = _op()
    op.kh, op.kw = 2049, 2049                                        # each axis allowed, 2^22 cells exceeded
    op.x2.sn = 1 << 40
    refused(op, 1, -4)
    op = _op()
    op.cout, op.y.h, op.y.w = 2, 8193, 16384                         # each axis allowed, 2^28 nodes exceeded
    refused(op, 1, -4)
    op = _op()
    op.cout, op.y.h, op.y.w = 16, 4096, 4097
    refused(op, 1, -4)
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1)                                             # an all-zero op is refused by name


def test_c_refusals_leave_the_output_untouched_on_the_host_side():
    """The refusals above return before the launcher is entered; here the same with a real host buffer standing in for the output:
    a refused DENSITY does not write it (the op that runs writes EVERY element)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    buf = np.full(5 * 100 * 120, 0x5A5A5A5A, np.int32)
    for path, value in (("cout", 0), ("y.h", 0), ("y.w", 20000), ("x.h", 0), ("x2.sn", 8), ("kh", 5000), ("bias", None)):
        op = _op()
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()


# -- the managers, with the GPU call replaced by a stub (the GPU runs are in tests/test_gpu_density.py) ---------------------
def _stub_info():
    return {1: {"bbox": np.array([[2, 3], [8, 9]]), "centroid": np.array([5.5, 4.5]), "contour": np.array([[3, 2], [3, 7], [8, 7], [8, 2]], np.int32),
                "type_prob": None, "type": None},
            4: {"bbox": np.array([[12, 10], [20, 15]]), "centroid": np.array([12.0, 15.5]), "contour": np.array([[10, 12], [10, 19], [14, 19], [14, 12]], np.int32),
                "type_prob": None, "type": None}}


def _load(path):
    with np.load(path) as z:
        assert sorted(z.files) == ["count", "origin", "radius", "step"]
        return DN.DensityMap(z["count"], tuple(z["origin"].tolist()), int(z["step"]), float(z["radius"]))


def test_process_file_list_writes_density_npz(tmp_path):
    from hover_net_amd import infer_manager as im

    inp = tmp_path / "in"
    inp.mkdir()
    np.save(inp / "a.npy", np.random.default_rng(0).integers(0, 256, (40, 50, 3), dtype=np.uint8))

    def process(images):
        return [(np.zeros(i.shape[:2], np.int32), _stub_info()) for i in images]

    mgr = im.InferManager({"model_args": {"nr_types": None, "mode": "original"}, "model_path": None}, process_fn=process)
    text = {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out)}
        if flag:
            args["density"] = {"radius": 6.0, "step": 4}
        assert mgr.process_file_list(args) == ["a"]
        assert (out / "density").exists() == flag
        text[flag] = open(out / "json" / "a.json").read()
    assert text[True] == text[False]                                 # json/ does not change
    dm = _load(tmp_path / "out1" / "density" / "a.npz")
    want = DN.of_info(_stub_info(), (40, 50), 6.0, 4, None)
    assert dm.origin == want.origin == (1.5, 1.5) and dm.step == 4 and dm.radius == 6.0 and dm.count.shape == (1, 10, 13)
    R.assert_same(dm.count, want.count, "tile manager")
    assert dm.count[0, 1, 1] == 1 and dm.count[0, 4, 3] == 1 and dm.count.sum() > 2
    for bad, exc in (({"radius": 5.0}, ValueError), ({"radius": 5.0, "step": 0}, ValueError), ({"radius": 5.0, "step": 2.0}, TypeError)):
        with pytest.raises(exc):
            mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "density": bad})
    assert not (tmp_path / "bad").exists()                           # refused before any file is touched


def test_process_wsi_list_writes_density_npz(tmp_path):
    from hover_net_amd import infer_manager as im

    inp = tmp_path / "slides"
    inp.mkdir()
    np.save(inp / "s.npy", np.random.default_rng(1).integers(30, 120, (64, 96, 3), dtype=np.uint8))
    mgr = im.WsiManager({"model_args": {"nr_types": None, "mode": "fast"}, "model_path": None}, wsi_fn=lambda slide, mask: (None, _stub_info()))
    text = {}
    for flag in (False, True):
        out = tmp_path / ("out%d" % flag)
        args = {"input_dir": str(inp), "output_dir": str(out)}
        if flag:
            args["density"] = {"radius": 6.0, "step": 8}
        assert mgr.process_wsi_list(args) == {"s": "done"}
        assert (out / "density").exists() == flag
        text[flag] = open(out / "s.json").read()
    assert text[True] == text[False]
    dm = _load(tmp_path / "out1" / "density" / "s.npz")
    want = DN.of_info(_stub_info(), (64, 96), 6.0, 8, None)
    assert dm.origin == (3.5, 3.5) and dm.step == 8 and dm.count.shape == (1, 8, 12) and int(dm.count.sum()) >= 2
    R.assert_same(dm.count, want.count, "wsi manager")
    with pytest.raises(ValueError):
        mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "density": {"step": 8}})
    assert not (tmp_path / "bad").exists()

"""CPU: hover_net_amd/ripley.py's host path against the all-pairs oracle tests/ripley_ref.py on every case the GPU tests run, its
properties (symmetry, the independent count of neighbours.py, K of a lattice against the Gauss circle count), the derived forms
(`K`, `L`, `rings`, `save`, `of_info`, `resolve`, `window_of`), the Python refusals and the C refusals of HVN_OP_NBR_PAIRS, which the
library decides before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ripley_ref as R
from hover_net_amd import neighbours as NB
from hover_net_amd import ripley as RP


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_equals_oracle(name):
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = RP.pairs_host(*args)
    assert isinstance(got, RP.PairCounts) and got.radii.tolist() == list(args[2]) and got.window == tuple(args[3])
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    R.assert_same(RP.pairs(*args, device=None), want, name)


def test_host_path_does_not_depend_on_the_round_size(monkeypatch):
    monkeypatch.setattr(RP, "_PAIRS", 700)           # hundreds of rounds
    for name in ("lattice", "edge", "outside", "r32", "sixteen_types"):
        args, want = R.case(name)
        R.assert_same(RP.pairs_host(*args), want, name)


def test_host_path_in_reversed_order():
    for name in ("lattice", "edge", "nine_types"):
        (xy, types, radii, window, t), want = R.case(name)
        R.assert_same(RP.pairs_host(np.ascontiguousarray(xy[::-1]), np.ascontiguousarray(types[::-1]), radii, window, t), want, name)


def test_the_accumulator_is_the_docstrings(monkeypatch):
    """The construction the docstring names, spelled out once more with an all-pairs kmin and m: the difference array's running sum is
    pairs_in."""
    (xy, types, radii, window, t), want = R.case("edge")
    rr = np.asarray(radii)
    d2 = NB.d2_of(xy[:, None, 0], xy[:, None, 1], xy[None, :, 0], xy[None, :, 1])
    kmin = np.searchsorted(rr * rr, d2, "left")
    m = np.searchsorted(rr, RP.border(xy, window), "right")
    acc = np.zeros((2, t, t, len(radii) + 1), np.int64)
    for i, j in zip(*np.nonzero((kmin < len(radii)) & ~np.eye(xy.shape[0], dtype=bool))):
        acc[0, types[i], types[j], kmin[i, j]] += 1
        if kmin[i, j] < m[i]:
            acc[1, types[i], types[j], kmin[i, j]] += 1
            acc[1, types[i], types[j], m[i]] -= 1        # the spare column takes m = R
    assert (acc[0, :, :, :-1].cumsum(-1) == want[0]).all() and (acc[1, :, :, :-1].cumsum(-1) == want[1]).all()


# -- properties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "outside", "nine_types", "widened"])
def test_the_largest_radius_equals_the_typed_counts_of_neighbours(name):
    """An independent path: pairs[a, b, R - 1] is the sum over the points i of type a of `neighbours.query_host`'s count[i, b] at
    r_{R-1}."""
    (xy, types, radii, window, t), _ = R.case(name)
    count = NB.query_host(xy, types, radii[-1], 1, t)["count"].astype(np.int64)
    want = np.zeros((t, t), np.int64)
    np.add.at(want, types, count)
    assert (RP.pairs_host(xy, types, radii, window, t).pairs[:, :, -1] == want).all() and want.sum() > 0


def test_pairs_is_symmetric_and_pairs_in_need_not_be():
    for name in ("lattice", "edge", "outside", "sixteen_types"):
        args, _ = R.case(name)
        pc = RP.pairs_host(*args)
        assert (pc.pairs == pc.pairs.transpose(1, 0, 2)).all(), name
    pc = RP.pairs_host(*R.case("outside")[0])
    assert (pc.pairs_in != pc.pairs_in.transpose(1, 0, 2)).any()


def test_K_of_a_full_lattice_is_the_gauss_circle_count():
    """The integer lattice 60 x 50, one type, the window of its pixels (area = n).  A point i that lies r inside the window has ALL
    lattice points within r of it as neighbours, G(r) - 1 of them with G(r) = #{(u, v) in Z^2 : u^2 + v^2 <= r^2}, so K(r) = area *
    pairs_in / (n_in * n) = G(r) - 1 whatever n_in is.  Every unit square centred on a counted lattice point lies within r + sqrt(2) / 2
    of the origin, and the disc of radius r - sqrt(2) / 2 is covered by those squares:
        pi (r - sqrt(2) / 2)^2 <= G(r) <= pi (r + sqrt(2) / 2)^2,   hence   |G(r) - pi r^2| <= pi (sqrt(2) r + 1 / 2),
    the bound K is held to here (plus the 1 of the point itself)."""
    yy, xx = np.mgrid[0:50, 0:60]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
    radii = (1.0, 2.5, 5.0, 8.0, 13.0)
    pc = RP.pairs_host(xy, None, radii, RP.window_of((50, 60)))
    k = RP.K(pc)
    assert RP.area_of(pc.window) == 3000.0 == float(pc.n[0]) and k.shape == (1, 1, 5)
    u = np.arange(-14, 15)
    for i, r in enumerate(radii):
        gauss = int(((u[:, None] ** 2 + u[None, :] ** 2) <= r * r).sum())
        assert pc.n_in[0, i] > 0 and pc.pairs_in[0, 0, i] == pc.n_in[0, i] * (gauss - 1)
        assert abs(k[0, 0, i] - (gauss - 1)) <= 1e-9 * gauss
        assert abs(k[0, 0, i] - math.pi * r * r) <= math.pi * (math.sqrt(2.0) * r + 0.5) + 1.0
    assert np.allclose(RP.L(pc), np.sqrt(k / math.pi)) and abs(RP.L(pc)[0, 0, 4] - 13.0) < 0.5


# -- K, L, rings, save, of_info, resolve -----------------------------------------------------------------------
def test_K_L_rings_on_hand_made_counts():
    pc = RP.PairCounts(np.array([[[2, 6], [1, 4]], [[1, 4], [0, 0]]], np.int64), np.array([[[2, 3], [1, 2]], [[0, 2], [0, 0]]], np.int64),
                       np.array([4, 2], np.int64), np.array([[2, 1], [0, 1]], np.int64), np.array([1.0, 2.0]), (0.0, 0.0, 10.0, 5.0))
    k = RP.K(pc)
    assert k[0, 0].tolist() == [50.0 * 2 / (2 * 4), 50.0 * 3 / (1 * 4)] and k[0, 1].tolist() == [50.0 * 1 / (2 * 2), 50.0 * 2 / (1 * 2)]     # n[b], not n[b] - 1
    assert np.isnan(k[1, :, 0]).all() and k[1, 0, 1] == 50.0 * 2 / (1 * 4) and k[1, 1, 1] == 0.0                                        # NaN where n_in is 0
    assert RP.K(pc, area=8.0)[0, 0, 0] == 8.0 * 2 / 8
    lo = RP.L(pc)
    assert lo[0, 0, 0] == math.sqrt(k[0, 0, 0] / math.pi) and np.isnan(lo[1, 0, 0])
    assert RP.rings(pc).tolist() == [[[2, 1], [1, 1]], [[0, 2], [0, 0]]] and RP.rings(pc).dtype == np.int64


def test_save_round_trips(tmp_path):
    pc = RP.pairs_host(*R.case("edge")[0])
    RP.save(str(tmp_path / "a.npz"), pc)
    with np.load(tmp_path / "a.npz") as z:
        assert sorted(z.files) == ["n", "n_in", "pairs", "pairs_in", "radii", "window"]
        assert all((z[f] == getattr(pc, f)).all() for f in z.files) and z["pairs"].dtype == z["pairs_in"].dtype == z["n_in"].dtype == np.int64
        assert z["radii"].tolist() == [2.0, 3.0, 4.5] and z["window"].tolist() == [0.0, 0.0, 20.0, 20.0]


def _hand_dict(typed=True):
    """Labels neither contiguous nor sorted, in a 10 x 14 image (window (-0.5, -0.5, 13.5, 9.5)).  40 and 7 are 2.5 apart (1.5, 2):
    exactly on the radius 2.5; 12 is alone; 3 is sqrt(8) from 40.  b: 40 -> 4 (to y = 9.5), 7 -> 2, 12 -> 0.5, 3 -> 4."""
    pts = {40: (5.5, 5.5, 1), 7: (7.0, 7.5, 0), 12: (13.0, 8.0, 1), 3: (3.5, 3.5, 2)}
    return {lab: {"bbox": np.zeros((2, 2), np.int64), "centroid": np.array([x, y]), "contour": None, "type_prob": None,
                  "type": t if typed else None} for lab, (x, y, t) in pts.items()}


def test_of_info_hand_made_dict():
    pc = RP.of_info(_hand_dict(), (10, 14), [2.5, 3.0], 3)
    assert isinstance(pc, RP.PairCounts) and pc.window == (-0.5, -0.5, 13.5, 9.5) and pc.radii.tolist() == [2.5, 3.0] and RP.area_of(pc.window) == 140.0
    want = np.zeros((3, 3, 2), np.int64)
    want[1, 0] = want[0, 1] = [1, 1]                             # 40 <-> 7 at d2 = 2.25 + 4 = 6.25 = r2_0 exactly
    want[1, 2] = want[2, 1] = [0, 1]                             # 40 <-> 3 at sqrt(8) <= 3
    assert (pc.pairs == want).all() and pc.n.tolist() == [1, 2, 1] and pc.n_in.tolist() == [[0, 0], [1, 1], [1, 1]]
    inside = want.copy()
    inside[0, 1] = 0                                             # 7 lies 2 from the window's edge: inside at no radius
    assert (pc.pairs_in == inside).all()
    wide = RP.of_info(_hand_dict(), (10, 14), [2.5, 3.0], 5, window=(-10.0, -10.0, 30.0, 30.0))
    assert (wide.pairs_in[:3, :3] == want).all() and wide.pairs.shape == (5, 5, 2) and not wide.pairs[3:].any() and wide.window == (-10.0, -10.0, 30.0, 30.0)


def test_of_info_untyped_and_empty():
    pc = RP.of_info(_hand_dict(typed=False), (10, 14), [2.5, 3.0], None)
    assert pc.pairs.tolist() == [[[2, 4]]] and pc.pairs_in.tolist() == [[[1, 3]]] and pc.n.tolist() == [4] and pc.n_in.tolist() == [[2, 2]]
    empty = RP.of_info({}, (10, 14), [2.5, 3.0], 5)
    assert empty.pairs.shape == empty.pairs_in.shape == (5, 5, 2) and empty.pairs.dtype == np.int64 and not empty.pairs.any() and not empty.pairs_in.any()
    assert empty.n.tolist() == [0] * 5 and empty.n_in.shape == (5, 2) and empty.window == (-0.5, -0.5, 13.5, 9.5) and np.isnan(RP.K(empty)).all()
    with pytest.raises(ValueError):
        RP.of_info(_hand_dict(typed=False), (10, 14), [2.5], 3)  # nr_types given, entries untyped
    with pytest.raises(ValueError):
        RP.of_info(_hand_dict(), (10, 14), [2.5], 2)             # a type outside [0, 2)
    with pytest.raises(ValueError):
        RP.of_info({}, (10, 14), [], 3)                          # also for an empty dict
    with pytest.raises(ValueError):
        RP.of_info({}, (0, 14), [2.5], 3)


def test_window_of_and_resolve():
    assert RP.window_of((900, 1000)) == (-0.5, -0.5, 999.5, 899.5) and RP.area_of(RP.window_of((900, 1000))) == 900000.0
    assert RP.resolve(None) is None and RP.resolve({"radii": [10, 20.5]}) == ((10.0, 20.5), None)
    assert RP.resolve({"radii": np.array([1.0, 2.0]), "window": [0, 0, 5, np.float64(6)]}) == ((1.0, 2.0), (0.0, 0.0, 5.0, 6.0))
    assert RP.resolve({"radii": (3,), "window": None}) == ((3.0,), None)
    for bad in ({"radius": 5}, {"radii": [5], "step": 2}, {"window": (0, 0, 1, 1)}, (5, 6), "5", {"radii": []}, {"radii": [0.0]}, {"radii": [-1.0, 2.0]},
                {"radii": [np.inf]}, {"radii": [np.nan]}, {"radii": [1.0, 1.0]}, {"radii": [2.0, 1.0]}, {"radii": list(range(1, 34))}, {"radii": [1.0e200]},
                {"radii": [1], "window": (0, 0, 0, 1)}, {"radii": [1], "window": (0, 5, 1, 1)}, {"radii": [1], "window": (0, 0, np.inf, 1)},
                {"radii": [1], "window": (np.nan, 0, 1, 1)}):
        with pytest.raises(ValueError):
            RP.resolve(bad)
    for bad in ({"radii": 5.0}, {"radii": "12"}, {"radii": ["1"]}, {"radii": [True]}, {"radii": [1], "window": (0, 0, 1)}, {"radii": [1], "window": "0011"},
                {"radii": [1], "window": (0, 0, 1, "1")}, {"radii": [1], "window": (0, 0, 1, True)}, {"radii": [1], "window": 4}):
        with pytest.raises(TypeError):
            RP.resolve(bad)


# -- refusals ----------------------------------------------------------------------------------------------
GOOD = dict(xy=np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.5]]), types=np.array([0, 1, 1], np.int32), radii=(1.0, 2.0), window=(0.0, 0.0, 4.0, 3.0),
            nr_types=None)

# one assertion per bound of the definition
BAD = [("xy", np.zeros((3, 2), np.float32), TypeError), ("xy", [[0.0, 0.0]], TypeError), ("xy", np.zeros((3, 3)), ValueError),
       ("xy", np.zeros((0, 2)), ValueError), ("xy", np.array([[0.0, np.nan], [1.0, 1.0], [2.0, 2.0]]), ValueError),
       ("xy", np.array([[0.0, np.inf], [1.0, 1.0], [2.0, 2.0]]), ValueError), ("xy", np.array([[-1.0e308, 0.0], [1.0e308, 1.0], [2.0, 2.0]]), ValueError),
       ("types", np.array([0, 1, 1], np.int64), TypeError), ("types", np.array([0, 1], np.int32), ValueError), ("types", np.array([0, 16, 1], np.int32), ValueError),
       ("types", np.array([0, -1, 1], np.int32), ValueError), ("nr_types", 1, ValueError), ("nr_types", 17, ValueError), ("nr_types", 2.0, TypeError),
       ("radii", (), ValueError), ("radii", tuple(float(k) for k in range(1, 34)), ValueError), ("radii", (0.0, 1.0), ValueError), ("radii", (-1.0,), ValueError),
       ("radii", (np.nan,), ValueError), ("radii", (1.0, np.inf), ValueError), ("radii", (1.0e200,), ValueError), ("radii", (1.0e-200, 1.0), ValueError),
       ("radii", (1.0, 1.0), ValueError), ("radii", (2.0, 1.0), ValueError), ("radii", 2.0, TypeError), ("radii", "12", TypeError), ("radii", ("2",), TypeError),
       ("radii", (True, 2.0), TypeError), ("radii", None, TypeError),
       ("window", (0.0, 0.0, 0.0, 3.0), ValueError), ("window", (0.0, 3.0, 4.0, 3.0), ValueError), ("window", (5.0, 0.0, 4.0, 3.0), ValueError),
       ("window", (np.nan, 0.0, 4.0, 3.0), ValueError), ("window", (0.0, 0.0, np.inf, 3.0), ValueError), ("window", (0.0, -np.inf, 4.0, 3.0), ValueError),
       ("window", (0.0, 0.0, 4.0), TypeError), ("window", None, TypeError), ("window", "abcd", TypeError), ("window", (0.0, 0.0, 4.0, "3"), TypeError),
       ("window", (0.0, 0.0, True, 3.0), TypeError)]


@pytest.mark.parametrize("field,value,exc", BAD, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BAD)])
def test_python_refusals_precede_any_work(field, value, exc, monkeypatch):
    """Both paths refuse in `_check`: before a grid is chosen and, for the device form, before anything is allocated or launched."""
    from hover_net_amd import lib as L
    from hover_net_amd import points as P

    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(L, "lib", no_work)
    monkeypatch.setattr(L, "call", no_work)
    monkeypatch.setattr(P, "grid", no_work)
    monkeypatch.setattr(P, "candidate_runs", no_work)
    args = dict(GOOD, **{field: value})
    for fn in (RP.pairs_host, RP.pairs_device, RP.pairs):
        with pytest.raises(exc):
            fn(args["xy"], args["types"], args["radii"], args["window"], args["nr_types"])


def test_too_many_bins_are_refused_and_the_bounds_themselves_admitted():
    xy = np.array([[0.0, 0.0], [0.5, 0.0]])
    r17, r16, r32 = tuple(float(k) for k in range(1, 18)), tuple(float(k) for k in range(1, 17)), tuple(float(k) for k in range(1, 33))
    with pytest.raises(ValueError, match="bins"):
        RP.pairs_host(xy, None, r17, (0.0, 0.0, 1.0, 1.0), 16)   # 16 * 16 * 17 > 4096
    assert RP._check(xy, None, r16, (0.0, 0.0, 1.0, 1.0), 16)[4] == 16           # 4096 bins exactly
    assert RP.pairs_host(xy, None, r32, (-40.0, -40.0, 40.0, 40.0), 11).pairs.shape == (11, 11, 32)
    assert RP.pairs_host(xy, None, r32, (-40.0, -40.0, 40.0, 40.0)).pairs_in[0, 0].tolist() == [2] * 32
    with pytest.raises(ValueError, match="bins"):
        RP.pairs_host(xy, None, r32, (0.0, 0.0, 1.0, 1.0), 12)   # 12 * 12 * 32 > 4096


def _op():
    """A well-formed PAIRS op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.x.h = PL.OP_NBR_PAIRS, ncy, ncx, n
    op.w, op.x2.base, op.x2.sn = P(1), P(2), NB.workspace_bytes(n, ncy * ncx)
    op.cout, op._rsv, op.bias = 5, 16, P(3)
    op.y.base = P(5)
    return op


# one entry per refusal that include/hvn.h lists for NBR_PAIRS: (field, value, status)
PAIRS_REFUSALS = [("y.base", None, -1), ("bias", None, -1), ("y.base", 0x15000004, -1), ("y.base", 0x15000002, -1), ("bias", 0x13000004, -1), ("cout", 0, -1),
                  ("cout", 17, -1), ("cout", -3, -1), ("_rsv", 0, -1), ("_rsv", 33, -1), ("_rsv", -1, -1)]
SHARED_REFUSALS = [("w", None, -1), ("x2.base", None, -1), ("w", 0x11000004, -1), ("x2.base", 0x12000004, -1), ("x.h", 0, -1), ("x.h", -5, -1),
                   ("kh", 0, -1), ("kw", -1, -1), ("x.h", (1 << 26) + 1, -4), ("kh", 4097, -4), ("kw", 4097, -4), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4),
                   ("x2.sn", 0, -4)]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_op_kind_18_is_in_the_header_and_the_plan():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    assert PL.OP_NBR_PAIRS == 18 and "HVN_OP_NBR_PAIRS = 18" in open(L.HEADER).read() and "hvn_pairs.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                      # no new export


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_PAIRS list: its status, a text that leads with the op's name, decided before any launch
    (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as tests/test_density_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_pairs:") and b"unknown op kind" not in err, (rc, err)

    for path, value, code in PAIRS_REFUSALS + SHARED_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 1, code)
    refused(_op(), 2, -1)                                            # batch must be 1
    op = _op()
    op.kh, op.kw = 2049, 2049                                        # each axis allowed, 2^22 cells exceeded
    op.x2.sn = 1 << 40
    refused(op, 1, -4)
    for t, r in ((16, 17), (12, 32), (15, 19)):                      # T and R allowed, 4096 bins exceeded
        op = _op()
        op.cout, op._rsv = t, r
        refused(op, 1, -4)
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1)                                             # an all-zero op is refused by name


def test_c_refusals_leave_the_output_untouched_on_the_host_side():
    """The refusals above return before the launcher is entered; here the same with a real host buffer standing in for the output:
    a refused PAIRS does not write it (the op that runs clears and writes EVERY element)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    buf = np.full(2 * 5 * 5 * 16, 0x5A5A5A5A, np.int64)
    for path, value in (("cout", 0), ("_rsv", 0), ("_rsv", 40), ("x.h", 0), ("x2.sn", 8), ("kh", 5000), ("bias", None)):
        op = _op()
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()


# -- the managers, with the GPU call replaced by a stub (the GPU runs are in tests/test_gpu_ripley.py) -----------------------
def _stub_info():
    return {1: {"bbox": np.array([[2, 3], [8, 9]]), "centroid": np.array([5.5, 4.5]), "contour": np.array([[3, 2], [3, 7], [8, 7], [8, 2]], np.int32),
                "type_prob": None, "type": None},
            4: {"bbox": np.array([[12, 10], [20, 15]]), "centroid": np.array([12.0, 15.5]), "contour": np.array([[10, 12], [10, 19], [14, 19], [14, 12]], np.int32),
                "type_prob": None, "type": None},
            9: {"bbox": np.array([[14, 12], [20, 18]]), "centroid": np.array([15.0, 19.5]), "contour": np.array([[12, 14], [12, 19], [17, 19], [17, 14]], np.int32),
                "type_prob": None, "type": None}}


def _load(path):
    with np.load(path) as z:
        assert sorted(z.files) == ["n", "n_in", "pairs", "pairs_in", "radii", "window"]
        return RP.PairCounts(z["pairs"], z["pairs_in"], z["n"], z["n_in"], z["radii"], tuple(z["window"].tolist()))


def test_process_file_list_writes_ripley_npz(tmp_path):
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
            args["ripley"] = {"radii": [4.0, 6.0]}
        assert mgr.process_file_list(args) == ["a"]
        assert (out / "ripley").exists() == flag
        text[flag] = open(out / "json" / "a.json").read()
    assert text[True] == text[False]                                 # json/ does not change
    pc = _load(tmp_path / "out1" / "ripley" / "a.npz")
    want = RP.of_info(_stub_info(), (40, 50), [4.0, 6.0], None)
    R.assert_same(pc, want[:4], "tile manager")
    assert pc.window == want.window == (-0.5, -0.5, 49.5, 39.5) and pc.radii.tolist() == [4.0, 6.0]
    assert pc.pairs.tolist() == [[[0, 2]]] and pc.pairs_in.tolist() == [[[0, 2]]] and pc.n.tolist() == [3] and pc.n_in.tolist() == [[3, 2]]   # 4 <-> 9 at distance 5; 1 lies 5 from y = -0.5
    for bad, exc in (({"radius": 5.0}, ValueError), ({"radii": []}, ValueError), ({"radii": 5.0}, TypeError)):
        with pytest.raises(exc):
            mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "ripley": bad})
    assert not (tmp_path / "bad").exists()                           # refused before any file is touched


def test_process_wsi_list_writes_ripley_npz(tmp_path):
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
            args["ripley"] = {"radii": [6.0], "window": (2.0, 2.0, 30.0, 30.0)}
        assert mgr.process_wsi_list(args) == {"s": "done"}
        assert (out / "ripley").exists() == flag
        text[flag] = open(out / "s.json").read()
    assert text[True] == text[False]
    pc = _load(tmp_path / "out1" / "ripley" / "s.npz")
    want = RP.of_info(_stub_info(), (64, 96), [6.0], None, window=(2.0, 2.0, 30.0, 30.0))
    R.assert_same(pc, want[:4], "wsi manager")
    assert pc.window == (2.0, 2.0, 30.0, 30.0) and pc.pairs.tolist() == [[[2]]] and pc.n_in.tolist() == [[2]]
    with pytest.raises(ValueError):
        mgr.process_wsi_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "ripley": {"window": (0, 0, 8, 8)}})
    assert not (tmp_path / "bad").exists()

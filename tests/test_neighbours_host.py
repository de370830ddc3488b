"""CPU: hover_net_amd/neighbours.py's host path against the O(N^2) oracle tests/neighbours_ref.py on every case the GPU tests run, the
derived forms (`distances`, `edges`, `annotate`), the Python refusals and the C refusals of HVN_OP_NBR_GRID / HVN_OP_NBR_QUERY, which
the library decides before any launch."""
import ctypes
import json

import numpy as np
import pytest
import torch

import neighbours_ref as R
from hover_net_amd import neighbours as NB


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_equals_oracle(name):
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = NB.query_host(*args)
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    if args[0].shape[0] <= 2000:
        R.assert_same(NB.query(*args, device=None), want, name)


def test_the_margin_is_needed():
    """The rounding case at c = r: the second and third point are neighbours by definition and land in cells 0 and 2."""
    (xy, _, r, _, _), want = R.case("rounding")
    assert float(xy[2, 0] - xy[1, 0]) == 1.0 and want["knn"][1].tolist() == [0, 2]
    at_r = NB.Grid(0.0, 0.0, r, 3, 8)
    assert NB.cells(xy, at_r)[0].tolist() == [0, 0, 2, 0]
    g = NB.grid(xy, r)
    assert g.c == r * (1.0 + 2.0 ** -20) and NB.cells(xy, g)[0].tolist() == [0, 0, 1, 0]


def test_host_path_does_not_depend_on_the_round_size(monkeypatch):
    args, want = R.case("random")
    monkeypatch.setattr(NB, "_PAIRS", 1000)          # hundreds of rounds instead of one
    R.assert_same(NB.query_host(*args), want)


def test_grid_caps():
    xy = np.array([[0.0, 0.0], [1.0e6, 3.0e5], [5.0, 5.0]])
    g = NB.grid(xy, 0.01)
    assert g.ncx <= 4096 and g.ncy <= 4096 and g.ncx * g.ncy <= 1 << 22 and g.c >= 0.01 * NB.MARGIN
    cx, cy = NB.cells(xy, g)
    assert 0 <= cx.min() and cx.max() == g.ncx - 1 and cy.max() == g.ncy - 1
    assert NB.workspace_bytes(3, g.ncx * g.ncy) == 72 + 4 * (2 * g.ncx * g.ncy + 1) + 4096


# -- distances, edges, annotate ----------------------------------------------------------------------------
def test_distances_and_edges():
    (xy, types, r, k, t), want = R.case("random")
    d = NB.distances(xy, want["knn"])
    assert d.dtype == np.float64 and d.shape == want["knn"].shape
    i = 17
    for s, j in enumerate(want["knn"][i]):
        dx, dy = xy[j, 0] - xy[i, 0], xy[j, 1] - xy[i, 1]
        assert d[i, s] == np.sqrt(dx * dx + dy * dy) and d[i, s] <= r
    assert (np.diff(d, axis=1) >= 0).all()
    dn = NB.distances(xy, want["nearest_of_type"])
    assert np.isinf(dn[want["nearest_of_type"] < 0]).all() and np.isfinite(dn[want["nearest_of_type"] >= 0]).all()
    assert (dn.min(1) == d[:, 0]).all()              # the nearest over all types is the first of knn
    e = NB.edges(want["knn"])
    pairs = {(min(a, int(b)), max(a, int(b))) for a in range(xy.shape[0]) for b in want["knn"][a] if b >= 0}
    assert e.dtype == np.int32 and e.tolist() == [list(p) for p in sorted(pairs)]
    assert NB.edges(np.full((3, 2), -1, np.int32)).shape == (0, 2)
    assert NB.edges(np.array([[1, -1], [0, -1], [-1, -1]], np.int32)).tolist() == [[0, 1]]


def _hand_dict(typed=True):
    """Labels neither contiguous nor sorted; dict order is the position order."""
    pts = {40: (10.0, 10.0, 1), 7: (13.0, 14.0, 0), 1000: (10.0, 15.5, 1), 3: (60.0, 60.0, 2), 12: (10.0, 10.0, 0)}
    return {lab: {"bbox": np.zeros((2, 2), np.int64), "centroid": np.array([x, y]), "contour": None, "type_prob": None,
                  "type": t if typed else None} for lab, (x, y, t) in pts.items()}


def test_annotate_hand_made_dict():
    info = _hand_dict()
    out = NB.annotate(info, 5.5, 2, 3)
    assert out is info and list(out) == [40, 7, 1000, 3, 12]
    n = {lab: e["neighbours"] for lab, e in out.items()}
    # 40 and 12 coincide (d 0, the only neighbour of either at distance 0); 7 is 5 away from both; 1000 is 5.5 away from both: at the radius
    assert n[40] == {"count": [2, 1, 0], "knn": [12, 7], "knn_dist": [0.0, 5.0], "nearest_of_type": [12, 1000, None],
                     "nearest_of_type_dist": [0.0, 5.5, None]}
    assert n[12]["knn"] == [40, 7] and n[12]["count"] == [1, 2, 0] and n[12]["nearest_of_type"] == [7, 40, None]
    assert n[7]["knn"] == [1000, 40] and n[7]["knn_dist"] == [np.sqrt(9.0 + 2.25), 5.0] and n[7]["count"] == [1, 2, 0]
    assert n[1000]["knn"] == [7, 40] and n[1000]["knn_dist"] == [np.sqrt(9.0 + 2.25), 5.5]          # 40 and 12 are equally far: position order
    assert n[3] == {"count": [0, 0, 0], "knn": [], "knn_dist": [], "nearest_of_type": [None, None, None], "nearest_of_type_dist": [None, None, None]}
    for e in n.values():
        assert json.loads(json.dumps(e)) == e
        assert all(type(v) is int for v in e["count"] + e["knn"]) and all(type(v) is float for v in e["knn_dist"])
    assert set(out[40]) == {"bbox", "centroid", "contour", "type_prob", "type", "neighbours"}


def test_annotate_untyped_and_empty():
    info = NB.annotate(_hand_dict(typed=False), 5.5, 4, None)
    assert info[40]["neighbours"] == {"count": [3], "knn": [12, 7, 1000], "knn_dist": [0.0, 5.0, 5.5], "nearest_of_type": [12],
                                      "nearest_of_type_dist": [0.0]}
    assert info[7]["neighbours"]["knn"] == [1000, 40, 12] and info[7]["neighbours"]["knn_dist"][1:] == [5.0, 5.0]      # a tie: position order
    empty = {}
    assert NB.annotate(empty, 5.0, 3, 5) is empty and empty == {}
    with pytest.raises(ValueError):
        NB.annotate(_hand_dict(typed=False), 5.5, 4, 3)          # nr_types given, entries untyped
    with pytest.raises(ValueError):
        NB.annotate(_hand_dict(), 5.5, 4, 2)                     # a type outside [0, 2)


def test_annotate_equals_query_on_a_case():
    (xy, types, r, k, t), want = R.case("slide")
    labels = [3 * i + 5 for i in range(xy.shape[0])][::-1]
    info = {lab: {"centroid": xy[i], "type": int(types[i])} for i, lab in enumerate(labels)}
    NB.annotate(info, r, k, t)
    d = NB.distances(xy, want["knn"])
    for i in (0, 100, 109, 555, 1999):
        e = info[labels[i]]["neighbours"]
        m = int((want["knn"][i] >= 0).sum())
        assert e["knn"] == [labels[j] for j in want["knn"][i][:m]] and e["knn_dist"] == d[i, :m].tolist()
        assert e["count"] == want["count"][i].tolist()
        assert e["nearest_of_type"] == [labels[j] if j >= 0 else None for j in want["nearest_of_type"][i]]


# -- refusals ----------------------------------------------------------------------------------------------
GOOD = dict(xy=np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.5]]), types=np.array([0, 1, 1], np.int32), radius=2.0, k=2, nr_types=2)

BAD = [("xy", np.zeros((3, 2), np.float32), TypeError), ("xy", [[0.0, 0.0]], TypeError), ("xy", np.zeros((3, 3)), ValueError),
       ("xy", np.zeros(6), ValueError), ("xy", np.zeros((0, 2)), ValueError), ("xy", np.array([[0.0, np.nan], [1.0, 1.0], [2.0, 2.0]]), ValueError),
       ("xy", np.array([[0.0, np.inf], [1.0, 1.0], [2.0, 2.0]]), ValueError), ("xy", np.array([[-1.0e308, 0.0], [1.0e308, 1.0], [2.0, 2.0]]), ValueError),
       ("types", np.array([0, 1, 1], np.int64), TypeError), ("types", [0, 1, 1], TypeError), ("types", np.array([0, 1], np.int32), ValueError),
       ("types", np.array([0, 2, 1], np.int32), ValueError), ("types", np.array([0, -1, 1], np.int32), ValueError),
       ("radius", 0.0, ValueError), ("radius", -1.0, ValueError), ("radius", np.nan, ValueError), ("radius", np.inf, ValueError),
       ("radius", 1.0e200, ValueError), ("radius", 1.0e-200, ValueError), ("radius", "2", TypeError), ("radius", True, TypeError),
       ("k", 0, ValueError), ("k", 17, ValueError), ("k", 2.0, TypeError), ("k", True, TypeError),
       ("nr_types", 0, ValueError), ("nr_types", 17, ValueError), ("nr_types", 2.0, TypeError)]


@pytest.mark.parametrize("field,value,exc", BAD, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BAD)])
def test_python_refusals_precede_any_work(field, value, exc, monkeypatch):
    """Both paths refuse in `_check`: before the grid is chosen and, for the device form, before anything is allocated or launched."""
    from hover_net_amd import lib as L

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "lib", no_launch)
    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(NB, "grid", no_launch)
    args = dict(GOOD, **{field: value})
    for fn in (NB.query_host, NB.query_device, NB.query):
        with pytest.raises(exc):
            fn(args["xy"], args["types"], args["radius"], args["k"], args["nr_types"])


def test_resolve():
    assert NB.resolve(None) is None and NB.resolve({"radius": 50, "k": 5}) == (50.0, 5)
    for bad in ({"radius": 50}, {"radius": 50, "k": 5, "types": 3}, (50, 5), "50", {"radius": 0, "k": 5}, {"radius": 5, "k": 17}):
        with pytest.raises(ValueError):
            NB.resolve(bad)
    with pytest.raises(TypeError):
        NB.resolve({"radius": 5, "k": 2.5})


def _ops():
    """A well-formed GRID and QUERY op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    ops = []
    for kind in (PL.OP_NBR_GRID, PL.OP_NBR_QUERY):
        op = L.hvn_op()
        op.kind, op.kh, op.kw, op.x.h = kind, ncy, ncx, n
        op.w, op.x2.base, op.x2.sn = P(1), P(2), NB.workspace_bytes(n, ncy * ncx)
        ops.append(op)
    ops[0].x.base, ops[0].res.base = P(3), P(4)
    ops[1].cout, ops[1]._rsv = 5, 8
    ops[1].y.base, ops[1].y2.base, ops[1].res.base = P(5), P(6), P(7)
    return ops


GRID_REFUSALS = [("x.base", None, -1), ("x.base", 0x13000004, -1), ("res.base", 0x14000002, -1)]
QUERY_REFUSALS = [("y.base", None, -1), ("y2.base", None, -1), ("res.base", None, -1), ("y.base", 0x15000002, -1), ("y2.base", 0x16000001, -1),
                  ("res.base", 0x17000002, -1), ("_rsv", 0, -1), ("_rsv", 17, -1), ("cout", 0, -1), ("cout", 17, -1)]
BOTH_REFUSALS = [("w", None, -1), ("x2.base", None, -1), ("w", 0x11000004, -1), ("x2.base", 0x12000004, -1), ("x.h", 0, -1), ("x.h", -5, -1),
                 ("kh", 0, -1), ("kw", -1, -1), ("x.h", (1 << 26) + 1, -4), ("kh", 4097, -4), ("kw", 4097, -4), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4),
                 ("x2.sn", 0, -4)]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR list: its status, a text that leads with the op's name, decided before any launch (the
    pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as tests/test_stain_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    names = (b"nbr_grid", b"nbr_query")

    def refused(op, batch, code, name):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(name + b":") and b"unknown op kind" not in err, (rc, err)

    for which, table in ((0, GRID_REFUSALS), (1, QUERY_REFUSALS), (0, BOTH_REFUSALS), (1, BOTH_REFUSALS)):
        for path, value, code in table:
            op = _ops()[which]
            _set(op, path, value)
            refused(op, 1, code, names[which])
    for which in (0, 1):
        refused(_ops()[which], 2, -1, names[which])                  # batch must be 1
        op = _ops()[which]
        op.kh, op.kw = 2049, 2049                                    # each axis allowed, 2^22 cells exceeded
        op.x2.sn = 1 << 40
        refused(op, 1, -4, names[which])
        zero = L.hvn_op()
        zero.kind = _ops()[which].kind
        refused(zero, 1, -1, names[which])                           # an all-zero op is refused by name


def test_c_refusals_leave_outputs_untouched_on_the_host_side():
    """The refusals above return before the launcher is entered; here the same with real host buffers standing in for the outputs:
    a refused QUERY does not write them."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    bufs = [np.full(64, 0x5A5A5A5A, np.int32) for _ in range(3)]
    for path, value in (("_rsv", 17), ("cout", 0), ("x.h", 0), ("x2.sn", 8), ("kh", 5000)):
        op = _ops()[1]
        op.y.base, op.y2.base, op.res.base = (b.ctypes.data for b in bufs)
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert all((b == 0x5A5A5A5A).all() for b in bufs)

"""CPU: hover_net_amd/clusters.py's host path against the O(N^2) oracle tests/clusters_ref.py on every case the GPU tests run, sklearn's
DBSCAN where it is comparable, the derived forms (`annotate`, `summarise`, `resolve`), the Python refusals and the C refusals of
HVN_OP_NBR_CLUSTER, which the library decides before any launch."""
import ctypes
import json

import numpy as np
import pytest
import torch

import clusters_ref as R
from hover_net_amd import clusters as CL
from hover_net_amd import neighbours as NB


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_equals_oracle(name):
    args, want = R.case(name)
    R.assert_case_facts(name, want)
    got = CL.cluster_host(*args)
    R.assert_same(got, want, name)
    R.assert_case_facts(name, got)
    if args[0].shape[0] <= 2000:
        R.assert_same(CL.cluster(*args, device=None), want, name)


def test_host_path_does_not_depend_on_the_round_size(monkeypatch):
    monkeypatch.setattr(CL, "_PAIRS", 1000)          # hundreds of rounds instead of one: clusters are united across rounds
    for name in ("random", "snake", "typed"):
        args, want = R.case(name)
        R.assert_same(CL.cluster_host(*args), want, name)


def test_host_path_in_reversed_order():
    """Reversing the rows reverses the positions; the oracle of the reversed input is the reference (roots are smallest POSITIONS, so
    the labels are not simply mirrored)."""
    for name in ("random", "bridge", "slide"):
        (xy, types, r, m, of), _ = R.case(name)
        rxy = np.ascontiguousarray(xy[::-1])
        R.assert_same(CL.cluster_host(rxy, types, r, m, of), R.cluster(rxy, types, r, m, of), name)


def test_d2_and_r2_are_those_of_neighbours():
    (xy, _t, r, _m, _of), want = R.case("lattice_m5")
    d2 = NB.d2_of(xy[:, None, 0], xy[:, None, 1], xy[None, :, 0], xy[None, :, 1])
    assert (d2 == R.NR.d2_matrix(xy)).all() and NB.r2_of(r) == 25.0
    assert ((d2 <= NB.r2_of(r)).sum(1) == want["degree"]).all()      # the point itself is on the diagonal


def test_cores_and_their_partition_equal_sklearn_dbscan():
    """On the random case no pair is within 1e-4 of the radius (asserted in the case's facts), so sklearn's sqrt and its <= decide every
    pair as this module does: the core sets, the partition of the cores and the noise sets are equal.  Border labels are not compared:
    sklearn gives a border point to the cluster that reached it first, this module to its nearest core."""
    sk = pytest.importorskip("sklearn.cluster")
    (xy, _t, r, m, _of), want = R.case("random")
    R.assert_case_facts("random", want)
    db = sk.DBSCAN(eps=r, min_samples=m).fit(xy)
    core = want["degree"] >= m
    assert sorted(db.core_sample_indices_.tolist()) == np.nonzero(core)[0].tolist()
    assert ((db.labels_ < 0) == (want["label"] < 0)).all()
    ours, theirs = want["label"][core], db.labels_[core]
    pairs = set(zip(ours.tolist(), theirs.tolist()))
    assert len(pairs) == len(set(ours.tolist())) == len(set(theirs.tolist())) == 54      # a bijection between the two namings
    border = ~core & (want["label"] >= 0)
    to_ours = {t: o for o, t in pairs}
    differ = sum(1 for o, t in zip(want["label"][border].tolist(), db.labels_[border].tolist()) if to_ours[t] != o)
    print("border points whose cluster differs from sklearn's: %d of %d" % (differ, int(border.sum())))


# -- annotate, summarise, resolve ----------------------------------------------------------------------------
def _hand_dict(typed=True):
    """Labels neither contiguous nor sorted; dict order is the position order.  40 and 12 coincide; 7 is 5 away from both; 1000 is at
    exactly 5.5 from both and sqrt(11.25) from 7; 3 is far away."""
    pts = {40: (10.0, 10.0, 1), 7: (13.0, 14.0, 0), 1000: (10.0, 15.5, 1), 3: (60.0, 60.0, 2), 12: (10.0, 10.0, 0)}
    return {lab: {"bbox": np.zeros((2, 2), np.int64), "centroid": np.array([x, y]), "contour": None, "type_prob": None,
                  "type": t if typed else None} for lab, (x, y, t) in pts.items()}


def test_annotate_hand_made_dict():
    info = _hand_dict()
    out = CL.annotate(info, 5.5, 4, 3)
    assert out is info and list(out) == [40, 7, 1000, 3, 12]
    c = {lab: e["cluster"] for lab, e in out.items()}
    # 40, 7, 1000 and 12 are pairwise within 5.5 (1000 is at exactly 5.5 from 40 and 12): degree 4 each, one cluster rooted at position 0
    assert c[40] == {"id": 40, "core": True, "degree": 4} and c[7] == c[1000] == c[12] == c[40]
    assert c[3] == {"id": None, "core": False, "degree": 1}
    for e in c.values():
        assert json.loads(json.dumps(e)) == e and type(e["core"]) is bool and type(e["degree"]) is int
    assert set(out[40]) == {"bbox", "centroid", "contour", "type_prob", "type", "cluster"}
    # of types 1 only: 40 and 1000 are selected and 5.5 apart; with m = 2 both are cores; everything else is unselected
    c = {lab: e["cluster"] for lab, e in CL.annotate(_hand_dict(), 5.5, 2, 3, of_types=[1]).items()}
    assert c[40] == c[1000] == {"id": 40, "core": True, "degree": 2}
    assert c[7] == c[12] == c[3] == {"id": None, "core": False, "degree": 0}
    # a border: m = 3 over types {0, 1} at radius 5.2: 40 and 12 see each other and 7 (degree 3), 7 sees all three (4), 1000 only 7 (2)
    c = {lab: e["cluster"] for lab, e in CL.annotate(_hand_dict(), 5.2, 3, 3, of_types=(0, 1)).items()}
    assert c[1000] == {"id": 40, "core": False, "degree": 2} and c[7] == {"id": 40, "core": True, "degree": 4}


def test_annotate_untyped_and_empty():
    info = CL.annotate(_hand_dict(typed=False), 5.5, 4, None)
    assert info[40]["cluster"] == {"id": 40, "core": True, "degree": 4} and info[3]["cluster"]["id"] is None
    empty = {}
    assert CL.annotate(empty, 5.0, 3, 5) is empty and empty == {}
    with pytest.raises(ValueError):
        CL.annotate(_hand_dict(typed=False), 5.5, 4, 3)                  # nr_types given, entries untyped
    with pytest.raises(ValueError):
        CL.annotate(_hand_dict(), 5.5, 4, 2)                             # a type outside [0, 2)
    with pytest.raises(ValueError):
        CL.annotate(_hand_dict(typed=False), 5.5, 4, None, of_types=[1])  # of_types without types


def test_annotate_equals_cluster_on_a_case_and_save_json_passes_it_through(tmp_path):
    from hover_net_amd import io_utils

    (xy, types, r, m, of), want = R.case("typed")
    labels = [3 * i + 5 for i in range(xy.shape[0])][::-1]
    info = {lab: {"centroid": xy[i], "type": int(types[i])} for i, lab in enumerate(labels)}
    CL.annotate(info, r, m, 5, of)
    for i in range(0, xy.shape[0], 37):
        e = info[labels[i]]["cluster"]
        lab = int(want["label"][i])
        assert e == {"id": labels[lab] if lab >= 0 else None, "core": bool(want["degree"][i] >= m), "degree": int(want["degree"][i])}
    io_utils.save_json(str(tmp_path / "a.json"), info)
    nuc = json.load(open(tmp_path / "a.json"))["nuc"]
    assert all(nuc[str(lab)]["cluster"] == e["cluster"] for lab, e in info.items())


def test_summarise():
    info = CL.annotate(_hand_dict(), 5.5, 4, 3)
    s = CL.summarise(info)
    assert s == {40: {"size": 4, "n_core": 4, "type_count": [2, 2, 0], "bbox": [[10.0, 10.0], [13.0, 15.5]], "centroid": [10.75, 12.375]}}
    assert json.loads(json.dumps(s[40])) == s[40]
    assert CL.summarise(info, nr_types=5)[40]["type_count"] == [2, 2, 0, 0, 0]
    assert CL.summarise(CL.annotate(_hand_dict(typed=False), 5.5, 4, None))[40]["type_count"] is None
    assert CL.summarise(CL.annotate(_hand_dict(), 5.5, 5, 3)) == {}      # nobody reaches degree 5: no cluster
    (xy, types, r, m, of), want = R.case("random")
    info = CL.annotate({i + 1: {"centroid": xy[i], "type": None} for i in range(xy.shape[0])}, r, m, None)
    s = CL.summarise(info)
    core = want["degree"] >= m
    assert len(s) == 54 and sum(v["size"] for v in s.values()) == 1613 + 271 and sum(v["n_core"] for v in s.values()) == 1613
    big = max(s, key=lambda k: s[k]["size"])
    mem = want["label"] == big - 1
    assert s[big]["size"] == 445 == int(mem.sum()) and s[big]["n_core"] == int((mem & core).sum())
    assert s[big]["bbox"] == [xy[mem].min(0).tolist(), xy[mem].max(0).tolist()] and s[big]["centroid"] == xy[mem].mean(0).tolist()


def test_resolve():
    assert CL.resolve(None) is None and CL.resolve({"radius": 50, "min_pts": 5}) == (50.0, 5, None)
    assert CL.resolve({"radius": 2.5, "min_pts": 1, "types": [3, 1, 3]}) == (2.5, 1, (1, 3))
    assert CL.resolve({"radius": 2.5, "min_pts": 1, "types": None}) == (2.5, 1, None)
    for bad in ({"radius": 50}, {"min_pts": 5}, {"radius": 50, "min_pts": 5, "k": 3}, (50, 5), "50", {"radius": 0, "min_pts": 5},
                {"radius": 5, "min_pts": 0}, {"radius": 5, "min_pts": (1 << 26) + 1}, {"radius": 5, "min_pts": 2, "types": []},
                {"radius": 5, "min_pts": 2, "types": [16]}, {"radius": 5, "min_pts": 2, "types": [-1]}):
        with pytest.raises(ValueError):
            CL.resolve(bad)
    for bad in ({"radius": 5, "min_pts": 2.5}, {"radius": "5", "min_pts": 2}, {"radius": 5, "min_pts": 2, "types": 3},
                {"radius": 5, "min_pts": 2, "types": [1.0]}, {"radius": 5, "min_pts": True}):
        with pytest.raises(TypeError):
            CL.resolve(bad)
    with pytest.raises(ValueError):
        CL.resolve({"radius": 5, "min_pts": 2, "types": [1]}, typed=False)
    assert CL.resolve({"radius": 5, "min_pts": 2}, typed=False) == (5.0, 2, None)


# -- refusals ----------------------------------------------------------------------------------------------
GOOD = dict(xy=np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.5]]), types=np.array([0, 1, 1], np.int32), radius=2.0, min_pts=2, of_types=(1,))

BAD = [("xy", np.zeros((3, 2), np.float32), TypeError), ("xy", [[0.0, 0.0]], TypeError), ("xy", np.zeros((3, 3)), ValueError),
       ("xy", np.zeros(6), ValueError), ("xy", np.zeros((0, 2)), ValueError), ("xy", np.array([[0.0, np.nan], [1.0, 1.0], [2.0, 2.0]]), ValueError),
       ("xy", np.array([[0.0, np.inf], [1.0, 1.0], [2.0, 2.0]]), ValueError), ("xy", np.array([[-1.0e308, 0.0], [1.0e308, 1.0], [2.0, 2.0]]), ValueError),
       ("types", np.array([0, 1, 1], np.int64), TypeError), ("types", [0, 1, 1], TypeError), ("types", np.array([0, 1], np.int32), ValueError),
       ("types", np.array([0, 16, 1], np.int32), ValueError), ("types", np.array([0, -1, 1], np.int32), ValueError), ("types", None, ValueError),
       ("radius", 0.0, ValueError), ("radius", -1.0, ValueError), ("radius", np.nan, ValueError), ("radius", np.inf, ValueError),
       ("radius", 1.0e200, ValueError), ("radius", 1.0e-200, ValueError), ("radius", "2", TypeError), ("radius", True, TypeError),
       ("min_pts", 0, ValueError), ("min_pts", -3, ValueError), ("min_pts", (1 << 26) + 1, ValueError), ("min_pts", 2.0, TypeError),
       ("min_pts", True, TypeError), ("of_types", (), ValueError), ("of_types", (16,), ValueError), ("of_types", (-1, 1), ValueError),
       ("of_types", 1, TypeError), ("of_types", (1.0,), TypeError), ("of_types", "1", TypeError)]


@pytest.mark.parametrize("field,value,exc", BAD, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BAD)])
def test_python_refusals_precede_any_work(field, value, exc, monkeypatch):
    """Both paths refuse in `_check`: before the grid is chosen and, for the device form, before anything is allocated or launched
    (`types` = None with `of_types` given is one of them)."""
    from hover_net_amd import lib as L

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(L, "lib", no_launch)
    monkeypatch.setattr(L, "call", no_launch)
    monkeypatch.setattr(NB, "grid", no_launch)
    args = dict(GOOD, **{field: value})
    for fn in (CL.cluster_host, CL.cluster_device, CL.cluster):
        with pytest.raises(exc):
            fn(args["xy"], args["types"], args["radius"], args["min_pts"], args["of_types"])


def test_type_mask_and_workspace():
    assert CL.type_mask(None) == -1 and CL.type_mask((1, 3)) == 0b1010 and CL.type_mask((0, 15)) == 0x8001
    assert CL.cluster_workspace_bytes(1000) == 12000


def _op():
    """A well-formed CLUSTER op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.x.h = PL.OP_NBR_CLUSTER, ncy, ncx, n
    op.w, op.x2.base, op.x2.sn = P(1), P(2), NB.workspace_bytes(n, ncy * ncx)
    op.cout, op.groups = 4, -1
    op.y.base, op.y2.base, op.res.base, op.res.sn = P(5), P(6), P(7), CL.cluster_workspace_bytes(n)
    return op


# one entry per refusal that include/hvn.h lists for NBR_CLUSTER: (field, value, status)
CLUSTER_REFUSALS = [("y.base", None, -1), ("y2.base", None, -1), ("res.base", None, -1), ("y.base", 0x15000002, -1), ("y2.base", 0x16000001, -1),
                    ("res.base", 0x17000004, -1), ("cout", 0, -1), ("cout", -7, -1), ("groups", 0, -1), ("cout", (1 << 26) + 1, -4),
                    ("res.sn", 11999, -4), ("res.sn", 0, -4)]
SHARED_REFUSALS = [("w", None, -1), ("x2.base", None, -1), ("w", 0x11000004, -1), ("x2.base", 0x12000004, -1), ("x.h", 0, -1), ("x.h", -5, -1),
                   ("kh", 0, -1), ("kw", -1, -1), ("x.h", (1 << 26) + 1, -4), ("kh", 4097, -4), ("kw", 4097, -4), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4),
                   ("x2.sn", 0, -4)]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_CLUSTER list: its status, a text that leads with the op's name, decided before any launch
    (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as tests/test_neighbours_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_cluster:") and b"unknown op kind" not in err, (rc, err)

    for path, value, code in CLUSTER_REFUSALS + SHARED_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 1, code)
    refused(_op(), 2, -1)                                            # batch must be 1
    op = _op()
    op.kh, op.kw = 2049, 2049                                        # each axis allowed, 2^22 cells exceeded
    op.x2.sn = 1 << 40
    refused(op, 1, -4)
    op = _op()
    op.res.sn = 12 * 1000 + 4096                                     # the second workspace has its own formula: NBR_GRID's is not grown
    op.x2.sn = NB.workspace_bytes(1000, 1200) - 1
    refused(op, 1, -4)
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1)                                             # an all-zero op is refused by name


def test_c_refusals_leave_outputs_untouched_on_the_host_side():
    """The refusals above return before the launcher is entered; here the same with real host buffers standing in for the outputs and
    the second workspace: a refused CLUSTER does not write them."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    bufs = [np.full(4096, 0x5A5A5A5A, np.int32) for _ in range(3)]
    for path, value in (("cout", 0), ("groups", 0), ("x.h", 0), ("res.sn", 8), ("x2.sn", 8), ("kh", 5000), ("cout", 1 << 27)):
        op = _op()
        op.y.base, op.y2.base, op.res.base = (b.ctypes.data for b in bufs)
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert all((b == 0x5A5A5A5A).all() for b in bufs)

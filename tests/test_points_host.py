"""CPU: hover_net_amd/points.py, the layer under neighbours.py, clusters.py and density.py -- the points of an instance dict, the
candidate runs and rounds against the all-pairs set, the round boundary, and the pipeline's one resolver."""
import copy

import numpy as np
import pytest

import clusters_ref
import density_ref
import neighbours_ref
from hover_net_amd import clusters as CL
from hover_net_amd import density as DN
from hover_net_amd import neighbours as NB
from hover_net_amd import points as P


# -- from_info -------------------------------------------------------------------------------------------------
def _info():
    """Seven typed entries; labels neither sorted nor contiguous; centroids as arrays, lists and tuples."""
    pts = {31: (np.array([10.0, 10.0]), 1), 4: ([13.0, 14.0], 0), 900: ((10.0, 15.5), 1), 2: (np.array([40.0, 41.0]), 2),
           17: ([10.0, 10.0], 0), 8: ((38.0, 44.5), 2), 5: (np.array([[12.5, 12.0]]), np.int64(1))}
    return {lab: {"centroid": c, "type": t} for lab, (c, t) in pts.items()}


def test_from_info_positions_follow_dict_order():
    labels, xy, types = P.from_info(_info(), 3)
    assert labels == [31, 4, 900, 2, 17, 8, 5]
    assert xy.dtype == np.float64 and xy.tolist() == [[10.0, 10.0], [13.0, 14.0], [10.0, 15.5], [40.0, 41.0], [10.0, 10.0], [38.0, 44.5], [12.5, 12.0]]
    assert types.dtype == np.int32 and types.tolist() == [1, 0, 1, 2, 0, 2, 1]
    labels, xy2, types = P.from_info(_info(), None)
    assert types is None and labels == [31, 4, 900, 2, 17, 8, 5] and (xy2 == xy).all()


def test_from_info_refusals():
    untyped = {lab: dict(e, type=None) for lab, e in _info().items()}
    with pytest.raises(ValueError, match="needs an integer type on every entry"):
        P.from_info(untyped, 3)
    for bad in (True, 1.0, "1"):
        info = _info()
        info[2]["type"] = bad
        with pytest.raises(ValueError, match="needs an integer type on every entry"):
            P.from_info(info, 3)
    with pytest.raises(ValueError, match=r"types outside \[0, 2\)"):
        P.from_info(_info(), 2)
    info = _info()
    info[2]["type"] = -1
    with pytest.raises(ValueError, match=r"types outside \[0, 3\)"):
        P.from_info(info, 3)


def test_the_three_modules_see_the_points_of_from_info():
    labels, xy, types = P.from_info(_info(), 3)
    r = 5.5
    want = neighbours_ref.query(xy, types, r, 3, 3)
    got = NB.annotate(copy.deepcopy(_info()), r, 3, 3)
    for i, lab in enumerate(labels):
        e = got[lab]["neighbours"]
        assert e["count"] == want["count"][i].tolist()
        assert e["knn"] == [labels[j] for j in want["knn"][i] if j >= 0]
        assert e["nearest_of_type"] == [labels[j] if j >= 0 else None for j in want["nearest_of_type"][i]]
    assert sum(len(got[lab]["neighbours"]["knn"]) for lab in labels) > 0
    want = clusters_ref.cluster(xy, types, r, 3, (0, 1))
    got = CL.annotate(copy.deepcopy(_info()), r, 3, 3, (0, 1))
    for i, lab in enumerate(labels):
        e = got[lab]["cluster"]
        assert e["degree"] == int(want["degree"][i]) and e["id"] == (labels[want["label"][i]] if want["label"][i] >= 0 else None)
    assert (want["label"] >= 0).any() and (want["label"] < 0).any()
    size = (50, 48)
    dm = DN.of_info(_info(), size, r, 4, 3)
    want = density_ref.density(xy, types, r, DN.raster_of(size, 4), 3)
    assert dm.count.dtype == np.int32 and dm.count.shape == want.shape and (dm.count == want).all() and want.sum() > 0


# -- candidate_runs, pair_rounds, round_end --------------------------------------------------------------------
def _border_points():
    """40 points on a grid of 3 x 3 cells for r = 10: the middle grid row is empty, so every point sits in a border cell; the extent's
    corners are points, and several coincide."""
    rng = np.random.default_rng(7)
    top = np.stack([rng.uniform(0.0, 25.0, 18), rng.uniform(0.0, 9.5, 18)], 1)
    bottom = np.stack([rng.uniform(0.0, 25.0, 16), rng.uniform(21.0, 25.0, 16)], 1)
    fixed = np.array([[0.0, 0.0], [25.0, 25.0], [25.0, 0.0], [0.0, 25.0], [12.0, 9.5], [12.0, 9.5]])
    return np.ascontiguousarray(np.concatenate([top, bottom, fixed]))


def test_rounds_yield_the_all_pairs_set_once():
    xy, r = _border_points(), 10.0
    assert xy.shape == (40, 2)
    g = P.grid(xy, r)
    order, lo, hi, cx, cy = P.candidate_runs(xy, g)
    assert (g.ncx, g.ncy) == (3, 3) and sorted(set(cy.tolist())) == [0, 2] and sorted(set(cx.tolist())) == [0, 1, 2]
    assert sorted(order.tolist()) == list(range(40)) and (np.diff((cy * g.ncx + cx)[order]) >= 0).all()
    r2 = P.r2_of(r)
    sx, sy = xy[order, 0], xy[order, 1]
    seen, rounds, queries = [], 0, []
    for a, b, qi, cand, d2 in P.pair_rounds(sx, sy, lo, hi, r2, 5):
        assert 0 <= a < b <= 40 and ((qi >= a) & (qi < b)).all() and (d2 <= r2).all()
        assert (d2 == P.d2_of(sx[qi], sy[qi], sx[cand], sy[cand])).all()
        queries += list(range(a, b))
        seen += list(zip(order[qi].tolist(), order[cand].tolist()))
        rounds += 1
    assert queries == list(range(40)) and rounds > 20          # every query in exactly one round, and many rounds
    want = {(int(i), int(j)) for i, j in np.argwhere(neighbours_ref.d2_matrix(xy) <= r2)}
    assert len(seen) == len(set(seen)) and set(seen) == want
    assert all((i, i) in want for i in range(40)) and len(want) > 40


def test_round_end():
    sizes = np.array([3, 0, 4, 20, 1, 1, 0, 0, 9, 2])
    ends = np.cumsum(sizes)
    a, got = 0, []
    while a < sizes.shape[0]:
        b = P.round_end(ends, a, 5)
        assert b >= a + 1
        got.append((a, b))
        a = b
    assert got == [(0, 2), (2, 3), (3, 4), (4, 8), (8, 9), (9, 10)]      # 20 and 9 exceed 5: rounds of their own
    assert P.round_end(ends, 0, 1 << 22) == 10 and P.round_end(np.array([7]), 0, 5) == 1


# -- resolve_specs ---------------------------------------------------------------------------------------------
def test_resolve_specs():
    s = P.resolve_specs(None, None, None, typed=False)
    assert s == (None, None, None) and not s.any_annotation
    s = P.resolve_specs({"radius": 50, "k": 5}, {"radius": 30.0, "min_pts": 4, "types": [2, 0]}, {"radius": 80, "step": 16}, typed=True)
    assert s.neighbours == (50.0, 5) and s.clusters == (30.0, 4, (0, 2)) and s.density == (80.0, 16) and s.any_annotation
    assert not P.resolve_specs(density={"radius": 80, "step": 16}).any_annotation
    assert P.resolve_specs(clusters={"radius": 3, "min_pts": 2}, typed=False).any_annotation
    for kw, mod in (("neighbours", NB), ("clusters", CL), ("density", DN)):
        good = {"neighbours": {"radius": 5, "k": 2}, "clusters": {"radius": 5, "min_pts": 2}, "density": {"radius": 5, "step": 2}}[kw]
        second = [k for k in good if k != "radius"][0]
        for bad in ({"radius": 5}, (5, 2), dict(good, radius=0), dict(good, radius="5"), dict(good, **{second: 2.5}), dict(good, **{second: 0})):
            with pytest.raises((ValueError, TypeError)) as own:
                mod.resolve(bad)
            with pytest.raises(own.type) as ours:
                P.resolve_specs(**{kw: bad})
            assert str(ours.value) == str(own.value)
    with pytest.raises(ValueError, match="needs a model with a type branch"):
        P.resolve_specs(clusters={"radius": 5, "min_pts": 2, "types": [1]}, typed=False)

"""CPU: hover_net_amd/points.py, the layer under neighbours.py, clusters.py, density.py, ripley.py and regions.py -- the points of an
instance dict, the shared validators, the candidate runs and rounds against the all-pairs set, the round boundary, and the pipeline's one
resolver and one table of summaries, alone and through the two managers."""
import copy
import json
import os

import numpy as np
import pytest

import clusters_ref
import density_ref
import neighbours_ref
from hover_net_amd import clusters as CL
from hover_net_amd import density as DN
from hover_net_amd import neighbours as NB
from hover_net_amd import points as P
from hover_net_amd import regions as RG
from hover_net_amd import ripley as RP


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
    s = P.resolve_specs(None, None, None, None, None, typed=False)
    assert s == (None, None, None, None, None) and s._fields == P.ARGS and not s.any_annotation
    s = P.resolve_specs({"radius": 50, "k": 5}, {"radius": 30.0, "min_pts": 4, "types": [2, 0]}, {"radius": 80, "step": 16}, typed=True)
    assert s.neighbours == (50.0, 5) and s.clusters == (30.0, 4, (0, 2)) and s.density == (80.0, 16) and s.any_annotation
    assert not P.resolve_specs(density={"radius": 80, "step": 16}).any_annotation
    assert P.resolve_specs(clusters={"radius": 3, "min_pts": 2}, typed=False).any_annotation
    rect = [[[(0, 0), (8, 0), (8, 8), (0, 8)]]]
    s = P.resolve_specs(ripley={"radii": [4, 6.0], "window": (0, 0, 9, 9)}, regions={"regions": [rect]})
    assert s.ripley == ((4.0, 6.0), (0.0, 0.0, 9.0, 9.0)) and isinstance(s.regions, RG.RegionSet) and len(s.regions) == 1 and not s.any_annotation
    assert s[:3] == (None, None, None)
    for kw, mod in (("neighbours", NB), ("clusters", CL), ("density", DN), ("ripley", RP), ("regions", RG)):
        good = {"neighbours": {"radius": 5, "k": 2}, "clusters": {"radius": 5, "min_pts": 2}, "density": {"radius": 5, "step": 2}}.get(kw)
        if good is None:
            bads = {"ripley": ({"radius": 5}, (5, 2), {"radii": [0]}, {"radii": ["5"]}, {"radii": [5, 5]}, {"radii": [5], "window": (0, 0, 0, 9)}),
                    "regions": ({"region": [rect]}, [rect], {"regions": 5}, {"regions": [rect], "scale": 0}, {"regions": [rect], "scale": "2"}, {"regions": []})}[kw]
        else:
            second = [k for k in good if k != "radius"][0]
            bads = ({"radius": 5}, (5, 2), dict(good, radius=0), dict(good, radius="5"), dict(good, **{second: 2.5}), dict(good, **{second: 0}))
        for bad in bads:
            with pytest.raises((ValueError, TypeError)) as own:
                mod.resolve(bad)
            with pytest.raises(own.type) as ours:
                P.resolve_specs(**{kw: bad})
            assert str(ours.value) == str(own.value)
    with pytest.raises(ValueError, match="needs a model with a type branch"):
        P.resolve_specs(clusters={"radius": 5, "min_pts": 2, "types": [1]}, typed=False)


# -- the five at once ------------------------------------------------------------------------------------------
SIZE = (64, 96)
SPECS = {"neighbours": {"radius": 14.0, "k": 3}, "clusters": {"radius": 9.0, "min_pts": 3, "types": [0, 2]}, "density": {"radius": 12.0, "step": 8},
         "ripley": {"radii": [5.0, 11.0, 20.0]}}
GEOJSON = {"type": "FeatureCollection", "features": [          # two rectangles that overlap in [30, 50] x [20, 40]
    {"type": "Feature", "properties": {"name": "left"}, "geometry": {"type": "Polygon", "coordinates": [[[4, 6], [50, 6], [50, 40], [4, 40], [4, 6]]]}},
    {"type": "Feature", "properties": {"name": "right"}, "geometry": {"type": "Polygon", "coordinates": [[[30, 20], [90, 20], [90, 60], [30, 60]]]}}]}


def _typed_stub():
    """40 nuclei of 3 types on a 64 x 96 image, as `post_proc.process` shapes its entries; labels not contiguous."""
    rng = np.random.default_rng(11)
    info = {}
    for i in range(40):
        x, y = int(rng.integers(3, SIZE[1] - 4)), int(rng.integers(3, SIZE[0] - 4))
        box = np.array([[x - 2, y - 2], [x + 2, y - 2], [x + 2, y + 2], [x - 2, y + 2]], np.int32)
        info[3 * i + 1] = {"bbox": np.array([[y - 2, x - 2], [y + 3, x + 3]]), "centroid": np.array([x + 0.25 * (i % 3), y + 0.5]), "contour": box,
                           "type_prob": 0.5 + 0.01 * i, "type": int(rng.integers(0, 3))}
    return info


def _all_specs(regions={"regions": GEOJSON}):
    return P.resolve_specs(**SPECS, regions=regions, typed=True)


def _same(a, b, where=""):
    """== for the nested dicts, tuples, lists and arrays of entries and results."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (tuple, list)) and not isinstance(a, str):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), where
    else:
        assert type(a) is type(b) and a == b, where


def _each_alone(info, t=3):
    """What every module gives for the stub when it is called alone, each on a fresh copy: the three annotations by label, the three
    summaries."""
    rs = RG.RegionSet.from_geojson(GEOJSON)
    nb = NB.annotate(copy.deepcopy(info), 14.0, 3, t)
    cl = CL.annotate(copy.deepcopy(info), 9.0, 3, t, (0, 2))
    rg = copy.deepcopy(info)
    rc = RG.of_info(rg, rs, t)
    RG.annotate(rg, rc)
    notes = {lab: {"neighbours": nb[lab]["neighbours"], "cluster": cl[lab]["cluster"], "region": rg[lab]["region"]} for lab in info}
    return notes, P.PointResults(DN.of_info(copy.deepcopy(info), SIZE, 12.0, 8, t), RP.of_info(copy.deepcopy(info), SIZE, [5.0, 11.0, 20.0], t), rc)


def _expected_entries(info):
    notes, _ = _each_alone(info)
    return {lab: dict(copy.deepcopy(e), **notes[lab]) for lab, e in info.items()}


def test_all_five_at_once_equal_each_alone():
    info = _typed_stub()
    assert len(info) == 40 and sorted({e["type"] for e in info.values()}) == [0, 1, 2]
    notes, want = _each_alone(info)
    specs = _all_specs()
    got = copy.deepcopy(info)
    assert P.annotate(got, specs, 3, None) is got
    res = P.summaries(got, SIZE, specs, 3, None)
    assert type(res) is P.PointResults and res._fields == ("density", "ripley", "regions")
    for name in res._fields:
        _same(tuple(getattr(res, name)), tuple(getattr(want, name)), name)
    for lab, e in got.items():
        assert list(e) == list(info[lab]) + ["neighbours", "cluster", "region"]
        _same({k: e[k] for k in info[lab]}, info[lab], "entry %d" % lab)
        _same({k: e[k] for k in notes[lab]}, notes[lab], "entry %d" % lab)
    # the cases are not empty ones: neighbours, clusters, both regions and their overlap, counts at every radius
    assert any(e["neighbours"]["knn"] for e in got.values()) and any(e["cluster"]["id"] is not None for e in got.values())
    assert set(res.regions.first.tolist()) == {-1, 0, 1} and res.regions.hits.max() == 2
    assert res.density.count.shape == (3, 8, 12) and res.density.count.sum() > 0 and (res.ripley.pairs.sum((0, 1)) > 0).all()
    off = P.resolve_specs()
    plain = copy.deepcopy(info)
    assert P.annotate(plain, off, 3, None) is plain and P.summaries(plain, SIZE, off, 3, None) == P.PointResults(None, None, None)
    _same(plain, info, "all off")
    assert P.output_dirs(off) == () and P.output_dirs(specs) == ("density", "ripley", "regions") and P.output_dirs(specs._replace(ripley=None)) == ("density", "regions")


def _load_npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs + [""])


def test_managers_write_all_five(tmp_path):
    """Both managers with the GPU call replaced by a stub that annotates as `process_images` / `WsiInference` do."""
    for which in ("tile", "wsi"):
        (tmp_path / which).mkdir()
        _managers_write_all_five(which, tmp_path / which)


def _managers_write_all_five(which, tmp_path):
    from hover_net_amd import infer_manager as im
    from hover_net_amd import io_utils

    inp, ann = tmp_path / "in", tmp_path / "ann"
    inp.mkdir()
    ann.mkdir()
    np.save(inp / "a.npy", np.random.default_rng(1).integers(30, 120, SIZE + (3,), dtype=np.uint8))
    (ann / "a.geojson").write_text(json.dumps(GEOJSON))
    on = [False]

    def stub():
        return P.annotate(_typed_stub(), _all_specs(None) if on[0] else P.resolve_specs(), 3, None)

    method = {"model_args": {"nr_types": 3, "mode": "fast"}, "model_path": None}
    if which == "tile":
        mgr = im.InferManager(method, process_fn=lambda images: [(np.zeros(i.shape[:2], np.int32), stub()) for i in images])
        run, done, json_at = mgr.process_file_list, ["a"], "json/a.json"
    else:
        mgr = im.WsiManager(method, wsi_fn=lambda slide, mask: (None, stub()))
        run, done, json_at = mgr.process_wsi_list, {"a": "done"}, "a.json"
    base = {"input_dir": str(inp)}
    five = dict(SPECS, regions={"dir": str(ann)})
    assert run(dict(base, output_dir=str(tmp_path / "absent"))) == done
    assert run(dict(base, output_dir=str(tmp_path / "none"), **{k: None for k in P.ARGS})) == done
    on[0] = True
    assert run(dict(base, output_dir=str(tmp_path / "five"), **five)) == done
    # all five off: the tree and the json are those of a run that never heard of them
    assert _tree(tmp_path / "none") == _tree(tmp_path / "absent") and (tmp_path / "none" / json_at).read_bytes() == (tmp_path / "absent" / json_at).read_bytes()
    # all five on: exactly the three sub-directories beside what was there, each .npz the module's own of_info, the json the annotated stub
    top = lambda d: set(os.listdir(tmp_path / d))                    # noqa: E731
    assert top("five") - top("absent") == {"density", "ripley", "regions"} and top("absent") <= top("five")
    _, want = _each_alone(_typed_stub())
    assert [os.listdir(tmp_path / "five" / sub) for sub in ("density", "ripley", "regions")] == [["a.npz"]] * 3
    for sub, save in (("density", DN.save), ("ripley", RP.save), ("regions", RG.save)):
        save(tmp_path / ("want_%s.npz" % sub), getattr(want, sub))
        _same(_load_npz(tmp_path / "five" / sub / "a.npz"), _load_npz(tmp_path / ("want_%s.npz" % sub)), sub)
    io_utils.save_json(str(tmp_path / "want.json"), _expected_entries(_typed_stub()), **({"mag": 40} if which == "wsi" else {"mag": None}))
    assert (tmp_path / "five" / json_at).read_bytes() == (tmp_path / "want.json").read_bytes()
    nuc = json.loads((tmp_path / "five" / json_at).read_text())["nuc"]
    assert all(list(e)[-3:] == ["neighbours", "cluster", "region"] for e in nuc.values()) and len(nuc) == 40
    # a bad spec for any one of the five: refused before the output directory exists
    bad = {"neighbours": {"radius": 0, "k": 3}, "clusters": {"radius": 9.0, "min_pts": 2.5}, "density": {"radius": 12.0, "step": 0},
           "ripley": {"radii": [5.0, 5.0]}, "regions": {"dir": str(ann), "scale": 0}}
    assert sorted(bad) == sorted(P.ARGS)
    for k in P.ARGS:
        with pytest.raises((ValueError, TypeError)):
            run(dict(base, output_dir=str(tmp_path / "bad"), **dict(five, **{k: bad[k]})))
        assert not (tmp_path / "bad").exists()


# -- the validators --------------------------------------------------------------------------------------------
def _new_check(xy, types, radius, k, nr_types):
    """The validators of points.py in the order of `neighbours._check`: xy, radius, k, types."""
    xy, r, k = P.check_xy(xy), P.check_radius(radius), NB._check_k(k)
    types, t = P.check_types(types, xy.shape[0], nr_types)
    return xy, types, r, k, t


def test_validators_report_what_check_reported():
    xy = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.5], [7.0, 1.0], [2.0, 9.0]])
    ty = np.array([0, 1, 2, 1, 0], np.int32)
    far, nan = xy.copy(), xy.copy()
    far[0, 0], far[1, 0], nan[2, 1] = 1e308, -1e308, np.nan
    R0 = "radius = 0: it must be positive and its square a normal, finite float64"
    RS = "radius must be a number, got '5'"
    # (xy, types, radius, k, nr_types) -> the exception of `neighbours._check`, literally
    rows = [((xy.astype(np.float32), ty, 3.0, 2, 3), TypeError, "xy must be a float64 numpy array [N, 2], got float32"),
            ((xy.tolist(), ty, 3.0, 2, 3), TypeError, "xy must be a float64 numpy array [N, 2], got list"),
            ((xy.reshape(2, 5), ty, 3.0, 2, 3), ValueError, "xy must be [N, 2] with N >= 1, got (2, 5)"),
            ((xy[:0], ty[:0], 3.0, 2, 3), ValueError, "xy must be [N, 2] with N >= 1, got (0, 2)"),
            ((nan, ty, 3.0, 2, 3), ValueError, "xy holds a coordinate that is not finite"),
            ((far, ty, 3.0, 2, 3), ValueError, "the extent of xy is not a finite float64"),
            ((xy, ty, 0, 2, 3), ValueError, R0),
            ((xy, ty, "5", 2, 3), TypeError, RS),
            ((xy, ty, True, 2, 3), TypeError, "radius must be a number, got True"),
            ((xy, ty, 1e-200, 2, 3), ValueError, "radius = 1e-200: it must be positive and its square a normal, finite float64"),
            ((xy, ty, 3.0, 2.0, 3), TypeError, "k must be an integer, got 2.0"),
            ((xy, ty, 3.0, 17, 3), ValueError, "k = 17 outside 1..16"),
            ((xy, ty[:3], 3.0, 2, 3), ValueError, "types (3,) is not parallel to xy (5, 2)"),
            ((xy, ty.astype(np.int64), 3.0, 2, 3), TypeError, "types must be an int32 numpy array [N] or None, got int64"),
            ((xy, ty + 5, 3.0, 2, 3), ValueError, "types outside [0, 3)"),
            ((xy, ty - 1, 3.0, 2, None), ValueError, "types outside [0, 2)"),
            ((xy, ty, 3.0, 2, 2.0), TypeError, "nr_types must be an integer or None, got 2.0"),
            ((xy, None, 3.0, 2, 17), ValueError, "17 types outside 1..16"),
            ((xy, ty + 5, 0, 2, 3), ValueError, R0),                 # two faults: the radius is reported, not the types
            ((xy, ty[:3], "5", 2, 3), TypeError, RS),
            ((nan, ty, 0, 2, 3), ValueError, "xy holds a coordinate that is not finite"),   # two faults: the points are reported, not the radius
            ((xy, ty + 5, 3.0, 0, 3), ValueError, "k = 0 outside 1..16")]
    for args, exc, text in rows:
        with pytest.raises(exc) as old:
            NB._check(*args)
        with pytest.raises(exc) as new:
            _new_check(*args)
        assert type(old.value) is type(new.value) is exc and str(old.value) == str(new.value) == text, text
    good = NB._check(xy[::-1], ty, 3, 2, None)                        # and what passes comes back the same: contiguous, converted
    _same(tuple(_new_check(xy[::-1], ty, 3, 2, None)), tuple(good))
    assert good[0].flags.c_contiguous and type(good[2]) is float and good[2:] == (3.0, 2, 3)
    _same(P.check_types(None, 5, None), (None, 1))
    # the four other modules: their first fault for the two-fault rows, as they reported it before the validators moved
    rs = RG.RegionSet.from_polygons([[[[(0, 0), (8, 0), (8, 8), (0, 8)]]]])
    raster, window = (0.0, 0.0, 1.0, 4, 4), (0, 0, 10, 10)
    for (r, types), exc, text, text_rg in (((0, ty + 5), ValueError, R0, "types outside [0, 3)"),
                                           (("5", ty[:3]), TypeError, RS, "types (3,) is not parallel to xy (5, 2)")):
        for call in (lambda: DN._check(xy, types, r, raster, 3), lambda: CL._check(xy, types, r, 3, None), lambda: RP._check(xy, types, [r], window, 3),
                     lambda: RP._check(xy, types, [2.0, r], window, 3), lambda: RG._check(xy, types, rs, 3, cell=r)):
            with pytest.raises(exc) as got:
                call()
            assert type(got.value) is exc and str(got.value) == text
        with pytest.raises(ValueError) as got:
            RG._check(xy, types, rs, 3)                              # no cell: nothing but the types is wrong
        assert str(got.value) == text_rg
    for call, text in ((lambda: DN._check(nan, ty, 0, raster, 3), "xy holds a coordinate that is not finite"),
                       (lambda: CL._check(nan, ty, 0, 3, None), "xy holds a coordinate that is not finite"),
                       (lambda: CL._check(xy, ty + 20, 3.0, 0, None), "23 types outside 1..16"),     # types before min_pts
                       (lambda: RP._check(nan, ty, [0], window, 3), R0),                             # radii before the points
                       (lambda: RG._check(nan, ty, rs, 3, cell=0), R0),                              # the cell before the points
                       (lambda: RG._check(nan, ty, [rs], 3, cell=0), "rs must be a RegionSet (RegionSet.from_polygons / from_geojson), got 'list'")):
        with pytest.raises((ValueError, TypeError)) as got:
            call()
        assert str(got.value) == text

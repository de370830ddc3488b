"""CPU: hover_net_amd.metrics (host pair table) against the reference's own metrics/stats_utils.py and compute_stats.py, run live in
a subprocess with the reference first on sys.path and a stub cv2 (build container only: skipped where the reference tree is
absent).  Equality means `==` (NaN equal to NaN), the same container kinds and dtypes, pairing lists equal element by element; an
exception is equal to an exception of the same type."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from hover_net_amd import metrics as M
from hover_net_amd.synth import synth_inst_pair

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "metrics", "stats_utils.py")), reason="needs the reference tree (build container only)")

_RUNNER = r'''
import pickle, sys, types
sys.path.insert(0, sys.argv[3])
sys.modules["cv2"] = types.ModuleType("cv2")
import numpy as np
import metrics.stats_utils as S
assert S.__file__.startswith(sys.argv[3]), S.__file__
calls, maps = pickle.load(open(sys.argv[1], "rb"))
out = []
for fn, names, kw, remap in calls:
    args = [maps[n] for n in names]
    try:
        if remap:
            args = [S.remap_label(a) for a in args]
        out.append(("ok", getattr(S, fn)(*args, **kw)))
    except Exception as e:
        out.append(("raise", type(e).__name__))
pickle.dump(out, open(sys.argv[2], "wb"))
'''


def same(a, b):
    if type(a) is not type(b):
        return False
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if isinstance(a, (float, np.floating)):
        return a == b or (np.isnan(a) and np.isnan(b))
    return bool(a == b)


def ours(fn, args, kw, remap):
    try:
        if remap:
            args = [M.remap_label(a, device="cpu") for a in args]
        return ("ok", getattr(M, fn)(*args, device="cpu", **kw) if fn != "pair_coordinates" else M.pair_coordinates(*args, **kw))
    except Exception as e:
        return ("raise", type(e).__name__)


def run_reference(tmp_path, calls, maps):
    pickle.dump((calls, maps), open(tmp_path / "in.pkl", "wb"))
    r = subprocess.run([sys.executable, "-W", "ignore", "-c", _RUNNER, str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl"), REF],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg"))
    assert r.returncode == 0, r.stderr[-3000:]
    return pickle.load(open(tmp_path / "out.pkl", "rb"))


def map_cases():
    """name -> (true, pred): merges / splits / misses / spurious, odd sizes, ids near the int32 maximum, an AJI tie, empty maps."""
    c = {}
    for i, (h, w, k) in enumerate([(64, 64, 12), (57, 91, 15), (96, 80, 25), (33, 47, 5)]):
        c["rand%d" % i] = synth_inst_pair(h, w, k, seed=10 + i, n_merge=1, n_split=1, n_miss=1, n_spurious=2, shift=(i % 3, 1))
    c["bigids"] = synth_inst_pair(48, 52, 10, seed=3, id_stride=7, id_base=2 ** 31 - 1 - 7 * 12)
    t = np.zeros((10, 12), np.int32)
    t[2:6, 2:8] = 5                                       # one true instance over two preds of equal IoU: argmax tie
    p = np.zeros_like(t)
    p[2:6, 2:5], p[2:6, 5:8] = 9, 4
    c["tie"] = (t, p)
    z = np.zeros((8, 8), np.int32)
    one = z.copy()
    one[3:5, 3:5] = 1
    c["both_empty"], c["true_empty"], c["pred_empty"] = (z, z), (z, one), (one, z)
    return c


@needs_ref
def test_every_function_equals_the_reference(tmp_path):
    cases = map_cases()
    maps, calls = {}, []
    for name, (t, p) in cases.items():
        maps[name + "_t"], maps[name + "_p"] = t, p
        tp = [name + "_t", name + "_p"]
        for fn in ("get_fast_aji", "get_fast_aji_plus", "get_fast_dice_2"):
            calls.append((fn, tp, {}, True))
        for mi in (0.3, 0.5, 0.7):
            calls.append(("get_fast_pq", tp, {"match_iou": mi}, True))
        for fn in ("get_dice_1", "get_dice_2"):
            calls.append((fn, tp, {}, False))
        for side in tp:
            calls.append(("remap_label", [side], {}, False))
            calls.append(("remap_label", [side], {"by_size": True}, False))
    # contiguous ids passed straight to get_fast_* (no remap) and by_size ties (equal areas keep ascending id)
    ties = np.zeros((12, 12), np.int32)
    ties[0:2, 0:2], ties[4:6, 4:6], ties[8:11, 8:11], ties[0:2, 8:10] = 7, 3, 5, 11
    maps["ties"] = ties
    calls += [("remap_label", ["ties"], {"by_size": True}, False), ("remap_label", ["ties"], {}, False)]
    r1, r2 = M.remap_label(cases["rand0"][0], device="cpu"), M.remap_label(cases["rand0"][1], device="cpu")
    maps["c_t"], maps["c_p"] = r1, r2
    calls += [("get_fast_pq", ["c_t", "c_p"], {}, False), ("get_fast_aji", ["c_t", "c_p"], {}, False)]
    ref = run_reference(tmp_path, calls, maps)
    bad = []
    for (fn, names, kw, remap), want in zip(calls, ref):
        got = ours(fn, [maps[n] for n in names], kw, remap)
        if not same(got, want):
            bad.append((fn, names, kw, got, want))
    assert not bad, bad[:3]
    # the reference's behaviour on empty maps, pinned (the table of the metrics issue)
    want = {"both_empty": {"get_fast_pq": "ZeroDivisionError", "get_fast_aji": "ValueError", "get_fast_dice_2": "ZeroDivisionError"},
            "pred_empty": {"get_fast_aji": "ValueError"}}
    for (fn, names, kw, remap), w in zip(calls, ref):
        case = names[0][:-2]
        if case in want and fn in want[case]:
            assert w == ("raise", want[case][fn]), (case, fn, w)


@needs_ref
def test_stacks_mixed_dtypes_and_float_maps_equal_the_reference(tmp_path):
    """A [2, H, W] stack is ONE map to the reference's functions; pred ids keep the pred map's dtype; float maps holding whole
    numbers are scored by remap_label / get_dice_1 / get_dice_2 and make get_fast_* raise TypeError, as in the reference."""
    (t1, p1), (t2, p2) = synth_inst_pair(64, 64, 10, seed=1), synth_inst_pair(64, 64, 12, seed=2)
    maps = {"T": np.stack([t1, t2]), "P": np.stack([p1, p2]), "rt": M.remap_label(t1, device="cpu"),
            "rp64": M.remap_label(p1, device="cpu").astype(np.int64), "tf": t1.astype(np.float64), "pf": p1.astype(np.float64)}
    calls = [("get_dice_1", ["T", "P"], {}, False), ("get_dice_2", ["T", "P"], {}, False), ("remap_label", ["T"], {}, False),
             ("get_fast_pq", ["T", "P"], {}, True), ("get_fast_aji", ["T", "P"], {}, True), ("get_fast_aji_plus", ["T", "P"], {}, True),
             ("get_fast_dice_2", ["T", "P"], {}, True), ("get_fast_pq", ["rt", "rp64"], {}, False),
             ("get_fast_pq", ["rt", "rp64"], {"match_iou": 0.3}, False), ("get_fast_aji", ["rp64", "rt"], {}, False),
             ("remap_label", ["tf"], {}, False), ("remap_label", ["pf"], {"by_size": True}, False), ("get_dice_1", ["tf", "pf"], {}, False),
             ("get_dice_2", ["tf", "pf"], {}, False), ("get_fast_pq", ["tf", "pf"], {}, True)]
    calls += [(fn, ["tf", "pf"], {}, False) for fn in ("get_fast_pq", "get_fast_aji", "get_fast_aji_plus", "get_fast_dice_2")]
    ref = run_reference(tmp_path, calls, maps)
    assert sum(r[0] == "raise" for r in ref) == 4
    for (fn, names, kw, remap), want in zip(calls, ref):
        got = ours(fn, [maps[n] for n in names], kw, remap)
        assert same(got, want), (fn, names, kw, got, want)


@needs_ref
def test_pair_coordinates_equals_the_reference(tmp_path):
    a = np.array([[0, 0], [10, 0], [0, 10], [30, 30], [5, 5]], np.float32)
    b = np.array([[5, 0], [0, 5], [30, 42], [100, 100], [5, 5], [10, 5]], np.float32)   # equal distances; |(30,30)-(30,42)| == 12
    rng = np.random.default_rng(0)
    c, d = rng.integers(0, 60, (40, 2)).astype(np.float32), rng.integers(0, 60, (37, 2)).astype(np.float32)
    maps = {"a": a, "b": b, "c": c, "d": d, "e": np.zeros((0, 2), np.float32)}
    calls = [("pair_coordinates", ["a", "b"], {"radius": 12}, False), ("pair_coordinates", ["b", "a"], {"radius": 5}, False),
             ("pair_coordinates", ["c", "d"], {"radius": 12}, False), ("pair_coordinates", ["c", "d"], {"radius": 3}, False)]
    ref = run_reference(tmp_path, calls, maps)
    for (fn, names, kw, _), want in zip(calls, ref):
        got = ours(fn, [maps[n] for n in names], kw, False)
        assert same(got, want), (names, kw, got, want)


def _write_mat_dirs(root, cases):
    import scipy.io as sio

    from hover_net_amd.metrics import remap_label

    os.makedirs(root / "true", exist_ok=True)
    os.makedirs(root / "pred", exist_ok=True)
    rng = np.random.default_rng(5)
    for k, (name, (t, p)) in enumerate(cases.items()):
        for sub, m in (("true", t), ("pred", p)):
            r = remap_label(m, device="cpu")
            ids = np.unique(r)[1:]
            cen = np.array([np.argwhere(r == i).mean(0)[::-1] for i in ids], np.float64).reshape(-1, 2)
            typ = rng.integers(1, 4, (len(ids), 1)).astype(np.int32)
            sio.savemat(str(root / sub / ("img%02d_%s.mat" % (k, name))), {"inst_map": m, "inst_centroid": cen, "inst_type": typ})


_CS_RUNNER = r'''
import io, contextlib, pickle, sys, types
sys.path[:0] = sys.argv[2].split(":")
sys.modules["cv2"] = types.ModuleType("cv2")
import compute_stats, metrics.stats_utils as S
assert compute_stats.__file__.startswith(sys.argv[3]), compute_stats.__file__
out = {"metrics_from": S.__file__}
for mode in ("inst", "type"):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        if mode == "inst":
            r = compute_stats.run_nuclei_inst_stat(sys.argv[1] + "/pred", sys.argv[1] + "/true", print_img_stats=True)
        else:
            r = compute_stats.run_nuclei_type_stat(sys.argv[1] + "/pred/", sys.argv[1] + "/true/")
    out[mode] = (r, buf.getvalue())
pickle.dump(out, sys.stdout.buffer)
'''


@needs_ref
def test_compute_stats_with_the_shim_equals_the_reference(tmp_path, capsys):
    """The reference's compute_stats.py, unmodified: with its own metrics, then with this repository's `metrics` shim ahead on
    sys.path; and hover_net_amd.compute_stats.  Arrays and stdout equal."""
    import contextlib
    import io

    from hover_net_amd import compute_stats as CS

    cases = {k: v for k, v in map_cases().items() if k not in ("both_empty", "pred_empty")}
    _write_mat_dirs(tmp_path, cases)
    res = {}
    for tag, path in (("ref", REF), ("shim", REPO + ":" + REF)):
        r = subprocess.run([sys.executable, "-W", "ignore", "-c", _CS_RUNNER, str(tmp_path), path, REF], capture_output=True, timeout=900,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        res[tag] = pickle.loads(r.stdout)
    assert res["ref"]["metrics_from"].startswith(REF) and res["shim"]["metrics_from"].startswith(os.path.join(REPO, "metrics"))
    for mode in ("inst", "type"):
        assert same(res["shim"][mode][0], res["ref"][mode][0]), mode
        assert res["shim"][mode][1] == res["ref"][mode][1], (res["shim"][mode][1], res["ref"][mode][1])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = CS.run_nuclei_inst_stat(str(tmp_path / "pred"), str(tmp_path / "true"), print_img_stats=True, device="cpu")
    assert same(got, res["ref"]["inst"][0]) and buf.getvalue() == res["ref"]["inst"][1]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = CS.run_nuclei_type_stat(str(tmp_path / "pred") + "/", str(tmp_path / "true") + "/")
    assert got is None and buf.getvalue() == res["ref"]["type"][1]


def test_undefined_inputs_raise_value_error():
    t, p = synth_inst_pair(40, 40, 8, seed=1)
    for fn in (M.get_fast_pq, M.get_fast_aji, M.get_fast_aji_plus, M.get_fast_dice_2):
        with pytest.raises(ValueError):
            fn(t * 2, M.remap_label(p, device="cpu"), device="cpu")          # non-contiguous ids
        with pytest.raises(ValueError):
            fn(np.ones_like(t), M.remap_label(p, device="cpu"), device="cpu")  # no background
    neg = t.copy()
    neg[0, 0] = -3
    big = t.astype(np.int64)
    big[0, 0] = 2 ** 31
    for fn in (M.get_fast_pq, M.get_fast_aji, M.get_fast_aji_plus, M.get_fast_dice_2, M.get_dice_1, M.get_dice_2):
        for bad in (neg, big):
            with pytest.raises(ValueError):
                fn(bad, p, device="cpu")
    for bad in (neg, big, np.ones_like(t)):
        with pytest.raises(ValueError):
            M.remap_label(bad, device="cpu")
    z = np.zeros((5, 5), np.int32)
    assert M.remap_label(z, device="cpu") is z                             # no label: the input itself


def test_instance_stats_rows_equal_the_single_functions():
    pairs = [synth_inst_pair(h, w, k, seed=s) for s, (h, w, k) in enumerate([(64, 64, 10), (64, 64, 14), (50, 70, 9)])]
    rows = M.instance_stats([t for t, _ in pairs], [p for _, p in pairs], device="cpu")
    for (t, p), row in zip(pairs, rows):
        rt, rp = M.remap_label(t, device="cpu"), M.remap_label(p, device="cpu")
        dq, sq, pq = M.get_fast_pq(rt, rp, device="cpu")[0]
        want = [M.get_dice_1(rt, rp, device="cpu"), M.get_fast_aji(rt, rp, device="cpu"), dq, sq, pq, M.get_fast_aji_plus(rt, rp, device="cpu")]
        assert row.tolist() == [float(v) for v in want]
    tabs = M.pair_tables([t for t, _ in pairs], [p for _, p in pairs], device="cpu")
    for (t, p), tab in zip(pairs, tabs):
        assert np.array_equal(tab.triples, M.host_triples(t, p))
        ids, areas = tab.true_areas()
        u, c = np.unique(t, return_counts=True)
        assert np.array_equal(ids, u) and np.array_equal(areas, c)


def test_refimport_evicts_the_metrics_shim():
    """oracle/refimport.py: with the repository root first, `metrics.stats_utils` is the shim; after use_reference() it is the reference's."""
    if not os.path.isdir(os.path.join(REF, "metrics")):
        pytest.skip("needs the reference tree (build container only)")
    code = ("import sys, types; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "sys.modules.setdefault('cv2', types.ModuleType('cv2'))\n"
            "import metrics.stats_utils as shim\n"
            "assert shim.__file__.startswith(%r), shim.__file__\n"
            "sys.path.insert(0, %r)\n"
            "from refimport import ref_import, use_reference\n"
            "use_reference()\n"
            "m = ref_import('metrics.stats_utils')\n"
            "assert m.__file__.startswith('/root/reference/'), m.__file__\n"
            "print('ok')\n") % (REF, REPO, os.path.join(REPO, "metrics"), os.path.join(REPO, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_shim_does_not_import_cv2_or_matplotlib():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import metrics.stats_utils, hover_net_amd.compute_stats\n"
            "bad = [m for m in ('cv2', 'matplotlib', 'pandas') if m in sys.modules]\n"
            "assert not bad, bad\nprint('ok')\n") % REPO
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]

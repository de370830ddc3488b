"""CPU: the random-labelling test of hover_net_amd/ripley.py -- the permutation against the scalar oracle tests/ripley_sims_ref.py,
`sims_host` against the all-pairs oracle per labelling on every case the GPU tests run, its invariants and its unbiasedness, the
statistics (`K_sims`, `envelope`, `p_value`), the pipeline (`resolve`, `of_info`, `save`, the managers), the Python refusals and the C
refusals of HVN_OP_NBR_PAIRS_SIM, which the library decides before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import ripley_ref as R
import ripley_sims_ref as SR
from hover_net_amd import neighbours as NB
from hover_net_amd import ripley as RP

SIZES = [1, 2, 3, 4, 5, 64, 65, 1024, 1025, 4097]


# -- the permutation -----------------------------------------------------------------------------------------
def test_round_keys_equal_the_scalar_reference():
    for seed in (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1):
        keys = RP.round_keys(seed, 5)
        assert keys.dtype == np.uint64 and keys.shape == (5, 8)
        assert [[int(v) for v in row] for row in keys] == [SR.keys(seed, s) for s in range(5)]
    assert SR.mix(0) == 0 and SR.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF            # the first output of splitmix64 seeded with 0


@pytest.mark.parametrize("n", SIZES)
def test_permutation_equals_the_scalar_reference_and_is_one(n):
    for s in range(3):
        want, longest = SR.permutation(n, SR.keys(11, s))
        got, steps = RP._walk(n, RP.round_keys(11, 3)[s])
        assert got.dtype == np.int64 and got.tolist() == want and sorted(want) == list(range(n))
        assert (RP.permutation(n, RP.round_keys(11, 3)[s]) == got).all()
        bound = (1 << max(2, (n - 1).bit_length())) - n + 1
        assert steps == longest <= bound, (n, steps, bound)           # the walk never exceeds 2^b - N + 1


def test_every_ordering_of_four_points_occurs():
    keys = RP.round_keys(3, 2400)
    seen = {tuple(RP.permutation(4, k).tolist()) for k in keys}
    assert len(seen) == 24


# -- sims_host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_host_equals_oracle(name):
    args, want = SR.case(name, 3)
    _, obs = R.case(name)
    got = RP.sims_host(*args, sims=3)
    assert isinstance(got, RP.LabelSims) and isinstance(got.observed, RP.PairCounts) and got.seed == 0
    R.assert_same(got.observed, obs, name)
    SR.assert_same(got, want, name)
    SR.assert_same(RP.sims(*args, sims=3, device=None), want, name)
    t, nr = args[4], len(args[2])
    assert got.pairs_in.shape == (3, t, t, nr) and got.n_in.shape == (3, t, nr)
    if args[1] is None:                                              # T = 1: every simulation is the observed counts
        assert (got.pairs_in == got.observed.pairs_in[None]).all() and (got.n_in == got.observed.n_in[None]).all()
    # a relabelling moves pairs between type bins and keeps their number, and the number of points inside
    assert (got.pairs_in.sum((1, 2)) == got.observed.pairs_in.sum((0, 1))[None]).all()
    assert (got.n_in.sum(1) == got.observed.n_in.sum(0)[None]).all()


def test_simulation_s_does_not_depend_on_S_and_seeds_differ(monkeypatch):
    args, _ = R.case("outside")
    seven, three = RP.sims_host(*args, sims=7, seed=5), RP.sims_host(*args, sims=3, seed=5)
    assert (seven.pairs_in[:3] == three.pairs_in).all() and (seven.n_in[:3] == three.n_in).all() and seven.seed == three.seed == 5
    assert len({a.tobytes() for a in seven.pairs_in}) == 7            # the simulations differ from each other
    other = RP.sims_host(*args, sims=3, seed=6)
    assert (other.pairs_in != three.pairs_in).any() and (other.observed.pairs_in == three.observed.pairs_in).all()
    monkeypatch.setattr(RP, "_HOST_SIMS", 2)                         # chunks of two simulations, the last one short
    monkeypatch.setattr(RP, "_PAIRS", 900)                           # and many rounds
    again = RP.sims_host(*args, sims=7, seed=5)
    assert (again.pairs_in == seven.pairs_in).all() and (again.n_in == seven.n_in).all()


def test_random_labelling_is_unbiased():
    """600 uniform points of 3 types, one radius, S = 199.  Under a uniformly random permutation of the labels an ordered pair (i, j)
    gets the types (a, b) with probability n_a n_b / (N (N - 1)), and n_a (n_a - 1) / (N (N - 1)) for a = b, so the expectation of
    pairs_in[s, a, b] is P_in times that, P_in the pairs of all types.  Each mean over s is held to within 5 of its own standard errors
    (the std over s divided by sqrt(S)); the run is seeded."""
    rng = np.random.default_rng(77)
    xy = rng.random((600, 2)) * 100.0
    types = rng.integers(0, 3, 600).astype(np.int32)
    ls = RP.sims_host(xy, types, (6.0,), (0.0, 0.0, 100.0, 100.0), 3, sims=199, seed=2024)
    n, big = ls.observed.n.astype(np.float64), 600.0
    p_in = float(ls.observed.pairs_in.sum())
    want = p_in * (n[:, None] * n[None, :] - np.diag(n)) / (big * (big - 1.0))
    got = ls.pairs_in[:, :, :, 0].astype(np.float64)
    z = (got.mean(0) - want) / (got.std(0) / np.sqrt(199.0))
    print("largest |z| = %.2f" % np.abs(z).max())
    assert p_in > 3000 and (got.std(0) > 0).all() and (np.abs(z) <= 5.0).all(), z.tolist()


def test_two_separated_clumps_are_significant():
    """Type 0 around (20, 20), type 1 around (80, 80), 30 points each, all well inside the window: no cross pair at r = 8 and every
    within-type pair, which no relabelling reaches -- both p-values are the smallest a test of S simulations can give."""
    rng = np.random.default_rng(5)
    xy = np.concatenate([[20.0, 20.0] + rng.normal(0.0, 2.0, (30, 2)), [80.0, 80.0] + rng.normal(0.0, 2.0, (30, 2))])
    types = np.repeat([0, 1], 30).astype(np.int32)
    ls = RP.sims_host(xy, types, (8.0, 20.0), (0.0, 0.0, 100.0, 100.0), 2, sims=99, seed=1)
    assert ls.observed.pairs_in[0, 1].tolist() == [0, 0] and (ls.pairs_in[:, 0, 1, 0] > 0).all()
    assert RP.p_value(ls, "less")[0, 1, 0] == RP.p_value(ls, "less")[1, 0, 0] == 1.0 / 100.0
    assert RP.p_value(ls, "greater")[0, 0, 0] == RP.p_value(ls, "greater")[1, 1, 0] == 1.0 / 100.0
    assert RP.p_value(ls, "greater")[0, 1, 0] == 1.0 and RP.p_value(ls, "less")[0, 0, 0] == 1.0
    lo, hi = RP.envelope(ls)
    k = RP.K(ls.observed)
    assert k[0, 1, 0] < lo[0, 1, 0] <= hi[0, 1, 0] and k[0, 0, 0] > hi[0, 0, 0] >= lo[0, 0, 0]


# -- K_sims, envelope, p_value -----------------------------------------------------------------------------------
def _hand():
    """S = 3, T = 1, R = 2 in a window of area 10 with n = 4: K = 10 pairs_in / (4 n_in).  Bin 1 of simulation 1 has n_in = 0."""
    obs = RP.PairCounts(np.array([[[5, 7]]], np.int64), np.array([[[4, 6]]], np.int64), np.array([4], np.int64), np.array([[2, 1]], np.int64),
                        np.array([1.0, 2.0]), (0.0, 0.0, 5.0, 2.0))
    return RP.LabelSims(obs, np.array([[[[2, 6]]], [[[4, 2]]], [[[6, 4]]]], np.int64), np.array([[[2, 1]], [[2, 0]], [[1, 1]]], np.int64), 0)


def test_statistics_on_hand_made_counts():
    ls = _hand()
    k = RP.K_sims(ls)
    assert k.shape == (3, 1, 1, 2) and k[:, 0, 0, 0].tolist() == [2.5, 5.0, 15.0] and k[0, 0, 0, 1] == 15.0 and np.isnan(k[1, 0, 0, 1]) and k[2, 0, 0, 1] == 10.0
    assert RP.K(ls.observed).reshape(-1).tolist() == [5.0, 15.0] and RP.K_sims(ls, area=20.0)[0, 0, 0, 0] == 5.0
    lo, hi = RP.envelope(ls)
    assert lo.shape == hi.shape == (1, 1, 2) and lo[0, 0, 0] == 2.5 and hi[0, 0, 0] == 15.0 and np.isnan(lo[0, 0, 1]) and np.isnan(hi[0, 0, 1])
    lo, hi = RP.envelope(ls, rank=2)
    assert lo[0, 0, 0] == hi[0, 0, 0] == 5.0
    lo, hi = RP.envelope(ls, rank=3)
    assert lo[0, 0, 0] == 15.0 and hi[0, 0, 0] == 2.5
    for bad in (0, 4, 1.0):
        with pytest.raises(ValueError):
            RP.envelope(ls, rank=bad)
    pg, pl = RP.p_value(ls, "greater"), RP.p_value(ls, "less")
    assert pg[0, 0, 0] == 0.75 and pl[0, 0, 0] == 0.75 and np.isnan(pg[0, 0, 1]) and np.isnan(pl[0, 0, 1])       # the tie at 5.0 counts on both sides
    with pytest.raises(ValueError):
        RP.p_value(ls, "two-sided")
    nan_obs = ls._replace(observed=ls.observed._replace(n_in=np.array([[0, 1]], np.int64)))
    assert np.isnan(RP.p_value(nan_obs, "greater")[0, 0, 0]) and RP.envelope(nan_obs)[0][0, 0, 0] == 2.5          # the envelope does not read the observed n_in


def test_K_sims_uses_n_in_of_a_and_n_of_b():
    obs = RP.PairCounts(np.zeros((2, 2, 1), np.int64), np.zeros((2, 2, 1), np.int64), np.array([2, 3], np.int64), np.array([[1], [2]], np.int64),
                        np.array([1.0]), (0.0, 0.0, 3.0, 2.0))
    ls = RP.LabelSims(obs, np.array([[[[1], [2]], [[3], [4]]]], np.int64), np.array([[[1], [2]]], np.int64), 0)
    assert RP.K_sims(ls)[0, :, :, 0].tolist() == [[6.0 * 1 / (1 * 2), 6.0 * 2 / (1 * 3)], [6.0 * 3 / (2 * 2), 6.0 * 4 / (2 * 3)]]


# -- resolve, of_info, save ---------------------------------------------------------------------------------------
def test_resolve():
    assert RP.resolve({"radii": [10, 20.5]}) == ((10.0, 20.5), None)                                    # the 2-tuple is unchanged without "sims"
    assert RP.resolve({"radii": [3], "window": (0, 0, 5, 6)}) == ((3.0,), (0.0, 0.0, 5.0, 6.0))
    assert RP.resolve({"radii": [3], "sims": 99}) == ((3.0,), None, 99, 0)
    assert RP.resolve({"radii": [3], "window": (0, 0, 5, 6), "sims": np.int64(9999), "seed": (1 << 64) - 1}) == ((3.0,), (0.0, 0.0, 5.0, 6.0), 9999, (1 << 64) - 1)
    assert RP.resolve({"radii": [3], "sims": 1, "seed": 0}) == ((3.0,), None, 1, 0)
    for bad in ({"radii": [3], "seed": 4}, {"radii": [3], "sims": 0}, {"radii": [3], "sims": 10000}, {"radii": [3], "sims": -1}, {"radii": [3], "sims": 5, "seed": -1},
                {"radii": [3], "sims": 5, "seed": 1 << 64}, {"radii": [3], "sims": 5, "rank": 1}, {"sims": 5}):
        with pytest.raises(ValueError):
            RP.resolve(bad)
    for bad in ({"radii": [3], "sims": 5.0}, {"radii": [3], "sims": True}, {"radii": [3], "sims": None}, {"radii": [3], "sims": "9"}, {"radii": [3], "sims": 5, "seed": 1.5},
                {"radii": [3], "sims": 5, "seed": None}):
        with pytest.raises(TypeError):
            RP.resolve(bad)


def _hand_dict():
    pts = {40: (5.5, 5.5, 1), 7: (7.0, 7.5, 0), 12: (13.0, 8.0, 1), 3: (3.5, 3.5, 2), 8: (6.0, 4.0, 0), 21: (8.0, 5.0, 2)}
    return {lab: {"bbox": np.zeros((2, 2), np.int64), "centroid": np.array([x, y]), "contour": None, "type_prob": None, "type": t} for lab, (x, y, t) in pts.items()}


def test_of_info_save_and_the_points_layer(tmp_path):
    from hover_net_amd import points as P

    info = _hand_dict()
    ls = RP.of_info(info, (10, 14), [2.5, 3.0], 3, sims=4, seed=9)
    plain = RP.of_info(info, (10, 14), [2.5, 3.0], 3)
    assert isinstance(ls, RP.LabelSims) and isinstance(plain, RP.PairCounts) and ls.seed == 9 and ls.pairs_in.shape == (4, 3, 3, 2) and ls.n_in.shape == (4, 3, 2)
    R.assert_same(ls.observed, plain[:4], "of_info")
    _, xy, types = P.from_info(info, 3)
    SR.assert_same(ls, SR.sims(xy, types, [2.5, 3.0], RP.window_of((10, 14)), 3, 4, 9), "of_info")
    empty = RP.of_info({}, (10, 14), [2.5, 3.0], 5, sims=6, seed=2)
    assert empty.pairs_in.shape == (6, 5, 5, 2) and empty.n_in.shape == (6, 5, 2) and empty.pairs_in.dtype == empty.n_in.dtype == np.int64
    assert not empty.pairs_in.any() and not empty.n_in.any() and empty.seed == 2 and empty.observed.pairs.shape == (5, 5, 2) and np.isnan(RP.K_sims(empty)).all()
    with pytest.raises(ValueError):
        RP.of_info({}, (10, 14), [2.5], 3, sims=0)                   # also for an empty dict
    specs = P.resolve_specs(ripley={"radii": [2.5, 3.0], "sims": 4, "seed": 9})
    assert specs.ripley == ((2.5, 3.0), None, 4, 9) and P.resolve_specs(ripley={"radii": [2.5]}).ripley == ((2.5,), None)
    res = P.summaries(info, (10, 14), specs, 3, None)
    assert isinstance(res.ripley, RP.LabelSims) and (res.ripley.pairs_in == ls.pairs_in).all() and (res.ripley.n_in == ls.n_in).all()
    (tmp_path / "ripley").mkdir()
    P.save_results(str(tmp_path), "a", P.PointResults(None, res.ripley, None))
    RP.save(str(tmp_path / "p.npz"), plain)
    with np.load(tmp_path / "ripley" / "a.npz") as z, np.load(tmp_path / "p.npz") as p:
        assert sorted(p.files) == ["n", "n_in", "pairs", "pairs_in", "radii", "window"]
        assert sorted(z.files) == sorted(p.files + ["seed", "sim_n_in", "sim_pairs_in"])
        assert all((z[f] == p[f]).all() for f in p.files)            # the six old arrays under their old names
        assert (z["sim_pairs_in"] == ls.pairs_in).all() and (z["sim_n_in"] == ls.n_in).all() and z["sim_pairs_in"].dtype == z["sim_n_in"].dtype == np.int64
        assert z["seed"].dtype == np.uint64 and int(z["seed"]) == 9


def test_process_file_list_writes_the_simulations(tmp_path):
    from hover_net_amd import infer_manager as im

    inp = tmp_path / "in"
    inp.mkdir()
    np.save(inp / "a.npy", np.random.default_rng(0).integers(0, 256, (10, 14, 3), dtype=np.uint8))
    info = {lab: dict(e, type=None) for lab, e in _hand_dict().items()}
    mgr = im.InferManager({"model_args": {"nr_types": None, "mode": "original"}, "model_path": None},
                          process_fn=lambda images: [(np.zeros(i.shape[:2], np.int32), info) for i in images])
    assert mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "out"), "ripley": {"radii": [2.5, 3.0], "sims": 5, "seed": 3}}) == ["a"]
    want = RP.of_info(info, (10, 14), [2.5, 3.0], None, sims=5, seed=3)
    with np.load(tmp_path / "out" / "ripley" / "a.npz") as z:
        assert len(z.files) == 9 and (z["sim_pairs_in"] == want.pairs_in).all() and (z["sim_n_in"] == want.n_in).all() and int(z["seed"]) == 3
        assert (z["pairs_in"] == want.observed.pairs_in).all() and (z["sim_pairs_in"] == z["pairs_in"][None]).all()           # untyped
    with pytest.raises(ValueError):
        mgr.process_file_list({"input_dir": str(inp), "output_dir": str(tmp_path / "bad"), "ripley": {"radii": [2.5], "seed": 3}})
    assert not (tmp_path / "bad").exists()                           # refused before any file is touched


# -- refusals ----------------------------------------------------------------------------------------------
GOOD = dict(xy=np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.5]]), types=np.array([0, 1, 1], np.int32), radii=(1.0, 2.0), window=(0.0, 0.0, 4.0, 3.0),
            nr_types=None, sims=3, seed=0)
BAD = [("sims", 0, ValueError), ("sims", 10000, ValueError), ("sims", -2, ValueError), ("sims", None, TypeError), ("sims", 2.0, TypeError), ("sims", True, TypeError),
       ("seed", -1, ValueError), ("seed", 1 << 64, ValueError), ("seed", 0.0, TypeError), ("seed", None, TypeError),
       ("xy", np.zeros((3, 2), np.float32), TypeError), ("types", np.array([0, 16, 1], np.int32), ValueError), ("radii", (2.0, 1.0), ValueError),
       ("window", (0.0, 0.0, 0.0, 3.0), ValueError), ("nr_types", 1, ValueError)]


@pytest.mark.parametrize("field,value,exc", BAD, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BAD)])
def test_python_refusals_precede_any_work(field, value, exc, monkeypatch):
    from hover_net_amd import lib as L
    from hover_net_amd import points as P

    def no_work(*a, **k):
        raise AssertionError("work was started")

    monkeypatch.setattr(L, "lib", no_work)
    monkeypatch.setattr(L, "call", no_work)
    monkeypatch.setattr(P, "grid", no_work)
    monkeypatch.setattr(P, "candidate_runs", no_work)
    monkeypatch.setattr(RP, "round_keys", no_work)
    args = dict(GOOD, **{field: value})
    for fn in (RP.sims_host, RP.sims_device, RP.sims):
        with pytest.raises(exc):
            fn(args["xy"], args["types"], args["radii"], args["window"], args["nr_types"], args["sims"], args["seed"])


def test_the_batch_fits_the_lds(monkeypatch):
    """SB is `_BATCH` where SB histograms and the staged labels fit a workgroup's LDS, and as many as fit otherwise: 8 at the cap."""
    assert RP._BATCH == 8 and RP.batch_of(5, 16) == RP.batch_of(1, 1) == RP.batch_of(16, 16) == 8
    monkeypatch.setattr(RP, "_BATCH", 100)
    assert RP.batch_of(5, 16) == RP.batch_of(1, 1) == 32                 # the op's own bound
    assert RP.batch_of(16, 16) == 8 and RP._lds_bytes(8, 4096) <= RP._MAX_LDS < RP._lds_bytes(9, 4096)
    assert RP.batch_of(11, 32) == 8 and RP.batch_of(9, 32) == 12 and RP._lds_bytes(12, 81 * 32) <= RP._MAX_LDS < RP._lds_bytes(13, 81 * 32)
    monkeypatch.setattr(RP, "_BATCH", 0)
    assert RP.batch_of(5, 16) == 1


def _op():
    """A well-formed PAIRS_SIM op over made-up pointers (never dereferenced: every call below is refused on the host)."""
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731
    n, ncy, ncx = 1000, 30, 40
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.x.h = PL.OP_NBR_PAIRS_SIM, ncy, ncx, n
    op.w, op.x2.base, op.x2.sn = P(1), P(2), NB.workspace_bytes(n, ncy * ncx)
    op.cout, op._rsv, op.bias, op.nbatch = 5, 16, P(3), 6
    op.res.base, op.w2, op.y2.base, op.y2.sn = P(4), P(6), P(7), 4 * n * 2
    op.y.base = P(5)
    return op


# one entry per refusal that include/hvn.h lists for NBR_PAIRS_SIM: (field, value, status)
SIM_REFUSALS = [("y.base", None, -1), ("bias", None, -1), ("w2", None, -1), ("y2.base", None, -1), ("y.base", 0x15000004, -1), ("w2", 0x16000004, -1),
                ("bias", 0x13000004, -1), ("res.base", 0x14000002, -1), ("y2.base", 0x17000002, -1), ("cout", 0, -1), ("cout", 17, -1), ("_rsv", 0, -1), ("_rsv", 33, -1),
                ("nbatch", 0, -1), ("nbatch", 33, -1), ("nbatch", -4, -1), ("stride", 3, -1), ("stride", -1, -1), ("y2.sn", 4 * 1000 * 2 - 1, -4), ("y2.sn", 6 * 1000, -4), ("y2.sn", 0, -4)]
SHARED_REFUSALS = [("w", None, -1), ("x2.base", None, -1), ("w", 0x11000004, -1), ("x2.base", 0x12000004, -1), ("x.h", 0, -1), ("x.h", -5, -1),
                   ("kh", 0, -1), ("kw", -1, -1), ("x.h", (1 << 26) + 1, -4), ("kh", 4097, -4), ("kw", 4097, -4), ("x2.sn", 24 * 1000 + 4 * 2401 + 4095, -4),
                   ("x2.sn", 0, -4)]


def _set(op, path, value):
    obj = op
    *head, last = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, last, value)


def test_op_kind_20_is_in_the_header_and_the_plan():
    from hover_net_amd import lib as L
    from hover_net_amd import plan as PL

    assert PL.OP_NBR_PAIRS_SIM == 20 and "HVN_OP_NBR_PAIRS_SIM = 20" in open(L.HEADER).read() and "hvn_pairs_sim.hip" in L.SOURCES
    assert len(L.EXPORTS) == 53                                      # no new export


def test_c_refusals_launch_nothing():
    """Every refusal of include/hvn.h's NBR_PAIRS_SIM list: its status, a text that leads with the op's name, decided before any launch
    (the pointers are made up, so a launch would not go unnoticed; skipped where a GPU is present, as tests/test_ripley_host.py is)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()

    def refused(op, batch, code):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(b"nbr_pairs_sim:") and b"unknown op kind" not in err, (rc, err)

    for path, value, code in SIM_REFUSALS + SHARED_REFUSALS:
        op = _op()
        _set(op, path, value)
        refused(op, 1, code)
    refused(_op(), 2, -1)                                            # batch must be 1
    for t, r in ((16, 17), (12, 32), (15, 19)):                      # T and R allowed, 4096 bins exceeded
        op = _op()
        op.cout, op._rsv = t, r
        refused(op, 1, -4)
    for t, r, sb in ((16, 16, 9), (9, 32, 13), (6, 32, 32)):         # T, R and SB allowed, the histograms do not fit the LDS
        op = _op()
        op.cout, op._rsv, op.nbatch, op.y2.sn = t, r, sb, 1 << 30
        refused(op, 1, -4)
        assert b"LDS" in l.hvn_last_error()
    zero = L.hvn_op()
    zero.kind = _op().kind
    refused(zero, 1, -1)                                             # an all-zero op is refused by name
    buf = np.full(6 * (5 * 5 * 16 + 5 * 17), 0x5A5A5A5A, np.int64)      # a real host buffer as the output: a refused op does not write it
    for path, value in (("cout", 0), ("nbatch", 0), ("nbatch", 40), ("x.h", 0), ("y2.sn", 8), ("w2", None)):
        op = _op()
        op.y.base = buf.ctypes.data
        _set(op, path, value)
        assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    assert (buf == 0x5A5A5A5A).all()

"""CPU: hover_net_amd.tune -- the one pick rule, the forced-form path, the candidate function and the knob table, on hand-built
hvn_op structs (as tests/test_conv_launch_refusals.py builds them) and fake `measure` callables.  Nothing is launched."""
import itertools

import pytest

from hover_net_amd import lib as L
from hover_net_amd import tune as T
from hover_net_amd.tune import MARGIN, T256X64, X3G_128, X3G_256, X3R

BASE = 0x10000000          # never dereferenced
INF = float("inf")
CAND_SETS = [(128, 64), (128, X3G_256, X3G_128), (128, 64, X3G_256, X3G_128)]


def view(base, h, w, c):
    return L.hvn_view(base=base, sn=h * w * c, sy=w * c, sx=c, h=h, w=w, c=c, sc=1)


def conv_op(act_dtype=0, cin=128, cout=128, hw=32, kind=2, groups=1, pre=False, x2=False, res=False, cout2=0):
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.stride, op.cout, op.tile_n, op.act_dtype, op.groups, op.nbatch = kind, 1, 1, 1, cout, 128, act_dtype, groups, 1
    op.x = view(BASE, hw, hw, cin)
    op.y = view(BASE + (1 << 26), hw, hw, cout)
    if res:
        op.res = view(BASE + (2 << 26), hw, hw, cout)
    if x2:
        op.x2 = view(BASE + (3 << 26), hw, hw, x2)
    if pre:
        op.pre_scale, op.pre_shift = BASE + (4 << 26), BASE + (5 << 26)
    op.cout2 = cout2
    return op


class Measure:
    """measure(c) -> times[c]; an Exception instance is raised instead; calls are recorded."""

    def __init__(self, times):
        self.times, self.calls = times, []

    def __call__(self, c):
        self.calls.append(c)
        if isinstance(self.times[c], Exception):
            raise self.times[c]
        return self.times[c]


# ---- the pick rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cands", CAND_SETS, ids=["2", "3", "4"])
def test_baseline_is_kept_at_the_margin_and_lost_just_below_it(cands):
    t_base = 2.0
    for winner in cands[1:]:
        for t_alt, expect in ((MARGIN * t_base, cands[0]), (MARGIN * t_base * (1 + 1e-12), cands[0]), (t_base, cands[0]),
                              (MARGIN * t_base * (1 - 1e-12), winner)):
            times = {c: 3.0 for c in cands}
            times[cands[0]], times[winner] = t_base, t_alt
            choice, ms_base, ms_best, ms = T.choose({}, ("dev", "fam"), cands, Measure(times))
            assert choice == expect
            assert (ms_base, ms_best, ms) == (t_base, t_alt, times)


@pytest.mark.parametrize("cands", CAND_SETS, ids=["2", "3", "4"])
def test_a_refused_optional_candidate_is_never_chosen_and_a_refused_required_one_propagates(cands):
    for refused in cands[1:]:
        times = {c: 1.0 for c in cands}
        times[cands[0]], times[refused] = 2.0, L.HvnError("refused")
        if refused in T.OPTIONAL:
            m = Measure(times)
            entry = T.choose({}, ("dev", "fam"), cands, m)
            assert entry[0] != refused and entry[3][refused] == INF and m.calls == list(cands)      # the pass went on
            if len(cands) == 2:
                assert entry[0] == cands[0]
        else:
            with pytest.raises(L.HvnError):
                T.choose({}, ("dev", "fam"), cands, Measure(times))
    with pytest.raises(L.HvnError):          # the baseline is never optional here
        T.choose({}, ("dev", "fam"), cands, Measure({**{c: 1.0 for c in cands}, cands[0]: L.HvnError("refused")}))
    # every optional candidate refused: the baseline
    times = {c: (L.HvnError("refused") if c in T.OPTIONAL else 5.0) for c in cands}
    times[cands[0]] = 2.0
    assert T.choose({}, ("dev", "fam"), cands, Measure(times))[0] == cands[0]


@pytest.mark.parametrize("cands", CAND_SETS, ids=["2", "3", "4"])
def test_one_measurement_per_key_candidates_device_and_family(cands):
    cache, times = {}, {c: 1.0 for c in cands + (T256X64,)}
    m = Measure(times)
    first = T.choose(cache, ("dev0", "infer-conv", 32, 3), cands, m)
    assert m.calls == list(cands)
    assert T.choose(cache, ("dev0", "infer-conv", 32, 3), cands, m) is first and m.calls == list(cands)    # zero further calls
    for key, cs in ((("dev1", "infer-conv", 32, 3), cands), (("dev0", "train-conv", 32, 3), cands), (("dev0", "infer-conv", 16, 3), cands),
                    (("dev0", "infer-conv", 32, 3), cands + (T256X64,))):
        before = len(m.calls)
        T.choose(cache, key, cs, m)
        assert len(m.calls) == before + len(cs)
    assert len(cache) == 5


def parent_bf16_choice(t, margin=MARGIN):
    """The bf16 engine's wording of the rule before tune.py (min over all candidates, then fall back), kept as the expected value."""
    best = min(t, key=t.get)
    if t[best] == float("inf") or (best != 128 and t[best] >= margin * t[128]):
        best = 128
    return best


def test_the_bf16_wording_is_the_same_rule():
    cands = (128, X3G_256, X3G_128)
    grid = (0.5, 0.98, MARGIN, 0.99, 1.0, 1.5, INF)
    for ts in itertools.product(grid, repeat=3):
        t = dict(zip(cands, ts))
        assert T.choose({}, (), cands, Measure(t))[0] == parent_bf16_choice(t), t


# ---- forced forms ------------------------------------------------------------------------------------------------------------
def test_forced_forms():
    cands = (128, 64, X3G_256, X3G_128)
    key = ("dev", "infer-conv", 32)
    times = {128: 2.0, 64: 1.0, X3G_256: 3.0, X3G_128: 3.0}
    cache = {}
    unforced = T.choose(cache, key, cands, Measure(times))
    snapshot = dict(cache)
    m = Measure(times)
    assert T.pick(cache, key, cands, m, forced=X3G_256) == X3G_256 and m.calls == [X3G_256]            # eligible: launched once, kept
    m = Measure({**times, X3G_128: L.HvnError("refused")})
    assert T.pick(cache, key, cands, m, forced=X3G_128) == 128 and m.calls == [X3G_128]                # refused: the baseline
    assert cache == snapshot and cache[key + (cands,)] is unforced                                     # unforced entries untouched
    m = Measure(times)
    assert T.pick(cache, key, (128, 64), m, forced=X3G_256) == 64 and m.calls == [128, 64]              # not eligible: the normal path
    assert T.pick({}, key, cands, Measure(times), forced=64) == 64 and T.pick({}, key, cands, Measure({**times, 64: 9.0}), forced=64) == 128
    fresh = {}
    assert T.pick(fresh, key, (128, X3R), Measure({128: 1.0, X3R: L.HvnError("refused")}), forced=X3R) == 128 and not fresh


def test_forced_form_reads_the_three_knobs(monkeypatch):
    x3, bf16, chain = conv_op(3), conv_op(1), conv_op(3, cin=64, kind=T.OP_CHAIN, cout2=64)
    assert (T.forced_form(x3), T.forced_form(bf16), T.forced_form(chain)) == (None, None, None)
    monkeypatch.setenv("HVN_X3G_FORCE", str(X3G_128))
    monkeypatch.setenv("HVN_BF16G_FORCE", str(X3G_256))
    monkeypatch.setenv("HVN_CHAIN_X3R", "force")
    assert (T.forced_form(x3), T.forced_form(bf16), T.forced_form(chain)) == (X3G_128, X3G_256, X3R)


# ---- candidates --------------------------------------------------------------------------------------------------------------
def test_candidates_of_conv_launches():
    assert T.candidates(conv_op(3)) == (128, 64, X3G_256, X3G_128)
    assert T.candidates(conv_op(0)) == (128, 64)
    # the 256-row form with a prologue keeps 2 x cin floats next to its rings: the first cin past the CU's LDS drops it
    ring = 3 * 256 * 128 + 2 * 3 * 128 * 64
    cin_fits = (160 * 1024 - ring) // 8
    assert T.candidates(conv_op(3, cin=cin_fits, pre=True)) == (128, 64, X3G_256, X3G_128)
    assert T.candidates(conv_op(3, cin=cin_fits + 1, pre=True)) == (128, 64, X3G_128)
    assert T.candidates(conv_op(3, cin=cin_fits + 1)) == (128, 64, X3G_256, X3G_128)
    assert T.candidates(conv_op(0, cout=64)) == (64, T256X64)
    assert T.candidates(conv_op(3, cout=64)) == ()
    assert T.candidates(conv_op(0, cout=64, x2=64)) == ()
    assert T.candidates(conv_op(0, groups=4)) == () and T.candidates(conv_op(3, groups=4)) == ()
    assert T.candidates(conv_op(0, cout=32)) == ()
    assert T.candidates(conv_op(0, kind=7)) == ()                                   # not a CONV / CHAIN launch


def test_candidates_of_bf16_and_chain_launches(monkeypatch):
    assert T.candidates(conv_op(1)) == (128, X3G_256, X3G_128)
    assert T.candidates(conv_op(1, pre=True)) == () and T.candidates(conv_op(1, cout=64)) == ()
    batched = conv_op(1)
    batched.nbatch = 36
    assert T.candidates(batched) == ()
    chain = dict(kind=T.OP_CHAIN, cout2=64)
    assert T.candidates(conv_op(0, **chain)) == (128, 64)
    assert T.candidates(conv_op(1, **chain)) == ()
    assert T.candidates(conv_op(3, cin=64, **chain)) == (128, X3R)
    assert T.candidates(conv_op(3, cin=128, **chain)) == ()
    assert T.candidates(conv_op(3, cin=64, x2=64, **chain)) == (128, X3R)
    assert T.candidates(conv_op(3, cin=64, x2=128, **chain)) == ()
    assert T.candidates(conv_op(3, cin=64, x2=64, res=True, **chain)) == ()
    assert T.candidates(conv_op(3, cin=64, x2=64, kind=T.OP_CHAIN, cout2=128)) == ()
    monkeypatch.setenv("HVN_CHAIN_X3R", "0")
    monkeypatch.setenv("HVN_BF16G", "0")
    assert T.candidates(conv_op(3, cin=64, **chain)) == () and T.candidates(conv_op(1)) == ()


def test_hvn_x3g_narrows_inference_and_training_launches_alike(monkeypatch):
    infer = conv_op(3, hw=80, res=True)                     # as Engine._bind leaves it: plan tile, residual, sample-major views
    train = conv_op(2, hw=80)                               # as TrainEngine._net leaves it: tensor-major views, nine-term products
    train.x.sn, train.y.sn = 128, 128
    for value, forms in (("1", (X3G_256, X3G_128)), ("0", ()), (str(X3G_256), (X3G_256,)), (str(X3G_128), (X3G_128,))):
        monkeypatch.setenv("HVN_X3G", value)
        assert T.candidates(infer) == T.candidates(train) == (128, 64) + forms
        assert T.x3g_forms_for(infer) == forms


# ---- knobs -------------------------------------------------------------------------------------------------------------------
def test_every_knob_is_read_at_call_time(monkeypatch):
    for i, (name, (default, meaning)) in enumerate(T.KNOBS.items()):
        assert meaning
        monkeypatch.delenv(name, raising=False)
        assert T.knob(name) == default
        monkeypatch.setenv(name, "v%d" % i)
        assert T.knob(name) == "v%d" % i


def test_tile_select_is_one_parsed_value(monkeypatch):
    monkeypatch.delenv("HVN_TILE_SELECT", raising=False)
    assert T.tile_select() == "auto"
    for v in ("auto", "model", "0"):
        monkeypatch.setenv("HVN_TILE_SELECT", v)
        assert T.tile_select() == v
    monkeypatch.setenv("HVN_TILE_SELECT", "1")
    with pytest.raises(ValueError):
        T.tile_select()


def test_the_rounds_model_follows_its_knobs(monkeypatch):
    from hover_net_amd import plan as PL

    for k in ("HVN_TILE_SELECT", "HVN_FORCE_TILE_N", "HVN_WG_SLOTS_64", "HVN_NARROW_COST"):
        monkeypatch.delenv(k, raising=False)
    buf = PL.Buf("b", 80, 80, 256)
    op = PL.Op(PL.OP_CONV, "c", x=PL.View(buf, 0, 0, 80, 80), y=PL.View(buf, 0, 0, 80, 80), cout=256, tile_n=128)
    # batch 11: 550 row tiles x 2 = 1100 wide workgroups = 3 rounds of 512; 2200 narrow ones = 3 rounds of 768 at 0.45 each
    assert T.pick_tile_n(op, 11) == 64
    monkeypatch.setenv("HVN_NARROW_COST", "1.0")
    assert T.pick_tile_n(op, 11) == 128
    monkeypatch.setenv("HVN_WG_SLOTS_64", "2200")
    assert T.pick_tile_n(op, 11) == 64
    monkeypatch.setenv("HVN_FORCE_TILE_N", "128")
    assert T.pick_tile_n(op, 11) == 128
    monkeypatch.setenv("HVN_FORCE_TILE_N", "64")
    monkeypatch.setenv("HVN_TILE_SELECT", "0")
    assert T.pick_tile_n(op, 11) == 128


def test_time_launch_reads_the_repetitions_at_call_time(monkeypatch):
    class Event:
        clock = 0.0

        def __init__(self, enable_timing):
            self.t = None

        def record(self):
            self.t = Event.clock

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return other.t - self.t

    calls = []

    def launch():
        calls.append(1)
        Event.clock += 10.0 if len(calls) <= 2 else 4.0        # the warm-up round is the slow one and is not counted

    monkeypatch.setattr(T.torch.cuda, "Event", Event)
    monkeypatch.setenv("HVN_TUNE_REPS", "1")
    assert T.time_launch(launch, runs=2) == 4.0 and len(calls) == 4          # warm-up + 1 timing, two runs each, per run
    monkeypatch.delenv("HVN_TUNE_REPS")
    calls.clear()
    T.time_launch(launch)
    assert len(calls) == 4                                                   # warm-up + the default 3
    calls.clear()
    monkeypatch.setenv("HVN_TUNE_REPS", "5")
    T.time_launch(launch, reps=2)
    assert len(calls) == 6

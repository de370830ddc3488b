"""-m gpu: validation statistics accumulated on the device (hover_net_amd/csrc/hvn_valid.hip through include/hvn.h and
hover_net_amd/valid_stats.py) against `run_desc.proc_valid_step_output` on the same arrays on the host (which
tests/test_host_contracts.py pins to the reference's own function) and plain numpy counts.

Bounds: the integer state equals numpy's exactly, so np_acc / np_dice / tp_dice_k are bit-equal (same integers, same float64
expression).  hv_mse is a sum of n = 2 * N * h * w identical non-negative float64 terms in another order: each order is within
(n - 1) * 2^-53 relative of the exact sum, hence |got - want| <= 2 * n * 2^-53 * want, computed from n in `_close_mse`."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 7, 9),          # less than one wave, ragged tail
          (3, 80, 80),        # the original mask
          (2, 164, 164),      # the fast mask
          (5, 164, 164)]      # many workgroups, a pixel count no power of two divides


@functools.lru_cache(maxsize=None)
def _case(shape, nt, seed=0):
    """Seeded inputs with the planted edge values, their numpy counts and the host path's scalars (computed once per case and shared;
    the arrays are read-only)."""
    from hover_net_amd import run_desc

    n, h, w = shape
    P = n * h * w
    rng = np.random.default_rng([seed, n, h, w, nt or 0])
    c0 = 0 if nt is None else 1
    pred = rng.standard_normal((n, h, w, c0 + 3)).astype(np.float32)
    prob = rng.random((n, h, w), dtype=np.float32).reshape(-1)
    half = np.float32(0.5)
    plant = [0, 1, P // 2, P - 1]
    prob[plant] = [half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)), np.float32(np.nan)]
    pred[..., c0] = prob.reshape(n, h, w)
    np_map = rng.integers(0, 2, (n, h, w)).astype(np.int32)
    np_map.reshape(-1)[plant] = [1, 1, 1, 0]                  # 0.5 -> miss, 0.5 + ulp -> hit, 0.5 - ulp -> miss, NaN -> background, correct
    hv_map = rng.uniform(-1, 1, (n, h, w, 2)).astype(np.float32)
    feed = {"np_map": np_map, "hv_map": hv_map}
    raw = {"prob_np": pred[..., c0], "true_np": np_map.astype(np.int64), "pred_hv": pred[..., c0 + 1:c0 + 3], "true_hv": hv_map}
    if nt is not None:
        pred[..., 0] = rng.integers(0, nt, (n, h, w)).astype(np.float32)           # whole numbers only
        tp_map = rng.integers(0, nt, (n, h, w)).astype(np.int32)
        tp_map.reshape(-1)[2] = nt                                                 # out of range: counted by nobody
        feed["tp_map"] = tp_map
        raw.update(pred_tp=pred[..., 0], true_tp=tp_map.astype(np.int64))
    pred_np = (pred[..., c0] > 0.5).astype(np.int32)
    counts = [P, int((pred_np == np_map).sum()), int(((pred_np == 1) & (np_map == 1)).sum()), int((pred_np == 1).sum() + (np_map == 1).sum())]
    for t in range(nt or 0):
        a, b = feed["tp_map"] == t, pred[..., 0] == t
        counts += [int((a & b).sum()), int(a.sum() + b.sum())]
    want = run_desc.proc_valid_step_output(raw, nr_types=nt)["scalar"]
    for a in (pred, np_map, hv_map) + ((feed["tp_map"],) if nt is not None else ()):
        a.setflags(write=False)
    return pred, feed, np.array(counts, np.int64), want


def _dev(pred, feed):
    return torch.tensor(pred).cuda(), {k: torch.tensor(v).cuda() for k, v in feed.items()}        # copies: the cached arrays are read-only


def _close_mse(got, want, n_terms):
    bound = 2.0 * n_terms * 2.0 ** -53 * want
    print("hv_mse got %.17g want %.17g |diff| %.3g bound %.3g (n = %d)" % (got, want, abs(got - want), bound, n_terms))
    assert abs(got - want) <= bound, (got, want, bound)


def _same_scalars(got, want, n_terms):
    assert list(got) == list(want)
    for k in want:
        if k == "hv_mse":
            _close_mse(got[k], want[k], n_terms)
        else:
            assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])


@pytest.mark.parametrize("nt", [None, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_numpy(shape, nt):
    from hover_net_amd.valid_stats import ValidStats

    pred, feed, counts, want = _case(shape, nt)
    vs = ValidStats(nt, "cuda")
    vs.update(*_dev(pred, feed))
    np.testing.assert_array_equal(vs.counts.cpu().numpy(), counts)
    _same_scalars(vs.scalars(), want, 2 * shape[0] * shape[1] * shape[2])
    assert vs.track()["image"] == {}


def test_host_feed_is_uploaded():
    """The loader's dict may hold host arrays or tensors of the reference loader's dtypes (int64 maps)."""
    from hover_net_amd.valid_stats import ValidStats

    pred, feed, counts, _ = _case((1, 7, 9), 5)
    vs = ValidStats(5, "cuda")
    vs.update(torch.tensor(pred).cuda(), {"np_map": feed["np_map"].astype(np.int64), "hv_map": torch.tensor(feed["hv_map"]),
                                          "tp_map": torch.from_numpy(feed["tp_map"].astype(np.int64))})
    np.testing.assert_array_equal(vs.counts.cpu().numpy(), counts)


def test_same_updates_give_the_same_bits():
    from hover_net_amd.valid_stats import ValidStats

    batches = [_dev(*_case(s, 5, seed)[:2]) for s, seed in (((2, 164, 164), 1), ((5, 164, 164), 2), ((3, 80, 80), 3))]
    vs = ValidStats(5, "cuda")
    bits = []
    for _ in range(2):
        vs.reset()
        for pred, feed in batches:
            vs.update(pred, feed)
        bits.append(vs._buf.cpu().clone())
    assert float(bits[0][-1:].view(torch.float64)) > 0.0
    assert torch.equal(bits[0], bits[1])                      # int64 view: the float64 sum bit for bit


def test_counts_accumulate_in_64_bits():
    from hover_net_amd.valid_stats import ValidStats

    pred, feed, counts, _ = _case((1, 7, 9), 5)
    vs = ValidStats(5, "cuda")
    vs.counts.fill_(2 ** 31 - 5)
    vs.update(*_dev(pred, feed))
    np.testing.assert_array_equal(vs.counts.cpu().numpy(), counts + (2 ** 31 - 5))
    assert vs.counts.cpu().numpy()[0] > 2 ** 31


def test_two_updates_one_read():
    from hover_net_amd.valid_stats import ValidStats

    a, b = _case((3, 80, 80), 5, 0), _case((3, 80, 80), 5, 7)
    da, db = _dev(*a[:2]), _dev(*b[:2])
    vs = ValidStats(5, "cuda")
    vs.update(*da)
    vs.update(*db)                                            # no read, no sync in between
    np.testing.assert_array_equal(vs.counts.cpu().numpy(), a[2] + b[2])
    n_terms = 2 * 2 * 3 * 80 * 80
    e = [np.asarray(c[0][..., 2:4], np.float64) - np.asarray(c[1]["hv_map"], np.float64) for c in (a, b)]
    want = (np.concatenate(e) * np.concatenate(e)).sum() / (2 * 3 * 80 * 80)
    _close_mse(vs.scalars()["hv_mse"], want, n_terms)


def test_refusals_leave_the_state_unchanged():
    from hover_net_amd import lib as L
    from hover_net_amd import valid_stats as V

    pred4, feed4, _, _ = _case((1, 7, 9), 5)
    pred3, feed3, _, _ = _case((1, 7, 9), None)
    p4, f4 = _dev(pred4, feed4)
    p3, f3 = _dev(pred3, feed3)
    vs = V.ValidStats(5, "cuda")
    vs.update(p4, f4)                                         # a state that is not all zero
    before = vs._buf.clone()
    ws = torch.empty(int(L.lib().hvn_valid_stats_workspace_bytes(1, 7, 9)), dtype=torch.uint8, device="cuda")

    def refused(fn):
        with pytest.raises(L.HvnError):
            fn()
        torch.cuda.synchronize()
        assert torch.equal(vs._buf, before)

    good = (p4, f4["np_map"], f4["hv_map"], f4["tp_map"], (1, 7, 9, 4), 5, vs.counts, vs.hv_sse, ws)
    call = lambda **kw: V.launch(*[kw.get(k, v) for k, v in zip(("pred", "np_map", "hv_map", "tp_map", "shape", "nr_types", "counts", "hv_sse", "ws"), good)])  # noqa: E731
    for c in (2, 5):                                          # C not 3 or 4
        refused(lambda: call(shape=(1, 7, 9, c)))
    refused(lambda: vs.update(torch.zeros(1, 7, 9, 5, device="cuda"), f4))
    refused(lambda: vs.update(p3, f4))                        # tp_map given with C == 3
    refused(lambda: call(pred=p3, shape=(1, 7, 9, 3), nr_types=0))
    refused(lambda: vs.update(p4, f3))                        # tp_map missing with nr_types > 0
    refused(lambda: call(tp_map=None))
    refused(lambda: call(nr_types=17))                        # above the cap of 16
    for shape in ((0, 7, 9, 4), (1, -7, 9, 4), (1, 7, 0, 4)):
        refused(lambda: call(shape=shape))                    # non-positive sizes
    refused(lambda: call(ws=ws[:ws.numel() - 1]))             # workspace one byte short
    call()                                                    # and the good call still runs
    assert int(vs.counts[0]) == 2 * 63


def _net(mode, nt):
    from hover_net_amd import net_desc
    from hover_net_amd.synth import synth_state_dict

    net = net_desc.create_model(mode=mode, nr_types=nt, input_ch=3)
    net.load_state_dict(synth_state_dict(mode, nt, seed=3), strict=True)
    return net.to("cuda").eval()


@pytest.mark.parametrize("nt", [5, None])
def test_valid_step_stats_equals_the_host_path(nt):
    """Two batches of a resident valid loader through `valid_step_stats` and through `valid_step` + the accumulate / process callbacks."""
    from hover_net_amd import augment as G
    from hover_net_amd import run_desc
    from hover_net_amd import run_engine as RE
    from hover_net_amd.valid_stats import ValidStats

    rng = np.random.default_rng(4)
    p, s = 4, 270
    img = rng.integers(0, 256, (p, s, s, 3), dtype=np.uint8)
    ann = np.zeros((p, s, s, 2), np.int32)
    for k in range(p):
        for i in range(1, 30):
            y, x = rng.integers(0, s - 20), rng.integers(0, s - 20)
            ann[k, y:y + rng.integers(8, 20), x:x + rng.integers(8, 20)] = (i, rng.integers(1, 5))
    data = np.concatenate([img.astype(np.int32), ann], -1)
    ld = G.DevicePatchLoader(data, (256, 256), (164, 164), batch_size=2, mode="valid", with_type=nt is not None)
    net = _net("fast", nt)
    stats = ValidStats(nt, "cuda")
    info = {"net": {"desc": net}, "valid_stats": stats}
    state = RE.State()
    acc = RE.AccumulateRawOutput()
    batches = list(ld)
    assert [int(b["img"].shape[0]) for b in batches] == [2, 2]
    for feed in batches:
        assert run_desc.valid_step_stats(feed, [info, {}]) == {"raw": {}}
    got = stats.track()
    for feed in batches:
        state.step_output = run_desc.valid_step(feed, [{"net": {"desc": net}}, {}])
        acc.run(state, RE.Events.STEP_COMPLETED)
    want = run_desc.proc_valid_step_output(state.epoch_accumulated_output, nr_types=nt)
    assert got["image"] == {} and want["image"] == {}
    assert int(stats.counts[0]) == 4 * 164 * 164
    _same_scalars(got["scalar"], want["scalar"], 2 * 4 * 164 * 164)
    assert 0.0 < got["scalar"]["np_acc"] <= 1.0 and got["scalar"]["hv_mse"] > 0.0


def test_run_phases_device_valid_matches_the_default(tmp_path):
    """The smallest run_phases schedule of tests/test_gpu_train.py (two phases on a repeated synthetic batch), one epoch each: the
    `valid` rows follow the rule above, the `train` rows are bit-equal (the valid path does not touch the training step)."""
    from hover_net_amd import train
    from hover_net_amd.synth import synth_state_dict

    mode, nt = "original", None
    torch.save({"desc": synth_state_dict(mode, nt, seed=2)}, str(tmp_path / "init.tar"))

    class Fixed:
        def __init__(self, bs, steps):
            self.b = next(iter(train.SyntheticLoader(bs, 1, mode, nt, seed=77)))
            self.steps = steps

        def __iter__(self):
            return iter([self.b] * self.steps)

    def run(**kw):
        cfg = train.get_config(nt, mode)
        cfg["phase_list"][0]["run_info"]["net"]["pretrained"] = str(tmp_path / "init.tar")
        hist, _ = train.run_phases(cfg, lambda pi, bs: {"train": Fixed(2, 6), "valid": Fixed(2, 1)}, nr_epochs=1, **kw)
        return hist

    want, got = run(), run(device_valid=True)
    assert [h["phase"] for h in got] == [0, 1] and all(h["valid_steps"] == 1 for h in got)
    for g, w in zip(got, want):
        assert g["train"] == w["train"] and g["steps"] == w["steps"] and g["lr"] == w["lr"]
        _same_scalars(g["valid"], w["valid"], 2 * 2 * 80 * 80)

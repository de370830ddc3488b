"""GPU: the run loop's picture on the device (csrc/hvn_viz.hip, `hvn_viz_strip`) against its host definition
(`run_desc.viz_step_output`), `==` everywhere.  Every strip is drawn into the middle of a buffer with sentinel rows on both sides,
which must come back intact; the buffer also places blocks at byte offsets that are no multiple of four."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "viz_strip.npz")
FILL = 0xA5
PAD = 3             # sentinel rows on either side


def _raw(rng, n, hw, img_hw, nr_types):
    """Dense random host inputs: values beyond the ranges, NaN, +-inf, denormals, type ids outside 0..T."""
    h, w = hw
    raw = {"img": rng.integers(0, 256, (n, *img_hw, 3)).astype(np.uint8)}
    pred_np = (rng.random((n, h, w)) * 1.5 - 0.25).astype(np.float32)
    pred_hv = (rng.random((n, h, w, 2)) * 3 - 1.5).astype(np.float32)
    true_hv = (rng.random((n, h, w, 2)) * 2 - 1).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1.0e-40, -1.0e-40, 1.0e30, -1.0e30], np.float32)
    for a in (pred_np, pred_hv, true_hv):
        k = min(special.size, a.size)
        a.reshape(-1)[rng.permutation(a.size)[:k]] = special[rng.permutation(special.size)[:k]]
    raw["np"] = (rng.integers(0, 2, (n, h, w)).astype(np.int64), pred_np)
    raw["hv"] = (true_hv, pred_hv)
    if nr_types is not None:
        raw["tp"] = (rng.integers(-1, nr_types + 2, (n, h, w)).astype(np.int64), rng.integers(-1, nr_types + 2, (n, h, w)).astype(np.float32))
    return raw


def _pack(raw, nr_types):
    """Host raw_data -> the kernel's device layout (img, pred [n,h,w,3|4], np_map, hv_map, tp_map)."""
    planes = [raw["np"][1], raw["hv"][1][..., 0], raw["hv"][1][..., 1]]
    tp_map = None
    if nr_types is not None:
        planes.insert(0, raw["tp"][1])
        tp_map = torch.tensor(raw["tp"][0].astype(np.int32)).cuda()
    pred = torch.tensor(np.ascontiguousarray(np.stack(planes, -1), np.float32)).cuda()
    return (torch.tensor(raw["img"]).cuda(), pred, torch.tensor(raw["np"][0].astype(np.int32)).cuda(), torch.tensor(raw["hv"][0]).cuda(), tp_map)


def _host_blocks(raw, nr_types):
    """The host picture of every sample, as [n, 2h, ncol * w, 3]."""
    from hover_net_amd import run_desc

    n = raw["img"].shape[0]
    strip = run_desc.viz_step_output(raw, nr_types)
    return strip.reshape(n, strip.shape[0] // n, strip.shape[1], 3)


def _framed(n_blocks, h, w, ncol):
    buf = torch.full((n_blocks * 2 * h + 2 * PAD, ncol * w, 3), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[PAD:PAD + n_blocks * 2 * h]


def _check(buf, blocks, sel, n_blocks):
    """Sentinels intact, every block named in `sel` equal to the host's picture of its sample, every other block still FILL."""
    got = buf.cpu().numpy()
    assert (got[:PAD] == FILL).all() and (got[-PAD:] == FILL).all()
    body = got[PAD:-PAD].reshape(n_blocks, -1, got.shape[1], 3)
    named = {}
    for s, b in sel:
        named[b] = s
    for b in range(n_blocks):
        if b in named:
            assert np.array_equal(body[b], blocks[named[b]]), (b, named[b])
        else:
            assert (body[b] == FILL).all(), b


def _draw_and_check(raw, nr_types, sel, n_blocks):
    from hover_net_amd import viz

    blocks = _host_blocks(raw, nr_types)
    h, w = raw["np"][1].shape[1:3]
    buf, out = _framed(n_blocks, h, w, 4 if nr_types is None else 5)
    res = viz.strip_device(*_pack(raw, nr_types), sel, out=out, nr_types=nr_types)
    assert res is out
    _check(buf, blocks, sel, n_blocks)


SHAPES = [((1, 1), (1, 1)), ((1, 1), (4, 3)), ((3, 5), (6, 8)), ((3, 5), (6, 9)), ((7, 65), (7, 65)), ((7, 65), (10, 70)), ((16, 16), (24, 24)),
          ((80, 80), (270, 270)), ((164, 164), (256, 256))]


@pytest.mark.parametrize("nr_types", [None, 5])
@pytest.mark.parametrize("hw,img_hw", SHAPES)
def test_shapes(hw, img_hw, nr_types):
    """1x1, odd widths, more than one workgroup per block, the two product shapes, image == map, odd and even crop differences; three
    samples into five blocks in a mixed order, so block bases fall on every byte alignment the shape allows."""
    raw = _raw(np.random.default_rng([hw[0], hw[1], nr_types or 0]), 3, hw, img_hw, nr_types)
    _draw_and_check(raw, nr_types, [(2, 0), (0, 3), (1, 1), (0, 4)], 5)


@pytest.mark.parametrize("nr_types", [1, 2, 3, 5, 6, 7, 16])
def test_every_type_id(nr_types):
    """Every k in 0..T, as truth and as predicted type, and k > T and k < 0: k / T * 256 decides the table index."""
    ids = np.arange(-3, nr_types + 4)
    w = ids.size
    raw = _raw(np.random.default_rng(nr_types), 2, (3, w), (4, w + 1), nr_types)
    raw["tp"][0][:, 0, :] = ids
    raw["tp"][1][:, 1, :] = ids[::-1]
    raw["tp"][0][0, 2, :2] = [2 ** 31 - 1, -2 ** 31]
    _draw_and_check(raw, nr_types, [(0, 0), (1, 1)], 2)


@functools.lru_cache(maxsize=None)
def _edge_values(vmin, vmax):
    """The range ends, every vmin + j (vmax - vmin) / 256 with its two float32 neighbours, denormals, NaN, +-inf, values far outside."""
    j = np.arange(257, dtype=np.float64)
    mid = (vmin + j * (vmax - vmin) / 256).astype(np.float32)
    vals = [mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)),
            np.array([vmin, vmax, np.nan, np.inf, -np.inf, 1.0e-45, -1.0e-45, 1.0e-39, -1.0e-39, 0.0, -0.0, 3.0e38, -3.0e38, 1.0e9, -1.0e9], np.float32)]
    return np.concatenate(vals).astype(np.float32)


@pytest.mark.parametrize("nr_types", [None, 5, 7, 16])
def test_prediction_edge_values(nr_types):
    ranges = [(0, 1), (-1, 1)] + ([] if nr_types is None else [(0, nr_types)])
    n_vals = _edge_values(0, 1).size
    h, w = 6, -(-n_vals // 6)
    raw = _raw(np.random.default_rng(9), 1, (h, w), (h + 1, w + 3), nr_types)
    for (vmin, vmax), plane in zip(ranges, [raw["np"][1], raw["hv"][1][..., 0]] + ([] if nr_types is None else [raw["tp"][1]])):
        plane.flat[:n_vals] = _edge_values(vmin, vmax)                                       # .flat writes through a strided view
    raw["hv"][1][..., 1].flat[:n_vals] = _edge_values(-1, 1)[::-1]
    raw["hv"][0][..., 0].flat[:n_vals] = _edge_values(-1, 1)
    assert np.isnan(raw["hv"][1][..., 0]).any() and (raw["hv"][1][..., 1] == np.float32(3.0e38)).any()
    _draw_and_check(raw, nr_types, [(0, 0)], 1)


@pytest.fixture(scope="module")
def small():
    raw = _raw(np.random.default_rng(21), 4, (5, 7), (8, 9), 3)
    for v in raw.values():
        for a in (v,) if isinstance(v, np.ndarray) else v:
            a.setflags(write=False)
    return raw, _host_blocks(raw, 3)


@pytest.mark.parametrize("sel", [[(1, 0), (1, 1), (1, 4), (3, 2)], [(3, 0), (2, 1), (1, 2), (0, 3)], []], ids=["duplicates", "reversed", "empty"])
def test_sel_orders(small, sel):
    from hover_net_amd import viz

    raw, blocks = small
    buf, out = _framed(5, 5, 7, 5)
    viz.strip_device(*_pack(raw, 3), sel, out=out, nr_types=3)
    _check(buf, blocks, sel, 5)
    dev_sel = torch.tensor(np.asarray(sel, np.int32).reshape(-1, 2)).cuda()                 # the same pairs as a device tensor
    buf2, out2 = _framed(5, 5, 7, 5)
    viz.strip_device(*_pack(raw, 3), dev_sel, out=out2, nr_types=3)
    assert torch.equal(buf, buf2)


def test_new_out_is_zeroed_and_sized(small):
    from hover_net_amd import viz

    raw, blocks = small
    out = viz.strip_device(*_pack(raw, 3), [(2, 1)], n_blocks=3, nr_types=3).cpu().numpy().reshape(3, 10, 35, 3)
    assert np.array_equal(out[1], blocks[2]) and not out[0].any() and not out[2].any()
    out = viz.strip_device(*_pack(raw, 3), [(0, 0), (3, 1)], nr_types=3).cpu().numpy().reshape(2, 10, 35, 3)     # n_blocks = n_sel
    assert np.array_equal(out[0], blocks[0]) and np.array_equal(out[1], blocks[3])
    # a typed prediction without type truths: four columns
    img, pred, np_map, hv_map, _tp = _pack(raw, 3)
    four = viz.strip_device(img, pred, np_map, hv_map, None, [(1, 0)], nr_types=3).cpu().numpy()
    assert np.array_equal(four, blocks[1][:, :28])


def test_non_default_stream(small):
    from hover_net_amd import viz

    raw, blocks = small
    packed = _pack(raw, 3)
    buf, out = _framed(2, 5, 7, 5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        viz.strip_device(*packed, [(3, 1), (0, 0)], out=out, nr_types=3)
    side.synchronize()
    _check(buf, blocks, [(3, 1), (0, 0)], 2)


def _raw_call(packed, h, w, nr_types, sel, out, n_blocks, ih=None, iw=None, c=None):
    from hover_net_amd import lib as L
    from hover_net_amd import viz

    img, pred, np_map, hv_map, tp_map = packed
    lut = torch.tensor(np.array(viz.jet_lut())).cuda()
    sel_dev = torch.tensor(np.asarray(sel, np.int32).reshape(-1, 2)).cuda()
    rc = L.lib().hvn_viz_strip(img.data_ptr(), int(img.shape[0]), int(img.shape[1]) if ih is None else ih, int(img.shape[2]) if iw is None else iw,
                               pred.data_ptr(), int(pred.shape[3]) if c is None else c, np_map.data_ptr(), hv_map.data_ptr(),
                               None if tp_map is None else tp_map.data_ptr(), h, w, nr_types, sel_dev.data_ptr(), len(sel), lut.data_ptr(),
                               out.data_ptr(), n_blocks, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_out_of_range_pairs_draw_nothing(small):
    """Through the raw call: a sample or a block out of range is skipped, the pairs around it draw, untouched blocks keep their fill."""
    raw, blocks = small
    buf, out = _framed(3, 5, 7, 5)
    sel = [(0, 2), (4, 0), (-1, 0), (1, 3), (1, -1), (2 ** 31 - 1, 1), (2, 0)]
    assert _raw_call(_pack(raw, 3), 5, 7, 3, sel, out, 3) == 0
    _check(buf, blocks, [(0, 2), (2, 0)], 3)


@pytest.mark.parametrize("sel", [[(4, 0)], [(-1, 0)], [(0, 2)], [(0, -1)], [(0, 0), (1, 5)]])
def test_python_refuses_out_of_range_pairs(small, sel):
    from hover_net_amd import viz

    raw, _blocks = small
    buf, out = _framed(2, 5, 7, 5)
    with pytest.raises(ValueError):
        viz.strip_device(*_pack(raw, 3), sel, out=out, nr_types=3)
    with pytest.raises(ValueError):
        viz.strip_device(*_pack(raw, 3), torch.tensor(sel, dtype=torch.int32).cuda(), out=out, nr_types=3)
    torch.cuda.synchronize()
    assert (buf == FILL).all()


def test_refusals_return_minus_one_and_leave_out_untouched(small):
    raw, _blocks = small
    packed = _pack(raw, 3)
    buf, out = _framed(2, 5, 7, 5)
    sel = [(0, 0), (1, 1)]
    assert _raw_call(packed, 5, 7, 3, sel, out, 2, ih=4) == -1                               # ih < h
    assert _raw_call(packed, 5, 7, 3, sel, out, 2, iw=6) == -1                               # iw < w
    assert _raw_call(packed, 5, 7, 0, sel, out, 2) == -1                                     # c == 4 without types
    assert _raw_call(packed, 5, 7, 3, sel, out, 2, c=3) == -1                                # types with c == 3
    assert _raw_call(packed, 5, 7, 17, sel, out, 2) == -1                                    # nr_types > 16
    assert (buf == FILL).all()
    assert _raw_call(packed, 5, 7, 3, [], out, 2) == 0                                       # n_sel == 0: nothing launched
    assert (buf == FILL).all()


@pytest.mark.parametrize("case,nr_types", [("m16", None), ("m16t5", 5), ("m5x7", None), ("m5x7t5", 5)])
def test_fixture_strips_from_device_inputs(case, nr_types):
    """tests/golden/viz_strip.npz holds the reference's own pictures: `viz_step_output_device` on the same inputs as device tensors."""
    from hover_net_amd import run_desc

    d = np.load(FIXTURE)
    raw = {"img": torch.tensor(d[case + "_img"]).cuda()}
    for k in ("np", "hv") + (("tp",) if nr_types is not None else ()):
        raw[k] = (torch.tensor(d["%s_%s_true" % (case, k)]).cuda(), torch.tensor(d["%s_%s_pred" % (case, k)]).cuda())
    strip = run_desc.viz_step_output_device(raw, nr_types)
    assert strip.is_cuda and strip.dtype == torch.uint8
    assert np.array_equal(strip.cpu().numpy(), d[case + "_strip"])


@pytest.mark.parametrize("nt", [None, 3])
def test_plan_viz_over_three_batches(nt):
    """Batches of 4, 4 and a ragged 3: the strip equals proc_valid_step_output(image=True, selected_idx=...) on the same arrays, a
    planned sample the epoch never reaches leaves its block zero, and the scalars are what they are without a plan."""
    from hover_net_amd import run_desc
    from hover_net_amd.valid_stats import ValidStats

    rng = np.random.default_rng([3, nt or 0])
    h, w, c0 = 6, 5, 0 if nt is None else 1
    batches = []
    for n in (4, 4, 3):
        raw = _raw(rng, n, (h, w), (9, 8), nt)
        finite = lambda a: np.clip(np.nan_to_num(a, nan=0.25), -2.0, 2.0)                    # noqa: E731  (the scalars are compared too)
        raw["hv"] = (finite(raw["hv"][0]), finite(raw["hv"][1]))
        raw["np"] = (raw["np"][0], finite(raw["np"][1]))
        if nt is not None:
            raw["tp"] = (np.clip(raw["tp"][0], 0, nt), raw["tp"][1])
        batches.append(raw)
    cat = lambda f: np.concatenate([f(b) for b in batches])                                  # noqa: E731
    host = {"imgs": cat(lambda b: b["img"]), "true_np": cat(lambda b: b["np"][0]), "prob_np": cat(lambda b: b["np"][1]),
            "true_hv": cat(lambda b: b["hv"][0]), "pred_hv": cat(lambda b: b["hv"][1])}
    if nt is not None:
        host.update(true_tp=cat(lambda b: b["tp"][0]), pred_tp=cat(lambda b: b["tp"][1]))
    plan = [10, 0, 3, 4, 4, 7, 25, 9]

    def epoch(vs):
        for b in batches:
            img, pred, np_map, hv_map, tp_map = _pack(b, nt)
            feed = {"img": torch.tensor(b["img"]), "np_map": np_map, "hv_map": hv_map}       # the image as a host tensor: uploaded
            if nt is not None:
                feed["tp_map"] = tp_map
            vs.update(pred, feed)
        return vs.track()

    plain = epoch(ValidStats(nt, "cuda"))
    vs = ValidStats(nt, "cuda")
    vs.plan_viz(plan, (9, 8))
    got = epoch(vs)
    assert plain["image"] == {} and list(got["scalar"]) == list(plain["scalar"])
    for k in plain["scalar"]:
        assert np.float64(got["scalar"][k]).tobytes() == np.float64(plain["scalar"][k]).tobytes(), k
    assert vs.viz_missing == 1
    reached = [i for i in plan if i < 11]
    want = run_desc.proc_valid_step_output(host, nt, image=True, selected_idx=reached)["image"]["output"]
    want = want.reshape(len(reached), 2 * h, -1, 3)
    strip = got["image"]["output"]
    assert strip.dtype == np.uint8 and strip.shape == (8 * 2 * h, (4 if nt is None else 5) * w, 3)
    strip = strip.reshape(8, 2 * h, -1, 3)
    assert not strip[6].any()
    assert np.array_equal(np.delete(strip, 6, axis=0), want)
    vs.reset()
    assert vs._plan is None and vs._strip is None
    assert epoch(vs)["image"] == {}                                                          # the plan does not outlive its epoch


def test_train_step_device_raw_gives_the_host_strip():
    """One training engine at batch 2 and an optimizer that does not move the weights: from the same seed the default `train_step`
    and the `viz = "device"` one pick the same two samples, report the same loss bits, and `VisualizeOutput` turns the device raw
    into the strip the host function draws from the default raw."""
    from hover_net_amd import net_desc, run_desc
    from hover_net_amd import run_engine as RE
    from hover_net_amd.synth import synth_state_dict, synth_train_batch

    class NoStep:
        def step(self):
            pass

    mode, nt = "original", None
    net = net_desc.create_model(mode=mode, nr_types=nt, input_ch=3, freeze=True)
    net.load_state_dict(synth_state_dict(mode, nt, seed=9), strict=True)
    net = net.to("cuda")
    batch = {k: torch.from_numpy(v) for k, v in synth_train_batch(2, mode, nt, seed=31).items()}
    loss = {"np": {"bce": 1, "dice": 1}, "hv": {"mse": 1, "msge": 1}}
    outs = []
    for extra in ({"loss": loss}, {"loss": loss, "viz": "device"}, {"loss": loss, "viz": "host"}):
        torch.manual_seed(5)
        outs.append(run_desc.train_step(batch, [{"net": {"desc": net, "optimizer": NoStep(), "extra_info": extra}}, {}]))
    host, dev, other = outs
    assert list(host["EMA"]) == list(dev["EMA"])
    for k in host["EMA"]:
        assert np.float64(host["EMA"][k]).tobytes() == np.float64(dev["EMA"][k]).tobytes(), k
    assert isinstance(other["raw"]["img"], np.ndarray) and np.array_equal(other["raw"]["img"], host["raw"]["img"])      # any other value: today's
    assert dev["raw"]["img"].is_cuda and dev["raw"]["np"][1].is_cuda and dev["raw"]["hv"][1].is_cuda
    assert np.array_equal(dev["raw"]["img"].cpu().numpy(), host["raw"]["img"])
    assert np.array_equal(dev["raw"]["np"][1].cpu().numpy(), host["raw"]["np"][1])
    want = run_desc.viz_step_output(host["raw"])
    assert want.shape == (2 * 2 * 80, 4 * 80, 3)
    state = RE.State()
    state.step_output = dev
    RE.VisualizeOutput(run_desc.viz_step_output).run(state, RE.Events.EPOCH_COMPLETED)
    got = state.tracked_step_output["image"]["output"]
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)

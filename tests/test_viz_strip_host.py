"""CPU: the run loop's picture on the host -- `viz.jet_lut`, `viz.colorize`, `run_desc.viz_step_output`,
`proc_valid_step_output(image=True)` -- against tests/golden/viz_strip.npz (made by tools/make_golden_viz.py with the reference's
own viz_step_output) and, where the reference tree exists, against the live reference functions; the ABI of `hvn_viz_strip`; the
bookkeeping of `run_engine.VisualizeOutput` and `ValidStats.plan_viz` on a CPU state.  `==` everywhere."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from hover_net_amd import lib as L
from hover_net_amd import run_desc, viz
from hover_net_amd import run_engine as RE
from hover_net_amd.valid_stats import ValidStats

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
FIXTURE = os.path.join(REPO, "tests", "golden", "viz_strip.npz")
CASES = {"m16": None, "m16t5": 5, "m5x7": None, "m5x7t5": 5}
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "models")), reason="needs the reference tree (build container only)")


def fixture_raw(d, case):
    raw = {"img": d[case + "_img"], "np": (d[case + "_np_true"], d[case + "_np_pred"]), "hv": (d[case + "_hv_true"], d[case + "_hv_pred"])}
    if CASES[case] is not None:
        raw["tp"] = (d[case + "_tp_true"], d[case + "_tp_pred"])
    return raw


def random_raw(rng, n, hw, img_hw, nr_types):
    """Dense random inputs with everything that decides a pixel: values beyond the ranges, NaN, +-inf, denormals, type ids outside 0..T."""
    h, w = hw
    raw = {"img": rng.integers(0, 256, (n, *img_hw, 3)).astype(np.uint8)}
    pred_np = (rng.random((n, h, w)) * 1.5 - 0.25).astype(np.float32)
    pred_hv = (rng.random((n, h, w, 2)) * 3 - 1.5).astype(np.float32)
    true_hv = (rng.random((n, h, w, 2)) * 2 - 1).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1.0e-40, -1.0e-40, np.nextafter(np.float32(1), np.float32(0)), 1.0e30, -1.0e30],
                       np.float32)
    for a in (pred_np, pred_hv, true_hv):
        k = min(special.size, a.size)
        a.reshape(-1)[rng.permutation(a.size)[:k]] = special[:k]
    raw["np"] = (rng.integers(0, 2, (n, h, w)).astype(np.int64), pred_np)
    raw["hv"] = (true_hv, pred_hv)
    if nr_types is not None:
        raw["tp"] = (rng.integers(-1, nr_types + 2, (n, h, w)).astype(np.int64), rng.integers(-1, nr_types + 2, (n, h, w)).astype(np.float32))
    return raw


def with_channel_axis(raw):
    """Copies with the NP / TP maps as [n,h,w,1]: the only form the reference's aligned_shape takes under numpy >= 1.24."""
    out = {"img": raw["img"].copy(), "hv": tuple(a.copy() for a in raw["hv"])}
    for k in ("np", "tp"):
        if k in raw:
            out[k] = tuple(a[..., None].copy() for a in raw[k])
    return out


@pytest.fixture
def reference():
    """The reference's run_desc module, imported through oracle/refimport.py with a stub cv2 and matplotlib on Agg."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import refimport

    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    refimport.use_reference()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import matplotlib

    matplotlib.use("Agg")
    try:
        yield refimport.ref_import("models.hovernet.run_desc")
    finally:
        sys.path[:] = saved_path
        for name in list(sys.modules):
            if name.split(".")[0] in ("models", "dataloader", "misc", "metrics", "infer", "run_utils", "cv2"):
                if name in saved_mods:
                    sys.modules[name] = saved_mods[name]
                else:
                    del sys.modules[name]


def test_jet_lut_is_the_fixture_table():
    lut = viz.jet_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert np.array_equal(lut, np.load(FIXTURE)["lut"])


def test_jet_lut_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    assert np.array_equal(viz.jet_lut(), (plt.get_cmap("jet")(np.arange(256))[:, :3] * 255).astype("uint8"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_strip_equals_the_fixture(case):
    d = np.load(FIXTURE)
    raw = fixture_raw(d, case)
    before = {k: (v.copy() if k == "img" else tuple(a.copy() for a in v)) for k, v in raw.items()}
    strip = run_desc.viz_step_output(raw, CASES[case])
    assert strip.dtype == np.uint8 and np.array_equal(strip, d[case + "_strip"])
    assert np.array_equal(run_desc.viz_step_output(with_channel_axis(raw), CASES[case]), d[case + "_strip"])
    for k, v in before.items():                       # the inputs are left as they were
        for a, b in zip((v,) if k == "img" else v, (raw[k],) if k == "img" else raw[k]):
            assert np.array_equal(a, b, equal_nan=True)
    from models.hovernet.run_desc import viz_step_output as shim

    assert shim is run_desc.viz_step_output


def test_colorize_table_indices():
    """Every k / T * 256 decides a table index: integer type ids over 0..T for every T the kernel takes, and the range ends."""
    lut = viz.jet_lut()
    for t in range(1, 17):
        k = np.arange(-1, t + 2)
        want = np.minimum((np.clip(k, 0, t).astype(np.float32) / np.float32(t) * np.float32(256)).astype(np.int64), 255)
        assert np.array_equal(viz.colorize(k, 0, t), lut[want])
    assert np.array_equal(viz.colorize(np.array([-1.0, 1.0, 0.0, np.nan, np.inf, -np.inf], np.float32), -1, 1),
                          np.stack([lut[0], lut[255], lut[128], [0, 0, 0], lut[255], lut[0]]))


@pytest.mark.parametrize("hw,img_hw", [((1, 1), (1, 1)), ((1, 1), (4, 3)), ((1, 6), (2, 6)), ((5, 1), (8, 2))])
def test_host_strip_of_maps_one_pixel_high_or_wide(hw, img_hw):
    """Shapes the reference's squeeze cannot draw: the strip is the pixels `colorize` gives, at their places."""
    raw = random_raw(np.random.default_rng(4), 2, hw, img_hw, 2)
    (h, w), lut = hw, viz.jet_lut()
    strip = run_desc.viz_step_output(raw, 2)
    assert strip.shape == (2 * 2 * h, 5 * w, 3) and strip.dtype == np.uint8
    y0, x0 = int((img_hw[0] - h) * 0.5), int((img_hw[1] - w) * 0.5)
    for i in range(2):
        top, low = strip[2 * i * h:(2 * i + 1) * h], strip[(2 * i + 1) * h:(2 * i + 2) * h]
        crop = raw["img"][i, y0:y0 + h, x0:x0 + w]
        assert np.array_equal(top[:, :w], crop) and np.array_equal(low[:, :w], crop)
        assert np.array_equal(top[:, w:2 * w], lut[np.where(raw["np"][0][i] > 0, 255, 0)])
        assert np.array_equal(low[:, 4 * w:], viz.colorize(raw["tp"][1][i].reshape(-1), 0, 2).reshape(h, w, 3))


@needs_reference
@pytest.mark.parametrize("nr_types,hw,img_hw", [(None, (16, 16), (24, 24)), (5, (5, 7), (8, 9)), (3, (9, 4), (9, 11)), (16, (6, 6), (6, 6))])
def test_host_strip_equals_the_live_reference(reference, nr_types, hw, img_hw):
    raw = random_raw(np.random.default_rng(11), 3, hw, img_hw, nr_types)
    with np.errstate(invalid="ignore"):
        want = reference.viz_step_output(with_channel_axis(raw), nr_types)
    got = run_desc.viz_step_output(raw, nr_types)
    assert got.dtype == want.dtype == np.uint8 and np.array_equal(got, want)


def valid_raw(rng, n, nr_types):
    raw = random_raw(rng, n, (6, 5), (9, 8), nr_types)
    finite = lambda a: np.clip(np.nan_to_num(a, nan=0.25), -2.0, 2.0)                         # noqa: E731  (the scalars are compared too)
    out = {"imgs": list(raw["img"]), "true_np": list(raw["np"][0]), "prob_np": list(raw["np"][1]), "true_hv": list(finite(raw["hv"][0])),
           "pred_hv": list(finite(raw["hv"][1]))}
    if nr_types is not None:
        out["true_tp"], out["pred_tp"] = list(raw["tp"][0]), list(raw["tp"][1])
    return out


@needs_reference
@pytest.mark.parametrize("nr_types", [None, 4])
def test_proc_valid_step_output_image_equals_the_reference(reference, nr_types):
    raw = valid_raw(np.random.default_rng(5), 11, nr_types)
    # the reference's picture needs [n,h,w,1] maps under this numpy; its scalars do not care
    ref_raw = dict(raw, true_np=[a[..., None] for a in raw["true_np"]], prob_np=[a[..., None] for a in raw["prob_np"]])
    if nr_types is not None:
        ref_raw.update(true_tp=[a[..., None] for a in raw["true_tp"]], pred_tp=[a[..., None] for a in raw["pred_tp"]])
    for seed in (0, 7):
        np.random.seed(seed)
        with np.errstate(invalid="ignore"):
            want = reference.proc_valid_step_output(ref_raw, nr_types)
        after_reference = np.random.randint(0, 1 << 30)
        np.random.seed(seed)
        got = run_desc.proc_valid_step_output(raw, nr_types, image=True)
        assert np.array_equal(got["image"]["output"], want["image"]["output"])
        assert got["image"]["output"].shape == (8 * 2 * 6, (4 if nr_types is None else 5) * 5, 3)
        assert np.random.randint(0, 1 << 30) == after_reference                               # eight draws from the global stream, no more


def test_proc_valid_step_output_default_is_unchanged_and_selected_idx():
    raw = valid_raw(np.random.default_rng(6), 5, 3)
    np.random.seed(3)
    state = np.random.get_state()[1].copy()
    plain = run_desc.proc_valid_step_output(raw, 3)
    assert plain["image"] == {} and np.array_equal(np.random.get_state()[1], state)          # no picture, no random draw
    assert run_desc.proc_valid_step_output(raw, 3, image=False) == plain
    idx = [4, 0, 0, 2]
    pic = run_desc.proc_valid_step_output(raw, 3, image=True, selected_idx=idx)
    assert pic["scalar"] == plain["scalar"] and np.array_equal(np.random.get_state()[1], state)
    take = lambda key: np.array([raw[key][i] for i in idx])                                   # noqa: E731
    want = run_desc.viz_step_output({"img": take("imgs"), "np": (take("true_np"), take("prob_np")), "hv": (take("true_hv"), take("pred_hv")),
                                     "tp": (take("true_tp"), take("pred_tp"))}, 3)
    assert np.array_equal(pic["image"]["output"], want) and want.shape == (4 * 12, 25, 3)


def test_refusals_are_host_arithmetic():
    lib = L.lib()
    # refusals are host arithmetic: no device is touched.  Dummy non-null, aligned "pointers" are never dereferenced.
    p = ctypes.c_void_p(4096)

    def call(ih=8, iw=8, c=3, h=4, w=4, nr_types=0, n_sel=1, n_blocks=1):
        return lib.hvn_viz_strip(p, 1, ih, iw, p, c, p, p, p, h, w, nr_types, p, n_sel, p, p, n_blocks, None)

    assert call(ih=3) == -1 and call(iw=3) == -1
    assert call(c=4, nr_types=0) == -1 and call(c=3, nr_types=2) == -1 and call(c=5) == -1
    assert call(c=4, nr_types=17) == -1 and call(c=3, nr_types=-1) == -1
    assert call(n_sel=-1) == -1 and call(n_blocks=0) == -1 and call(h=0) == -1
    assert b"viz_strip" in lib.hvn_last_error()
    assert call(n_sel=0) == 0 and call(c=4, nr_types=16, n_sel=0) == 0                        # nothing to draw: nothing launched


def test_visualize_output_protocol_on_a_host_state():
    calls = []

    def proc(raw):
        calls.append(raw)
        return np.full((2, 2, 3), 7, np.uint8)

    state = RE.State()
    cb = RE.VisualizeOutput(proc, per_n_epoch=3)
    assert cb.per_n_epoch == 3 and cb.proc_func is proc and cb.engine_trigger is False
    cb.run(state, RE.Events.EPOCH_COMPLETED)                                                  # an epoch without a step
    assert calls == [] and state.tracked_step_output["image"] == {}
    state.step_output = {"EMA": {}, "raw": {"img": np.zeros((1, 4, 4, 3), np.uint8)}}
    state.tracked_step_output["scalar"]["loss"] = 1.0
    cb.run(state, RE.Events.EPOCH_COMPLETED)
    assert calls == [state.step_output["raw"]]
    assert np.array_equal(state.tracked_step_output["image"]["output"], np.full((2, 2, 3), 7, np.uint8))
    assert state.tracked_step_output["scalar"] == {"loss": 1.0}
    # through an engine: the picture is of the epoch's LAST step, drawn by the real host function
    raws = [random_raw(np.random.default_rng(s), 2, (4, 4), (6, 6), None) for s in (1, 2)]
    eng = RE.RunEngine("train", [0, 1], lambda batch, info: {"EMA": {}, "raw": raws[batch]}, {})
    eng.add_event_handler(RE.Events.EPOCH_COMPLETED, RE.VisualizeOutput(run_desc.viz_step_output))
    eng.run(1)
    assert np.array_equal(eng.state.tracked_step_output["image"]["output"], run_desc.viz_step_output(raws[1]))
    assert eng.state.dataloader == [0, 1]


def test_plan_viz_bookkeeping_on_a_cpu_state():
    vs = ValidStats(2, device="cpu")
    vs.counts[:] = torch.tensor([100, 90, 40, 85, 30, 62, 20, 41])
    plain = vs.track()
    assert plain["image"] == {} and vs.viz_missing == 0
    vs.plan_viz([5, 0, 5, 2], (9, 8))
    assert vs._plan.tolist() == [5, 0, 5, 2] and vs._img_hw == (9, 8) and not vs._drawn.any()
    planned = vs.track()                                                                       # no update ever drew: no strip, all missing
    assert planned["scalar"] == plain["scalar"] and planned["image"] == {} and vs.viz_missing == 4
    with pytest.raises(ValueError):
        vs.plan_viz([-1])
    with pytest.raises(L.HvnError):
        vs.update(torch.zeros((1, 2, 2, 4)), {})                                               # drawing, like counting, needs the device
    vs.reset()
    assert vs._plan is None and vs._strip is None and vs._seen == 0 and int(vs.counts.sum()) == 0
    vs._seen = 3
    with pytest.raises(ValueError):
        vs.plan_viz([1])                                                                       # mid-epoch: positions would be ambiguous


def test_device_valid_stats_plans_from_the_loaders_n_samples():
    class Loader:
        n_samples, input_shape = 37, (9, 8)

    vs = ValidStats(None, device="cpu")
    cb = RE.DeviceValidStats(vs, viz_samples=8, seed=3)
    state = RE.State()
    state.dataloader = Loader()
    cb.run(state, RE.Events.EPOCH_STARTED)
    first = vs._plan.copy()
    assert first.shape == (8,) and (first >= 0).all() and (first < 37).all() and vs._img_hw == (9, 8)
    assert np.array_equal(first, np.random.default_rng([3, 0]).integers(0, 37, size=8))
    vs.counts[0] = 1
    cb.run(state, RE.Events.EPOCH_COMPLETED)
    assert vs._plan is None and state.tracked_step_output["image"] == {}
    cb.run(state, RE.Events.EPOCH_STARTED)
    assert np.array_equal(vs._plan, np.random.default_rng([3, 1]).integers(0, 37, size=8))
    # a loader that cannot say how many samples an epoch holds gets no picture; viz_samples = 0 plans nothing
    vs.reset()
    state.dataloader = [1, 2, 3]
    cb.run(state, RE.Events.EPOCH_STARTED)
    assert vs._plan is None
    state.dataloader = Loader()
    RE.DeviceValidStats(vs).run(state, RE.Events.EPOCH_STARTED)
    assert vs._plan is None


def test_device_patch_loader_n_samples():
    from hover_net_amd.augment import DevicePatchLoader

    patches = np.zeros((11, 12, 12, 5), np.int32)
    mk = lambda mode, **kw: DevicePatchLoader(patches, (8, 8), (4, 4), 4, mode=mode, device="cpu", **kw)      # noqa: E731
    assert mk("valid").n_samples == 11 and mk("train").n_samples == 8                          # every patch; whole batches only
    assert mk("valid", rank=1, world=2).n_samples == 5 and mk("valid", rank=0, world=2).n_samples == 6
    assert mk("train", rank=1, world=2).n_samples == 4
    ld = mk("train")
    ld.batch_size = 2                                                                          # phase 1 runs smaller batches over the same set
    assert ld.n_samples == 10


def test_strip_device_refuses_host_tensors():
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        viz.strip_device(img, torch.zeros((1, 4, 4, 3)), torch.zeros((1, 4, 4), dtype=torch.int32), torch.zeros((1, 4, 4, 2)), None, [(0, 0)])
    with pytest.raises(ValueError):
        run_desc.viz_step_output_device({"img": img, "np": (img, img), "hv": (img, img)})


@needs_reference
def test_recipe_regenerates_the_fixture(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", HVN_GOLDEN_OUT=str(tmp_path), MPLBACKEND="Agg")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-W", "ignore", os.path.join(REPO, "tools", "make_golden_viz.py")], capture_output=True, text=True,
                       env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.listdir(tmp_path) == ["viz_strip.npz"]
    new, old = np.load(tmp_path / "viz_strip.npz"), np.load(FIXTURE)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = new[k], old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.dtype != object, k
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k

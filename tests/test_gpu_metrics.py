"""GPU: the metric tables of csrc/hvn_metrics.hip against their host restatements and the recorded reference values
(tests/golden/metrics_cases.npz; the reference tree itself is never read here)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from hover_net_amd import metrics as M
from hover_net_amd.synth import synth_inst_pair

from metrics_fixture import FIXTURE, case_values, cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def sorted_triples(tr):
    tr = np.asarray(tr, np.int64)
    return tr[np.lexsort((tr[:, 1], tr[:, 0]))]


def check_batch(true, pred):
    """device table == host table per image, and a second device run gives the same triples."""
    t_d, p_d = torch.from_numpy(np.ascontiguousarray(true)).to(DEV), torch.from_numpy(np.ascontiguousarray(pred)).to(DEV)
    a = [sorted_triples(x) for x in M.device_triples(t_d, p_d, DEV)]
    b = [sorted_triples(x) for x in M.device_triples(t_d, p_d, DEV)]
    assert len(a) == len(true)
    for i in range(len(true)):
        want = M.host_triples(true[i], pred[i])
        assert a[i].shape == want.shape and np.array_equal(a[i], want), i
        assert np.array_equal(a[i], b[i]), i


def test_pair_table_one_instance_over_the_whole_foreground():
    t = np.ones((3, 301, 517), np.int32)                  # every pixel the same key (the LDS counters and the run fold)
    p = np.full_like(t, 7)
    p[1, :, :200] = 0
    t[2] = 0
    check_batch(t, p)


def test_pair_table_one_pixel_checkerboard():
    h, w = 257, 263                                       # every pixel a new key: the LDS table overflows into the global one
    yy, xx = np.mgrid[:h, :w]
    t = np.where((yy + xx) % 2 == 0, 1 + yy * w + xx, 0).astype(np.int32)
    p = np.where((yy + xx) % 2 == 1, 5 + yy * w + xx, 0).astype(np.int32)
    p2 = (1 + yy * w + xx).astype(np.int32)               # no (0, 0) pixel at all
    check_batch(np.stack([t, t]), np.stack([p, p2]))


def test_pair_table_consep_sized_maps():
    pairs = [synth_inst_pair(1000, 1000, 600, seed=s) for s in range(3)]
    check_batch(np.stack([t for t, _ in pairs]), np.stack([p for _, p in pairs]))


def test_pair_table_odd_shapes_and_mixed_instance_counts():
    for (h, w) in [(1, 1), (1, 4097), (63, 65), (129, 31), (270, 270)]:
        pairs = [synth_inst_pair(h, w, k, seed=k) for k in (0, 1, 3, 40)] if h > 1 else [synth_inst_pair(h, w, k, seed=k, r_lo=0, r_hi=1) for k in (0, 5)]
        check_batch(np.stack([t for t, _ in pairs]), np.stack([p for _, p in pairs]))


def test_pair_table_labels_near_int32_max():
    big = 2 ** 31 - 1
    pairs = [synth_inst_pair(200, 210, 50, seed=s, id_stride=1 + s, id_base=big - (1 + s) * 70) for s in range(3)]
    t, p = np.stack([t for t, _ in pairs]), np.stack([p for _, p in pairs])
    t[0, 0, 0], p[1, 5, 5] = big, big
    check_batch(t, p)


def spread_ids_map(seed):
    """300 x 300, ~400 instances whose ids are drawn without repeats from [1, 5e6]: present ids in ~39 of the bitmap's 4096-word
    blocks, so the prefix carries across blocks (rl_scan_sums) and into each block (rl_word_prefix) are not zero."""
    t, _ = synth_inst_pair(300, 300, 400, seed=seed)
    ids = np.unique(t)[1:]
    new = np.sort(np.random.default_rng(seed).choice(np.arange(1, 5_000_001), len(ids), replace=False)).astype(np.int32)
    lut = np.zeros(int(t.max()) + 1, np.int32)
    lut[ids] = new
    out = lut[t]
    assert (out.max() >> 5) // 4096 >= 30
    return out


@pytest.mark.parametrize("by_size", [False, True])
def test_remap_label_device_equals_host(by_size):
    maps = [synth_inst_pair(h, w, k, seed=k, id_stride=s, id_base=b)[1]
            for (h, w, k, s, b) in [(64, 64, 10, 1, 0), (257, 300, 90, 13, 1000), (100, 90, 30, 1, 2 ** 31 - 40)]]
    ties = np.zeros((12, 12), np.int32)
    ties[0:2, 0:2], ties[4:6, 4:6], ties[8:11, 8:11], ties[0:2, 8:10] = 7, 3, 5, 11
    maps.append(ties)
    for m in maps:
        got = M.remap_label(torch.from_numpy(m).to(DEV), by_size=by_size)
        assert got.is_cuda and got.dtype == torch.int32
        want = M.remap_label(m, by_size=by_size, device="cpu")
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(M.remap_label(m, by_size=by_size, device=DEV), want)
    spread = spread_ids_map(7)
    got = M.remap_label(torch.from_numpy(spread).to(DEV), by_size=by_size).cpu().numpy()
    assert np.array_equal(got, M.remap_label(spread, by_size=by_size, device="cpu"))
    batch = torch.from_numpy(np.stack([synth_inst_pair(96, 96, k, seed=k, id_stride=3)[0] for k in (1, 20, 45)] +
                                      [spread_ids_map(8)[:96, :96]])).to(DEV)
    got = M.remap_device(batch, by_size).cpu().numpy()
    for i in range(4):
        assert np.array_equal(got[i], M.remap_label(batch[i].cpu().numpy(), by_size=by_size, device="cpu"))
    z = torch.zeros((5, 5), dtype=torch.int32, device=DEV)
    assert M.remap_label(z) is z
    for bad in (torch.ones((5, 5), dtype=torch.int32, device=DEV), torch.full((5, 5), -2, dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError):
            M.remap_label(bad)


def test_device_path_reproduces_the_recorded_reference_values():
    d = np.load(FIXTURE)
    for c in cases(d):
        vals, pairs = case_values(d[c + "_true"], d[c + "_pred"], DEV)
        assert np.array_equal(vals, d[c + "_vals"]), c
        assert np.array_equal(pairs, d[c + "_pairs"]), c
    names = list(d["inst_names"])
    rows = M.instance_stats([d[c + "_true"] for c in names], [d[c + "_pred"] for c in names], device=DEV)
    assert np.array_equal(rows.T, d["inst_stat"])


def test_instance_stats_on_process_batch_device_output():
    from hover_net_amd import post_proc
    from hover_net_amd.synth import synth_pred_maps

    pm = synth_pred_maps(6, 164, 164, 5, seed=11)[0]
    pm2 = pm.copy()
    pm2[..., -2:] += np.random.default_rng(1).normal(0, 0.05, pm2[..., -2:].shape).astype(pm2.dtype)
    true, _, _ = post_proc.process_batch_device(torch.from_numpy(pm).to(DEV), nr_types=5)
    pred, _, _ = post_proc.process_batch_device(torch.from_numpy(np.ascontiguousarray(pm2)).to(DEV), nr_types=5)
    assert true.is_cuda and pred.is_cuda and true.dtype == torch.int32
    rows = M.instance_stats(true, pred)
    tn, pn = true.cpu().numpy(), pred.cpu().numpy()
    want = M.instance_stats(list(tn), list(pn), device="cpu")
    assert rows.shape == (6, 6) and np.array_equal(rows, want)
    assert (rows[:, 2] > 0).all()                          # the two segmentations do pair up


def test_compute_stats_on_mat_files_returns_the_recorded_arrays(tmp_path):
    import scipy.io as sio

    from hover_net_amd import compute_stats as CS

    d = np.load(FIXTURE)
    for sub in ("true", "pred"):
        os.makedirs(tmp_path / sub)
        for c in d["inst_names"]:
            sio.savemat(str(tmp_path / sub / (str(c) + ".mat")), {"inst_map": d[str(c) + "_" + sub]})
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = CS.run_nuclei_inst_stat(str(tmp_path / "pred"), str(tmp_path / "true"), print_img_stats=True)
    assert got.dtype == np.float64 and np.array_equal(got, d["inst_stat"])
    assert buf.getvalue().replace(str(tmp_path / "pred"), "<pred_dir>") == str(d["inst_stdout"])


def test_device_tables_reject_negative_labels():
    t, p = synth_inst_pair(40, 40, 8, seed=1)
    t[3, 3] = -5
    with pytest.raises(ValueError):
        M.pair_tables(torch.from_numpy(t[None]).to(DEV), torch.from_numpy(p[None]).to(DEV))


def test_reference_named_functions_score_a_stack_as_one_map_and_accept_float_maps():
    pairs = [synth_inst_pair(64, 64, k, seed=k) for k in (10, 12)]
    t, p = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    td, pd = torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV)
    assert M.get_dice_1(td, pd) == M.get_dice_1(t.reshape(1, -1), p.reshape(1, -1), device="cpu")
    assert M.get_dice_2(td, pd) == M.get_dice_2(t, p, device="cpu")
    tf, pf = t.astype(np.float64), p.astype(np.float64)
    assert M.get_dice_1(tf, pf, device=DEV) == M.get_dice_1(t, p, device="cpu")
    assert np.array_equal(M.remap_label(tf[0], device=DEV), M.remap_label(t[0], device="cpu"))
    with pytest.raises(TypeError):
        M.get_fast_pq(tf[0], pf[0], device=DEV)

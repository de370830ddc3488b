"""CPU: the host half of hover_net_amd/valid_stats.py -- the scalars from a hand-filled state, the rank merge over gloo
(int64 SUM all-reduce of the counts, rank-order sum of the all-gathered float64) and the ABI bookkeeping of the two exports.
The kernel itself is covered on the GPU by tests/test_gpu_valid_stats.py."""
import os
import struct

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_scalars_from_a_hand_filled_state():
    from hover_net_amd.valid_stats import ValidStats

    vs = ValidStats(3, "cpu")
    assert vs.counts.shape == (10,) and vs.hv_sse.shape == (1,) and vs.hv_sse.dtype == torch.float64
    #                          pixels np_correct np_inter np_total  type 0   type 1 (never seen)  type 2
    vs.counts.copy_(torch.tensor([1000, 901, 120, 260, 700, 1450, 0, 0, 2 ** 33, 2 ** 34 + 7]))
    vs.hv_sse[0] = 12.625
    got = vs.scalars()
    assert list(got) == ["np_acc", "np_dice", "tp_dice_0", "tp_dice_1", "tp_dice_2", "hv_mse"]
    assert got["np_acc"] == 901 / 1000
    assert got["np_dice"] == 2.0 * 120 / (260 + 1.0e-8)
    assert got["tp_dice_0"] == 2.0 * 700 / (1450 + 1.0e-8)
    assert got["tp_dice_1"] == 0.0                                        # 0 / (0 + 1e-8)
    assert got["tp_dice_2"] == 2.0 * 2 ** 33 / (2 ** 34 + 7 + 1.0e-8)     # counts beyond 2^31
    assert got["hv_mse"] == 12.625 / 1000
    assert vs.track() == {"scalar": got, "image": {}}
    vs.reset()
    assert not vs.counts.any() and vs.hv_sse[0] == 0.0

    no_types = ValidStats(None, "cpu")
    assert no_types.counts.shape == (4,)
    no_types.counts.copy_(torch.tensor([10, 5, 1, 4]))
    assert list(no_types.scalars()) == ["np_acc", "np_dice", "hv_mse"]


def test_update_has_no_cpu_fallback():
    import pytest

    from hover_net_amd import lib as L
    from hover_net_amd.valid_stats import ValidStats

    with pytest.raises(L.HvnError):
        ValidStats(None, "cpu").update(torch.zeros(1, 2, 2, 3), {"np_map": torch.zeros(1, 2, 2), "hv_map": torch.zeros(1, 2, 2, 2)})


_SSE = (1.0e16, 1.0, -1.0e16)       # (a + b) + c = 0, a + (b + c) = 0 too, but (a + c) + b = 1: the order of the additions shows


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _merge_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hover_net_amd.valid_stats import ValidStats

    vs = ValidStats(2, "cpu")
    vs.counts.copy_(torch.arange(8, dtype=torch.int64) * (rank + 1) + (2 ** 31 if rank == 0 else 0))
    vs.hv_sse[0] = _SSE[rank]
    vs.merge_ranks()
    q.put((rank, vs.counts.tolist(), _bits(vs.hv_sse[0])))
    dist.destroy_process_group()


def test_merge_ranks_over_gloo_gives_every_rank_the_rank_order_sum():
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30300 + (os.getpid() % 400)
    procs = [ctx.Process(target=_merge_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
    want_counts = [2 ** 31 + 6 * j for j in range(8)]              # j * (1 + 2 + 3) + rank 0's offset
    want_sse = (_SSE[0] + _SSE[1]) + _SSE[2]
    assert want_sse != (_SSE[0] + _SSE[2]) + _SSE[1]
    for rank, counts, sse_bits in res:
        assert counts == want_counts, (rank, counts)
        assert sse_bits == _bits(want_sse), (rank, sse_bits)


def test_merge_ranks_without_a_process_group_changes_nothing():
    from hover_net_amd.valid_stats import ValidStats

    assert not dist.is_initialized()
    vs = ValidStats(1, "cpu")
    vs.counts.copy_(torch.tensor([9, 8, 7, 6, 5, 4]))
    vs.hv_sse[0] = 0.1
    before = vs._buf.clone()
    vs.merge_ranks()
    assert torch.equal(vs._buf, before)


def test_workspace_size_is_host_arithmetic():
    from hover_net_amd import lib as L

    lib = L.lib()
    # the size query is host arithmetic: one float64 and 35 uint32 counts per workgroup of 1024 pixels, each part 256-byte aligned
    assert lib.hvn_valid_stats_workspace_bytes(1, 7, 9) == 256 + 256
    assert lib.hvn_valid_stats_workspace_bytes(16, 164, 164) == -(-421 * 8 // 256) * 256 + -(-421 * 35 * 4 // 256) * 256
    assert lib.hvn_valid_stats_workspace_bytes(0, 7, 9) == 0 and lib.hvn_valid_stats_workspace_bytes(1, -7, 9) == 0

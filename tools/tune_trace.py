#!/usr/bin/env python
"""Which launches does an engine build TIME?  One engine of one configuration is built in this (fresh) process with HVN_TUNE_REPS=1
while the library's single-launch entry points are wrapped by a recorder; prints the sorted set of
(entry point, op index, tile_n | mode at the launch, batch) and then the forms the engine ended up bound to.  The set depends on
the selection logic only (which shapes are timed on which candidates), the final forms on timing noise as well: compare the first
between two trees, read the second side by side.
usage: python tools/tune_trace.py cfg2 | cfg3 | train0 | train1
       (cfg 2: 'original', 5 types, fp32, batch 32; cfg 3: 'fast', 6 types, bf16, batch 64; the phase-0 / phase-1 training engines)"""
import ctypes
import os
import sys

os.environ["HVN_TUNE_REPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hover_net_amd import lib as L  # noqa: E402
from hover_net_amd import net_desc  # noqa: E402
from hover_net_amd.synth import synth_state_dict  # noqa: E402

CONFIGS = {"cfg2": ("original", 5, "fp32", 32), "cfg3": ("fast", 6, "bf16", 64), "train0": ("original", 5, True, 16), "train1": ("original", 5, False, 4)}


def main():
    name = sys.argv[1]
    mode, nt, how, bs = CONFIGS[name]
    lib = L.lib()
    seen = []                       # (entry point, address, count, code, batch)
    run_op, run_top = lib.hvn_run_op, lib.hvn_run_train_plan

    def rec_op(ptr, n, stream):
        seen.append(("op", int(ptr), 1, int(L.hvn_op.from_address(int(ptr)).tile_n), int(n)))
        return run_op(ptr, n, stream)

    def rec_top(ptr, count, n, stream):
        seen.append(("top", int(ptr), int(count), int(L.hvn_top.from_address(int(ptr)).mode) if count == 1 else -1, int(n)))
        return run_top(ptr, count, n, stream)

    lib.hvn_run_op, lib.hvn_run_train_plan = rec_op, rec_top
    net = net_desc.create_model(mode=mode, nr_types=nt, input_ch=3, **({"freeze": how} if name.startswith("train") else {}))
    net.load_state_dict(synth_state_dict(mode, nt, seed=0), strict=True)
    if name.startswith("train"):
        from hover_net_amd.train_engine import TrainEngine
        eng = TrainEngine(net.to("cuda"), bs)
        where = {ctypes.addressof(o): i for i, o in enumerate(eng._keep) if isinstance(o, L.hvn_op)}
        tbase, tsz = ctypes.addressof(eng.bwd_ops), ctypes.sizeof(L.hvn_top)
        final = [("op %d" % i, int(o.tile_n)) for i, o in enumerate(eng._keep) if isinstance(o, L.hvn_op) and o.kind == 2]
        final += [("top %d" % i, int(eng.bwd_ops[i].mode)) for i in range(len(eng.bwd_ops)) if eng.bwd_ops[i].kind == 5]
        final.append(("wgrad_stream", int(bool(eng.wgrad_stream))))
    else:
        net.max_batch, net.compute_dtype = bs, how
        eng = net.to("cuda").eval().engine(bs)
        obase, osz = ctypes.addressof(eng.ops), ctypes.sizeof(L.hvn_op)
        where = {obase + i * osz: i for i in range(len(eng.ops))}
        tbase, tsz = 0, 1
        final = [("op %d" % i, int(o.tile_n)) for i, o in enumerate(eng.ops) if o.kind in (2, 8)]
        final.append(("stream_offset", int(eng._stream_off)))
    lib.hvn_run_op, lib.hvn_run_train_plan = run_op, run_top
    timed = sorted({(ep, where[ptr] if ep == "op" else (ptr - tbase) // tsz, cnt, code, n) for ep, ptr, cnt, code, n in seen})
    print("# %s: %d timing launches, %d distinct (entry point, op index, ops in the call, tile_n | mode, batch)" % (name, len(seen), len(timed)))
    for row in timed:
        print("timed %s %d %d %d %d" % row)
    for what, v in final:
        print("final %s %d" % (what, v))


if __name__ == "__main__":
    main()

"""Launch-form selection for the inference and training engines.

Several launches exist in more than one bit-identical form (workgroup tile, LDS-DMA or register-resident kernel, split of the
weight-gradient sum, rotation of the stream pool).  Which form a launch runs on is invisible in every result, so it is decided by
time, once per process and launch shape: `candidates` says which forms a bound launch may run on, `time_launch` times one,
`choose` applies the one pick rule and keeps the answer in `CACHE`.  The engines own the rest: which ops they tune, at which
batch, and how one launch is issued."""
import math

import torch

from . import lib as L
from .knobs import KNOBS, knob  # noqa: F401  (the table and its reader, importable from here as before)
from .plan import OP_CHAIN, OP_CONV, _tile_n

MARGIN = 0.985              # a candidate replaces the baseline only when it is faster by more than 1.5 %
X3G_256, X3G_128 = 128 + 0x300, 128 + 0x200     # hvn_op.tile_n of the LDS-DMA forms of the bf16x3 / bf16 convolution (include/hvn.h)
X3R = 128 + 0x400                               # hvn_op.tile_n of the bf16x3 CHAIN with a register-resident input tile
T256X64 = 64 + 0x100                            # hvn_op.tile_n of the 256 x 64 workgroup tile of the 64-channel fp32 CONV
OPTIONAL = (X3G_256, X3G_128, X3R)              # forms the launcher may refuse for a geometry (32-bit reach of a 256-row tile)
WGRAD_TARGETS = (1536, 1024, 768, 512, 384)     # workgroups a non-deterministic weight-gradient launch may aim at (hvn_top.mode)
WG_SLOTS = 512              # resident 128x128 conv workgroups: 2 per CU (VGPRs) x 256 CUs

# (device, family, ...launch shape..., candidates) -> (choice, ms of the baseline, ms of the fastest other candidate, {candidate: ms}),
# one per process; family: infer-conv | infer-chain | infer-chain-x3 | infer-bf16 | train-conv | train-wgrad | streams
CACHE = {}


def tile_select():
    """HVN_TILE_SELECT as one value: "auto" | "model" | "0"."""
    v = knob("HVN_TILE_SELECT")
    if v not in ("auto", "model", "0"):
        raise ValueError("HVN_TILE_SELECT=%r: auto, model or 0" % v)
    return v


def time_launch(launch, reps=3, runs=1):
    """ms of `launch()` on the current stream: one warm-up, then the minimum over HVN_TUNE_REPS (default `reps`) HIP-event timings
    of `runs` calls each, per call."""
    reps = max(1, int(knob("HVN_TUNE_REPS") or reps))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for r in range(reps + 1):
        e0.record()
        for _ in range(runs):
            launch()
        e1.record()
        e1.synchronize()
        if r:
            best = min(best, e0.elapsed_time(e1) / runs)
    return best


def choose(cache, key, candidates, measure, margin=MARGIN, optional=OPTIONAL):
    """The pick rule.  `measure(c)` binds candidate c and returns its ms.  candidates[0] is the baseline; the fastest other one wins
    only if t < margin * t_baseline.  An `optional` candidate the launcher refuses (L.HvnError) counts as inf, any other refusal
    propagates.  One measurement per key and candidate tuple; -> the cache entry."""
    key = tuple(key) + (tuple(candidates),)
    if key not in cache:
        t = {}
        for c in candidates:
            try:
                t[c] = measure(c)
            except L.HvnError:
                if c not in optional:
                    raise
                t[c] = float("inf")
        base = candidates[0]
        best = min(candidates[1:], key=t.get)
        cache[key] = (best if t[best] < margin * t[base] else base, t[base], t[best], t)
    return cache[key]


def forced_form(o):
    """The optional form HVN_X3G_FORCE / HVN_BF16G_FORCE / HVN_CHAIN_X3R=force asks for on inference launches of o's kind, or None."""
    if o.kind == OP_CHAIN:
        return X3R if knob("HVN_CHAIN_X3R") == "force" else None
    v = knob("HVN_BF16G_FORCE" if o.act_dtype == 1 else "HVN_X3G_FORCE")
    return int(v) if v else None


def pick(cache, key, candidates, measure, forced=None, optional=OPTIONAL, **kw):
    """-> the form to bind.  `forced` names an optional form to take untimed: where it is a candidate it is launched through
    `measure` once and kept, a refusal gives the baseline, and the cache is neither read nor written; anywhere else it means nothing."""
    if forced in optional and forced in candidates[1:]:
        try:
            measure(forced)
            return forced
        except L.HvnError:
            return candidates[0]
    return choose(cache, key, candidates, measure, optional=optional, **kw)[0]


def entries(family, device=None):
    """[(key, entry)] of one family (tools: the key's launch shape starts at key[2], with the batch)."""
    return [(k, v) for k, v in CACHE.items() if k[1] == family and (device is None or k[0] == str(device))]


def launch_key(device, family, o, batch):
    """Cache key of a bound CONV / CHAIN launch: everything its time depends on."""
    return (str(device), family, int(batch), o.kh, o.kw, o.stride, o.pad_t, o.x.c, o.cout, o.cout2, o.y.h, o.y.w, o.x.h, o.x.w, bool(o.res.base),
            bool(o.pre_scale), bool(o.post_scale), int(o.nbatch), int(o.x2.c) if o.x2.base else 0, int(o.act_dtype), int(o.groups))


def x3g_forms_for(o):
    """The LDS-DMA workgroup shapes (csrc/hvn_conv_x3g.hip) a bf16x3 CONV launch may run on besides hvn_conv_x3.hip's, as tile_n codes:
    they need >= 128 output channels and -- the 256-row form with a prologue -- its two per-channel vectors next to the operand rings
    in the CU's 160 KB of LDS.  Same packing, same bits (tests/test_gpu_x3.py)."""
    want = knob("HVN_X3G")
    if want == "0" or o.cout < 128 or o.groups > 1:
        return ()
    forms = []
    for code, bm, na in ((X3G_256, 256, 3), (X3G_128, 128, 2)):
        if want not in ("1", str(code)):
            continue
        if o.pre_scale and bm == 256 and na * bm * 128 + 2 * 3 * 128 * 64 + 2 * o.x.c * 4 > 160 * 1024:
            continue                                   # (the 128-row form reads the prologue's vectors from global memory)
        forms.append(code)
    return tuple(forms)


def candidates(o):
    """The forms (tile_n codes) a bound hvn_op may run on, baseline first; () = nothing to choose.  All forms of a launch read the
    same packed weights and keep the k order of every output element: same bits."""
    x3, bf16 = o.act_dtype in (2, 3), o.act_dtype == 1
    if o.kind == OP_CHAIN:
        if x3:      # csrc/hvn_conv_chain_x3r.hip exists for a 64-channel input (and, with a fused shortcut, 64 -> 64 without a residual)
            if knob("HVN_CHAIN_X3R") == "0" or o.x.c != 64 or (o.x2.base and (o.x2.c != 64 or o.res.base or o.cout2 != 64)):
                return ()
            return (128, X3R)
        return () if bf16 else (128, 64)                # chained 1x1 convs: 128 or 64 pixels per workgroup
    if o.kind != OP_CONV or o.groups > 1:
        return ()
    static = _tile_n(o.cout)
    if bf16:        # csrc/hvn_conv_bf16g.hip: >= 128 output channels, no prologue, one problem per launch
        if static != 128 or o.pre_scale or o.nbatch > 1 or knob("HVN_BF16G") == "0":
            return ()
        return (128, X3G_256, X3G_128)
    if static == 128:
        return (128, 64) + (x3g_forms_for(o) if x3 else ())
    if static == 64 and not x3 and not o.x2.base:       # the fused-shortcut and bf16x3 instantiations have no 256 x 64 tile
        return (64, T256X64)
    return ()


def pick_tile_n(op, batch):
    """Column tile (128 or 64) of a CONV launch by its wave quantisation -- the MODEL behind `HVN_TILE_SELECT=model` and the
    starting point of the measured selection (`Engine.autotune_tiles`, the default): a launch of W workgroups runs in
    ceil(W / slots) rounds, so 1092 workgroups of 128x128 tiles (2.13 rounds -> 3) lose 29 % to the last round.  The packed
    weights are the same for both widths (cout is padded to 128) and so is every output bit (same k order per element).  Only
    plain launches with cout >= 128 are re-tiled; HVN_TILE_SELECT=0 keeps the static choice of plan._tile_n."""
    if op.tile_n != 128 or tile_select() == "0":
        return op.tile_n
    force = knob("HVN_FORCE_TILE_N")
    if force:
        return int(force)
    slots64 = int(knob("HVN_WG_SLOTS_64"))
    cost64 = float(knob("HVN_NARROW_COST"))
    m_tiles = math.ceil(batch * op.y.h * op.y.w / 128.0)
    nb = int(op.extra.get("nbatch", 1))
    wide = math.ceil(m_tiles * math.ceil(op.cout / 128.0) * nb / WG_SLOTS)
    narrow = math.ceil(m_tiles * math.ceil(op.cout / 64.0) * nb / slots64) * cost64
    return 64 if narrow < wide else 128

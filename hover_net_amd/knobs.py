"""Every HVN_* environment variable the package and libhvn_hip.so read: name -> (default, meaning).

The environment is the configuration surface; this table is its one description (INTEGRATION.md prints it) and `knob` its one reader
on the Python side: the string from the environment at CALL time, never at import, or the table's default.  Callers parse what they
get (`int(...)`, `!= "0"`).  A default of "" means: unset -- either the switch is off, or the default depends on the caller, who keeps
its own `or`-fallback.  The names of `C_KNOBS` are read by the library (csrc/hvn_env.h is its one reader); their defaults are listed
here as the library applies them.  tests/test_knobs.py holds the table, the two readers and the document to each other."""
import os

PY_KNOBS = {
    # which library is loaded
    "HVN_LIB_VARIANT": ("", "prev | trace | fullepi: load libhvn_hip_<variant>.so instead of libhvn_hip.so (lib.VARIANTS; A/B and diagnosis runs)"),
    # the network as the model object sees it
    "HVN_DTYPE": ("fp32", "fp32 | bf16: compute type of a HoVerNet built without one"),
    "HVN_BF16_CHAIN": ("d0d1", "d0 | d0d1: the blocks whose conv3 -> conv1 seams the bf16 plan chains (default from the measurement: DESIGN section 4.8) | 0: none"),
    # the inference plan
    "HVN_CHAIN": ("1", "0: no chained 1x1 launches in the fp32 plan (same bits unchained)"),
    "HVN_CHAIN_MAXN2": ("128", "most output channels (64 | 128) of the second convolution of a chained launch"),
    "HVN_WINOGRAD": ("4", "output tile m of F(m x m, 5x5) for the decoder's 5x5 convs | 0: direct convolutions"),
    "HVN_WINOGRAD_STAGES": ("u3:6", "per decoder stage override of that tile, e.g. u3:6,u2:4"),
    "HVN_WINOGRAD3": ("128", "minimum channel count for the Winograd form of the encoder's 3x3 convs | 0: off"),
    "HVN_WINOGRAD3_M": ("6", "its output tile: F(6x6,3x3) | 4: F(4x4,3x3)"),
    "HVN_WINO_CACHE_MB": ("2048", "bound of the host cache of Winograd-packed weights"),
    "HVN_X3": ("6", "partial products of the bf16x3 convolutions: 6 | 9 | 0: every conv on the fp32 matrix pipe"),
    "HVN_X3_D1": ("1", "0: d1's 1x1 convs stay chained pairs on the fp32 pipe"),
    "HVN_X3_CHAIN": ("d0", "d0 | d0d1: the blocks whose chained seams run on the bf16 pipe (bf16x3) | empty: chains on the fp32 pipe"),
    "HVN_FUSE_UPADD": ("0", "1: UpSample2x + skip add folded into the Winograd input transform (measured slower; kept for its test)"),
    # the inference engine
    "HVN_SPLIT": ("", "encoder sub-batches of the inference engine (default 2 for fp32, 1 for bf16)"),
    "HVN_LANES": ("", "extra streams for the decoder branches (default 2 for fp32, 0 for bf16: one launch stream)"),
    "HVN_SPLIT_DECODER": ("0", "1: the decoder launches run per encoder sub-batch too, not on the whole batch"),
    # launch-form selection (tune.py)
    "HVN_TILE_SELECT": ("auto", "auto: forms picked by time at engine build | model: inference CONV tiles by pick_tile_n's rounds model, nothing timed | 0: the plan's static tiles"),
    "HVN_TUNE_REPS": ("", "timings per candidate after the warm-up launch (default 3; 2 for the weight-gradient stream pass)"),
    "HVN_TUNE_SUB": ("1", "0: a split inference engine times its encoder launches at the full batch instead of the sub-batch"),
    "HVN_FORCE_TILE_N": ("", "64 | 128: that column tile for every re-tileable fp32 inference CONV, nothing timed"),
    "HVN_WG_SLOTS_64": ("768", "rounds model: resident 128x64 workgroups on the chip"),
    "HVN_NARROW_COST": ("0.45", "rounds model: time of a round of 128x64 tiles relative to a round of 128x128 tiles"),
    "HVN_X3G": ("1", "LDS-DMA forms of the bf16x3 CONV: 0 none | 896 | 640 that form only | 1 both"),
    "HVN_X3G_FORCE": ("", "896 | 640: that bf16x3 LDS-DMA form wherever it is a candidate, nothing timed"),
    "HVN_BF16G": ("1", "0: no LDS-DMA forms of the bf16 CONV"),
    "HVN_BF16G_FORCE": ("", "896 | 640: that bf16 LDS-DMA form wherever it is a candidate, nothing timed"),
    "HVN_CHAIN_X3R": ("1", "register-resident form of the bf16x3 CHAIN: 0 never | force wherever it is a candidate | 1 by time"),
    "HVN_STREAM_SELECT": ("1", "0: the inference launch schedule keeps rotation 0 of the stream pool"),
    "HVN_TILE_SHARE": ("1", "0: data-parallel ranks keep their own measured launch shapes (no broadcast from rank 0)"),
    "HVN_TILE_FILE": ("", "path of a JSON list of per-op tile_n codes an fp32 inference engine binds instead of timing"),
    # the training engine
    "HVN_TRAIN_DETERMINISTIC": ("1", "0: weight-gradient sums by atomics instead of stored partials in a fixed order"),
    "HVN_TRAIN_WINOGRAD": ("1", "0: the decoder's 5x5 convs direct in all three passes"),
    "HVN_TRAIN_FIRST_STORE": ("1", "0: every backward launch accumulates and the whole gradient arena is cleared per step"),
    "HVN_TRAIN_BRANCH_STREAMS": ("1", "0: the decoder branches on one stream"),
    "HVN_TRAIN_WGRAD_STREAM": ("auto", "auto: weight gradients on a side stream if timed faster at engine build | 1 | 0 force it"),
    "HVN_TRAIN_X3": ("6", "partial products of the training convs: 6 | 9 | 0: the fp32 pipe"),
    "HVN_TRAIN_WGRAD_X3": ("1", "1: weight gradients as the forward convs | 6 | 9 | 0: the fp32 pipe"),
    "HVN_TRAIN_PACK_MULTI": ("1", "0: one weight-packing launch per layer instead of one multi-layer launch"),
    # whole-slide inference
    "HVN_WSI_LANES": ("3", "post-processing lanes (stream + workspace) of the whole-slide pipeline"),
    "HVN_WSI_HOST_MERGE": ("0", "1: merge tile instances on the host instead of the device"),
}

C_KNOBS = {
    "HVN_HOST_THREADS": ("", "host threads of the contour tracer (default: the hardware's, at most 16)"),
    "HVN_WGRAD_WGS": ("", "workgroups a weight-gradient launch aims at, over the engine's choice (default 1536); read per launch"),
    "HVN_WGRAD_MIN_ROWS": ("256", "least pixels per split of a weight-gradient sum; read per launch"),
    "HVN_WS_GLOBAL": ("0", "1: the watershed replays every tile whole (the reference path of its test)"),
    "HVN_WS_WAVE": ("1", "0: every watershed component floods on the one-lane binary heap (A/B and tests)"),
    "HVN_WS_BITMAP": ("1", "0: watershed windows beyond the LDS keep keys and labels in HBM scratch (the round-2 form, A/B)"),
    "HVN_WS_STATS": ("", "set: print which replay each watershed component took (synchronous)"),
    "HVN_CONV_TRACE": ("", "path: per-workgroup timestamps of the last fp32 CONV launch (synchronous; tools/conv_trace.py)"),
    "HVN_CHAIN_TRACE": ("", "path: per-workgroup timestamps of the last fp32 CHAIN launch (synchronous)"),
}

KNOBS = {**PY_KNOBS, **C_KNOBS}


def knob(name):
    return os.environ.get(name, KNOBS[name][0])

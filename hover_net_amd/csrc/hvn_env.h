// hvn_env.h -- the library's one reader of the process environment: no other file under csrc/ calls getenv.
//
// The names read on this side (hover_net_amd/knobs.py holds the whole table with defaults and meanings, INTEGRATION.md prints it):
//   once per process (a function-local `static const`, initialised thread-safely at the first launch that asks)
//     HVN_WS_GLOBAL, HVN_WS_WAVE, HVN_WS_BITMAP   forms of the watershed flood
//     HVN_CONV_TRACE, HVN_CHAIN_TRACE             presence switches the per-workgroup stamps on (the buffer is allocated once) ...
//   at every launch
//     HVN_CONV_TRACE, HVN_CHAIN_TRACE             ... and the value is the path the stamps of the LAST launch are written to
//     HVN_WGRAD_WGS, HVN_WGRAD_MIN_ROWS           split of the weight-gradient sum (tools/wgrad_sweep.py changes them between launches)
//     HVN_HOST_THREADS                            host threads of the contour tracer (default: the hardware's, at most 16)
//     HVN_WS_STATS                                presence: print which replay each watershed component took (synchronous)
#pragma once
#include <stdlib.h>

// the value of `name`, or nullptr when it is not set (presence switches test the pointer)
static inline const char *hvn_env_str(const char *name) { return getenv(name); }

// atoi of `name`'s value, or `dflt` when it is not set
static inline int hvn_env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

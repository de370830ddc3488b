// hvn_forest.hip -- the minimum spanning forest and the connected components of a CSR graph over nucleus centroids, by Boruvka rounds
// (hover_net_amd/forest.py is the definition).  HVN_OP_NBR_FOREST reads the points by position and a symmetric CSR graph
// (graph.py's CellGraph, rows in any order) and needs no grid.
//
//   key{i, j} = (d2(i, j), min(i, j), max(i, j)), lexicographic; d2 by hvn_nbr_d2, as every op of the family.  d2 is >= +0.0 and never
//   NaN for checked points, so its bit pattern as a uint64 orders as the double does, and the all-ones word is above every key.
//   {i, j} is in the forest  <=>  its ends are not connected by edges of strictly smaller key.
// Keys are pairwise distinct, so the forest is unique and every component's smallest outgoing edge belongs to it (the cut property).
//
// The workspace, by position: best_d2, best_pair (uint64 [N]), parent, comp, minpos (int32 [N]) and 64 control words.  comp[i] is the
// root of i's component so far -- a position -- and parent is read and written at roots only.
//   fo_start      comp = parent = i, minpos = INT_MAX, best_* = all ones; tree and the control words are cleared by memset in stream order
// one round r, four kernels, a lane per vertex:
//   fo_pick_d2    walks row i; over the j with comp[j] != comp[i] the smallest d2 bits; atomicMin on best_d2[comp[i]], after a read of that
//                 word that skips the atomic where it is already no larger; sets found[r].  Returns at once when round r - 1 hooked nothing
//   fo_pick_pair  walks row i again; over the outgoing j whose bits equal best_d2[comp[i]] the smallest (lo << 32 | hi); atomicMin on
//                 best_pair[comp[i]], filtered in the same way
//   fo_hook       the one vertex that is an end of best_pair[comp[i]] and whose other end j lies outside: sets `tree` at its entry of row
//                 i and, after a scan of row j for i, at that entry too; parent[comp[i]] = comp[j], unless comp[j] picked the same edge
//                 and comp[i] < comp[j] (a mutual pick: the smaller root stays); the hooks are counted per wave into hooks[r]
//   fo_flatten    comp[i] = the root above comp[i], with path halving; best_*[i] = all ones for the next round
//                 (the last three return at once when found[r] is 0: nothing was picked, so nothing is left to reset either)
// after max(1, ceil(log2 N)) rounds -- the components that still have an outgoing edge at least halve per round --
//   fo_minpos     atomicMin(minpos[comp[i]], i), one atomic per wave where the wave shares one root
//   fo_name       component[i] = minpos[comp[i]]; lane 0 counts the rounds whose hooks word is not 0 into the rounds word
// No output depends on atomic arrival: the atomics are integer minima and a count that is only compared with 0; `tree` is addressed by
// CSR entry, `component` is a minimum of positions; parent[c] has one writer per round; path halving stores ancestors only.
//
// Bounds, whatever the arrays hold: every indptr value is clamped into [0, E]; an indices entry outside [0, N) is skipped; comp and parent
// values are written by these kernels from values checked against N, and fo_flatten checks what it reads all the same and ends after N
// steps; the row scans are bounded by a row's length; the round loop by R.  A graph that is not symmetric gives wrong numbers, never an
// access outside the arrays or a loop without an end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define FO_T 256
#define FO_NONE 0xFFFFFFFFFFFFFFFFull
#define FO_HOOKS 0                    // control words: hooks[32]
#define FO_ROUNDS 32                  //                the rounds that hooked anything
#define FO_FOUND 33                   //                found[HVN_NBR_FOREST_MAX_ROUNDS]

typedef unsigned long long fo_u64;

struct ForestDev {
    const double *xy;
    const long long *indptr;
    const int *indices;
    int *component;
    unsigned char *tree;
    fo_u64 *best_d2, *best_pair;
    int *parent, *comp, *minpos;
    unsigned *ctrl;
    long long E;
    int N, round, no_filter;
};

// row i as [b, e), both clamped into [0, E]
__device__ __forceinline__ void fo_row(const ForestDev &a, int i, long long &b, long long &e)
{
    b = a.indptr[i];
    e = a.indptr[i + 1];
    b = b < 0 ? 0 : (b > a.E ? a.E : b);
    e = e < 0 ? 0 : (e > a.E ? a.E : e);
}

__device__ __forceinline__ fo_u64 fo_bits(const ForestDev &a, int i, double xi, double yi, int j)
{
    return (fo_u64)__double_as_longlong(hvn_nbr_d2(a.xy[2 * (long)j], a.xy[2 * (long)j + 1], xi, yi));
}

// atomicMin(word, v), skipped where a read of the word shows it is already no larger (the word only ever falls)
__device__ __forceinline__ void fo_min(const ForestDev &a, fo_u64 *word, fo_u64 v)
{
    if (a.no_filter || __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(word, v);
}

__global__ __launch_bounds__(FO_T) void fo_start(const ForestDev a)
{
    const long q = (long)blockIdx.x * FO_T + threadIdx.x;
    if (q >= a.N) return;
    a.comp[q] = (int)q;
    a.parent[q] = (int)q;
    a.minpos[q] = 0x7FFFFFFF;
    a.best_d2[q] = FO_NONE;
    a.best_pair[q] = FO_NONE;
}

__global__ __launch_bounds__(FO_T) void fo_pick_d2(const ForestDev a)
{
    if (a.round > 0 && a.ctrl[FO_HOOKS + a.round - 1] == 0) return;               // the round before hooked nothing: the forest is done
    const long q = (long)blockIdx.x * FO_T + threadIdx.x;
    if (q >= a.N) return;
    const int i = (int)q, c = a.comp[i];
    const double xi = a.xy[2 * q], yi = a.xy[2 * q + 1];
    long long b, e;
    fo_row(a, i, b, e);
    fo_u64 m = FO_NONE;
    for (long long k = b; k < e; ++k) {
        const int j = a.indices[k];
        if ((unsigned)j >= (unsigned)a.N || a.comp[j] == c) continue;
        const fo_u64 d = fo_bits(a, i, xi, yi, j);
        m = d < m ? d : m;
    }
    if (m == FO_NONE) return;
    fo_min(a, a.best_d2 + c, m);
    a.ctrl[FO_FOUND + a.round] = 1u;
}

__global__ __launch_bounds__(FO_T) void fo_pick_pair(const ForestDev a)
{
    if (a.ctrl[FO_FOUND + a.round] == 0) return;
    const long q = (long)blockIdx.x * FO_T + threadIdx.x;
    if (q >= a.N) return;
    const int i = (int)q, c = a.comp[i];
    const fo_u64 target = a.best_d2[c];
    if (target == FO_NONE) return;                                                // a finished component
    const double xi = a.xy[2 * q], yi = a.xy[2 * q + 1];
    long long b, e;
    fo_row(a, i, b, e);
    fo_u64 m = FO_NONE;
    for (long long k = b; k < e; ++k) {
        const int j = a.indices[k];
        if ((unsigned)j >= (unsigned)a.N || a.comp[j] == c || fo_bits(a, i, xi, yi, j) != target) continue;
        const fo_u64 pair = i < j ? ((fo_u64)(unsigned)i << 32) | (unsigned)j : ((fo_u64)(unsigned)j << 32) | (unsigned)i;
        m = pair < m ? pair : m;
    }
    if (m != FO_NONE) fo_min(a, a.best_pair + c, m);
}

__global__ __launch_bounds__(FO_T) void fo_hook(const ForestDev a)
{
    if (a.ctrl[FO_FOUND + a.round] == 0) return;
    const long q = (long)blockIdx.x * FO_T + threadIdx.x;
    bool hooked = false;
    if (q < a.N) {
        const int i = (int)q, c = a.comp[i];
        const fo_u64 pair = a.best_pair[c];
        const unsigned lo = (unsigned)(pair >> 32), hi = (unsigned)pair;
        // the pick of component c is {lo, hi}; the lane of its end inside c takes it
        const unsigned other = lo == (unsigned)i ? hi : (hi == (unsigned)i ? lo : 0xFFFFFFFFu);
        if (pair != FO_NONE && other < (unsigned)a.N) {
            const int j = (int)other, cj = a.comp[j];
            if (cj != c) {
                long long b, e;
                fo_row(a, i, b, e);
                for (long long k = b; k < e; ++k) {
                    if (a.indices[k] == j) {
                        a.tree[k] = 1;
                        break;
                    }
                }
                fo_row(a, j, b, e);
                for (long long k = b; k < e; ++k) {
                    if (a.indices[k] == i) {
                        a.tree[k] = 1;
                        break;
                    }
                }
                if (!(a.best_pair[cj] == pair && c < cj)) {                       // not the smaller root of a mutual pick
                    a.parent[c] = cj;
                    hooked = true;
                }
            }
        }
    }
    const fo_u64 m = __ballot(hooked);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(a.ctrl + FO_HOOKS + a.round, (unsigned)__popcll(m));
}

__global__ __launch_bounds__(FO_T) void fo_flatten(const ForestDev a)
{
    if (a.ctrl[FO_FOUND + a.round] == 0) return;
    const long q = (long)blockIdx.x * FO_T + threadIdx.x;
    if (q >= a.N) return;
    int s = a.comp[q];
    for (int n = 0; n < a.N; ++n) {                                               // at most N steps, whatever parent holds
        const int p = __hip_atomic_load(a.parent + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)p >= (unsigned)a.N || p == s) break;                        // a root
        const int pp = __hip_atomic_load(a.parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)pp < (unsigned)a.N && pp != p) __hip_atomic_store(a.parent + s, pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // an ancestor
        s = p;
    }
    a.comp[q] = s;
    a.best_d2[q] = FO_NONE;
    a.best_pair[q] = FO_NONE;
}

__global__ __launch_bounds__(FO_T) void fo_minpos(const ForestDev a)
{
    const long q = (long)blockIdx.x * FO_T + threadIdx.x;
    const bool valid = q < a.N;
    const int root = valid ? a.comp[q] : -1;
    const fo_u64 lanes = __ballot(valid);
    if (!lanes) return;                                                           // wave-uniform
    const int first = __ffsll((long long)lanes) - 1;
    const int root0 = __shfl(root, first, 64);
    if (__ballot(valid && root != root0)) {                                       // several components in this wave: one atomic per vertex
        if (valid) atomicMin(a.minpos + root, (int)q);
        return;
    }
    if ((threadIdx.x & 63) == first) atomicMin(a.minpos + root0, (int)q);         // one component: its first lane holds the smallest position
}

__global__ __launch_bounds__(FO_T) void fo_name(const ForestDev a)
{
    const long q = (long)blockIdx.x * FO_T + threadIdx.x;
    if (q >= a.N) return;
    a.component[q] = a.minpos[a.comp[q]];
    if (q == 0) {
        unsigned rounds = 0;
        for (int r = 0; r < HVN_NBR_FOREST_MAX_ROUNDS; ++r) rounds += a.ctrl[FO_HOOKS + r] != 0 ? 1u : 0u;
        a.ctrl[FO_ROUNDS] = rounds;
    }
}

int hvn_launch_nbr_forest(const NbrForestArgs &a, hipStream_t stream)
{
    ForestDev d;
    char *w = (char *)a.workspace;
    d.xy = a.xy; d.indptr = a.indptr; d.indices = a.indices; d.component = a.component; d.tree = a.tree;
    d.best_d2 = (fo_u64 *)w; d.best_pair = d.best_d2 + a.N;
    d.parent = (int *)(d.best_pair + a.N); d.comp = d.parent + a.N; d.minpos = d.comp + a.N;
    d.ctrl = (unsigned *)(d.minpos + a.N);
    d.E = a.E; d.N = a.N; d.round = 0; d.no_filter = a.no_filter;
    const dim3 grid((unsigned)(((long)a.N + FO_T - 1) / FO_T)), block(FO_T);
    int rounds = 1;
    while ((1L << rounds) < (long)a.N) ++rounds;                                  // max(1, ceil(log2 N)) <= 26
    if (a.phase == 0 || a.phase == 1) {
        if (a.E > 0 && hipMemsetAsync(a.tree, 0, (size_t)a.E, stream) != hipSuccess) return HVN_E_LAUNCH;
        if (hipMemsetAsync(d.ctrl, 0, 256, stream) != hipSuccess) return HVN_E_LAUNCH;
        hipLaunchKernelGGL(fo_start, grid, block, 0, stream, d);
    }
    if (a.phase == 0 || a.phase == 2) {
        for (int r = a.phase == 2 ? a.round : 0; r < (a.phase == 2 ? a.round + 1 : rounds); ++r) {
            d.round = r;
            hipLaunchKernelGGL(fo_pick_d2, grid, block, 0, stream, d);
            hipLaunchKernelGGL(fo_pick_pair, grid, block, 0, stream, d);
            hipLaunchKernelGGL(fo_hook, grid, block, 0, stream, d);
            hipLaunchKernelGGL(fo_flatten, grid, block, 0, stream, d);
        }
    }
    if (a.phase == 0 || a.phase == 3) {
        hipLaunchKernelGGL(fo_minpos, grid, block, 0, stream, d);
        hipLaunchKernelGGL(fo_name, grid, block, 0, stream, d);
    }
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

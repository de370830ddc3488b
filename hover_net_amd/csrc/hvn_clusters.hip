// hvn_clusters.hip -- DBSCAN clusters of nucleus centroids over the neighbour grid (hover_net_amd/clusters.py is the definition,
// DESIGN.md 4.19).  HVN_OP_NBR_CLUSTER runs after HVN_OP_NBR_GRID on the same stream and reads its workspace as that op left it.
//
// A point is SELECTED when the type mask holds its type (mask 0xFFFFFFFF: every point).  degree = 1 + the number of selected
// neighbours (d2 <= r2 with hvn_neighbours.hip's d2, float64, one rounding per operation) of a selected point, 0 otherwise; a CORE has
// degree >= min_pts; a cluster is a connected component of the cores, named by the smallest POSITION among its cores; a selected
// non-core takes the label of its (d2, j)-smallest core neighbour, everything else -1.
//
// All work is in SLOT space (the cell-ordered index of the grid workspace).  The 3 x 3 cells of a point are three contiguous runs of
// slots (hvn_neighbours.hip); `cl_walk` is the one candidate loop of all three walking kernels: a lane owns one slot, a wave forms
// the union of its lanes' runs per grid row and walks that union with wave-uniform bounds, so every lane reads the same candidate
// (one address per wave: a broadcast) and tests it only inside its own run.  This is the plain form: candidates come from global
// memory (L1 / the scalar cache), not through an LDS staging tile as in nb_query.
//   cl_degree   counts the selected neighbours; writes degree by slot (second workspace) and by position (output), parent[s] = s,
//               minpos[s] = none: every word of the second workspace that a later kernel reads is written here
//   cl_link     every core slot s tests the core candidates t < s and unites the two trees where d2 <= r2 (lock-free union-find:
//               the larger root is hooked under the smaller with one atomicCAS).  A lane remembers the ancestor its last union
//               left it with and skips a candidate whose root is that slot: ancestors stay ancestors (only roots are ever hooked),
//               so the skipped pair is in one tree already.  Most pairs of a grown cluster end there, after one find that all lanes
//               of the wave share (the candidate is wave-uniform), instead of a divergent find from every lane's own slot
//   cl_roots    every core: atomicMin(minpos[find(s)], spos[s]) -- the root's name is the smallest position, whatever the arrival
//               order inside a cell made of the slots; a wave whose cores share one root reduces first and sends one atomic
//   cl_assign   core: label = minpos[find(s)]; selected non-core: the (d2, j)-smallest core candidate, kept in registers, gives its
//               label, or -1; unselected: -1
// The trees depend on arrival order; the outputs do not: degree is an integer sum, the partition of the cores is the set of
// connected components, a root's name is a minimum over its cores, a border's choice a minimum under the total order (d2, j).
//
// Termination, for ANY content of the two workspaces (these loops never wait for another thread):
//   * cl_find steps from s only to a parent p with 0 <= p < s and otherwise takes s for a root: at most N steps, all inside [0, N);
//     path halving stores only such a p (an ancestor, strictly smaller) into parent[s];
//   * cl_unite retries only when the failed atomicCAS returned a value strictly below the slot it tried to hook; the next pair of
//     roots is then strictly below that slot, so the larger of the two falls with every retry: at most N retries;
//   * every candidate loop runs from a clamped cell_start value to a clamped cell_start value, both in [0, N];
//   * every output row (a position read from the workspace) is checked against N.
// A workspace that HVN_OP_NBR_GRID did not fill gives wrong numbers, no access outside the arrays and no loop without an end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define CL_T 256
#define CL_NONE 0x7FFFFFFF

struct ClusterDev {
    const double *sx, *sy, *table;
    const int *spos, *stype, *cell_start;
    int *parent, *minpos, *sdeg;        // the second workspace, by slot
    int *label, *degree;                // the outputs, by position
    int N, ncy, ncx, min_pts;
    unsigned mask;
};

__device__ __forceinline__ bool cl_selected(unsigned mask, int type) { return mask == 0xFFFFFFFFu || ((unsigned)type < 16u && ((mask >> type) & 1u)); }

// this lane's slot: its point, its cell; false past the end
struct ClusterLane {
    double x, y;
    int pos, type, cx, cy;
};

__device__ __forceinline__ bool cl_lane(const ClusterDev &a, long q, ClusterLane &l)
{
    l.x = l.y = 0.0;
    l.pos = -1;
    l.type = -1;
    l.cx = l.cy = 0;
    if (q >= a.N) return false;
    l.x = a.sx[q];
    l.y = a.sy[q];
    l.pos = a.spos[q];
    l.type = a.stype[q];
    l.cx = hvn_nbr_axis(l.x, a.table[0], a.table[2], a.ncx);
    l.cy = hvn_nbr_axis(l.y, a.table[1], a.table[2], a.ncy);
    return true;
}

// f(g) for every slot g < cap in the 3 x 3 cells of an active lane.  Called by every lane of the wave (the shuffles need them all).
template <class F>
__device__ __forceinline__ void cl_walk(const ClusterDev &a, bool active, const ClusterLane &l, int cap, F &&f)
{
    const int N = a.N;
    for (int r = 0; r < 3; ++r) {
        const int yy = l.cy + r - 1;
        int lo = CL_NONE, hi = 0;           // this lane's run in grid row yy; empty: (CL_NONE, 0)
        if (active && yy >= 0 && yy < a.ncy) {
            const long row = (long)yy * a.ncx;
            const int ca = l.cx > 0 ? l.cx - 1 : 0, cb = l.cx + 1 < a.ncx ? l.cx + 1 : a.ncx - 1;
            lo = hvn_nbr_clamp(a.cell_start[row + ca], N);
            hi = hvn_nbr_clamp(a.cell_start[row + cb + 1], N);
            hi = hi < cap ? hi : cap;
            if (hi <= lo) {
                lo = CL_NONE;
                hi = 0;
            }
        }
        int wlo = lo, whi = hi;             // the wave's union
        for (int d = 32; d > 0; d >>= 1) {
            const int ol = __shfl_xor(wlo, d, 64), oh = __shfl_xor(whi, d, 64);
            wlo = ol < wlo ? ol : wlo;
            whi = oh > whi ? oh : whi;
        }
        wlo = __builtin_amdgcn_readfirstlane(wlo);
        whi = __builtin_amdgcn_readfirstlane(whi);
        for (int g = wlo; g < whi; ++g)     // 0 <= wlo, whi <= N
            if (g >= lo && g < hi) f(g);
    }
}

__device__ __forceinline__ double cl_d2(const ClusterDev &a, int g, const ClusterLane &l) { return hvn_nbr_d2(a.sx[g], a.sy[g], l.x, l.y); }

// the root of s, s in [0, N): steps only to a strictly smaller slot.  HALVE: inside cl_link, where the trees change -- agent-scope
// loads, path halving; otherwise the trees are final (a later launch) and plain loads do, which the L1 may keep
template <bool HALVE>
__device__ __forceinline__ int cl_find(int *parent, int s)
{
    for (;;) {
        const int p = HALVE ? __hip_atomic_load(parent + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : parent[s];
        if ((unsigned)p >= (unsigned)s) return s;           // s itself, or a value that is no smaller slot: a root
        if (HALVE) {
            const int pp = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)pp < (unsigned)p) __hip_atomic_store(parent + s, pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s = p;
    }
}

// unites the trees of s and t; -> a slot that is from now on an ancestor (or the self) of both: the smaller root
__device__ __forceinline__ int cl_unite(int *parent, int s, int t)
{
    int rs = cl_find<true>(parent, s), rt = cl_find<true>(parent, t);
    while (rs != rt) {
        const int hi = rs > rt ? rs : rt, lo = rs > rt ? rt : rs;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;                           // hooked
        if ((unsigned)old >= (unsigned)hi) return lo;       // not a strictly smaller slot: nothing to follow
        rs = cl_find<true>(parent, old);                    // <= old < hi
        rt = cl_find<true>(parent, lo);                     // <= lo < hi
    }
    return rs;
}

__global__ __launch_bounds__(CL_T) void cl_degree(const ClusterDev a)
{
    const long q = (long)blockIdx.x * CL_T + threadIdx.x;
    ClusterLane l;
    const bool valid = cl_lane(a, q, l);
    const bool sel = valid && cl_selected(a.mask, l.type);
    const double r2 = a.table[3];
    const unsigned mask = a.mask;
    int cnt = sel ? 1 : 0;                                  // the point counts itself
    cl_walk(a, sel, l, a.N, [&](int g) {
        if (g == (int)q || !cl_selected(mask, a.stype[g])) return;
        cnt += cl_d2(a, g, l) <= r2 ? 1 : 0;
    });
    if (!valid) return;
    a.parent[q] = (int)q;
    a.minpos[q] = CL_NONE;
    a.sdeg[q] = cnt;
    if ((unsigned)l.pos < (unsigned)a.N) a.degree[l.pos] = cnt;
}

__global__ __launch_bounds__(CL_T) void cl_link(const ClusterDev a)
{
    const long q = (long)blockIdx.x * CL_T + threadIdx.x;
    ClusterLane l;
    const bool valid = cl_lane(a, q, l);
    const bool core = valid && a.sdeg[q] >= a.min_pts;
    const double r2 = a.table[3];
    int mine = (int)(valid ? q : 0);                        // an ancestor of this slot, or itself: what the last union left
    cl_walk(a, core, l, mine, [&](int g) {                  // candidates t < s: every pair is tested once
        if (a.sdeg[g] < a.min_pts || !(cl_d2(a, g, l) <= r2)) return;
        const int pg = __hip_atomic_load(a.parent + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int up = (unsigned)pg < (unsigned)g ? pg : g; // an ancestor of g, or g itself
        if (up == mine) return;                             // one tree already; the root's own word is not read: in a grown cluster
                                                            // every wave of the chip would read that ONE address once per candidate
        const int rg = cl_find<true>(a.parent, up);         // g is wave-uniform: the lanes that get here walk ONE chain together
        if (rg != mine) mine = cl_unite(a.parent, mine, rg);
    });
}

__global__ __launch_bounds__(CL_T) void cl_roots(const ClusterDev a)
{
    const long q = (long)blockIdx.x * CL_T + threadIdx.x;
    const bool core = q < a.N && a.sdeg[q] >= a.min_pts;
    const int root = core ? cl_find<false>(a.parent, (int)q) : -1;
    int v = core ? a.spos[q] : CL_NONE;
    const unsigned long long cores = __ballot(core);
    if (!cores) return;                                     // wave-uniform
    const int root0 = __shfl(root, __ffsll((long long)cores) - 1, 64);
    if (__ballot(core && root != root0)) {                  // several clusters in this wave: one atomic per core
        if (core) atomicMin(a.minpos + root, v);
        return;
    }
    for (int d = 32; d > 0; d >>= 1) {                      // one cluster: one atomic per wave (a grown cluster has ONE such word)
        const int o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == __ffsll((long long)cores) - 1) atomicMin(a.minpos + root0, v);
}

__global__ __launch_bounds__(CL_T) void cl_assign(const ClusterDev a)
{
    const long q = (long)blockIdx.x * CL_T + threadIdx.x;
    ClusterLane l;
    const bool valid = cl_lane(a, q, l);
    const int deg = valid ? a.sdeg[q] : 0;
    const bool core = deg >= a.min_pts, border = deg > 0 && !core;      // deg > 0 <=> selected
    const double r2 = a.table[3];
    double bd = __builtin_inf();
    int bj = CL_NONE, bt = -1;                              // the (d2, j)-smallest core candidate: its position and its slot
    cl_walk(a, border, l, a.N, [&](int g) {
        if (a.sdeg[g] < a.min_pts) return;
        const double d2 = cl_d2(a, g, l);
        const int j = a.spos[g];
        if (d2 <= r2 && hvn_nbr_less(d2, j, bd, bj)) {
            bd = d2;
            bj = j;
            bt = g;
        }
    });
    if (!valid || (unsigned)l.pos >= (unsigned)a.N) return;
    const int from = core ? (int)q : bt;
    int lab = -1;
    if (from >= 0) {
        lab = a.minpos[cl_find<false>(a.parent, from)];
        lab = lab == CL_NONE ? -1 : lab;
    }
    a.label[l.pos] = lab;
}

int hvn_launch_nbr_cluster(const NbrClusterArgs &a, hipStream_t stream)
{
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    ClusterDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table;
    d.spos = w.spos; d.stype = w.stype; d.cell_start = w.cell_start;
    d.parent = (int *)a.workspace2; d.minpos = d.parent + a.N; d.sdeg = d.minpos + a.N;
    d.label = a.label; d.degree = a.degree;
    d.N = a.N; d.ncy = a.ncy; d.ncx = a.ncx; d.min_pts = a.min_pts; d.mask = a.mask;
    const dim3 grid((unsigned)(((long)a.N + CL_T - 1) / CL_T)), block(CL_T);
    hipLaunchKernelGGL(cl_degree, grid, block, 0, stream, d);
    hipLaunchKernelGGL(cl_link, grid, block, 0, stream, d);
    hipLaunchKernelGGL(cl_roots, grid, block, 0, stream, d);
    hipLaunchKernelGGL(cl_assign, grid, block, 0, stream, d);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

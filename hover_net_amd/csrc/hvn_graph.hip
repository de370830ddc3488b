// hvn_graph.hip -- the cell graph of nucleus centroids: exact Gabriel edges of length <= r over the neighbour grid
// (hover_net_amd/graph.py is the definition).  HVN_OP_NBR_GRAPH runs after HVN_OP_NBR_GRID on the same stream and reads
// its workspace.
//
//   j is a neighbour of i  <=>  j != i and d2(i, j) <= r2                                   (hvn_nbr_d2, as every op of the family)
//   dot(i, j, k) = ((xi - xk) * (xj - xk)) + ((yi - yk) * (yj - yk))
//   k blocks (i, j)        <=>  k != i, k != j, k is a neighbour of i AND of j, and dot(i, j, k) < 0
//   (i, j) is an edge      <=>  j is a neighbour of i and no k blocks (i, j)
// every operation one float64 rounding (the library is built with -ffp-contract=off; the code names the roundings all the same).  The
// kernel does not test k != i and k != j: for k = i or k = j, and for any k that coincides with either, one factor of each product is
// an exact zero and the other is finite (all three are neighbours of i), so dot is +-0 and never < 0.  i is identified by its SLOT in
// the cell order, which names a point as its position does.
//
// Two modes of one kernel (gr_graph<STORE>), the same search in both:
//   count  degree[pos(i)] = the number of edges of i; with a table `first` [N][W] the first W edges a wave finds also go to row pos(i) of
//          it (gr_graph<true>), so that a graph whose largest degree is at most W needs no second search (graph.py)
//   fill   the positions of i's graph neighbours go to indices[indptr[pos(i)] ..), in the order the wave finds them
// The host puts every row into (d2, j) order (graph.py), so no output depends on the order of the points inside a cell or on the order
// in which a wave finds a row's edges.
//
// A WAVE takes one query at a time, GR_QPW consecutive slots per wave, four waves per workgroup, nothing shared between the waves (no
// workgroup barrier anywhere).  Per query:
//   1  its lanes stride the three candidate runs of the 3 x 3 cells ([cell_start[row][cx - 1], cell_start[row][cx + 2)), as nb_query)
//      and compact the true neighbours (x, y, slot) into the wave's own LDS list by ballot / popcount; past GR_CAP entries only the
//      count goes on;
//   2  at most GR_CAP neighbours (the FAST path).  Blockers are neighbours of i, so the list holds them all.  2a: lane l takes
//      j = list[l], list[l + 64], .. and walks k over the list's first GR_PRUNE entries -- every lane reads the same address, an LDS
//      broadcast -- leaving at the first blocker; most pairs end here.  2b: the pairs that survive are taken one at a time by the
//      whole wave, lane l testing k = list[GR_PRUNE + l], list[GR_PRUNE + l + 64], .., and a ballot ends the pair at the first step
//      that holds a blocker.  So a true edge, which has to see every k, costs cnt / 64 steps of the wave and not cnt steps of one lane
//      for which 63 others wait;
//   3  more than GR_CAP neighbours (the SLOW path, exact and unbounded): lane l takes its j from the candidate runs again and walks k
//      over the three runs in global memory (a wave-uniform address), testing "neighbour of i" there too.  Nothing is capped: a degree
//      or a neighbourhood of any size is counted and filled exactly.
// Every loop bound is a cell_start value clamped to [0, N] (or the list length, at most GR_CAP); a query whose position is outside
// [0, N) writes nothing; every store of the fill pass is bounded by its row's own end and by E, every store into the count pass's
// table by its row's W slots.  A workspace or an indptr that does not
// match gives wrong numbers, never an access outside the arrays or a loop without an end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define GR_T 256                      // four waves
#define GR_QPW 4                      // queries per wave
#define GR_CAP HVN_NBR_GRAPH_LIST_CAP // entries of a wave's LDS list: 20 bytes each, 40 KiB per workgroup
#define GR_PRUNE 16                   // blockers tried per pair by the pair's own lane before the wave takes the survivors

struct GraphDev {
    const double *sx, *sy, *table;
    const int *spos, *cell_start;
    int *degree;                // count, else NULL
    const long long *indptr;    // fill, else NULL
    int *indices;               // fill: [E]; count: the table [N][width] or NULL
    long long E;
    int N, ncy, ncx, width;
};

// dot(i, j, k) < 0, the four differences, two products and one sum each rounded once
__device__ __forceinline__ bool gr_obtuse(double xi, double yi, double xj, double yj, double xk, double yk)
{
    const double ax = __dsub_rn(xi, xk), bx = __dsub_rn(xj, xk), ay = __dsub_rn(yi, yk), by = __dsub_rn(yj, yk);
    return __dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)) < 0.0;
}

// the three candidate runs of a slot's 3 x 3 cells, empty ones as (0, 0)
__device__ __forceinline__ void gr_runs(const GraphDev &a, int cx, int cy, int lo[3], int hi[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int yy = cy + r - 1;
        lo[r] = hi[r] = 0;
        if (yy >= 0 && yy < a.ncy) {
            const long row = (long)yy * a.ncx;
            const int ca = cx > 0 ? cx - 1 : 0, cb = cx + 1 < a.ncx ? cx + 1 : a.ncx - 1;
            const int l = hvn_nbr_clamp(a.cell_start[row + ca], a.N), h = hvn_nbr_clamp(a.cell_start[row + cb + 1], a.N);
            if (l < h) {
                lo[r] = l;
                hi[r] = h;
            }
        }
    }
}

// the slow path's blocker walk for one (i, j): k over the three runs in global memory, wave-uniform addresses
__device__ __forceinline__ bool gr_blocked_global(const GraphDev &a, const int lo[3], const int hi[3], int q, double qx, double qy, double jx, double jy,
                                                  double r2)
{
    for (int r = 0; r < 3; ++r) {
        for (int k = lo[r]; k < hi[r]; ++k) {
            const double kx = a.sx[k], ky = a.sy[k];
            if (k == q || !(hvn_nbr_d2(kx, ky, qx, qy) <= r2)) continue;          // not a neighbour of i
            if (hvn_nbr_d2(kx, ky, jx, jy) <= r2 && gr_obtuse(qx, qy, jx, jy, kx, ky)) return true;
        }
    }
    return false;
}

template <bool STORE>
__global__ __launch_bounds__(GR_T) void gr_graph(const GraphDev a)
{
    __shared__ double s_x[GR_T / 64][GR_CAP], s_y[GR_T / 64][GR_CAP];
    __shared__ int s_s[GR_T / 64][GR_CAP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, N = a.N;
    double *lx = s_x[wv], *ly = s_y[wv];
    int *ls = s_s[wv];
    const double x0 = a.table[0], y0 = a.table[1], c = a.table[2], r2 = a.table[3];
    const unsigned long long below = (1ull << lane) - 1ull;
    const long q0 = ((long)blockIdx.x * (GR_T / 64) + wv) * GR_QPW;
    for (int qi = 0; qi < GR_QPW; ++qi) {
        const long ql = q0 + qi;
        if (ql >= N) break;                                                       // wave-uniform
        const int q = (int)ql;
        const double qx = a.sx[q], qy = a.sy[q];
        const int qpos = a.spos[q];
        if ((unsigned)qpos >= (unsigned)N) continue;                              // no row to write: wave-uniform
        int lo[3], hi[3];
        gr_runs(a, hvn_nbr_axis(qx, x0, c, a.ncx), hvn_nbr_axis(qy, y0, c, a.ncy), lo, hi);
        // 1: the neighbours of i, compacted
        int cnt = 0;
        for (int r = 0; r < 3; ++r) {
            for (int base = lo[r]; base < hi[r]; base += 64) {
                const int s = base + lane;
                bool nb = false;
                double x = 0.0, y = 0.0;
                if (s < hi[r]) {
                    x = a.sx[s];
                    y = a.sy[s];
                    nb = s != q && hvn_nbr_d2(x, y, qx, qy) <= r2;
                }
                const unsigned long long m = __ballot(nb);
                const int at = cnt + __popcll(m & below);
                if (nb && at < GR_CAP) {
                    lx[at] = x;
                    ly[at] = y;
                    ls[at] = s;
                }
                cnt += __popcll(m);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                    // the list is read by other lanes than wrote it
        __builtin_amdgcn_wave_barrier();
        long long row = 0, room = 0;                                              // this row's first index and one past the last it may write
        if (STORE) {
            if (a.indptr) {
                const long long b = a.indptr[qpos], e = a.indptr[qpos + 1];
                row = b < 0 ? 0 : b;
                room = e < a.E ? e : a.E;
            } else {
                row = (long long)qpos * a.width;
                room = row + a.width;
            }
        }
        int found = 0;                                                            // edges so far, wave-uniform
        if (cnt <= GR_CAP) {
            // 2: j and k from the list
            const int P = cnt < GR_PRUNE ? cnt : GR_PRUNE;
            for (int jb = 0; jb < cnt; jb += 64) {
                const int jj = jb + lane;
                bool alive = jj < cnt;
                if (alive) {                                                      // 2a: a lane per j, the list's first P as k
                    const double jx = lx[jj], jy = ly[jj];
                    for (int k = 0; k < P; ++k) {
                        const double kx = lx[k], ky = ly[k];
                        if (hvn_nbr_d2(kx, ky, jx, jy) <= r2 && gr_obtuse(qx, qy, jx, jy, kx, ky)) {
                            alive = false;
                            break;
                        }
                    }
                }
                unsigned long long m = __ballot(alive);
                while (m) {                                                       // 2b: the survivors one by one, a lane per k
                    const int sj = jb + __builtin_ctzll(m);                       // wave-uniform, below cnt
                    m &= m - 1ull;
                    const double jx = lx[sj], jy = ly[sj];
                    bool blocked = false;
                    for (int k0 = P; k0 < cnt; k0 += 64) {
                        const int k = k0 + lane;
                        bool hit = false;
                        if (k < cnt) {
                            const double kx = lx[k], ky = ly[k];
                            hit = hvn_nbr_d2(kx, ky, jx, jy) <= r2 && gr_obtuse(qx, qy, jx, jy, kx, ky);
                        }
                        if (__ballot(hit)) {
                            blocked = true;
                            break;
                        }
                    }
                    if (blocked) continue;
                    if (STORE && lane == 0) {
                        const long long w = row + found;
                        if (w < room) a.indices[w] = a.spos[ls[sj]];             // a list entry: a slot in [0, N)
                    }
                    ++found;
                }
            }
        } else {
            // 3: j from the runs, k from the runs
            for (int r = 0; r < 3; ++r) {
                for (int base = lo[r]; base < hi[r]; base += 64) {
                    const int s = base + lane;
                    bool edge = false;
                    if (s < hi[r] && s != q) {
                        const double jx = a.sx[s], jy = a.sy[s];
                        if (hvn_nbr_d2(jx, jy, qx, qy) <= r2) edge = !gr_blocked_global(a, lo, hi, q, qx, qy, jx, jy, r2);
                    }
                    const unsigned long long m = __ballot(edge);
                    if (STORE && edge) {
                        const long long w = row + found + __popcll(m & below);
                        if (w < room) a.indices[w] = a.spos[s];
                    }
                    found += __popcll(m);
                }
            }
        }
        if (a.degree && lane == 0) a.degree[qpos] = found;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                    // the list has been read before the next query overwrites it
        __builtin_amdgcn_wave_barrier();
    }
}

int hvn_launch_nbr_graph(const NbrGraphArgs &a, hipStream_t stream)
{
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    GraphDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table;
    d.spos = w.spos; d.cell_start = w.cell_start;
    d.degree = a.fill ? nullptr : a.degree;
    d.indptr = a.fill ? a.indptr : nullptr;
    d.indices = a.fill ? a.indices : a.first;
    d.E = a.E;
    d.N = a.N; d.ncy = a.ncy; d.ncx = a.ncx; d.width = a.width;
    const long per = (GR_T / 64) * GR_QPW;
    const dim3 grid((unsigned)(((long)a.N + per - 1) / per)), block(GR_T);
    if (d.indices) hipLaunchKernelGGL(gr_graph<true>, grid, block, 0, stream, d);
    else hipLaunchKernelGGL(gr_graph<false>, grid, block, 0, stream, d);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

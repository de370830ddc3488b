// hvn_neighbours.hip -- fixed-radius neighbours of nucleus centroids (hover_net_amd/neighbours.py is the definition).
//
// j is a neighbour of i  <=>  j != i and d2(i, j) <= r2, d2 = (dx * dx) + (dy * dy) with dx = xj - xi, dy = yj - yi, every operation one
// float64 rounding (the library is built with -ffp-contract=off; the code names the roundings all the same).  The device returns
// integers only: counts per type, the k smallest neighbours and the smallest of every type under the total order (d2, j).
//
// Grid (hvn_launch_nbr_grid): the cell of a point is (floor((y - y0) / c), floor((x - x0) / c)).  The quotient is brought into
// [0, 4096] as a double BEFORE the conversion (a NaN compares false and becomes 0) and into [0, n) as an integer after it, so no
// input value indexes outside the workspace.  The host chose c so that two neighbours are at most one cell apart per axis
// (neighbours.py: `grid`), hence the 3 x 3 cells around a point hold all its neighbours.
//   nb_count     one integer atomic per point on its cell's counter
//   nb_bsum / nb_bscan / nb_cscan   exclusive scan of the cell counts in blocks of 4096 cells (at most 1024 blocks): block sums,
//                their scan by one workgroup, then every block scans its cells (a thread owns 16 consecutive ones) -> cell_start
//                [cells + 1]; the counters are left holding cell_start as the scatter's cursors
//   nb_scatter   slot = atomic increment of the cell's cursor; x, y, type and position are written there (cell-ordered copies).  A
//                slot outside [0, N) is not written (it cannot arise unless xy changes between the two passes).
// The order of the points INSIDE a cell depends on atomic arrival.  No output of the query does: counts are integer sums, both
// selections are minima under (d2, j), and j is unique.
//
// Query (nb_query): cells of one grid row are adjacent in the cell-ordered arrays, so the 3 x 3 cells of a point are three contiguous
// runs [cell_start[row][cx - 1], cell_start[row][cx + 2)).  A workgroup owns NB_T consecutive cell-ordered points -- a run of cells --
// one per lane.  Per grid row offset it forms the union of its lanes' runs, stages that union through LDS in tiles of NB_TILE
// candidates (x, y, position, type: 24 KiB), and every wave walks the part of the tile that its own lanes' runs cover (wave-uniform
// bounds: every lane reads the same LDS address, a broadcast); a lane tests a candidate only inside its own run.  The k best (d2, j)
// live in registers as a sorted list (a carried compare-and-swap pass per insertion), the T counts and per-type bests too (the
// update is unrolled over the types: registers take no dynamic index).  Every loop bound is a cell_start value clamped to [0, N]:
// a workspace that the grid op did not fill gives wrong numbers, never an access outside the arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define NB_T 256
#define NB_TILE 1024
#define NB_BLOCK 4096         // cells per scan block
#define NB_NONE 0x7FFFFFFF

// hvn_nbr_axis, hvn_nbr_clamp, hvn_nbr_less, hvn_nbr_d2 and the workspace carve-up live in hvn_kernels.h: hvn_clusters.hip and
// hvn_density.hip read the same grid

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NB_T) void nb_count(const double *__restrict__ xy, const double *__restrict__ table, int *__restrict__ cursor, int N, int ncy,
                                                 int ncx)
{
    const double x0 = table[0], y0 = table[1], c = table[2];
    for (long i = (long)blockIdx.x * NB_T + threadIdx.x; i < N; i += (long)gridDim.x * NB_T) {
        const int cx = hvn_nbr_axis(xy[2 * i], x0, c, ncx), cy = hvn_nbr_axis(xy[2 * i + 1], y0, c, ncy);
        atomicAdd(cursor + (long)cy * ncx + cx, 1);
    }
}

// exclusive prefix of v over the workgroup's 256 threads in thread order
__device__ __forceinline__ int nb_block_scan(int v, int *wave_sums)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[wv] = inc;
    __syncthreads();
    int before = 0;
    for (int i = 0; i < NB_T / 64; ++i)
        if (i < wv) before += wave_sums[i];
    __syncthreads();
    return before + inc - v;
}

__global__ __launch_bounds__(NB_T) void nb_bsum(const int *__restrict__ cursor, int *__restrict__ bsum, int cells)
{
    __shared__ int s[NB_T / 64];
    const int c0 = blockIdx.x * NB_BLOCK;
    int v = 0;
    for (int i = threadIdx.x; i < NB_BLOCK; i += NB_T)
        if (c0 + i < cells) v += cursor[c0 + i];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ __launch_bounds__(NB_T) void nb_bscan(int *__restrict__ bsum, int nblocks)
{
    __shared__ int wave_sums[NB_T / 64];
    int v[4], mine = 0;
    for (int i = 0; i < 4; ++i) {
        const int b = threadIdx.x * 4 + i;
        v[i] = b < nblocks ? bsum[b] : 0;
        mine += v[i];
    }
    int off = nb_block_scan(mine, wave_sums);
    for (int i = 0; i < 4; ++i) {
        const int b = threadIdx.x * 4 + i;
        if (b < nblocks) bsum[b] = off;
        off += v[i];
    }
}

__global__ __launch_bounds__(NB_T) void nb_cscan(int *__restrict__ cursor, const int *__restrict__ bsum, int *__restrict__ cell_start, int cells, int N)
{
    __shared__ int wave_sums[NB_T / 64];
    const int c0 = blockIdx.x * NB_BLOCK + threadIdx.x * 16;      // this thread's 16 consecutive cells
    int v[16], mine = 0;
    for (int i = 0; i < 16; ++i) {
        v[i] = c0 + i < cells ? cursor[c0 + i] : 0;
        mine += v[i];
    }
    int at = bsum[blockIdx.x] + nb_block_scan(mine, wave_sums);
    for (int i = 0; i < 16; ++i) {
        if (c0 + i < cells) {
            cell_start[c0 + i] = at;
            cursor[c0 + i] = at;
        }
        at += v[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cell_start[cells] = N;
}

__global__ __launch_bounds__(NB_T) void nb_scatter(const double *__restrict__ xy, const int *__restrict__ types, const double *__restrict__ table,
                                                   int *__restrict__ cursor, double *__restrict__ sx, double *__restrict__ sy, int *__restrict__ spos,
                                                   int *__restrict__ stype, int N, int ncy, int ncx)
{
    const double x0 = table[0], y0 = table[1], c = table[2];
    for (long i = (long)blockIdx.x * NB_T + threadIdx.x; i < N; i += (long)gridDim.x * NB_T) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        const int cx = hvn_nbr_axis(x, x0, c, ncx), cy = hvn_nbr_axis(y, y0, c, ncy);
        const int slot = atomicAdd(cursor + (long)cy * ncx + cx, 1);
        if ((unsigned)slot < (unsigned)N) {
            sx[slot] = x;
            sy[slot] = y;
            spos[slot] = (int)i;
            stype[slot] = types ? types[i] : 0;
        }
    }
}

int hvn_launch_nbr_grid(const NbrGridArgs &a, hipStream_t stream)
{
    const long cells = (long)a.ncy * a.ncx;
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, cells);
    const int nblocks = (int)((cells + NB_BLOCK - 1) / NB_BLOCK);
    const long pb = ((long)a.N + NB_T - 1) / NB_T;
    const dim3 pgrid((unsigned)(pb < 2048 ? pb : 2048));
    if (hipMemsetAsync(w.cursor, 0, sizeof(int) * cells, stream) != hipSuccess) return HVN_E_LAUNCH;
    hipLaunchKernelGGL(nb_count, pgrid, dim3(NB_T), 0, stream, a.xy, a.table, w.cursor, a.N, a.ncy, a.ncx);
    hipLaunchKernelGGL(nb_bsum, dim3(nblocks), dim3(NB_T), 0, stream, w.cursor, w.bsum, (int)cells);
    hipLaunchKernelGGL(nb_bscan, dim3(1), dim3(NB_T), 0, stream, w.bsum, nblocks);
    hipLaunchKernelGGL(nb_cscan, dim3(nblocks), dim3(NB_T), 0, stream, w.cursor, w.bsum, w.cell_start, (int)cells, a.N);
    hipLaunchKernelGGL(nb_scatter, pgrid, dim3(NB_T), 0, stream, a.xy, a.types, a.table, w.cursor, w.sx, w.sy, w.spos, w.stype, a.N, a.ncy, a.ncx);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

// ---------------------------------------------------------------------------------------------
struct NbrQueryDev {
    const double *sx, *sy, *table;
    const int *spos, *stype, *cell_start;
    int *count, *knn, *nearest;
    int N, ncy, ncx, T, k;
};

template <int KM, int TM>
__global__ __launch_bounds__(NB_T) void nb_query(const NbrQueryDev a)
{
    __shared__ double tx[NB_TILE], ty[NB_TILE];
    __shared__ int tj[NB_TILE], tt[NB_TILE];
    __shared__ int s_lo[3], s_hi[3];
    const int N = a.N, tid = threadIdx.x;
    if (tid < 3) {
        s_lo[tid] = NB_NONE;
        s_hi[tid] = 0;
    }
    const double x0 = a.table[0], y0 = a.table[1], c = a.table[2], r2 = a.table[3];
    const long q = (long)blockIdx.x * NB_T + tid;
    const bool valid = q < N;
    double qx = 0.0, qy = 0.0;
    int qpos = -1, cx = 0, cy = 0;
    if (valid) {
        qx = a.sx[q];
        qy = a.sy[q];
        qpos = a.spos[q];
        cx = hvn_nbr_axis(qx, x0, c, a.ncx);
        cy = hvn_nbr_axis(qy, y0, c, a.ncy);
    }
    double bd[KM], td[TM];
    int bj[KM], tb[TM], cnt[TM];
#pragma unroll
    for (int s = 0; s < KM; ++s) {
        bd[s] = __builtin_inf();
        bj[s] = NB_NONE;
    }
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        td[t] = __builtin_inf();
        tb[t] = NB_NONE;
        cnt[t] = 0;
    }
    __syncthreads();
    for (int r = 0; r < 3; ++r) {
        const int yy = cy + r - 1;
        int lo = NB_NONE, hi = 0;           // this lane's run of candidates in grid row yy; empty: (NB_NONE, 0)
        if (valid && yy >= 0 && yy < a.ncy) {
            const long row = (long)yy * a.ncx;
            const int ca = cx > 0 ? cx - 1 : 0, cb = cx + 1 < a.ncx ? cx + 1 : a.ncx - 1;
            lo = hvn_nbr_clamp(a.cell_start[row + ca], N);
            hi = hvn_nbr_clamp(a.cell_start[row + cb + 1], N);
            if (hi <= lo) {
                lo = NB_NONE;
                hi = 0;
            }
        }
        int wlo = lo, whi = hi;             // the wave's union, then the workgroup's
        for (int d = 32; d > 0; d >>= 1) {
            const int ol = __shfl_xor(wlo, d, 64), oh = __shfl_xor(whi, d, 64);
            wlo = ol < wlo ? ol : wlo;
            whi = oh > whi ? oh : whi;
        }
        wlo = __builtin_amdgcn_readfirstlane(wlo);
        whi = __builtin_amdgcn_readfirstlane(whi);
        if ((tid & 63) == 0 && wlo < whi) {
            atomicMin(&s_lo[r], wlo);
            atomicMax(&s_hi[r], whi);
        }
        __syncthreads();
        const int LO = s_lo[r], HI = s_hi[r];
        for (int base = LO; base < HI; base += NB_TILE) {
            const int n = HI - base < NB_TILE ? HI - base : NB_TILE;
            __syncthreads();                // the previous tile has been read
            for (int i = tid; i < n; i += NB_T) {
                tx[i] = a.sx[base + i];
                ty[i] = a.sy[base + i];
                tj[i] = a.spos[base + i];
                tt[i] = a.stype[base + i];
            }
            __syncthreads();
            const int c0 = (wlo > base ? wlo : base) - base;
            const int c1 = (whi < base + n ? whi : base + n) - base;
            for (int i = c0; i < c1; ++i) {
                const int g = base + i;
                if (g < lo || g >= hi) continue;
                const double d2 = hvn_nbr_d2(tx[i], ty[i], qx, qy);
                const int j = tj[i];
                if (!(d2 <= r2) || j == qpos) continue;
                if (hvn_nbr_less(d2, j, bd[KM - 1], bj[KM - 1])) {
                    double cd = d2;
                    int cj = j;
#pragma unroll
                    for (int s = 0; s < KM; ++s) {
                        const bool sw = hvn_nbr_less(cd, cj, bd[s], bj[s]);
                        const double od = bd[s];
                        const int oj = bj[s];
                        bd[s] = sw ? cd : od;
                        bj[s] = sw ? cj : oj;
                        cd = sw ? od : cd;
                        cj = sw ? oj : cj;
                    }
                }
                const int ty_ = tt[i];      // a type outside [0, T) matches no column
#pragma unroll
                for (int t = 0; t < TM; ++t) {
                    const bool m = ty_ == t;
                    cnt[t] += m ? 1 : 0;
                    const bool b = m && hvn_nbr_less(d2, j, td[t], tb[t]);
                    td[t] = b ? d2 : td[t];
                    tb[t] = b ? j : tb[t];
                }
            }
        }
    }
    if (!valid || (unsigned)qpos >= (unsigned)N) return;
    int *count = a.count + (long)qpos * a.T, *nearest = a.nearest + (long)qpos * a.T, *knn = a.knn + (long)qpos * a.k;
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        if (t < a.T) {
            count[t] = cnt[t];
            nearest[t] = tb[t] == NB_NONE ? -1 : tb[t];
        }
    }
#pragma unroll
    for (int s = 0; s < KM; ++s)
        if (s < a.k) knn[s] = bj[s] == NB_NONE ? -1 : bj[s];
}

int hvn_launch_nbr_query(const NbrQueryArgs &a, hipStream_t stream)
{
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    NbrQueryDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table;
    d.spos = w.spos; d.stype = w.stype; d.cell_start = w.cell_start;
    d.count = a.count; d.knn = a.knn; d.nearest = a.nearest;
    d.N = a.N; d.ncy = a.ncy; d.ncx = a.ncx; d.T = a.T; d.k = a.k;
    const dim3 grid((unsigned)(((long)a.N + NB_T - 1) / NB_T)), block(NB_T);
    const int tm = a.T == 1 ? 1 : (a.T <= 8 ? 8 : 16);
    if (a.k <= 8) {
        if (tm == 1) hipLaunchKernelGGL((nb_query<8, 1>), grid, block, 0, stream, d);
        else if (tm == 8) hipLaunchKernelGGL((nb_query<8, 8>), grid, block, 0, stream, d);
        else hipLaunchKernelGGL((nb_query<8, 16>), grid, block, 0, stream, d);
    } else {
        if (tm == 1) hipLaunchKernelGGL((nb_query<16, 1>), grid, block, 0, stream, d);
        else if (tm == 8) hipLaunchKernelGGL((nb_query<16, 8>), grid, block, 0, stream, d);
        else hipLaunchKernelGGL((nb_query<16, 16>), grid, block, 0, stream, d);
    }
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

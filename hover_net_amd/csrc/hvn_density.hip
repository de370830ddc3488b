// hvn_density.hip -- typed counts of nucleus centroids within a radius of every node of a regular raster (hover_net_amd/density.py is
// the definition).  HVN_OP_NBR_DENSITY runs after HVN_OP_NBR_GRID on the same stream and reads its workspace as that
// op left it.
//
// Node (u, v) lies at px = ox + (u * s), py = oy + (v * s); with dx = xj - px, dy = yj - py, d2 = (dx * dx) + (dy * dy), every operation
// one float64 rounding (the library is built with -ffp-contract=off; the code names the roundings all the same),
//     count[t][v][u] = #{ j : type[j] == t and d2 <= r2 }.
// A point exactly on a node counts: nodes are not points, nothing is excluded.  Node positions are computed here, never stored.
//
// A node's cell is hvn_nbr_axis of its position: the formula and the clamp of the points' cells.  Clamping moves a node's cell towards
// the points' cells, the per-axis argument of neighbours.py holds for any node that has a point within the radius at all, and a
// node without one only meets candidates that fail the test (density.py): the 3 x 3 cells around the clamped cell hold every point
// with d2 <= r2.
//
// dn_density: a workgroup of 256 lanes owns an 8 x 8 block of nodes; each of its four waves holds the whole block, one node per lane,
// and walks every fourth candidate; the waves' counts are added through LDS at the end (integer sums: the order does not matter).
// A slide-sized raster has few nodes (a 20000 x 20000 px slide at step 64: 10^5, one wave per SIMD and a half as one node per lane of
// a 16 x 16 block, which measured latency-bound: 99 x 99 nodes took as long as 313 x 313); four waves per 64 nodes give four times
// the waves and a quarter of the chain per wave.
// px is monotone in u and hvn_nbr_axis in its argument (every step is a monotone rounding, c > 0), so the block's cells span
// [cell(first node), cell(last node)] per axis: four uniform evaluations give the block's grid rows Y0 - 1 .. Y1 + 1 and cell columns
// CA .. CB.
// nb_query's union in slot space would not do here: a block of nodes spans several grid rows, and the union of its lanes' runs over
// ALL rows would stage whole grid rows in between.  Instead the grid rows are walked one by one; a row that no lane of the workgroup
// needs (|row - cy| > 1 for all of them: coarse rasters) is skipped; of the others the run [cell_start[row][CA], cell_start[row][CB + 1])
// is staged through LDS in tiles of NB_TILE candidates (x, y, type: 20 KiB), and every wave walks its quarter of the part of the tile
// that the block's runs cover (wave-uniform bounds: every lane reads the same LDS address, a broadcast).  A lane tests a candidate only when
// |row - cy| <= 1 and the slot lies in its own run [cell_start[row][cx - 1], cell_start[row][cx + 2)).  The T counts live in registers,
// the update unrolled over the types (registers take no dynamic index); a type outside [0, T) matches no column.  Wave 0 stores,
// rows of 8 nodes along u, one plane per type, and EVERY element of count is stored: no atomics, nothing to clear.
//
// Every bound is a cell_start value clamped to [0, N] and the row loop runs over at most ncy rows: a workspace that the grid op did
// not fill (or a table that breaks the monotonicity above) gives wrong numbers, never an access outside the arrays and never a loop
// without an end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define DN_B 8                // nodes per block side: one block per wave
#define DN_W 4                // waves per workgroup, each walking every DN_W-th candidate of the same block
#define DN_T (DN_B * DN_B * DN_W)
#define DN_TILE 1024          // candidates per staging tile, as nb_query's NB_TILE
#define DN_NONE (1 << 30)     // an empty run's lower end: above every slot (N <= 2^26), and DN_NONE + DN_W does not overflow

struct DensityDev {
    const double *sx, *sy, *table, *raster;
    const int *stype, *cell_start;
    int *count;
    int N, ncy, ncx, T, H, W;
};

__device__ __forceinline__ double dn_node(double o, int i, double s) { return __dadd_rn(o, __dmul_rn((double)i, s)); }

template <int TM>
__global__ __launch_bounds__(DN_T) void dn_density(const DensityDev a)
{
    __shared__ double tx[DN_TILE], ty[DN_TILE];
    __shared__ int tt[DN_TILE];
    __shared__ int red[DN_W - 1][TM][64];
    const int N = a.N, tid = threadIdx.x;
    const double x0 = a.table[0], y0 = a.table[1], c = a.table[2], r2 = a.table[3];
    const double ox = a.raster[0], oy = a.raster[1], s = a.raster[2];
    const int u0 = blockIdx.x * DN_B, v0 = blockIdx.y * DN_B;
    const int lane = tid & 63, wave = tid >> 6;
    const int u = u0 + (lane & (DN_B - 1)), v = v0 + (lane >> 3);
    const bool valid = u < a.W && v < a.H;
    const double px = dn_node(ox, u, s), py = dn_node(oy, v, s);
    const int cx = hvn_nbr_axis(px, x0, c, a.ncx), cy = hvn_nbr_axis(py, y0, c, a.ncy);
    const int ca = cx > 0 ? cx - 1 : 0, cb = cx + 1 < a.ncx ? cx + 1 : a.ncx - 1;
    // the block's span of cells, from its first and its last node (uniform over the workgroup)
    const int u1 = u0 + DN_B - 1 < a.W ? u0 + DN_B - 1 : a.W - 1, v1 = v0 + DN_B - 1 < a.H ? v0 + DN_B - 1 : a.H - 1;
    const int X0 = hvn_nbr_axis(dn_node(ox, u0, s), x0, c, a.ncx), X1 = hvn_nbr_axis(dn_node(ox, u1, s), x0, c, a.ncx);
    const int Y0 = hvn_nbr_axis(dn_node(oy, v0, s), y0, c, a.ncy), Y1 = hvn_nbr_axis(dn_node(oy, v1, s), y0, c, a.ncy);
    const int CA = X0 > 0 ? X0 - 1 : 0, CB = X1 + 1 < a.ncx ? X1 + 1 : a.ncx - 1;
    const int RA = Y0 > 0 ? Y0 - 1 : 0, RB = Y1 + 1 < a.ncy ? Y1 + 1 : a.ncy - 1;
    int cnt[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) cnt[t] = 0;
    for (int yy = RA; yy <= RB; ++yy) {     // at most ncy rows
        const bool mine = valid && yy >= cy - 1 && yy <= cy + 1;
        if (!__syncthreads_or(mine ? 1 : 0)) continue;      // uniform; also the barrier that ends the reading of the previous tile
        const long row = (long)yy * a.ncx;
        int lo = DN_NONE, hi = 0;           // this lane's run of candidates in grid row yy; empty: (DN_NONE, 0)
        if (mine) {
            lo = hvn_nbr_clamp(a.cell_start[row + ca], N);
            hi = hvn_nbr_clamp(a.cell_start[row + cb + 1], N);
            if (hi <= lo) {
                lo = DN_NONE;
                hi = 0;
            }
        }
        int wlo = lo, whi = hi;             // the block's union (the same in all four waves)
        for (int d = 32; d > 0; d >>= 1) {
            const int ol = __shfl_xor(wlo, d, 64), oh = __shfl_xor(whi, d, 64);
            wlo = ol < wlo ? ol : wlo;
            whi = oh > whi ? oh : whi;
        }
        wlo = __builtin_amdgcn_readfirstlane(wlo);
        whi = __builtin_amdgcn_readfirstlane(whi);
        const int LO = CA <= CB ? hvn_nbr_clamp(a.cell_start[row + CA], N) : 0;      // the workgroup's run: uniform
        const int HI = CA <= CB ? hvn_nbr_clamp(a.cell_start[row + CB + 1], N) : 0;
        for (int base = LO; base < HI; base += DN_TILE) {
            const int n = HI - base < DN_TILE ? HI - base : DN_TILE;
            if (base != LO) __syncthreads();        // the previous tile has been read
            for (int i = tid; i < n; i += DN_T) {
                tx[i] = a.sx[base + i];
                ty[i] = a.sy[base + i];
                tt[i] = a.stype[base + i];
            }
            __syncthreads();
            const int c0 = (wlo > base ? wlo : base) - base;
            const int c1 = (whi < base + n ? whi : base + n) - base;
            // no branch in the body: the bounds are the wave's, so every lane walks every candidate anyway, and a straight body lets the
            // compiler keep the LDS reads of several candidates in flight (few waves per SIMD on a slide-sized raster: latency-bound)
#pragma unroll 4
            for (int i = c0 + wave; i < c1; i += DN_W) {
                const int g = base + i;
                const double d2 = hvn_nbr_d2(tx[i], ty[i], px, py);
                const int hit = (g >= lo && g < hi && d2 <= r2) ? tt[i] : -1;      // a type outside [0, T) matches no column
#pragma unroll
                for (int t = 0; t < TM; ++t) cnt[t] += hit == t ? 1 : 0;
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < TM; ++t) red[wave - 1][t][lane] = cnt[t];
    }
    __syncthreads();
    if (wave > 0 || !valid) return;
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int w = 0; w < DN_W - 1; ++w) cnt[t] += red[w][t][lane];
    int *out = a.count + (long)v * a.W + u;
    const long plane = (long)a.H * a.W;
#pragma unroll
    for (int t = 0; t < TM; ++t)
        if (t < a.T) out[t * plane] = cnt[t];
}

int hvn_launch_nbr_density(const NbrDensityArgs &a, hipStream_t stream)
{
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    DensityDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table; d.raster = a.raster;
    d.stype = w.stype; d.cell_start = w.cell_start;
    d.count = a.count;
    d.N = a.N; d.ncy = a.ncy; d.ncx = a.ncx; d.T = a.T; d.H = a.H; d.W = a.W;
    const dim3 grid((unsigned)((a.W + DN_B - 1) / DN_B), (unsigned)((a.H + DN_B - 1) / DN_B)), block(DN_T);
    if (a.T == 1) hipLaunchKernelGGL((dn_density<1>), grid, block, 0, stream, d);
    else if (a.T <= 8) hipLaunchKernelGGL((dn_density<8>), grid, block, 0, stream, d);
    else hipLaunchKernelGGL((dn_density<16>), grid, block, 0, stream, d);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

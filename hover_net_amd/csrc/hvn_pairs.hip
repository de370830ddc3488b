// hvn_pairs.hip -- typed pair counts of nucleus centroids by distance bin, the integers under Ripley's cross-type K function
// (hover_net_amd/ripley.py is the definition).  HVN_OP_NBR_PAIRS runs after HVN_OP_NBR_GRID on the same stream and
// reads its workspace as that op left it.
//
// With d2 = (dx * dx) + (dy * dy), dx = xj - xi, dy = yj - yi, every operation one float64 rounding (the library is built with
// -ffp-contract=off; the code names the roundings all the same), radii r_0 < .. < r_{R-1}, r2_k = r_k * r_k (formed on the host) and the
// window (wx0, wy0, wx1, wy1):
//     kmin(i, j) = the smallest k with d2 <= r2_k                         (none where d2 > r2_{R-1}: the pair is not counted)
//     b_i = min(x_i - wx0, wx1 - x_i, y_i - wy0, wy1 - y_i);   m_i = #{ k : r_k <= b_i }
// and per ordered pair (i, j), j != i, both types in [0, T):
//     acc[0][ti][tj][kmin] += 1
//     acc[1][ti][tj][kmin] += 1 and, where m_i < R, acc[1][ti][tj][m_i] -= 1          only if kmin < m_i
// Plane 1 is a difference array: its running sum at k counts the pairs with kmin <= k < m_i, that is d2 <= r2_k and b_i >= r_k.
//
// rp_pairs: a workgroup of 256 lanes owns 256 consecutive slots of the cell order, one query per lane, and stages the union of its
// lanes' candidate runs through LDS in tiles of RP_TILE candidates, per grid row offset, as nb_query does; every wave walks the part
// of the tile that its own lanes' runs cover, so the candidate -- and with it tj -- is the same in all 64 lanes.  j != i is a
// comparison of SLOTS (a slot is a point).  kmin is a bisection over the r2 table in LDS, padded with +inf to 32 entries: five
// steps, no bound to test.  m_i and ti are per-lane constants.
//
// The histogram lives in LDS as two planes of T T R 32-bit words.  Plane h0 is acc[0]'s.  Plane hx is NOT acc[1]'s: a lane with
// m_i < R adds 1 at hx[ti][tj][max(kmin, m_i)], a lane with m_i == R (at least r_{R-1} inside the window: nearly every nucleus of a
// slide) adds nothing, and the flush forms acc[1] += h0 - hx.  Case by case: kmin >= m_i gives h0 and hx the same bin, net 0; kmin <
// m_i < R gives +1 at kmin and -1 at m_i; m_i == R gives +1 at kmin.  One LDS add per counted pair of an interior point, two otherwise.
//
// Lanes collide in LDS only where they share (ti, kmin), and every counting lane simply adds 1.  Two forms that cut same-address adds
// with wave ballots were measured against this one and lost on slide-like points (DESIGN.md 4.21 has the numbers): grouping the
// wave's counting lanes by bin costs more than the collisions it saves.
//
// Overflow.  A lane tests a candidate at most once and adds at most 1 to one word of each plane for it, so between two flushes no
// word grows by more than the tests of the workgroup in between.  A tile is at most RP_TILE candidates for 256 lanes: 2^18 tests.
// The histogram is flushed after every RP_FLUSH = 32 tiles, so a word stays below 2^23 + 1 and h0 - hx is formed in 64 bits.  Without
// that flush a workgroup could reach 256 N = 2^34 tests on one bin (N <= 2^26 coincident points of one type).  The flush adds the
// non-zero words into acc with 64-bit global integer atomics (a negative difference as its two's complement: sums are modulo 2^64
// and the final values lie in [-2^52, 2^52]) and clears the planes.  acc itself is cleared in stream order before the launch, so
// every element is written whatever it held; integer sums make it a function of the inputs alone.
//
// Every loop bound is a cell_start value clamped to [0, N]; a bin index is built from ti, tj in [0, T) and k <= R - 1: a workspace
// that the grid op did not fill, or tables that do not ascend, give wrong numbers, never an access outside the arrays and never a
// loop without an end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

struct PairsDev {
    const double *sx, *sy, *table, *rt;
    const int *stype, *cell_start;
    unsigned long long *acc;
    int N, ncy, ncx, T, R;
};

// h0 and hx into acc, non-zero words only, and both planes cleared; the caller puts a barrier before and after
__device__ __forceinline__ void rp_flush(unsigned *hist, unsigned long long *acc, int bins, int tid)
{
    for (int b = tid; b < bins; b += RP_T) {
        const unsigned v0 = hist[b], vx = hist[bins + b];
        const long long v1 = (long long)v0 - (long long)vx;
        if (v0) atomicAdd(acc + b, (unsigned long long)v0);
        if (v1) atomicAdd(acc + bins + b, (unsigned long long)v1);
        hist[b] = 0u;
        hist[bins + b] = 0u;
    }
}

__global__ __launch_bounds__(RP_T) void rp_pairs(const PairsDev a)
{
    extern __shared__ unsigned hist[];              // [2][T][T][R]: h0, hx
    __shared__ double tx[RP_TILE], ty[RP_TILE], s_r2[32];
    __shared__ int tt[RP_TILE];
    __shared__ int s_lo[3], s_hi[3];
    const int N = a.N, T = a.T, R = a.R, tid = threadIdx.x, lane = tid & 63;
    const int bins = T * T * R;
    for (int b = tid; b < 2 * bins; b += RP_T) hist[b] = 0u;
    if (tid < 32) s_r2[tid] = tid < R ? a.rt[4 + R + tid] : __builtin_inf();
    if (tid < 3) {
        s_lo[tid] = RP_NONE;
        s_hi[tid] = 0;
    }
    const double x0 = a.table[0], y0 = a.table[1], c = a.table[2], r2max = a.table[3];
    const long q = (long)blockIdx.x * RP_T + tid;
    bool valid = q < N;
    double qx = 0.0, qy = 0.0;
    int cx = 0, cy = 0, ti = 0, mi = 0;
    if (valid) {
        qx = a.sx[q];
        qy = a.sy[q];
        ti = a.stype[q];
        cx = hvn_nbr_axis(qx, x0, c, a.ncx);
        cy = hvn_nbr_axis(qy, y0, c, a.ncy);
        double b = __dsub_rn(qx, a.rt[0]);
        const double b1 = __dsub_rn(a.rt[2], qx), b2 = __dsub_rn(qy, a.rt[1]), b3 = __dsub_rn(a.rt[3], qy);
        b = b1 < b ? b1 : b;
        b = b2 < b ? b2 : b;
        b = b3 < b ? b3 : b;
        for (int k = 0; k < R; ++k) mi += a.rt[4 + k] <= b ? 1 : 0;         // a prefix of the radii: they ascend
    }
    const bool typed = valid && ti >= 0 && ti < T;      // a type outside [0, T) lands in no bin, as i ..
    const int row_i = typed ? ti * T : 0;
    unsigned *const h0 = hist, *const hx = hist + bins;
    int tiles = 0;
    __syncthreads();
    for (int r = 0; r < 3; ++r) {
        const int yy = cy + r - 1;
        int lo = RP_NONE, hi = 0;           // this lane's run of candidates in grid row yy; empty: (RP_NONE, 0)
        if (valid && yy >= 0 && yy < a.ncy) {
            const long row = (long)yy * a.ncx;
            const int ca = cx > 0 ? cx - 1 : 0, cb = cx + 1 < a.ncx ? cx + 1 : a.ncx - 1;
            lo = hvn_nbr_clamp(a.cell_start[row + ca], N);
            hi = hvn_nbr_clamp(a.cell_start[row + cb + 1], N);
            if (hi <= lo) {
                lo = RP_NONE;
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
        if (lane == 0 && wlo < whi) {
            atomicMin(&s_lo[r], wlo);
            atomicMax(&s_hi[r], whi);
        }
        __syncthreads();
        const int LO = s_lo[r], HI = s_hi[r];
        for (int base = LO; base < HI; base += RP_TILE) {
            const int n = HI - base < RP_TILE ? HI - base : RP_TILE;
            rp_adds_done();
            __syncthreads();                // the previous tile has been read and every wave's adds for it are in the histogram
            if (tiles == RP_FLUSH) {        // uniform: LO, HI and the count are the workgroup's
                rp_flush(hist, a.acc, bins, tid);
                tiles = 0;
            }
            ++tiles;
            for (int i = tid; i < n; i += RP_T) {
                tx[i] = a.sx[base + i];
                ty[i] = a.sy[base + i];
                tt[i] = a.stype[base + i];
            }
            __syncthreads();                // also: the flush's clearing is done before any add
            const int c0 = (wlo > base ? wlo : base) - base;
            const int c1 = (whi < base + n ? whi : base + n) - base;
            for (int i = c0; i < c1; ++i) {
                const int g = base + i;
                const int tj = tt[i];               // .. and as j
                const double d2 = hvn_nbr_d2(tx[i], ty[i], qx, qy);
                const bool hit = typed && tj >= 0 && tj < T && g >= lo && g < hi && g != (int)q && d2 <= r2max;
                int k = 0;                          // #{ k : r2_k < d2 } = kmin; the padding is +inf
#pragma unroll
                for (int s = 16; s > 0; s >>= 1) k += s_r2[k + s - 1] < d2 ? s : 0;
                k = k < R ? k : R - 1;              // only for tables that break table[3] == r2_{R-1}
                if (hit) {
                    atomicAdd(h0 + (row_i + tj) * R + k, 1u);
                    if (mi < R) atomicAdd(hx + (row_i + tj) * R + (k > mi ? k : mi), 1u);
                }
            }
        }
    }
    rp_adds_done();
    __syncthreads();
    rp_flush(hist, a.acc, bins, tid);
}

int hvn_launch_nbr_pairs(const NbrPairsArgs &a, hipStream_t stream)
{
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    PairsDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table; d.rt = a.rt;
    d.stype = w.stype; d.cell_start = w.cell_start;
    d.acc = (unsigned long long *)a.acc;
    d.N = a.N; d.ncy = a.ncy; d.ncx = a.ncx; d.T = a.T; d.R = a.R;
    const size_t words = 2 * (size_t)a.T * a.T * a.R;
    if (hipMemsetAsync(a.acc, 0, sizeof(long long) * words, stream) != hipSuccess) return HVN_E_LAUNCH;
    const dim3 grid((unsigned)(((long)a.N + RP_T - 1) / RP_T)), block(RP_T);
    hipLaunchKernelGGL(rp_pairs, grid, block, sizeof(unsigned) * words, stream, d);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

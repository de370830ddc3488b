// hvn_margins.hip -- nuclei by distance to an annotation's boundary: for N points and the boundary segments of G regions, the nearest
// region within the largest of B widths, the squared distance to it, the side, and per (region, side, band, type) the ring counts
// (hover_net_amd/margins.py is the definition).  HVN_OP_NBR_MARGINS runs after HVN_OP_NBR_GRID on the same stream and
// reads its workspace as that op left it.
//
// A segment is (ax, ay, bx, by) with (ay, ax) <= (by, bx), followed by its box (x0, y0, x1, y1), both made on the host: eight doubles.
// Point (px, py) CROSSES it by the rule of hvn_regions.hip (a horizontal segment, ay == by, is never crossed).  The point is IN THE BOX
// iff x0 <= px <= x1 and y0 <= py <= y1, comparisons only, and then
//     ux = bx - ax   uy = by - ay   vx = px - ax   vy = py - ay
//     dot = ux*vx + uy*vy           len2 = ux*ux + uy*uy
//     dot <= 0    : d2 = vx*vx + vy*vy
//     dot >= len2 : d2 = (px-bx)*(px-bx) + (py-by)*(py-by)
//     otherwise   : c = ux*vy - uy*vx ;  d2 = (c*c) / len2                   every operation one float64 rounding, each named; the
//                                                                            library is built with -ffp-contract=off as well
// and the segment is NEAR the point iff d2 <= w2_{B-1}.  Per (point, region): inside = the parity of the crossings, dmin2 = the
// minimum of d2 over the near segments.  Per point: near = the region with the smallest dmin2 (ties: the smallest region), near_d2,
// near_inside.  Per region: hist[g][side][kmin][t] = the points of type t whose first band is kmin, the smallest k with dmin2 <= w2_k;
// margins.py forms the cumulative counts with an integer running sum.
//
// mg_margins has the shape of rg_regions: a workgroup of 256 lanes owns 256 consecutive slots of the cell order, one point per lane,
// serves the grid rows its lanes occupy smallest first, and stages that row's list -- the segments whose box touches the row, in region
// order -- through LDS in tiles of MG_TILE segments.  Every lane reads the same staged segment (an LDS broadcast), so a region boundary
// is uniform across the workgroup.  A lane keeps one parity bit and one running dmin2; the crossing test and the four box comparisons
// run for every staged segment, the distance arithmetic with its division only under the box test.
//
// The commit at the end of a region's run.  near / near_d2 / near_inside are updated in registers (strictly smaller wins, and the runs
// of a row ascend, so the smallest region keeps a tie).  The run's near lanes then have to become at most one global atomicAdd per
// non-zero word of hist[g] per workgroup.  CHOICE: an LDS histogram of 2 B T <= 512 words, not ballots.  The ballot form of
// rg_commit costs one ballot per word, here up to 512 per wave and commit, whatever the lanes hold; the lanes of a commit are few and
// spread over few words (the points of two grid rows next to one stretch of boundary), so one LDS add per near lane, one barrier, and
// one sweep of two words per lane is the cheaper form, and it does not grow with B T.  The sweep issues the global adds and clears the
// words it read, so the histogram is all zero between commits.  LDS adds without a return value are waited for by hand before the
// barrier (rp_adds_done: the hazard hvn_kernels.h documents for hvn_pairs.hip -- adds still on their way when a barrier is passed);
// the sweep's clearing stores are ordered before the next commit's adds by that commit's first barrier (__syncthreads_or).  A run with
// no typed near lane in the whole workgroup -- most runs: the lists hold every segment within W of the row, a workgroup's points sit
// next to few of them -- costs that one barrier.
//
// The x-cull of the staged tile (mg_margins<true>, the default).  A row of the grid is as wide as the slide, 256 consecutive slots are
// a short stretch of it, and the row's list holds the segments of the whole row.  The workgroup takes xa, the smallest px of the lanes
// it serves in this row, and leaves out of the tile every segment with box[2] < xa while it stages: such a segment is near none of the
// lanes (px <= box[2] fails) and crossed by none (max(ax, bx) <= box[2] < px: the cull regions.py proves, by comparisons alone).  The
// staged entries keep their order -- a wave ballot gives a lane its place, four LDS words the waves' offsets -- so region runs stay
// runs; a region whose segments are all left out is committed nowhere, and nothing of it was near.  Segments to the RIGHT of all lanes
// stay: they can be crossed, and the crossing rule on them is not provably the straddle test alone (a product may underflow to -0).
// `stride` != 0 of the op selects mg_margins<false>, the form without it, for the A/B of tools/margins_bench.py.
// The host leaves out of the lists the segments that no point at all can be near or cross.
//
// Bounds.  A row comes from hvn_nbr_axis, in [0, ncy); row_start values are clamped to [0, M], segment numbers to [0, S), a region id
// outside [0, G) is committed nowhere, a position outside [0, N) is not written, a type outside [0, T) is counted nowhere (the point
// still gets near): tables the host did not fill give wrong numbers, never an access outside the arrays and never a loop without an
// end.  hist is cleared in stream order before the launch and near / near_d2 / near_inside are stored for every slot, so every
// element of the output is written whatever it held.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define MG_T 256
#define MG_TILE 512           // segments per staging tile: 512 * (64 + 4) bytes = 34 KiB, with the histogram 36.5 KiB of LDS: four workgroups to a CU
#define MG_DONE 0x7FFFFFFF
#define MG_WORDS (2 * HVN_NBR_MARGINS_MAX_B * 16)

struct MarginsDev {
    const double *sx, *sy, *table, *seg, *w2;
    const int *spos, *stype, *seg_region, *rows;
    double *near_d2;
    int *near, *near_inside, *hist;
    int N, ncy, T, G, S, M, B;
};
static_assert(MG_TILE % MG_T == 0, "the staging passes are whole");

// the crossing rule of hvn_regions.hip, every rounding named
__device__ __forceinline__ bool mg_crosses(double px, double py, double ax, double ay, double bx, double by)
{
    const double lhs = __dmul_rn(__dsub_rn(px, ax), __dsub_rn(by, ay));
    const double rhs = __dmul_rn(__dsub_rn(bx, ax), __dsub_rn(py, ay));
    return ay <= py && py < by && lhs < rhs;
}

// d2 of the header, every rounding named
__device__ __forceinline__ double mg_d2(double px, double py, double ax, double ay, double bx, double by)
{
    const double ux = __dsub_rn(bx, ax), uy = __dsub_rn(by, ay), vx = __dsub_rn(px, ax), vy = __dsub_rn(py, ay);
    const double dot = __dadd_rn(__dmul_rn(ux, vx), __dmul_rn(uy, vy));
    const double len2 = __dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy));
    if (dot <= 0.0) return __dadd_rn(__dmul_rn(vx, vx), __dmul_rn(vy, vy));
    if (dot >= len2) {
        const double wx = __dsub_rn(px, bx), wy = __dsub_rn(py, by);
        return __dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy));
    }
    const double c = __dsub_rn(__dmul_rn(ux, vy), __dmul_rn(uy, vx));
    return __ddiv_rn(__dmul_rn(c, c), len2);
}

// the run of region g has ended with this lane's parity `in` and its `dmin` (+inf: no near segment): near / near_d2 / near_inside in
// registers, and the WORKGROUP's near lanes into hist[g].  Called by all 256 lanes alike (g is the workgroup's).
__device__ __forceinline__ void mg_commit(const MarginsDev &a, unsigned *s_hist, const double *s_w2, int g, bool in, double dmin, int ti, int tid,
                                          double &nd2, int &near, int &nin)
{
    if (g < 0 || g >= a.G) return;                  // uniform
    const bool isnear = dmin <= s_w2[a.B - 1];
    if (isnear && dmin < nd2) {
        nd2 = dmin;
        near = g;
        nin = in ? 1 : 0;
    }
    const bool typed = isnear && ti >= 0 && ti < a.T;
    if (!__syncthreads_or(typed)) return;           // uniform
    if (typed) {
        int k = 0;
        while (k < a.B - 1 && !(dmin <= s_w2[k])) ++k;
        atomicAdd(s_hist + ((in ? a.B : 0) + k) * a.T + ti, 1u);
    }
    rp_adds_done();
    __syncthreads();
    const int words = 2 * a.B * a.T;                // <= MG_WORDS
    for (int b = tid; b < words; b += MG_T) {
        const unsigned v = s_hist[b];
        if (v) {
            atomicAdd(a.hist + (long)g * words + b, (int)v);
            s_hist[b] = 0u;
        }
    }
}

template <bool CULL>
__global__ __launch_bounds__(MG_T) void mg_margins(const MarginsDev a)
{
    __shared__ double ts[MG_TILE][8];
    __shared__ int tg[MG_TILE];
    __shared__ int s_next[MG_T / 64], s_kept[MG_T / 64];
    __shared__ double s_xa[MG_T / 64];
    __shared__ unsigned s_hist[MG_WORDS];
    __shared__ double s_w2[HVN_NBR_MARGINS_MAX_B];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long q = (long)blockIdx.x * MG_T + tid;
    const bool valid = q < a.N;
    for (int b = tid; b < MG_WORDS; b += MG_T) s_hist[b] = 0u;
    if (tid < HVN_NBR_MARGINS_MAX_B) s_w2[tid] = a.w2[tid < a.B ? tid : a.B - 1];      // read after the first round's barrier
    double px = 0.0, py = 0.0;
    int ti = -1, cy = MG_DONE;                      // MG_DONE: served, or no point
    if (valid) {
        px = a.sx[q];
        py = a.sy[q];
        ti = a.stype[q];
        cy = hvn_nbr_axis(py, a.table[1], a.table[2], a.ncy);
    }
    double nd2 = __longlong_as_double(0x7FF0000000000000LL);        // +inf
    const double inf = nd2;
    int near = -1, nin = -1;
    for (int served = 0; served < MG_T; ++served) {                 // every round serves at least one lane
        int m = cy;
        for (int d = 32; d > 0; d >>= 1) {
            const int o = __shfl_xor(m, d, 64);
            m = o < m ? o : m;
        }
        if (lane == 0) s_next[wave] = m;
        __syncthreads();
        int row = s_next[0];
#pragma unroll
        for (int w = 1; w < MG_T / 64; ++w) row = s_next[w] < row ? s_next[w] : row;
        __syncthreads();                            // s_next has been read before the next round writes it
        if (row == MG_DONE) break;                  // uniform
        const bool mine = cy == row;
        double xa = 0.0;                            // CULL: the smallest px of the lanes served in this round
        if (CULL) {
            double x = mine ? px : inf;
            for (int d = 32; d > 0; d >>= 1) {
                const double o = __shfl_xor(x, d, 64);
                x = o < x ? o : x;
            }
            if (lane == 0) s_xa[wave] = x;
            __syncthreads();                        // the next round writes s_xa two barriers after these reads
            xa = s_xa[0];
#pragma unroll
            for (int w = 1; w < MG_T / 64; ++w) xa = s_xa[w] < xa ? s_xa[w] : xa;
        }
        const int lo = hvn_nbr_clamp(a.rows[row], a.M), hi = hvn_nbr_clamp(a.rows[row + 1], a.M);
        const int *entries = a.rows + a.ncy + 1;
        int g = -1;                                 // the region of the current run; -1: none yet
        bool in = false;
        double dmin = inf;
        for (int base = lo; base < hi; base += MG_TILE) {
            int n = hi - base < MG_TILE ? hi - base : MG_TILE;
            __syncthreads();                        // the previous tile has been read
            if (!CULL) {
                for (int i = tid; i < n; i += MG_T) {
                    int e = entries[base + i];
                    e = e < 0 ? 0 : (e > a.S - 1 ? a.S - 1 : e);
                    const double *p = a.seg + 8L * e;
#pragma unroll
                    for (int c = 0; c < 8; ++c) ts[i][c] = p[c];
                    tg[i] = a.seg_region[e];
                }
            } else {
                int kept = 0;                       // uniform: the tile's entries so far, <= i0
                for (int i0 = 0; i0 < n; i0 += MG_T) {          // uniform: at most MG_TILE / MG_T passes
                    const int i = i0 + tid;
                    double v[8];
                    int rg = 0;
                    bool keep = false;
                    if (i < n) {
                        int e = entries[base + i];
                        e = e < 0 ? 0 : (e > a.S - 1 ? a.S - 1 : e);
                        const double *p = a.seg + 8L * e;
#pragma unroll
                        for (int c = 0; c < 8; ++c) v[c] = p[c];
                        rg = a.seg_region[e];
                        keep = !(v[6] < xa);
                    }
                    const unsigned long long bal = __ballot(keep);
                    if (lane == 0) s_kept[wave] = __popcll(bal);
                    __syncthreads();
                    int at = kept + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
                    for (int w = 0; w < MG_T / 64; ++w) {
                        at += w < wave ? s_kept[w] : 0;
                        kept += s_kept[w];
                    }
                    if (keep) {                     // at < kept <= i0 + MG_T <= MG_TILE
#pragma unroll
                        for (int c = 0; c < 8; ++c) ts[at][c] = v[c];
                        tg[at] = rg;
                    }
                    __syncthreads();                // s_kept has been read before the next pass writes it; the last pass: the tile is staged
                }
                n = kept;
            }
            __syncthreads();
            for (int i = 0; i < n; ++i) {
                const int eg = tg[i];
                if (eg != g) {                      // uniform: every lane reads the same word
                    mg_commit(a, s_hist, s_w2, g, in, dmin, ti, tid, nd2, near, nin);
                    g = eg;
                    in = false;
                    dmin = inf;
                }
                const double ax = ts[i][0], ay = ts[i][1], bx = ts[i][2], by = ts[i][3];
                in ^= mine && mg_crosses(px, py, ax, ay, bx, by);
                if (mine && ts[i][4] <= px && px <= ts[i][6] && ts[i][5] <= py && py <= ts[i][7]) {
                    const double d2 = mg_d2(px, py, ax, ay, bx, by);
                    if (d2 <= s_w2[a.B - 1]) dmin = d2 < dmin ? d2 : dmin;
                }
            }
        }
        mg_commit(a, s_hist, s_w2, g, in, dmin, ti, tid, nd2, near, nin);
        if (mine) cy = MG_DONE;
    }
    if (valid) {
        const int pos = a.spos[q];
        if (pos >= 0 && pos < a.N) {
            a.near_d2[pos] = nd2;
            a.near[pos] = near;
            a.near_inside[pos] = nin;
        }
    }
}

int hvn_launch_nbr_margins(const NbrMarginsArgs &a, hipStream_t stream)
{
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    MarginsDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table; d.seg = a.seg; d.w2 = a.w2;
    d.spos = w.spos; d.stype = w.stype; d.seg_region = a.seg_region; d.rows = a.rows;
    d.near_d2 = (double *)a.out;
    d.near = (int *)a.out + 2L * a.N; d.near_inside = d.near + a.N; d.hist = d.near_inside + a.N;
    d.N = a.N; d.ncy = a.ncy; d.T = a.T; d.G = a.G; d.S = a.S; d.M = a.M; d.B = a.B;
    if (hipMemsetAsync(d.hist, 0, sizeof(int) * 2 * (size_t)a.G * a.B * a.T, stream) != hipSuccess) return HVN_E_LAUNCH;
    const dim3 grid((unsigned)(((long)a.N + MG_T - 1) / MG_T)), block(MG_T);
    if (a.no_cull)
        hipLaunchKernelGGL(mg_margins<false>, grid, block, 0, stream, d);
    else
        hipLaunchKernelGGL(mg_margins<true>, grid, block, 0, stream, d);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

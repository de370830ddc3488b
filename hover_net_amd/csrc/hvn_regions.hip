// hvn_regions.hip -- nuclei in annotated regions: exact point-in-polygon of N points against the canonical edges of G regions
// (hover_net_amd/regions.py is the definition).  HVN_OP_NBR_REGIONS runs after HVN_OP_NBR_GRID on the same stream and
// reads its workspace as that op left it.
//
// An edge is (ax, ay, bx, by) with ay < by (made so on the host).  Point (px, py) CROSSES it iff
//     ay <= py  and  py < by                                                  comparisons only
//     (px - ax) * (by - ay)  <  (bx - ax) * (py - ay)                         four differences and two products, each one float64 rounding
//                                                                             (named; the library is built with -ffp-contract=off as well),
//                                                                             the products compared, never subtracted
// and lies inside region g iff it crosses an odd number of g's edges.  Per point: first = the smallest such g or -1, hits = their
// number; per (region, type): count = the points of that type inside.
//
// The host gives every grid ROW the list of the edges whose y-span touches it, in region order: row_start [ncy + 1] and the edge
// numbers `entries` [M], one int32 table.  The row of a y is hvn_nbr_axis, the formula NBR_GRID puts points into cells with, and it is
// monotone in y, so the list of a point's row holds every edge the point can cross.
//
// rg_regions: a workgroup of 256 lanes owns 256 consecutive slots of the cell order, one point per lane.  The cell order is row-major,
// so these slots lie in few grid rows (one or two where a row holds 256 points or more, which regions.py aims at).  The workgroup takes
// the rows its lanes occupy one after the other, smallest first -- the next row is the minimum over the lanes not yet served, so the
// walk needs no order in the workspace and ends after at most 256 rows -- and stages that row's list through LDS in tiles of RG_TILE
// edges; lanes of another row sit the list out.  Every lane reads the same edge of the tile (an LDS broadcast), hence the same region
// id: a region boundary is uniform across the workgroup.  A lane keeps one parity bit; at a boundary it commits first / hits in
// registers, and the waves count their inside-lanes per type with ballots, which the workgroup sums through sixteen LDS words per
// wave: one global atomicAdd per non-zero (region, type) per WORKGROUP.  (One per wave was measured first: count is a few cache
// lines that every workgroup adds into, and at a million points the atomics, not the tests, set the op's time -- DESIGN.md 4.22.)
// There are no LDS atomics: LDS sees plain stores, each separated from its readers by a barrier, so the missing-wait hazard that
// hvn_pairs.hip documents -- adds still on their way when a barrier is passed -- has nothing to act on here.
//
// No cull in the kernel.  The host leaves out of the lists the edges that no point at all can cross (wholly above, below or left of
// the points: regions.py proves it), which keeps the clamped end rows short; a per-workgroup x-cull (max(ax, bx) <= px can never
// cross) would be exact too, but the lists are short once they are binned by row.
//
// Bounds.  A row comes from hvn_nbr_axis, in [0, ncy); row_start values are clamped to [0, M], edge numbers to [0, E), a region id
// outside [0, G) is committed nowhere, a position outside [0, N) is not written: tables the host did not fill give wrong numbers,
// never an access outside the arrays and never a loop without an end.  count is cleared in stream order before the launch and first /
// hits are stored for every slot, so every element of the output is written whatever it held.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define RG_T 256
#define RG_TILE 512           // edges per staging tile: 512 * (32 + 4) bytes = 18 KiB of LDS, eight workgroups to a CU
#define RG_DONE 0x7FFFFFFF

struct RegionsDev {
    const double *sx, *sy, *table, *edges;
    const int *spos, *stype, *edge_region, *rows;
    int *first, *hits, *count;
    int N, ncy, T, G, E, M;
};

// the crossing rule, every rounding named
__device__ __forceinline__ bool rg_crosses(double px, double py, double ax, double ay, double bx, double by)
{
    const double lhs = __dmul_rn(__dsub_rn(px, ax), __dsub_rn(by, ay));
    const double rhs = __dmul_rn(__dsub_rn(bx, ax), __dsub_rn(py, ay));
    return ay <= py && py < by && lhs < rhs;
}

// the run of region g has ended with this lane's parity `in`: first / hits in registers, and the WORKGROUP's inside-lanes per type into
// count[g][.].  Called by all 256 lanes alike (g is the workgroup's).  Each wave counts its lanes per type with ballots and leaves the
// T numbers in its own row of s_cnt; after a barrier lane t of wave 0 adds the four and issues the one atomicAdd.  The barrier that
// opens the next commit (or the tile loop's) stands between these reads and the next stores.  A run with no typed inside-lane in the
// whole workgroup -- most of them -- costs the one barrier.
__device__ __forceinline__ void rg_commit(const RegionsDev &a, int (*s_cnt)[16], int g, bool in, int ti, int tid, int &first, int &hits)
{
    if (g < 0 || g >= a.G) return;                  // uniform
    if (in) {
        first = (first < 0 || g < first) ? g : first;
        ++hits;
    }
    const bool typed = in && ti >= 0 && ti < a.T;
    if (!__syncthreads_or(typed)) return;           // uniform
    const int lane = tid & 63, wave = tid >> 6;
    int mine = 0;                                   // lane t: the wave's inside-lanes of type t
    for (int t = 0; t < a.T; ++t) {
        const int c = __popcll(__ballot(typed && ti == t));
        mine = lane == t ? c : mine;
    }
    if (lane < 16) s_cnt[wave][lane] = mine;
    __syncthreads();
    if (tid < a.T) {
        int c = s_cnt[0][tid];
#pragma unroll
        for (int w = 1; w < RG_T / 64; ++w) c += s_cnt[w][tid];
        if (c) atomicAdd(a.count + (long)g * a.T + tid, c);
    }
}

__global__ __launch_bounds__(RG_T) void rg_regions(const RegionsDev a)
{
    __shared__ double te[RG_TILE][4];
    __shared__ int tg[RG_TILE];
    __shared__ int s_next[RG_T / 64], s_cnt[RG_T / 64][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long q = (long)blockIdx.x * RG_T + tid;
    const bool valid = q < a.N;
    double px = 0.0, py = 0.0;
    int ti = -1, cy = RG_DONE;                      // RG_DONE: served, or no point
    if (valid) {
        px = a.sx[q];
        py = a.sy[q];
        ti = a.stype[q];
        cy = hvn_nbr_axis(py, a.table[1], a.table[2], a.ncy);
    }
    int first = -1, hits = 0;
    for (int served = 0; served < RG_T; ++served) {                 // every round serves at least one lane
        int m = cy;
        for (int d = 32; d > 0; d >>= 1) {
            const int o = __shfl_xor(m, d, 64);
            m = o < m ? o : m;
        }
        if (lane == 0) s_next[wave] = m;
        __syncthreads();
        int row = s_next[0];
#pragma unroll
        for (int w = 1; w < RG_T / 64; ++w) row = s_next[w] < row ? s_next[w] : row;
        __syncthreads();                            // s_next has been read before the next round writes it
        if (row == RG_DONE) break;                  // uniform
        const bool mine = cy == row;
        const int lo = hvn_nbr_clamp(a.rows[row], a.M), hi = hvn_nbr_clamp(a.rows[row + 1], a.M);
        const int *entries = a.rows + a.ncy + 1;
        int g = -1;                                 // the region of the current run; -1: none yet
        bool in = false;
        for (int base = lo; base < hi; base += RG_TILE) {
            const int n = hi - base < RG_TILE ? hi - base : RG_TILE;
            __syncthreads();                        // the previous tile has been read
            for (int i = tid; i < n; i += RG_T) {
                int e = entries[base + i];
                e = e < 0 ? 0 : (e > a.E - 1 ? a.E - 1 : e);
                const double *p = a.edges + 4L * e;
                te[i][0] = p[0];
                te[i][1] = p[1];
                te[i][2] = p[2];
                te[i][3] = p[3];
                tg[i] = a.edge_region[e];
            }
            __syncthreads();
            for (int i = 0; i < n; ++i) {
                const int eg = tg[i];
                if (eg != g) {                      // uniform: every lane reads the same word
                    rg_commit(a, s_cnt, g, in, ti, tid, first, hits);
                    g = eg;
                    in = false;
                }
                in ^= mine && rg_crosses(px, py, te[i][0], te[i][1], te[i][2], te[i][3]);
            }
        }
        rg_commit(a, s_cnt, g, in, ti, tid, first, hits);
        if (mine) cy = RG_DONE;
    }
    if (valid) {
        const int pos = a.spos[q];
        if (pos >= 0 && pos < a.N) {
            a.first[pos] = first;
            a.hits[pos] = hits;
        }
    }
}

int hvn_launch_nbr_regions(const NbrRegionsArgs &a, hipStream_t stream)
{
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    RegionsDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table; d.edges = a.edges;
    d.spos = w.spos; d.stype = w.stype; d.edge_region = a.edge_region; d.rows = a.rows;
    d.first = a.out; d.hits = a.out + a.N; d.count = a.out + 2L * a.N;
    d.N = a.N; d.ncy = a.ncy; d.T = a.T; d.G = a.G; d.E = a.E; d.M = a.M;
    if (hipMemsetAsync(d.count, 0, sizeof(int) * (size_t)a.G * a.T, stream) != hipSuccess) return HVN_E_LAUNCH;
    const dim3 grid((unsigned)(((long)a.N + RG_T - 1) / RG_T)), block(RG_T);
    hipLaunchKernelGGL(rg_regions, grid, block, 0, stream, d);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

// hvn_pairs_sim.hip -- the border-corrected typed pair counts of hvn_pairs.hip under SB random relabellings of the points at once: the
// integers behind the random-labelling envelopes of Ripley's cross-type K (hover_net_amd/ripley.py holds the definition, `sims_host` its
// host form).  HVN_OP_NBR_PAIRS_SIM runs after HVN_OP_NBR_GRID on the same stream and reads its workspace as that op
// left it.
//
// Labelling s gives the point at position p the type types[pi_s(p)], pi_s a keyed Feistel bijection of [0, 2^b) walked until it lands
// below N (ripley.py: `permutation`); the eight round keys per simulation come from the host.  d2, kmin, b_i and m_i are those of
// hvn_pairs.hip and do not depend on s, so a pair's geometry is tested ONCE and only the typed adds are made per simulation:
//     per ordered pair (i, j), j != i, with kmin < m_i, and per s with both labels in [0, T):
//         acc[s][a_s][b_s][kmin] += 1   and, where m_i < R,   acc[s][a_s][b_s][m_i] -= 1
// which is plane 1 of hvn_pairs.hip's accumulator, a difference array whose running sum the host forms, and
//     cnt[s][a_s][m_i] += 1 per point i
// from which n_in[s][a][k] = the sum of cnt[s][a][m] over m > k.
//
// rp_labels: a lane per slot q.  It finds m_q, walks pi_s for s < SB from the slot's position, packs the SB labels into W = ceil(SB / 4)
// words of four bytes (0xFF: a type outside [0, T), and the simulations past SB of the last word) and counts cnt in an LDS histogram
// that the workgroup flushes with 64-bit global atomics.  The walk applies the bijection at most 2^b - N + 1 times: the cycle of a
// value below N holds at most the 2^b - N values that are not, then one that is.  The loop is bounded by that count whatever the keys
// are, and a position outside [0, N) is clamped before it starts.
//
// rp_pairs_sim follows rp_pairs: a workgroup of 256 lanes owns 256 consecutive slots, stages the union of its lanes' candidate runs
// through LDS in tiles of RP_TILE candidates per grid row offset -- here with the candidates' W label words -- and every wave walks the
// part of the tile that its own lanes' runs cover; j != i is a comparison of slots, kmin a bisection over the padded r2 table.  The
// histogram is ONE plane of T T R signed 32-bit words per simulation: +1 at kmin and -1 at m_i, both only where kmin < m_i (a lane with
// m_i == R, nearly every nucleus of a slide, makes one add per simulation).
//
// Overflow.  A lane tests a candidate at most once and then changes a word of a simulation's plane by at most 1 (kmin and m_i are
// different bins), so between two flushes no word moves by more than the tests of the workgroup in between: RP_FLUSH tiles of
// RP_TILE candidates for 256 lanes, 2^23.  The flush adds the non-zero words, sign-extended, into `out` with 64-bit global atomics
// (sums modulo 2^64; the final running sums lie in [0, 2^52]) and clears them.  `out` is cleared in stream order before the first
// launch, so every element is written whatever it held; integer sums make it a function of the inputs alone.
//
// Every loop bound is a cell_start value clamped to [0, N], SB, W or the walk's count; a bin index is built from labels tested against
// T, k <= R - 1 and m_i < R: a workspace that the grid op did not fill gives wrong numbers, never an access outside the arrays and
// never a loop without an end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

typedef unsigned long long u64;

struct PairsSimDev {
    const double *sx, *sy, *table, *rt;
    const int *spos, *types, *cell_start;
    const u64 *keys;
    unsigned *labels;
    u64 *out;
    long stride;                // words of one simulation in out: T T R + T (R + 1)
    int N, ncy, ncx, T, R, SB, W, hl, hh, walk;
};

// m of the definition for the point (qx, qy): b from four subtractions, then the prefix of the ascending radii that it reaches
__device__ __forceinline__ int rs_m(const double *rt, int R, double qx, double qy)
{
    double b = __dsub_rn(qx, rt[0]);
    const double b1 = __dsub_rn(rt[2], qx), b2 = __dsub_rn(qy, rt[1]), b3 = __dsub_rn(rt[3], qy);
    b = b1 < b ? b1 : b;
    b = b2 < b ? b2 : b;
    b = b3 < b ? b3 : b;
    int m = 0;
    for (int k = 0; k < R; ++k) m += rt[4 + k] <= b ? 1 : 0;
    return m;
}

__device__ __forceinline__ u64 rs_mix(u64 z)          // the splitmix64 finaliser
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// F_s of ripley.py on [0, 2^(hl + hh)): eight rounds, each an involution
__device__ __forceinline__ u64 rs_feistel(u64 x, const u64 *key, int hl, int hh)
{
    const u64 ml = (1ull << hl) - 1, mh = (1ull << hh) - 1;
    u64 lo = x & ml, hi = x >> hl;
#pragma unroll
    for (int r = 0; r < 8; r += 2) {
        hi ^= rs_mix(lo + key[r]) & mh;
        lo ^= rs_mix(hi + key[r + 1]) & ml;
    }
    return (hi << hl) | lo;
}

__global__ __launch_bounds__(RP_T) void rp_labels(const PairsSimDev a)
{
    extern __shared__ int cnt[];                    // [SB][T][R + 1]
    const int N = a.N, T = a.T, R = a.R, SB = a.SB, tid = threadIdx.x;
    const int words = SB * T * (R + 1);
    for (int b = tid; b < words; b += RP_T) cnt[b] = 0;
    __syncthreads();
    const long q = (long)blockIdx.x * RP_T + tid;
    if (q < N) {
        const int m = rs_m(a.rt, R, a.sx[q], a.sy[q]);
        int pos = a.spos[q];
        pos = pos < 0 ? 0 : (pos > N - 1 ? N - 1 : pos);
        for (int w = 0; w < a.W; ++w) {
            unsigned word = 0xFFFFFFFFu;
            for (int u = 0; u < 4 && 4 * w + u < SB; ++u) {
                const int s = 4 * w + u;
                u64 x = (u64)pos;
                for (int step = 0; step < a.walk; ++step) {     // at most 2^b - N + 1 applications reach a value below N
                    x = rs_feistel(x, a.keys + 8 * s, a.hl, a.hh);
                    if (x < (u64)N) break;
                }
                x = x < (u64)N ? x : (u64)pos;                   // only for a count that is not the walk's
                const int t = a.types ? a.types[x] : 0;
                if (t >= 0 && t < T) {
                    word ^= (0xFFu ^ (unsigned)t) << (8 * u);
                    atomicAdd(&cnt[(s * T + t) * (R + 1) + m], 1);
                }
            }
            a.labels[q * a.W + w] = word;
        }
    }
    __syncthreads();
    const int per = T * (R + 1);
    for (int b = tid; b < words; b += RP_T) {
        const int v = cnt[b];
        if (v) atomicAdd(a.out + (b / per) * a.stride + (a.stride - per) + b % per, (u64)v);
    }
}

// the SB planes into out, non-zero words only and sign-extended, and cleared; the caller puts a barrier before and after
__device__ __forceinline__ void rs_flush(int *hist, const PairsSimDev &a, int bins, int tid)
{
    for (int b = tid; b < a.SB * bins; b += RP_T) {
        const int v = hist[b];
        if (v) atomicAdd(a.out + (b / bins) * a.stride + b % bins, (u64)(long long)v);
        hist[b] = 0;
    }
}

// bit 7 of every byte of a label word that is no type: the byte is >= T (T <= 16; 0xFF is the label kernel's own mark, and whatever
// else the workspace may hold is caught all the same)
__device__ __forceinline__ unsigned rs_bad(unsigned word, int T)
{
    return (((word & 0x7F7F7F7Fu) + 0x01010101u * (unsigned)(0x80 - T)) | word) & 0x80808080u;
}

// the adds of one counted pair for the four simulations of a label word: +1 at kmin and, where m_i < R, -1 at m_i (kmin < m_i holds).
// CHECK: a simulation whose bit of `bad` is set -- a type outside [0, T) as i or as j, or a simulation past SB -- is left out.  The
// products stay below 2^24 (types < 16, R <= 32), so they are 24-bit multiplications.
template <bool CHECK>
__device__ __forceinline__ void rs_adds(int *plane, int bins, unsigned li, unsigned lj, unsigned bad, int T, int R, int k, int mi)
{
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (CHECK && (bad & (0x80u << (8 * u)))) continue;
        const int ti = (li >> (8 * u)) & 0xFF, tj = (lj >> (8 * u)) & 0xFF;
        int *const row = plane + u * bins + __mul24(__mul24(ti, T) + tj, R);
        atomicAdd(row + k, 1);
        if (mi < R) atomicAdd(row + mi, -1);
    }
}

__global__ __launch_bounds__(RP_T) void rp_pairs_sim(const PairsSimDev a)
{
    extern __shared__ int dyn[];                    // hist [SB][T][T][R], then tl [RP_TILE][W], then sl [W][RP_T]
    __shared__ double tx[RP_TILE], ty[RP_TILE], s_r2[32];
    __shared__ int s_lo[3], s_hi[3];
    const int N = a.N, T = a.T, R = a.R, SB = a.SB, W = a.W, tid = threadIdx.x, lane = tid & 63;
    const int bins = T * T * R;
    int *const hist = dyn;
    unsigned *const tl = (unsigned *)(dyn + SB * bins), *const sl = tl + RP_TILE * W;
    for (int b = tid; b < SB * bins; b += RP_T) hist[b] = 0;
    if (tid < 32) s_r2[tid] = tid < R ? a.rt[4 + R + tid] : __builtin_inf();
    if (tid < 3) {
        s_lo[tid] = RP_NONE;
        s_hi[tid] = 0;
    }
    const double x0 = a.table[0], y0 = a.table[1], c = a.table[2], r2max = a.table[3];
    const long q = (long)blockIdx.x * RP_T + tid;
    const bool valid = q < N;
    double qx = 0.0, qy = 0.0;
    int cx = 0, cy = 0, mi = 0;
    if (valid) {
        qx = a.sx[q];
        qy = a.sy[q];
        cx = hvn_nbr_axis(qx, x0, c, a.ncx);
        cy = hvn_nbr_axis(qy, y0, c, a.ncy);
        mi = rs_m(a.rt, R, qx, qy);
    }
    for (int w = 0; w < W; ++w) sl[w * RP_T + tid] = valid ? a.labels[q * W + w] : 0xFFFFFFFFu;     // a lane reads only its own
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
                rs_flush(hist, a, bins, tid);
                tiles = 0;
            }
            ++tiles;
            for (int i = tid; i < n; i += RP_T) {
                tx[i] = a.sx[base + i];
                ty[i] = a.sy[base + i];
            }
            for (int i = tid; i < n * W; i += RP_T) tl[i] = a.labels[(long)base * W + i];
            __syncthreads();                // also: the flush's clearing is done before any add
            const int c0 = (wlo > base ? wlo : base) - base;
            const int c1 = (whi < base + n ? whi : base + n) - base;
            for (int i = c0; i < c1; ++i) {
                const int g = base + i;
                const double d2 = hvn_nbr_d2(tx[i], ty[i], qx, qy);
                if (!(valid && g >= lo && g < hi && g != (int)q && d2 <= r2max)) continue;      // the bisection is for pairs within r_{R-1} only
                int k = 0;                          // #{ k : r2_k < d2 } = kmin; the padding is +inf
#pragma unroll
                for (int s = 16; s > 0; s >>= 1) k += s_r2[k + s - 1] < d2 ? s : 0;
                k = k < R ? k : R - 1;              // only for tables that break table[3] == r2_{R-1}
                if (k < mi) {                       // the geometry, once for all SB
                    for (int w = 0; w < W; ++w) {
                        const unsigned li = sl[w * RP_T + tid], lj = tl[i * W + w];
                        const unsigned past = 4 * w + 4 <= SB ? 0u : 0x80808080u << (8 * (SB - 4 * w));
                        const unsigned bad = rs_bad(li, T) | rs_bad(lj, T) | past;
                        int *const plane = hist + 4 * w * bins;
                        if (bad == 0u) rs_adds<false>(plane, bins, li, lj, 0u, T, R, k, mi);        // a slide: every type is one
                        else rs_adds<true>(plane, bins, li, lj, bad, T, R, k, mi);
                    }
                }
            }
        }
    }
    rp_adds_done();
    __syncthreads();
    rs_flush(hist, a, bins, tid);
}

int hvn_launch_nbr_pairs_sim(const NbrPairsSimArgs &a, hipStream_t stream)
{
    static std::atomic<unsigned long long> done{0};
    if (int rc = hvn_max_lds_once((const void *)rp_pairs_sim, (int)HVN_NBR_PAIRS_SIM_MAX_LDS, done)) return rc;
    const NbrWorkspace w = hvn_nbr_workspace(a.workspace, a.N, (long)a.ncy * a.ncx);
    PairsSimDev d;
    d.sx = w.sx; d.sy = w.sy; d.table = a.table; d.rt = a.rt;
    d.spos = w.spos; d.types = a.types; d.cell_start = w.cell_start;
    d.keys = a.keys; d.labels = a.labels; d.out = (u64 *)a.out;
    const int bins = a.T * a.T * a.R;
    d.stride = bins + a.T * (a.R + 1);
    d.N = a.N; d.ncy = a.ncy; d.ncx = a.ncx; d.T = a.T; d.R = a.R; d.SB = a.SB;
    d.W = HVN_NBR_PAIRS_SIM_WORDS(a.SB);
    int b = 0;                              // b = max(2, bit_length(N - 1)), split into hl low and hh high bits
    while (b < 32 && ((long)(a.N - 1) >> b)) ++b;
    b = b < 2 ? 2 : b;
    d.hl = b / 2;
    d.hh = b - d.hl;
    d.walk = (int)((1L << b) - a.N + 1);
    const dim3 grid((unsigned)(((long)a.N + RP_T - 1) / RP_T)), block(RP_T);
    if (a.phase != 2) {
        if (hipMemsetAsync(a.out, 0, sizeof(long long) * (size_t)a.SB * d.stride, stream) != hipSuccess) return HVN_E_LAUNCH;
        hipLaunchKernelGGL(rp_labels, grid, block, sizeof(int) * (size_t)a.SB * a.T * (a.R + 1), stream, d);
        if (hipGetLastError() != hipSuccess) return HVN_E_LAUNCH;
    }
    if (a.phase != 1) hipLaunchKernelGGL(rp_pairs_sim, grid, block, (size_t)HVN_NBR_PAIRS_SIM_LDS_BYTES(a.SB, bins), stream, d);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

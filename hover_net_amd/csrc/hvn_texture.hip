// hvn_texture.hip -- per-nucleus grey-level co-occurrence counts (HVN_OP_INST_TEXTURE; hover_net_amd/texture.py is the definition,
// DESIGN.md 4.27): the third pass over the label map, next to hvn_instance_table and hvn_instance_features.  Per record slot it
// delivers the grey power sums, the nucleus's own grey extremes, the histogram of 8 grey levels and the ORDERED co-occurrence counts
// glcm[d][a][b] at the four distance-1 offsets (1, 0), (1, 1), (0, 1), (-1, 1) (y down).  Everything is an integer, so the result is
// bit-reproducible; texture.py derives contrast, homogeneity, energy, correlation and entropy on the host.
//
// ONE WAVE PER RECORD SLOT, four slots per workgroup, no global atomics, no workspace.  The wave walks the record's bbox (clamped to
// the map) in column strips: lane i of a strip looks at column xs - 1 + i, the 62 lanes 1..62 OWN their column, lanes 0 and 63 are the
// halo that the offsets x +- 1 reach.  Per row the mask (inst == label, inside the bbox) is one 64-bit ballot and the levels of the
// neighbours come from cross-lane moves of the row's level register, never from second loads.  The pairs of a pixel are counted when
// the row BELOW it has been read (the row loop runs one row past the bbox; that row is a zero word, not a load), each pair once, at
// its upper or left pixel, by the strip that owns that pixel.
//
// The counts live in a per-wave LDS block of 264 words (hist + glcm) and are written out once.  Chromatin is smooth, so most lanes of
// a row want the same one or two words.  `tx_add` has two forms.  The plain one issues one LDS add per pair and lets the LDS unit
// serialise equal addresses; it is the product's form, because it measured three to five times faster than the other (DESIGN.md
// 4.27, profiles/texture_bench.txt).  The merged one first merges equal keys on chip -- one ballot per distinct key present in the
// row, the lowest lane of each key keeps the popcount -- and then issues ONE LDS add in which every address is distinct; it is kept
// as the template's other half, selected by the op's `stride`, so that tools/texture_bench.py can time the two against each other.
//
// scale "range" needs the nucleus's extremes before it can form a level: a first walk finds them (per-lane min / max, one wave
// reduction), a second walk forms levels and pairs.  A level is ((g - lo) * 8) / span with span = hi - lo + 1 in 1..256; the division
// is a multiplication by ceil(2^20 / span) and a shift, which is exact for every numerator up to 2040 (the error term n * (M * span -
// 2^20) stays below 2040 * 256 < 2^20).  Every loop is bounded by the map extent and nothing outside [0, H) x [0, W) is addressed,
// whatever the table says; a level is masked to three bits so that no input can index outside the wave's LDS block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define TX_T 256            // four waves = four record slots per workgroup (per-wave LDS, no barrier: an empty slot's wave just leaves)
#define TX_OWN 62           // owned columns of a strip (64 lanes - 1 halo column on either side)
#define TX_ACC (HVN_TEX_LEVELS + 4 * HVN_TEX_LEVELS * HVN_TEX_LEVELS)      // 264 words per wave: hist[8], glcm[4][8][8]

static_assert(HVN_TEX_LEVELS == 8 && HVN_TEX_WORDS == 12 + TX_ACC && HVN_TEX_WORDS % 2 == 0, "a slot is 12 header words, then hist and glcm: 138 qwords");

static __device__ __forceinline__ long long tx_wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

static __device__ __forceinline__ int tx_grey(const uint8_t *p)     // (77 R + 150 G + 29 B + 128) >> 8 in 0..255
{
    return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8;
}

// acc[key] += 1 for every lane with `valid`.  MERGE (the form that lost): equal keys are merged first, so that the one LDS add has
// distinct addresses.
template <bool MERGE>
static __device__ __forceinline__ void tx_add(unsigned *acc, int lane, bool valid, int key)
{
    if (!MERGE) {
        if (valid) atomicAdd(acc + key, 1u);
        return;
    }
    unsigned long long todo = __ballot(valid);
    unsigned cnt = 0;
    while (todo) {                                  // one round per distinct key: every round clears at least the leader's bit
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(valid && key == k);
        if (lane == leader) cnt = (unsigned)__popcll(same);
        todo &= ~same;
    }
    if (cnt) atomicAdd(acc + key, cnt);
}

template <bool MERGE>
__global__ __launch_bounds__(TX_T) void tx_texture(const int32_t *__restrict__ inst, const uint8_t *__restrict__ image, int H, int W,
                                                   const hvn_inst_rec *__restrict__ rec, int max_inst, long n_slots, int fixed,
                                                   int32_t *__restrict__ out_all)
{
    __shared__ unsigned s_acc[TX_T / 64][TX_ACC];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long slot = __builtin_amdgcn_readfirstlane((int)((long)blockIdx.x * (TX_T / 64) + wave));
    if (slot >= n_slots) return;
    const int map = (int)(slot / max_inst);
    const int label = (int)(slot - (long)map * max_inst) + 1;
    const hvn_inst_rec r = rec[slot];
    int32_t *out = out_all + slot * HVN_TEX_WORDS;

    // the bbox clamped to the map: nothing outside [0, H) x [0, W) is ever addressed
    const int r0 = r.rmin > 0 ? r.rmin : 0, r1 = r.rmax < H ? r.rmax : H;
    const int c0 = r.cmin > 0 ? r.cmin : 0, c1 = r.cmax < W ? r.cmax : W;
    if (r.area <= 0 || r0 >= r1 || c0 >= c1) {
#pragma unroll
        for (int k = 0; k < (HVN_TEX_WORDS / 2 + 63) / 64; ++k)       // 138 qwords: the output is 8-byte aligned and a slot is 1104 bytes
            if (lane + 64 * k < HVN_TEX_WORDS / 2) ((long long *)out)[lane + 64 * k] = 0ll;
        return;
    }
    const int32_t *m = inst + (long)map * H * W;
    const uint8_t *img = image + (long)map * H * W * 3;
    unsigned *acc = s_acc[wave];
#pragma unroll
    for (int k = 0; k < (TX_ACC + 63) / 64; ++k)
        if (lane + 64 * k < TX_ACC) acc[lane + 64 * k] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the block is cleared by other lanes than add to it
    __builtin_amdgcn_wave_barrier();

    int lo = 0, span = 256;
    if (!fixed) {       // the first walk: the extremes of the mask
        int gmin = 255, gmax = 0;
        // minima and maxima do not mind a pixel seen twice: a column or row past the box is clamped into it instead of masked out,
        // so that the loads are unconditional and four rows are in flight at once
        for (int xs = c0; xs < c1; xs += TX_OWN) {
            const int x = xs - 1 + lane < c0 ? c0 : xs - 1 + lane >= c1 ? c1 - 1 : xs - 1 + lane;
            for (int y = r0; y < r1; y += 4) {
                int lab[4], g[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long at = (long)(y + k < r1 ? y + k : r1 - 1) * W + x;
                    lab[k] = m[at];
                    g[k] = tx_grey(img + at * 3);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (lab[k] != label) continue;
                    gmin = g[k] < gmin ? g[k] : gmin;
                    gmax = g[k] > gmax ? g[k] : gmax;
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int a = __shfl_xor(gmin, d, 64), b = __shfl_xor(gmax, d, 64);
            gmin = a < gmin ? a : gmin;
            gmax = b > gmax ? b : gmax;
        }
        if (gmin <= gmax) { lo = gmin; span = gmax - gmin + 1; }    // no mask pixel at all: the levels are never used
    }
    const unsigned magic = ((1u << 20) + (unsigned)span - 1u) / (unsigned)span;     // wave-uniform: q = (n * magic) >> 20 == n / span, n <= 2040

    // every sum fits: 255^4 * (2^31 - 1) < 2^63, and a mask has fewer than 2^31 pixels
    long long s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    int gmin = 255, gmax = 0, seen = 0;
    const bool own = lane >= 1 && lane <= TX_OWN;

    for (int xs = c0; xs < c1; xs += TX_OWN) {
        const int x = xs - 1 + lane;
        const bool col_ok = x >= c0 && x < c1;
        unsigned long long mp = 0;                      // the mask of row y - 1
        int qp = 0;                                     // and its levels
        int next = 0, next_g = 0;                       // the row one ahead is in flight while this one is counted
        if (col_ok) {
            next = m[(long)r0 * W + x];
            next_g = tx_grey(img + ((long)r0 * W + x) * 3);
        }
        for (int y = r0; y <= r1; ++y) {
            const int cur = next, g = next_g;
            if (y + 1 < r1 && col_ok) {
                next = m[(long)(y + 1) * W + x];
                next_g = tx_grey(img + ((long)(y + 1) * W + x) * 3);
            }
            const bool in = y < r1 && col_ok && cur == label;
            const unsigned long long mc = __ballot(in);
            const int q = in ? (int)(((unsigned)((g - lo) * 8) * magic) >> 20) & (HVN_TEX_LEVELS - 1) : 0;
            if (in && own) {
                const int g2 = g * g;
                s1 += g; s2 += g2; s3 += (long long)g2 * g; s4 += (long long)g2 * g2;
                gmin = g < gmin ? g : gmin;
                gmax = g > gmax ? g : gmax;
            }
            seen += __popcll(__ballot(in && own));
            if (mp) {                                   // the pairs of row y - 1, now that the row below it is known
                const int qr = __shfl_down(qp, 1, 64);                          // the level right of the pixel, same row
                const int br = __shfl_down(q, 1, 64), bl = __shfl_up(q, 1, 64); // below right, below left
                const bool p = own && ((mp >> lane) & 1);
                tx_add<MERGE>(acc, lane, p, qp);
                tx_add<MERGE>(acc, lane, p && ((mp >> 1 >> lane) & 1), HVN_TEX_LEVELS + 0 * 64 + qp * 8 + qr);
                tx_add<MERGE>(acc, lane, p && ((mc >> 1 >> lane) & 1), HVN_TEX_LEVELS + 1 * 64 + qp * 8 + br);
                tx_add<MERGE>(acc, lane, p && ((mc >> lane) & 1), HVN_TEX_LEVELS + 2 * 64 + qp * 8 + q);
                tx_add<MERGE>(acc, lane, p && ((mc << 1 >> lane) & 1), HVN_TEX_LEVELS + 3 * 64 + qp * 8 + bl);
            }
            mp = mc; qp = q;
        }
    }

    s1 = tx_wave_sum(s1); s2 = tx_wave_sum(s2); s3 = tx_wave_sum(s3); s4 = tx_wave_sum(s4);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_xor(gmin, d, 64), b = __shfl_xor(gmax, d, 64);
        gmin = a < gmin ? a : gmin;
        gmax = b > gmax ? b : gmax;
    }
    if (gmin > gmax) gmin = gmax = 0;                   // no mask pixel inside the clamped box (a stale table)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the block is read by other lanes than added to it
    __builtin_amdgcn_wave_barrier();

    // the slot: gsum as 4 qwords, then seen, lo, hi, 0, then the 264 counts
    long long v = s1;
    v = lane == 1 ? s2 : v;
    v = lane == 2 ? s3 : v;
    v = lane == 3 ? s4 : v;
    if (lane < 4) ((long long *)out)[lane] = v;
    int h = seen;
    h = lane == 1 ? gmin : h;
    h = lane == 2 ? gmax : h;
    h = lane == 3 ? 0 : h;
    if (lane < 4) out[8 + lane] = h;
#pragma unroll
    for (int k = 0; k < (TX_ACC + 63) / 64; ++k)
        if (lane + 64 * k < TX_ACC) out[12 + lane + 64 * k] = (int32_t)acc[lane + 64 * k];
}

int hvn_launch_inst_texture(const InstTextureArgs &a, hipStream_t stream)
{
    const long n_slots = (long)a.N * a.max_inst;
    const long blocks = (n_slots + TX_T / 64 - 1) / (TX_T / 64);
    if (!a.merge)
        hipLaunchKernelGGL(tx_texture<false>, dim3((unsigned)blocks), dim3(TX_T), 0, stream, a.inst, a.image, a.H, a.W, a.rec, a.max_inst,
                           n_slots, a.fixed, a.out);
    else
        hipLaunchKernelGGL(tx_texture<true>, dim3((unsigned)blocks), dim3(TX_T), 0, stream, a.inst, a.image, a.H, a.W, a.rec, a.max_inst,
                           n_slots, a.fixed, a.out);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

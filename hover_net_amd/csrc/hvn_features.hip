// hvn_features.hip -- per-nucleus morphometric sums (second, richer pass over the label map next to hvn_instance_table): second
// moments about the bbox origin, the pixel count found inside the bbox, the three border-pixel classes of scikit-image's
// 4-neighbourhood perimeter estimator and, with an image, the per-channel colour sums.  Everything is an integer, so the result is
// bit-reproducible; hover_net_amd/features.py derives the float features on the host.
//
// ONE WAVE PER RECORD SLOT, no atomics, no init pass, no workspace.  The wave walks the record's bbox (clamped to the map) in column
// strips: lane i of a strip looks at column xs - 2 + i, the 60 lanes 2..61 OWN their column (sums and class counts), lanes 0, 1, 62, 63
// are the halo the 5 x 5 footprint of "border pixel with border neighbours" needs.  A nucleus (~20 px across) is one strip; a bbox
// wider than 60 columns is walked strip after strip by the same code, every pixel owned exactly once.  Per row the mask
// (inst == label, inside the bbox) is one 64-bit ballot, so the row words live in scalar registers:
//     border word  b(r) = m(r) & ~(m(r) << 1 & m(r) >> 1 & m(r-1) & m(r+1))
//     n4 / nd of lane i from bits i-1..i+1 of b(r-1), b(r), b(r+1); the class counts are popcounts of three ballots.
// The row loop runs two rows past the bbox so that the three-row pipeline drains; rows outside the bbox are zero words, not loads.
// The mask is the label INSIDE the record's bbox: for a table made from this map that is the whole label; for a stale or foreign
// table the clamp keeps every read inside the map and `seen != area` tells the caller.  Every loop is bounded by the map extent.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_error.h"   // include/hvn.h and hvn_fail

#define FT_T 256            // four waves = four record slots per workgroup (no LDS, no barrier: an empty slot's wave just leaves)
#define FT_OWN 60           // owned columns of a strip (64 lanes - 2 halo columns on either side)

static_assert(sizeof(hvn_inst_feat) == 88, "hvn_inst_feat is stored as 11 qwords");

static __device__ __forceinline__ long long ft_wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

static __device__ __forceinline__ int ft_bits3(unsigned long long word, int lane)   // bits lane-1, lane, lane+1 (lane in 1..62)
{
    return (int)(word >> (lane - 1)) & 7;
}

__global__ __launch_bounds__(FT_T) void ft_features(const int32_t *__restrict__ inst, const uint8_t *__restrict__ image, int H, int W,
                                                    const hvn_inst_rec *__restrict__ rec, int max_inst, long n_slots,
                                                    hvn_inst_feat *__restrict__ feats)
{
    const int lane = threadIdx.x & 63;
    const long slot = __builtin_amdgcn_readfirstlane((int)((long)blockIdx.x * (FT_T / 64) + (threadIdx.x >> 6)));
    if (slot >= n_slots) return;
    const int map = (int)(slot / max_inst);
    const int label = (int)(slot - (long)map * max_inst) + 1;
    const hvn_inst_rec r = rec[slot];
    unsigned long long *out = (unsigned long long *)(feats + slot);

    // the bbox clamped to the map: nothing outside [0, H) x [0, W) is ever addressed
    const int r0 = r.rmin > 0 ? r.rmin : 0, r1 = r.rmax < H ? r.rmax : H;
    const int c0 = r.cmin > 0 ? r.cmin : 0, c1 = r.cmax < W ? r.cmax : W;
    if (r.area <= 0 || r0 >= r1 || c0 >= c1) {
        if (lane < 11) out[lane] = 0ull;
        return;
    }
    const int32_t *m = inst + (long)map * H * W;
    const uint8_t *img = image ? image + (long)map * H * W * 3 : nullptr;

    long long sxx = 0, syy = 0, sxy = 0, cs0 = 0, cs1 = 0, cs2 = 0, cq0 = 0, cq1 = 0, cq2 = 0;
    int seen = 0, per0 = 0, per1 = 0, per2 = 0;   // wave-uniform (popcounts of ballots)
    const bool own = lane >= 2 && lane < 2 + FT_OWN;

    for (int xs = c0; xs < c1; xs += FT_OWN) {
        const int x = xs - 2 + lane;
        const bool col_ok = x >= c0 && x < c1;
        const long long dx = x - r.cmin;
        unsigned long long m0 = 0, m1 = 0, bA = 0, bB = 0;       // mask rows y-2, y-1; border rows y-3, y-2
        int next = col_ok ? m[(long)r0 * W + x] : 0;            // the row one ahead is in flight while this one is counted
        for (int y = r0; y < r1 + 2; ++y) {
            const int cur = next;
            if (y + 1 < r1) next = col_ok ? m[(long)(y + 1) * W + x] : 0;
            const bool in = y < r1 && col_ok && cur == label;
            const unsigned long long m2 = __ballot(in);
            if (in && own) {
                const long long dy = y - r.rmin;
                sxx += dx * dx; syy += dy * dy; sxy += dx * dy;
                if (img) {
                    const uint8_t *p = img + ((long)y * W + x) * 3;
                    const long long a = p[0], b = p[1], c = p[2];
                    cs0 += a; cs1 += b; cs2 += c;
                    cq0 += a * a; cq1 += b * b; cq2 += c * c;
                }
            }
            seen += __popcll(__ballot(in && own));
            // border of row y-1 (valid on lanes 1..62), then the classes of row y-2 (owned lanes) from border rows y-3, y-2, y-1
            const unsigned long long bC = m1 & ~((m1 << 1) & (m1 >> 1) & m0 & m2);
            if (bB) {
                const int a = own ? ft_bits3(bA, lane) : 0, b = own ? ft_bits3(bB, lane) : 0, c = own ? ft_bits3(bC, lane) : 0;
                const int n4 = (b & 1) + (b >> 2) + (a >> 1 & 1) + (c >> 1 & 1);
                const int nd = (a & 1) + (a >> 2) + (c & 1) + (c >> 2);
                const bool on = (b & 2) != 0;
                per0 += __popcll(__ballot(on && (n4 == 2 || n4 == 3) && nd <= 2));
                per1 += __popcll(__ballot(on && ((n4 == 0 && nd == 2) || (n4 == 1 && nd == 3))));
                per2 += __popcll(__ballot(on && n4 == 1 && (nd == 1 || nd == 2)));
            }
            m0 = m1; m1 = m2; bA = bB; bB = bC;
        }
    }

    sxx = ft_wave_sum(sxx); syy = ft_wave_sum(syy); sxy = ft_wave_sum(sxy);
    if (img) {
        cs0 = ft_wave_sum(cs0); cs1 = ft_wave_sum(cs1); cs2 = ft_wave_sum(cs2);
        cq0 = ft_wave_sum(cq0); cq1 = ft_wave_sum(cq1); cq2 = ft_wave_sum(cq2);
    }
    // the slot as 11 qwords, one per lane: sxx, syy, sxy, seen | per[0], per[1] | per[2], csum[3], csq[3]
    unsigned long long v = (unsigned long long)sxx;
    v = lane == 1 ? (unsigned long long)syy : v;
    v = lane == 2 ? (unsigned long long)sxy : v;
    v = lane == 3 ? ((unsigned long long)(unsigned)seen | (unsigned long long)(unsigned)per0 << 32) : v;
    v = lane == 4 ? ((unsigned long long)(unsigned)per1 | (unsigned long long)(unsigned)per2 << 32) : v;
    v = lane == 5 ? (unsigned long long)cs0 : v;
    v = lane == 6 ? (unsigned long long)cs1 : v;
    v = lane == 7 ? (unsigned long long)cs2 : v;
    v = lane == 8 ? (unsigned long long)cq0 : v;
    v = lane == 9 ? (unsigned long long)cq1 : v;
    v = lane == 10 ? (unsigned long long)cq2 : v;
    if (lane < 11) out[lane] = v;
}

extern "C" {

size_t hvn_instance_features_workspace_bytes(int n, int h, int w, int max_inst)
{
    (void)n; (void)h; (void)w; (void)max_inst;
    return 0;   // one wave per slot keeps its sums in registers
}

int hvn_instance_features(const int32_t *inst, const uint8_t *image, int n, int h, int w, const hvn_inst_rec *records, int max_inst,
                          hvn_inst_feat *feats, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    if (!inst || !records || !feats) return hvn_fail(HVN_E_ARG, "instance_features: null inst, records or feats");
    if (n <= 0 || h <= 0 || w <= 0 || max_inst <= 0) return hvn_fail(HVN_E_ARG, "instance_features: n, h, w or max_inst < 1 (max_inst = %d)", max_inst);
    if ((long)h * w >= (1L << 31)) return hvn_fail(HVN_E_ARG, "instance_features: h * w >= 2^31 (h = %d)", h);
    if (((uintptr_t)feats & 7) || ((uintptr_t)records & 7) || ((uintptr_t)inst & 3))
        return hvn_fail(HVN_E_ARG, "instance_features: feats and records must be 8-byte, inst 4-byte aligned");
    const long n_slots = (long)n * max_inst;
    if (n_slots >= (1L << 31)) return hvn_fail(HVN_E_SIZE, "instance_features: n * max_inst >= 2^31 (%ld slots)", n_slots);
    const long blocks = (n_slots + FT_T / 64 - 1) / (FT_T / 64);
    hipLaunchKernelGGL(ft_features, dim3((unsigned)blocks), dim3(FT_T), 0, (hipStream_t)stream, inst, image, h, w, records, max_inst,
                       n_slots, feats);
    return hvn_launched("instance_features");
}

}  // extern "C"

// hvn_valid.hip -- the validation statistics of the reference's proc_valid_step_output (models/hovernet/run_desc.py:262-333, scalar
// half) accumulated on the device: nucleus-pixel accuracy and Dice at p > 0.5, per-type Dice, HV squared error.  Every scalar is a
// ratio of integer counts or a sum of squares over a pixel count, so the state is 4 + 2 * nr_types int64 counts and one float64 sum;
// one launch pair per batch adds that batch into the caller's state with no host sync (hover_net_amd/valid_stats.py reads it once
// per epoch and does the divisions on the host).
//
//   vs_partial   one workgroup per VS_BLK pixels of the flattened [n * h * w] batch (the grid depends on the pixel count only).  The
//                interleaved [pixels][C] prediction map is read as whole 16-byte vectors, lanes on consecutive vectors: C = 4 is one
//                vector per pixel; C = 3 (12-byte pixels) goes through LDS, from which lane i takes pixel i at a stride of 3 words
//                (no bank conflict).  The targets are read with lanes on consecutive pixels.  Counts: one ballot + popcount per
//                predicate and wave, so they are wave-uniform integers (no atomics); the four waves' counts are added through LDS
//                and the workgroup STORES its VS_SLOTS counts and its squared-error sum as row blockIdx.x of the workspace.
//                Squared error: each lane adds its (up to) 2 * VS_PIX terms in pixel order, the wave sums by a butterfly, the four
//                waves are added in wave order -- the same tree every run.
//   vs_finalize  one workgroup: slot j's rows are added in 64-bit integers (any order is exact) and the float64 rows are added in
//                workgroup order by one lane, then the batch's sums are added to the state with plain stores.
// No float atomics, no integer atomics: the state after a call sequence is a fixed function of the inputs and that sequence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

// a term is the ROUNDED float64 square, added afterwards (numpy's (err * err).sum()): never a fused multiply-add into the running sum
#pragma clang fp contract(off)

#define VS_T 256                  // threads per workgroup (4 waves)
#define VS_PIX 4                  // pixels per thread
#define VS_BLK (VS_T * VS_PIX)    // 1024 pixels per workgroup: 421 workgroups at 164 x 164 x 16
#define VS_MAX_TYPES 16
#define VS_SLOTS (3 + 2 * VS_MAX_TYPES)   // np_correct, np_inter, np_total, then (tp_inter_t, tp_total_t) per type

static size_t vs_align(size_t x) { return (x + 255) & ~(size_t)255; }
static long vs_blocks(long P) { return (P + VS_BLK - 1) / VS_BLK; }

__device__ __forceinline__ unsigned vs_count(bool p) { return (unsigned)__popcll(__ballot(p)); }

template <int C>
__global__ void __launch_bounds__(VS_T) vs_partial(const float *__restrict__ pred, const int32_t *__restrict__ np_map,
                                                   const float *__restrict__ hv_map, const int32_t *__restrict__ tp_map, long P, int T,
                                                   double *__restrict__ part_sse, unsigned *__restrict__ part_cnt)
{
    __shared__ float4 tile[C == 3 ? VS_BLK * 3 / 4 : 1];
    __shared__ unsigned wcnt[VS_T / 64][VS_SLOTS];
    __shared__ double wsse[VS_T / 64];
    const long p0 = (long)blockIdx.x * VS_BLK;            // first pixel of the workgroup; p0 * C floats is a whole number of vectors
    if (C == 3) {
        const long F = P * 3, f0 = p0 * 3;                 // floats in the map / before this tile
        for (int j = 0; j < 3; ++j) {
            const int v = j * VS_T + threadIdx.x;          // vector of the tile
            const long f = f0 + 4L * v;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f + 3 < F)
                q = *(const float4 *)(pred + f);
            else if (f < F) {                              // the map's last, partial vector
                q.x = pred[f];
                if (f + 1 < F) q.y = pred[f + 1];
                if (f + 2 < F) q.z = pred[f + 2];
            }
            tile[v] = q;
        }
        __syncthreads();
    }
    unsigned cnt[VS_SLOTS];
#pragma unroll
    for (int j = 0; j < VS_SLOTS; ++j) cnt[j] = 0;
    double sse = 0.0;
#pragma unroll
    for (int k = 0; k < VS_PIX; ++k) {
        const int lp = k * VS_T + threadIdx.x;             // pixel of the tile: lanes on consecutive pixels
        const long i = p0 + lp;
        const bool act = i < P;
        float tp_f = 0.f, prob = 0.f, ph = 0.f, pv = 0.f;
        int tn = 0, tt = -1;
        float2 th = make_float2(0.f, 0.f);
        if (act) {
            if (C == 3) {
                const float *px = (const float *)tile + lp * 3;
                prob = px[0]; ph = px[1]; pv = px[2];
            } else {
                const float4 q = *(const float4 *)(pred + i * 4);
                tp_f = q.x; prob = q.y; ph = q.z; pv = q.w;
                tt = tp_map[i];
            }
            tn = np_map[i];
            th = *(const float2 *)(hv_map + i * 2);
        }
        const bool pn = act && prob > 0.5f;                // exactly 0.5 and NaN are not nucleus
        const bool t1 = act && tn == 1;
        cnt[0] += vs_count(act && (int)pn == tn);
        cnt[1] += vs_count(pn && t1);
        cnt[2] += vs_count(pn) + vs_count(t1);
        if (C == 4) {
#pragma unroll
            for (int t = 0; t < VS_MAX_TYPES; ++t)
                if (t < T) {                               // wave-uniform
                    const bool a = act && tt == t, b = act && tp_f == (float)t;     // the float channel against the integer label
                    cnt[3 + 2 * t] += vs_count(a && b);
                    cnt[4 + 2 * t] += vs_count(a) + vs_count(b);
                }
        }
        if (act) {
            const double d0 = (double)ph - (double)th.x, d1 = (double)pv - (double)th.y;
            const double s0 = d0 * d0, s1 = d1 * d1;
            sse += s0;
            sse += s1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sse += __shfl_xor(sse, o);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < VS_SLOTS; ++j) wcnt[wave][j] = cnt[j];
        wsse[wave] = sse;
    }
    __syncthreads();
    if (threadIdx.x < VS_SLOTS) {
        unsigned s = 0;
        for (int wv = 0; wv < VS_T / 64; ++wv) s += wcnt[wv][threadIdx.x];
        part_cnt[(long)blockIdx.x * VS_SLOTS + threadIdx.x] = s;
    }
    if (threadIdx.x == 64) {
        double s = wsse[0];
        for (int wv = 1; wv < VS_T / 64; ++wv) s += wsse[wv];
        part_sse[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(VS_T) vs_finalize(const double *__restrict__ part_sse, const unsigned *__restrict__ part_cnt, long rows,
                                                    long P, int T, long long *counts, double *hv_sse)
{
    __shared__ double stage[VS_T];
    if (threadIdx.x < 3 + 2 * T) {
        unsigned long long s = 0;
        for (long r = 0; r < rows; ++r) s += part_cnt[r * VS_SLOTS + threadIdx.x];
        counts[1 + threadIdx.x] += (long long)s;
    }
    if (threadIdx.x == VS_T - 1) counts[0] += (long long)P;
    double batch = 0.0;                                    // lane 0's: the rows in workgroup order, VS_T of them staged at a time
    for (long r0 = 0; r0 < rows; r0 += VS_T) {
        const long r = r0 + threadIdx.x;
        stage[threadIdx.x] = r < rows ? part_sse[r] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = rows - r0 < VS_T ? (int)(rows - r0) : VS_T;
            for (int j = 0; j < m; ++j) batch += stage[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *hv_sse += batch;
}

size_t hvn_valid_ws_bytes(long P)
{
    const size_t rows = (size_t)vs_blocks(P);
    return vs_align(rows * sizeof(double)) + vs_align(rows * VS_SLOTS * sizeof(unsigned));
}

// c = 3 (no type channel; tp_map and nr_types unused) | 4; the caller has checked the arguments.  -> 0, -4 (workspace), -2 (launch)
int hvn_launch_valid_stats(const float *pred, const int32_t *np_map, const float *hv_map, const int32_t *tp_map, long P, int c, int nr_types,
                           long long *counts, double *hv_sse, void *ws, size_t ws_bytes, hipStream_t stream)
{
    if (ws_bytes < hvn_valid_ws_bytes(P)) return HVN_E_SIZE;
    const long rows = vs_blocks(P);
    double *part_sse = (double *)ws;
    unsigned *part_cnt = (unsigned *)((unsigned char *)ws + vs_align((size_t)rows * sizeof(double)));
    if (c == 3)
        hipLaunchKernelGGL(vs_partial<3>, dim3((unsigned)rows), dim3(VS_T), 0, stream, pred, np_map, hv_map, tp_map, P, 0, part_sse, part_cnt);
    else
        hipLaunchKernelGGL(vs_partial<4>, dim3((unsigned)rows), dim3(VS_T), 0, stream, pred, np_map, hv_map, tp_map, P, nr_types, part_sse,
                           part_cnt);
    if (hipGetLastError() != hipSuccess) return HVN_E_LAUNCH;
    hipLaunchKernelGGL(vs_finalize, dim3(1), dim3(VS_T), 0, stream, (const double *)part_sse, (const unsigned *)part_cnt, rows, P,
                       c == 3 ? 0 : nr_types, counts, hv_sse);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

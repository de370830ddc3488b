// hvn_tissue.hip -- the automatic tissue mask of whole-slide inference on the device, bit-equal to hover_net_amd/tissue_mask.py
// (simple_get_mask: grey, Otsu threshold, tissue = dark side, drop small 8-connected objects, fill small 4-connected holes, dilate
// with a disk).  Integer arithmetic and integer atomics only: the result is a function of the input alone.  The Otsu threshold
// itself is float64 work on 256 counters and stays on the host, between the two entry points.
//
//   tm_gray_hist   grey = (R*4899 + G*9617 + B*1868 + 8192) >> 14 and its 256-bin histogram: counters per workgroup in LDS, merged
//                  into global memory with one integer atomic per non-empty bin.  Four pixels per lane as three dwords in, one dword
//                  out where both planes are dword-aligned; a byte form otherwise.
//   connected components, twice (objects: set = grey <= t, 8-connected; holes: set = object plane == 0, 4-connected).  The union-find
//   of hvn_postproc.hip, restated for components of millions of pixels:
//     tm_ccl_init    one wave per row, 64 pixels per step: a set pixel's parent is the first pixel of its horizontal run (from the
//                    ballot of the step and the run carried in from the step before), so no chain is ever as long as a row;
//     tm_ccl_merge   joins a pixel to the row above only where the pair is the FIRST contact of its two runs (the pair to its left
//                    does not join the same two runs), with path halving in every find;
//     tm_ccl_count   flattens, and adds one count per stretch of lanes of a wave that share a root -- not one per pixel: the
//                    background of a thumbnail is one component;
//     tm_ccl_filter  keeps components of at least `thr` pixels (objects), or writes the complement of that (holes).
//   disk dilation, exact, in two passes:
//     tm_hdist       one wave per row: distance along the row to the nearest set pixel, clamped to R + 1, uint8, from three ballots;
//     tm_vdilate     out(y, x) = OR over dy in [-R, R] of dist(y + dy, x) <= isqrt(R^2 - dy^2); a tile's rows and its 2R halo rows
//                    are staged in LDS, rows outside the image hold 255 and contribute nothing.
// Linear pixel indices are int32 (the launcher's caller bounds h * w by 2^30); byte offsets are 64-bit.  Every loop is bounded by
// the image, the radius or a parent chain whose indices strictly decrease.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define TM_T 256
#define TM_RMAX 32
#define TM_TH 32             // tm_vdilate: output rows per tile
#define TM_TW 64             // tm_vdilate: output columns per tile, one per lane

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t tm_gray(uint32_t r, uint32_t g, uint32_t b) { return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14; }

template <int VEC>
__global__ __launch_bounds__(TM_T) void tm_gray_hist(const uint8_t *__restrict__ rgb, long P, uint8_t *__restrict__ gray, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const long stride = (long)gridDim.x * TM_T;
    if (VEC) {
        const long Q = P >> 2;  // whole groups of four pixels: 12 bytes in, 4 out
        const uint32_t *src = (const uint32_t *)rgb;
        for (long q = (long)blockIdx.x * TM_T + threadIdx.x; q < Q; q += stride) {
            const uint32_t a = src[3 * q], b = src[3 * q + 1], c = src[3 * q + 2];
            const uint32_t g0 = tm_gray(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
            const uint32_t g1 = tm_gray(a >> 24, b & 255u, (b >> 8) & 255u);
            const uint32_t g2 = tm_gray((b >> 16) & 255u, b >> 24, c & 255u);
            const uint32_t g3 = tm_gray((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
            ((uint32_t *)gray)[q] = g0 | g1 << 8 | g2 << 16 | g3 << 24;
            atomicAdd(&lh[g0], 1u);
            atomicAdd(&lh[g1], 1u);
            atomicAdd(&lh[g2], 1u);
            atomicAdd(&lh[g3], 1u);
        }
    }
    for (long i = (VEC ? (P & ~3L) : 0L) + (long)blockIdx.x * TM_T + threadIdx.x; i < P; i += stride) {
        const uint32_t g = tm_gray(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
        gray[i] = (uint8_t)g;
        atomicAdd(&lh[g], 1u);
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(hist + threadIdx.x, c);
}

// ---------------------------------------------------------------------------------------------
// union-find on the plane (hvn_postproc.hip's, with path halving): par[i] <= i always, every store lowers a parent to an ancestor
__device__ __forceinline__ int tm_load(const int32_t *par, int i) { return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int tm_find(int32_t *par, int i)
{
    int p = tm_load(par, i);
    while (p != i) {
        const int g = tm_load(par, p);
        if (g != p) atomicMin(par + i, g);  // halve the path: g is an ancestor of i and below p
        i = p;
        p = g;
    }
    return i;
}

__device__ void tm_union(int32_t *par, int a, int b)
{
    for (;;) {
        a = tm_find(par, a);
        b = tm_find(par, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(par + a, b);  // attach the larger root under the smaller
        if (old == a) return;
        a = old;                                // a was no root any more: join what it pointed to instead
    }
}

// mode 0: set = src <= t (the dark side of the grey plane); mode 1: set = src == 0 (the complement of a mask)
__device__ __forceinline__ bool tm_set(const uint8_t *src, long i, int mode, int t) { return mode ? src[i] == 0 : (int)src[i] <= t; }

__global__ __launch_bounds__(TM_T) void tm_ccl_init(const uint8_t *__restrict__ src, int h, int w, int mode, int t, int32_t *__restrict__ par)
{
    const int y = blockIdx.x * (TM_T / 64) + (threadIdx.x >> 6);
    if (y >= h) return;  // whole waves leave: the ballots below see full waves of one row
    const int lane = threadIdx.x & 63;
    const long row = (long)y * w;
    int carry = -1;      // first pixel of the run that reaches the end of the step before (wave-uniform), -1 = none
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        const bool s = x < w && tm_set(src, row + x, mode, t);
        const unsigned long long m = __ballot(s);
        const unsigned long long gaps = ~m & ((1ull << lane) - 1ull);  // unset pixels of this step to the left of the lane
        int start;
        if (gaps)
            start = x0 + 64 - __clzll((long long)gaps);                // the pixel after the nearest of them
        else
            start = carry >= 0 ? carry : x0;
        if (x < w) par[row + x] = s ? (int)(row + start) : -1;
        carry = __shfl(s ? start : -1, 63);
    }
}

__global__ __launch_bounds__(TM_T) void tm_ccl_merge(int32_t *par, int h, int w, int conn8)
{
    const long i = (long)blockIdx.x * TM_T + threadIdx.x;
    if (i >= (long)h * w) return;
    if (tm_load(par, (int)i) < 0) return;
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    if (y == 0) return;
    const int up = (int)i - w;
    const bool u = tm_load(par, up) >= 0;
    const bool l = x > 0 && tm_load(par, (int)i - 1) >= 0;
    if (u) {
        // the pair to the left joins the same two runs unless one of its pixels is unset
        if (!(l && tm_load(par, up - 1) >= 0)) tm_union(par, (int)i, up);
    } else if (conn8) {
        // a diagonal pair counts only where neither straight neighbour makes the contact
        if (x > 0 && !l && tm_load(par, up - 1) >= 0) tm_union(par, (int)i, up - 1);
        if (x + 1 < w && tm_load(par, up + 1) >= 0 && tm_load(par, (int)i + 1) < 0) tm_union(par, (int)i, up + 1);
    }
}

__global__ __launch_bounds__(TM_T) void tm_ccl_count(int32_t *par, int32_t *cnt, long P)
{
    const long i = (long)blockIdx.x * TM_T + threadIdx.x;  // whole waves stay: lanes past the end take part in the ballot as unset
    const int lane = threadIdx.x & 63;
    int r = -1;
    if (i < P && par[i] >= 0) {
        r = (int)i;
        int p;
        while ((p = tm_load(par, r)) != r) r = p;
        par[i] = r;  // racing writers all store a valid ancestor; the final state is the root
    }
    const int prev = __shfl_up(r, 1);
    const bool head = lane == 0 || r != prev;              // first lane of a stretch of equal roots (or of unset pixels)
    const unsigned long long heads = __ballot(head);
    if (head && r >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int n = above ? __ffsll((long long)above) : 64 - lane;
        atomicAdd(cnt + r, n);
    }
}

// out = (set and its component has at least thr pixels) != invert
__global__ __launch_bounds__(TM_T) void tm_ccl_filter(const int32_t *__restrict__ par, const int32_t *__restrict__ cnt, long P, int thr, int invert,
                                                      uint8_t *__restrict__ out)
{
    const long i = (long)blockIdx.x * TM_T + threadIdx.x;
    if (i >= P) return;
    const int r = par[i];
    const int keep = r >= 0 && cnt[r] >= thr;
    out[i] = (uint8_t)(keep ^ invert);
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_T) void tm_hdist(const uint8_t *__restrict__ src, int h, int w, int radius, uint8_t *__restrict__ dist)
{
    const int y = blockIdx.x * (TM_T / 64) + (threadIdx.x >> 6);
    if (y >= h) return;
    const int lane = threadIdx.x & 63;
    const long row = (long)y * w;
    const int far = radius + 1;  // <= 33: the steps on either side of a lane's own (64 pixels each) hold every pixel that matters
    unsigned long long prev = 0ull, cur = __ballot(lane < w && src[row + lane] != 0);
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int xn = x0 + 64 + lane;
        const unsigned long long next = __ballot(xn < w && src[row + xn] != 0);
        int d = far;
        const unsigned long long le = cur & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);  // set pixels of this step at or left of the lane
        if (le)
            d = min(d, lane - (63 - __clzll((long long)le)));
        else if (prev)
            d = min(d, lane + 1 + __clzll((long long)prev));
        const unsigned long long ge = cur >> lane;                                           // ... at or right of it
        if (ge)
            d = min(d, __ffsll((long long)ge) - 1);
        else if (next)
            d = min(d, 64 - lane + __ffsll((long long)next) - 1);
        if (x0 + lane < w) dist[row + x0 + lane] = (uint8_t)d;
        prev = cur;
        cur = next;
    }
}

__global__ __launch_bounds__(TM_T) void tm_vdilate(const uint8_t *__restrict__ dist, int h, int w, int radius, int tiles_x, uint8_t *__restrict__ out)
{
    __shared__ uint8_t rows[TM_TH + 2 * TM_RMAX][TM_TW];
    __shared__ uint8_t reach[2 * TM_RMAX + 1];  // reach[dy + radius] = isqrt(radius^2 - dy^2)
    const int t = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x = tx * TM_TW + (t & 63), y0 = ty * TM_TH;
    if (t <= 2 * radius) {
        const int dy = t - radius, q = radius * radius - dy * dy;
        int r = 0;
        while ((r + 1) * (r + 1) <= q) ++r;  // at most `radius` steps
        reach[t] = (uint8_t)r;
    }
    const int nrows = TM_TH + 2 * radius;
    for (int j = t >> 6; j < nrows; j += TM_T / 64) {
        const int y = y0 - radius + j;
        rows[j][t & 63] = (y >= 0 && y < h && x < w) ? dist[(long)y * w + x] : (uint8_t)255;
    }
    __syncthreads();
    if (x >= w) return;
    for (int k = t >> 6; k < TM_TH; k += TM_T / 64) {
        const int y = y0 + k;
        if (y >= h) break;
        int hit = 0;
        for (int j = 0; j <= 2 * radius; ++j) hit |= rows[k + j][t & 63] <= reach[j];
        out[(long)y * w + x] = (uint8_t)hit;
    }
}

// ---------------------------------------------------------------------------------------------
static inline size_t tm_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t hvn_tissue_workspace_bytes(int h, int w)
{
    const size_t P = (size_t)h * (size_t)w;
    return 2 * tm_align(P * sizeof(int32_t)) + 3 * tm_align(P);  // par, cnt; objects, holes, dist
}

int hvn_launch_tissue_gray_hist(const uint8_t *rgb, int h, int w, uint8_t *gray, uint32_t *hist256, hipStream_t s)
{
    const long P = (long)h * w;
    if (hipMemsetAsync(hist256, 0, 256 * sizeof(uint32_t), s) != hipSuccess) return HVN_E_LAUNCH;
    const bool vec = (((uintptr_t)rgb | (uintptr_t)gray) & 3) == 0;
    const long items = vec ? (P >> 2) + 3 : P;
    long blocks = (items + TM_T - 1) / TM_T;
    blocks = blocks > 2048 ? 2048 : blocks;  // 8 workgroups per CU: each merges its 256 counters once
    if (vec)
        hipLaunchKernelGGL(tm_gray_hist<1>, dim3((unsigned)blocks), dim3(TM_T), 0, s, rgb, P, gray, hist256);
    else
        hipLaunchKernelGGL(tm_gray_hist<0>, dim3((unsigned)blocks), dim3(TM_T), 0, s, rgb, P, gray, hist256);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

int hvn_launch_tissue_mask(const uint8_t *gray, int h, int w, int threshold, int min_obj, int max_hole, int radius, uint8_t *mask,
                           uint8_t *tap_objects, uint8_t *tap_holes, void *workspace, hipStream_t s)
{
    const long P = (long)h * w;
    uint8_t *ws = (uint8_t *)workspace;
    int32_t *par = (int32_t *)ws;
    int32_t *cnt = (int32_t *)(ws + tm_align((size_t)P * sizeof(int32_t)));
    uint8_t *planes = ws + 2 * tm_align((size_t)P * sizeof(int32_t));
    uint8_t *obj = tap_objects ? tap_objects : planes;
    uint8_t *hol = tap_holes ? tap_holes : planes + tm_align((size_t)P);
    uint8_t *dist = planes + 2 * tm_align((size_t)P);
    const dim3 per_pixel((unsigned)((P + TM_T - 1) / TM_T)), per_row((unsigned)((h + TM_T / 64 - 1) / (TM_T / 64))), block(TM_T);

    for (int pass = 0; pass < 2; ++pass) {  // 0: objects of the thresholded grey plane; 1: holes = objects of the complement
        if (hipMemsetAsync(cnt, 0, (size_t)P * sizeof(int32_t), s) != hipSuccess) return HVN_E_LAUNCH;
        hipLaunchKernelGGL(tm_ccl_init, per_row, block, 0, s, pass ? obj : gray, h, w, pass, threshold, par);
        hipLaunchKernelGGL(tm_ccl_merge, per_pixel, block, 0, s, par, h, w, pass ? 0 : 1);
        hipLaunchKernelGGL(tm_ccl_count, per_pixel, block, 0, s, par, cnt, P);
        hipLaunchKernelGGL(tm_ccl_filter, per_pixel, block, 0, s, par, cnt, P, pass ? max_hole : min_obj, pass, pass ? hol : obj);
    }
    hipLaunchKernelGGL(tm_hdist, per_row, block, 0, s, hol, h, w, radius, dist);
    const int tiles_x = (w + TM_TW - 1) / TM_TW, tiles_y = (h + TM_TH - 1) / TM_TH;
    hipLaunchKernelGGL(tm_vdilate, dim3((unsigned)((long)tiles_x * tiles_y)), block, 0, s, dist, h, w, radius, tiles_x, mask);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

// hvn_contour_dev.hip -- the per-instance contours of process() (post_proc.py:132-143) traced on the device, bit-equal to the host
// tracer (hvn_contour.cpp) for maps in which EVERY LABEL IS ONE 8-CONNECTED PIECE (hvn_postproc's output: a watershed instance is
// 4-connected).  For such a label contours[0] is the outer border that starts at the label's first pixel in raster order, and
// Tracer::follow only ever asks "zero / non-zero" of a pixel -- the marks decide which border starts the raster scan recognises, not
// where a trace goes.  So no crop is framed, scanned or marked: one lane per record slot finds the start pixel on row rmin and walks
// the border, O(perimeter) steps, reading the instance map in place.
//
//   ct_trace<false>  count pass: points per slot (-1 = flagged) into the workspace; flags go to status[0] / status[2].
//   ct_scan          one workgroup: exclusive prefix sum of the counts in (map, slot) order, chunk by chunk with a carry -> offs;
//                    status[1] = the total does not fit.  The layout is a function of the input alone (no cursor).
//   ct_trace<true>   emit pass: the same walk again, storing the points of every slot whose range fits in max_pts.
//
// A step gathers the eight neighbours of the current pixel as independent loads into a bit mask (one memory latency per step) and
// finds the next direction with a shift and a find-first-set.  Foreground = (inst == label) AND inside the record's bbox (the host's
// framed crop), so nothing outside the map is read.  Every loop is bounded: the start search by the bbox width, the walk by
// 4 * area + 8 steps (a border pixel is visited at most four times); a record that breaks a bound, or whose walk does not span its
// bbox (a label of several pieces with different bboxes, a stale table), is FLAGGED and owns no points.  A second piece inside the
// first piece's bbox is not detected: one piece per label is the caller's contract.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_error.h"   // include/hvn.h and hvn_fail

#define CT_T 64          // one wave per workgroup: a few thousand live lanes, spread over as many CUs as possible
#define CT_SCAN_T 256
#define CT_SCAN_ITEMS 8  // counts per lane and chunk

static size_t ct_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the walk is plain integer code, compiled for the host too so that it can be checked against hvn_contour.cpp without a device
#define CT_HD __host__ __device__ __forceinline__
CT_HD int ct_min(int a, int b) { return a < b ? a : b; }
CT_HD int ct_max(int a, int b) { return a > b ? a : b; }

// bit s = neighbour s of (y, x) is foreground; neighbours counter-clockwise from east: E, NE, N, NW, W, SW, S, SE
CT_HD unsigned ct_neighbours(const int32_t *__restrict__ m, int W, int label, int r0, int r1, int c0, int c1, int y,
                                                  int x)
{
    constexpr int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
    constexpr int DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
    int v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {  // clamped into the bbox: eight unconditional, independent loads
        const int yy = ct_min(ct_max(y + DY[s], r0), r1 - 1), xx = ct_min(ct_max(x + DX[s], c0), c1 - 1);
        v[s] = m[(long)yy * W + xx];
    }
    unsigned mask = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int yy = y + DY[s], xx = x + DX[s];
        mask |= (unsigned)(yy >= r0 && yy < r1 && xx >= c0 && xx < c1 && v[s] == label) << s;
    }
    return mask;
}

// the step of direction s, two bits per direction (value + 1): no runtime-indexed table in the walk
CT_HD int ct_dx(int s) { return (int)(0x901Au >> (2 * s) & 3u) - 1; }
CT_HD int ct_dy(int s) { return (int)(0xA901u >> (2 * s) & 3u) - 1; }

// -> number of CHAIN_APPROX_SIMPLE points of the border, -1 = flagged.  EMIT: point k < cap goes to out[k].
template <bool EMIT>
CT_HD int ct_walk(const int32_t *__restrict__ m, int H, int W, const hvn_inst_rec *__restrict__ rec, int2 *out,
                                       int cap)
{
    const int label = rec->label, r0 = rec->rmin, r1 = rec->rmax, c0 = rec->cmin, c1 = rec->cmax;
    if (r0 < 0 || c0 < 0 || r1 > H || c1 > W || r1 <= r0 || c1 <= c0) return -1;
    // start: leftmost foreground pixel of row rmin, eight columns per round
    int x0 = -1;
    const int32_t *row = m + (long)r0 * W;
    for (int xb = c0; xb < c1 && x0 < 0; xb += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = row[ct_min(xb + k, c1 - 1)];
#pragma unroll
        for (int k = 7; k >= 0; --k)
            if (xb + k < c1 && v[k] == label) x0 = xb + k;
    }
    if (x0 < 0) return -1;
    const int y0 = r0;
    int n = 0;
    unsigned mask = ct_neighbours(m, W, label, r0, r1, c0, c1, y0, x0);
    // first neighbour: clockwise from west (NW, N, NE, E, SE, S, SW); west itself only ends the host's search
    int s = -1;
#pragma unroll
    for (int k = 7; k >= 1; --k)
        if (mask >> ((4 - k) & 7) & 1) s = (4 - k) & 7;
    if (s < 0) {  // isolated pixel
        if (r1 - r0 != 1 || c1 - c0 != 1) return -1;
        if (EMIT && cap > 0) out[0] = int2{x0, y0};
        return 1;
    }
    const int y1 = y0 + ct_dy(s), x1 = x0 + ct_dx(s);
    int y3 = y0, x3 = x0, prev_s = s ^ 4;
    int ymin = y0, ymax = y0, xmin = x0, xmax = x0;
    // 4 * area + 8 steps (hvn_trace_contours' bound: a border pixel is left at most four times); the foreground lies in the bbox, so
    // a stale area beyond the bbox's does not lengthen the bound, and the point count stays an int32
    const long box = (long)(r1 - r0) * (c1 - c0);
    const long by_area = 4L * (rec->area < box ? rec->area : box) + 8;
    const long max_steps = by_area < 0x7fffffffL ? by_area : 0x7fffffffL;
    for (long step = 0;; ++step) {
        if (step >= max_steps) return -1;
        // counter-clockwise search, starting after the direction we came from (s + 8 = that direction itself)
        const unsigned t = ((mask | mask << 8) >> (s + 1)) & 0xffu;
        if (!t) return -1;  // cannot happen on an unchanged map: the pixel we came from is foreground
        s = (s + __builtin_ffs((int)t)) & 7;
        const int y4 = y3 + ct_dy(s), x4 = x3 + ct_dx(s);
        if (s != prev_s) {
            if (EMIT && n < cap) out[n] = int2{x3, y3};
            ++n;
            prev_s = s;
        }
        if (y4 == y0 && x4 == x0 && y3 == y1 && x3 == x1) break;
        y3 = y4;
        x3 = x4;
        ymin = ct_min(ymin, y3); ymax = ct_max(ymax, y3);
        xmin = ct_min(xmin, x3); xmax = ct_max(xmax, x3);
        s = (s + 4) & 7;
        mask = ct_neighbours(m, W, label, r0, r1, c0, c1, y3, x3);
    }
    if (ymin != r0 || ymax != r1 - 1 || xmin != c0 || xmax != c1 - 1) return -1;  // the walk must span the record's bbox
    return n;
}

template <bool EMIT>
__global__ __launch_bounds__(CT_T) void ct_trace(const int32_t *__restrict__ inst, int H, int W, const hvn_inst_rec *__restrict__ recs,
                                                 int max_inst, long M, int32_t *__restrict__ cnt, const int64_t *__restrict__ offs,
                                                 int2 *__restrict__ pts, int64_t max_pts, int32_t *__restrict__ status)
{
    const long i = (long)blockIdx.x * CT_T + threadIdx.x;
    if (i >= M) return;
    const hvn_inst_rec *rec = recs + i;
    const int32_t *m = inst + (i / max_inst) * ((long)H * W);
    if (!EMIT) {
        int c = 0;
        if (rec->area > 0) {
            c = ct_walk<false>(m, H, W, rec, nullptr, 0);
            if (c < 0) {
                atomicAdd(status + 0, 1);
                atomicMin((unsigned *)status + 2, (unsigned)i);  // starts at 0xffffffff = -1: no record flagged
            }
        }
        cnt[i] = c;
    } else {
        const int c = cnt[i];
        if (c <= 0) return;
        const int64_t o = offs[i];
        if (o + c > max_pts) return;  // offs stays exact; the caller sizes a second call from offs[M]
        ct_walk<true>(m, H, W, rec, pts + o, c);
    }
}

__global__ __launch_bounds__(CT_SCAN_T) void ct_scan(const int32_t *__restrict__ cnt, long M, int64_t *__restrict__ offs, int64_t max_pts,
                                                     int32_t *__restrict__ status)
{
    __shared__ long long wsum[CT_SCAN_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long base = 0; base < M; base += CT_SCAN_T * CT_SCAN_ITEMS) {
        const long i0 = base + (long)threadIdx.x * CT_SCAN_ITEMS;
        int v[CT_SCAN_ITEMS];
        long long t = 0;
#pragma unroll
        for (int k = 0; k < CT_SCAN_ITEMS; ++k) {
            v[k] = i0 + k < M ? max(cnt[i0 + k], 0) : 0;  // a flagged record (-1) owns nothing
            t += v[k];
        }
        long long inc = t;  // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long u = __shfl_up(inc, d);
            if (lane >= d) inc += u;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CT_SCAN_T / 64; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        long long ex = carry + before + inc - t;
#pragma unroll
        for (int k = 0; k < CT_SCAN_ITEMS; ++k) {
            if (i0 + k < M) offs[i0 + k] = ex;
            ex += v[k];
        }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        offs[M] = carry;
        status[1] = carry > max_pts;
    }
}

extern "C" {

size_t hvn_contours_workspace_bytes(int n, int max_inst)
{
    if (n <= 0 || max_inst <= 0) return 0;
    return ct_align((size_t)n * max_inst * sizeof(int32_t));
}

int hvn_trace_contours_device(const int32_t *inst, int n, int h, int w, const hvn_inst_rec *records, int max_inst, int32_t *pts,
                              int64_t max_pts, int64_t *offs, int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!inst || !records || !offs || !status) return hvn_fail(HVN_E_ARG, "trace_contours_device: null inst, records, offs or status");
    if (n <= 0 || h <= 0 || w <= 0 || max_inst <= 0 || max_pts < 0)
        return hvn_fail(HVN_E_ARG, "trace_contours_device: n, h, w or max_inst < 1, or max_pts < 0 (max_inst = %d)", max_inst);
    if (max_pts > 0 && (!pts || ((uintptr_t)pts & 7)))   // points are stored as (x, y) pairs
        return hvn_fail(HVN_E_ARG, "trace_contours_device: pts NULL or not 8-byte aligned");
    if ((long)h * w >= (1L << 31)) return hvn_fail(HVN_E_ARG, "trace_contours_device: h * w >= 2^31 (h = %d)", h);
    const long M = (long)n * max_inst;
    if (M >= 0x7fffffffL) return hvn_fail(HVN_E_ARG, "trace_contours_device: n * max_inst >= 2^31 - 1 (%ld slots)", M);  // status[2] holds a slot index
    if (!workspace || workspace_bytes < hvn_contours_workspace_bytes(n, max_inst))
        return hvn_fail(HVN_E_SIZE, "trace_contours_device: workspace NULL or smaller than hvn_contours_workspace_bytes (%zu bytes given)", workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    int32_t *cnt = (int32_t *)workspace;
    const unsigned blocks = (unsigned)((M + CT_T - 1) / CT_T);
    if (hipMemsetAsync(status, 0, 4 * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(status + 2, 0xff, sizeof(int32_t), s) != hipSuccess)
        return hvn_fail(HVN_E_LAUNCH, "trace_contours_device: hipMemsetAsync failed");
    hipLaunchKernelGGL(ct_trace<false>, dim3(blocks), dim3(CT_T), 0, s, inst, h, w, records, max_inst, M, cnt, (const int64_t *)nullptr,
                       (int2 *)nullptr, (int64_t)0, status);
    hipLaunchKernelGGL(ct_scan, dim3(1), dim3(CT_SCAN_T), 0, s, (const int32_t *)cnt, M, offs, max_pts, status);
    hipLaunchKernelGGL(ct_trace<true>, dim3(blocks), dim3(CT_T), 0, s, inst, h, w, records, max_inst, M, cnt, (const int64_t *)offs,
                       (int2 *)pts, max_pts, status);
    return hvn_launched("trace_contours_device");
}

}  // extern "C"

// hvn_overlay.hip -- the overlay writer of tile mode (viz.visualize_instances_dict: closed contour polylines in the instance's colour,
// optional centroid dots) rasterised on the device, bit-equal to the host writer (viz.draw_contour / viz.draw_centroid_dot).
//
// The host draws primitive after primitive and later writes win: contour of instance 0, dot of instance 0, contour of instance 1, ...
// Here that order is a KEY per primitive -- 2 * slot + 1 for a slot's contour, 2 * slot + 2 for its dot, slot = image * slots + j --
// and an int32 owner map per pixel that takes the LARGEST key stamped on it (integer atomicMax: order-independent, the same bits
// run to run, no float atomics).  A pixel with no key keeps the image.
//
//   ov_mark_contours  one wave per slot, one lane per contour point k of the slot (64 at a time): the segment from point k to the
//                     slot's next point (the last closes to the first), pixels exactly as viz._segment_pixels, each stamped with the
//                     thickness square and clipped pixel by pixel.  A slot reads only its own offs pair, so any offs array is well
//                     defined: a reversed range or one that leaves [0, n_pts] draws nothing and is counted in status.
//   ov_mark_dots      one lane per (slot, pixel of the disc's bounding square): dx^2 + dy^2 <= r^2 around the int32 centre, clipped.
//   ov_paint          one pass over the pixels, four per lane: overlay = owner ? colour_of(owner) : image (in place allowed).
//
// The step loop of a segment is bounded by the IMAGE, not by the segment: along the major axis the host formula yields exactly
// p0 +- i (|d| = n there, and the error of n * (i / n) is far below the 0.5 that floor() leaves), so the steps whose stamp can touch
// the image are an integer range of at most max(h, w) + thickness - 1 values; a vertex at +-2^30 costs nothing and cannot hang a lane.
// Every loop is bounded; nothing is allocated or synchronised; the owner map lives in the caller's workspace, cleared on the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_error.h"   // include/hvn.h and hvn_fail

#define OV_T 256
#define OV_WAVES (OV_T / 64)
#define OV_PX 4  // pixels per lane of the paint pass

static size_t ov_align(size_t x) { return (x + 255) & ~(size_t)255; }

// 1 = the slot's range lies in [0, n_pts] and is not reversed
__device__ __forceinline__ bool ov_range_ok(int64_t o0, int64_t o1, int64_t n_pts) { return o0 >= 0 && o0 <= o1 && o1 <= n_pts; }

// the segment walk is plain integer / double code, compiled for the host too so that it can be checked against viz._segment_pixels
// without a device
#define OV_HD __host__ __device__ __forceinline__

// one coordinate of step i of n: floor(double(p0) + double(d) * (double(i) / double(n)) + 0.5), three separately rounded operations
// (the library is built with -ffp-contract=off; the device code names the roundings all the same)
OV_HD long long ov_coord(int p0, long long d, long long i, long long n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const double t = __ddiv_rn((double)i, (double)n);
    return (long long)floor(__dadd_rn(__dadd_rn((double)p0, __dmul_rn((double)d, t)), 0.5));
#else
    const double t = (double)i / (double)n;
    volatile double m = (double)d * t;
    volatile double a = (double)p0 + m;
    return (long long)floor(a + 0.5);
#endif
}

// stamps every pixel of the segment p0 -> p1 (both inclusive) that lies in [0, w) x [0, h): put(x, y) once per (step, offset)
template <class Put>
OV_HD void ov_segment(int2 p0, int2 p1, int h, int w, int lo, int hi, Put put)
{
    const long long dx = (long long)p1.x - p0.x, dy = (long long)p1.y - p0.y;
    const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const long long n = ax > ay ? ax : ay;
    // steps whose major coordinate m = p0 +- i lies in [-hi, size - 1 - lo]: only they can stamp a pixel of the image
    const bool xmaj = ax >= ay;
    const long long m0 = xmaj ? p0.x : p0.y, size = xmaj ? w : h;
    const bool up = (xmaj ? dx : dy) >= 0;
    long long i0 = up ? -hi - m0 : m0 - (size - 1 - lo);
    long long i1 = up ? size - 1 - lo - m0 : m0 + hi;
    if (i0 < 0) i0 = 0;
    if (i1 > n) i1 = n;
    if (i1 - i0 > size - 1 - lo + hi) i1 = i0 + (size - 1 - lo + hi);  // never true: the bound, in the loop's own terms
    for (long long i = i0; i <= i1; ++i) {
        const long long x = n ? ov_coord(p0.x, dx, i, n) : p0.x, y = n ? ov_coord(p0.y, dy, i, n) : p0.y;
        for (int sy = lo; sy <= hi; ++sy)
            for (int sx = lo; sx <= hi; ++sx) {
                const long long xx = x + sx, yy = y + sy;
                if (xx >= 0 && xx < w && yy >= 0 && yy < h) put((int)xx, (int)yy);
            }
    }
}

__global__ __launch_bounds__(OV_T) void ov_mark_contours(const int2 *__restrict__ pts, int64_t n_pts, const int64_t *__restrict__ offs,
                                                         int slots, long M, const uint8_t *__restrict__ rgba, int h, int w, int lo, int hi,
                                                         int32_t *__restrict__ owner, int32_t *__restrict__ status)
{
    const long g = (long)blockIdx.x * OV_WAVES + (threadIdx.x >> 6);  // slot, uniform over the wave
    const int lane = threadIdx.x & 63;
    if (g >= M) return;
    const int64_t o0 = offs[g], o1 = offs[g + 1];
    if (!ov_range_ok(o0, o1, n_pts)) {
        if (lane == 0) {
            atomicAdd(status + 0, 1);
            atomicMin((unsigned *)status + 1, (unsigned)g);  // starts at 0xffffffff = -1: no bad slot
        }
        return;
    }
    if (!rgba[g * 4 + 3]) return;
    int32_t *own = owner + (g / slots) * ((long)h * w);
    const int key = (int)(2 * g + 1);
    for (int64_t k = o0 + lane; k < o1; k += 64)  // at most ceil(n_pts / 64) rounds
        ov_segment(pts[k], pts[k + 1 < o1 ? k + 1 : o0], h, w, lo, hi, [=](int x, int y) { atomicMax(own + (long)y * w + x, key); });
}

// blockIdx.y = pixel of the disc's bounding square, lanes along the slots
__global__ __launch_bounds__(OV_T) void ov_mark_dots(const int2 *__restrict__ centres, int64_t n_pts, const int64_t *__restrict__ offs, int slots,
                                                     long M, const uint8_t *__restrict__ rgba, int h, int w, int r,
                                                     int32_t *__restrict__ owner)
{
    const long g = (long)blockIdx.x * OV_T + threadIdx.x;
    if (g >= M) return;
    const int side = 2 * r + 1;
    const int dy = (int)blockIdx.y / side - r, dx = (int)blockIdx.y % side - r;
    if (dx * dx + dy * dy > r * r) return;
    if (!rgba[g * 4 + 3] || !ov_range_ok(offs[g], offs[g + 1], n_pts)) return;
    const int2 c = centres[g];
    const long long xx = (long long)c.x + dx, yy = (long long)c.y + dy;
    if (xx >= 0 && xx < w && yy >= 0 && yy < h) atomicMax(owner + (g / slots) * ((long)h * w) + yy * w + xx, (int)(2 * g + 2));
}

// image and overlay may be the same buffer: a lane reads its own pixels before it writes them
__global__ __launch_bounds__(OV_T) void ov_paint(const uint8_t *image, uint8_t *overlay, long P, const int32_t *__restrict__ owner,
                                                 const uint8_t *__restrict__ rgba, uchar4 dot)
{
    const long p0 = ((long)blockIdx.x * OV_T + threadIdx.x) * OV_PX;
    if (p0 >= P) return;
    if (p0 + OV_PX <= P) {  // 16 bytes of keys, 12 bytes of pixels (both pointers are 4-byte aligned, p0 is a multiple of 4)
        const int4 k4 = *(const int4 *)(owner + p0);
        const int key[OV_PX] = {k4.x, k4.y, k4.z, k4.w};
        uint32_t v[3];
        uint8_t px[3 * OV_PX];
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = ((const uint32_t *)(image + 3 * p0))[j];
#pragma unroll
        for (int j = 0; j < 3 * OV_PX; ++j) px[j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
#pragma unroll
        for (int q = 0; q < OV_PX; ++q) {
            if (key[q] <= 0) continue;
            const uchar4 c = (key[q] & 1) ? *(const uchar4 *)(rgba + 4L * ((key[q] - 1) >> 1)) : dot;
            px[3 * q] = c.x;
            px[3 * q + 1] = c.y;
            px[3 * q + 2] = c.z;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
            ((uint32_t *)(overlay + 3 * p0))[j] = (uint32_t)px[4 * j] | (uint32_t)px[4 * j + 1] << 8 | (uint32_t)px[4 * j + 2] << 16 | (uint32_t)px[4 * j + 3] << 24;
        return;
    }
    for (long p = p0; p < P; ++p) {  // ragged tail: at most three pixels, byte by byte
        const int key = owner[p];
        uchar4 c = {image[3 * p], image[3 * p + 1], image[3 * p + 2], 0};
        if (key > 0) c = (key & 1) ? *(const uchar4 *)(rgba + 4L * ((key - 1) >> 1)) : dot;
        overlay[3 * p] = c.x;
        overlay[3 * p + 1] = c.y;
        overlay[3 * p + 2] = c.z;
    }
}

extern "C" {

size_t hvn_overlay_workspace_bytes(int n, int h, int w)
{
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return ov_align((size_t)n * h * w * sizeof(int32_t));
}

int hvn_draw_overlay(const uint8_t *image, uint8_t *overlay, int n, int h, int w, const int32_t *pts, int64_t n_pts, const int64_t *offs,
                     int slots, const uint8_t *rgba, const int32_t *centres, int thickness, int dot_radius, const uint8_t dot_rgb[3],
                     int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!image || !overlay || !offs || !rgba || !status || !dot_rgb) return hvn_fail(HVN_E_ARG, "draw_overlay: null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || slots <= 0 || n_pts < 0) return hvn_fail(HVN_E_ARG, "draw_overlay: n, h, w or slots < 1, or n_pts < 0 (slots = %d)", slots);
    if (n_pts > 0 && (!pts || ((uintptr_t)pts & 7))) return hvn_fail(HVN_E_ARG, "draw_overlay: pts NULL or not 8-byte aligned");  // points are read as (x, y) pairs
    if (((uintptr_t)image & 3) || ((uintptr_t)overlay & 3) || ((uintptr_t)rgba & 3) || ((uintptr_t)centres & 7))
        return hvn_fail(HVN_E_ARG, "draw_overlay: image, overlay and rgba must be 4-byte, centres 8-byte aligned");
    if ((long)h * w >= (1L << 31) || (long)n * h * w >= (1L << 40)) return hvn_fail(HVN_E_ARG, "draw_overlay: h * w >= 2^31 or n * h * w >= 2^40 (h = %d)", h);
    if (thickness < 1 || thickness > 7 || dot_radius < 0 || dot_radius > 15)
        return hvn_fail(HVN_E_SIZE, "draw_overlay: thickness %d outside [1, 7] or dot_radius %d outside [0, 15]", thickness, dot_radius);
    const long M = (long)n * slots;
    if (M >= (1L << 30) - 1) return hvn_fail(HVN_E_SIZE, "draw_overlay: n * slots >= 2^30 - 1 (%ld slots)", M);  // 2 * slot + 2 is an int32 key
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < hvn_overlay_workspace_bytes(n, h, w))
        return hvn_fail(HVN_E_SIZE, "draw_overlay: workspace NULL, not 16-byte aligned or smaller than hvn_overlay_workspace_bytes (%zu bytes given)", workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    int32_t *owner = (int32_t *)workspace;
    const long P = (long)n * h * w;
    if (hipMemsetAsync(owner, 0, (size_t)P * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(status, 0, 4 * sizeof(int32_t), s) != hipSuccess ||
        hipMemsetAsync(status + 1, 0xff, sizeof(int32_t), s) != hipSuccess)
        return hvn_fail(HVN_E_LAUNCH, "draw_overlay: hipMemsetAsync failed");
    const int lo = -((thickness - 1) / 2), hi = thickness / 2;
    hipLaunchKernelGGL(ov_mark_contours, dim3((unsigned)((M + OV_WAVES - 1) / OV_WAVES)), dim3(OV_T), 0, s, (const int2 *)pts, n_pts, offs, slots,
                       M, rgba, h, w, lo, hi, owner, status);
    if (centres) {
        const int side = 2 * dot_radius + 1;
        hipLaunchKernelGGL(ov_mark_dots, dim3((unsigned)((M + OV_T - 1) / OV_T), (unsigned)(side * side)), dim3(OV_T), 0, s,
                           (const int2 *)centres, n_pts, offs, slots, M, rgba, h, w, dot_radius, owner);
    }
    const long lanes = (P + OV_PX - 1) / OV_PX;
    hipLaunchKernelGGL(ov_paint, dim3((unsigned)((lanes + OV_T - 1) / OV_T)), dim3(OV_T), 0, s, image, overlay, P, (const int32_t *)owner, rgba,
                       uchar4{dot_rgb[0], dot_rgb[1], dot_rgb[2], 0});
    return hvn_launched("draw_overlay");
}

}  // extern "C"

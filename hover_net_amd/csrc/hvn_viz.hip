// hvn_viz.hip -- the picture of the run loop (models/hovernet/run_desc.py:201-256 viz_step_output) on the device, bit-equal to
// hover_net_amd/viz.py: per selected sample one block of two rows of tiles (truths above predictions), each row being the image's
// centre crop, then NP (0..1), H and V (-1..1) and, with types, TP (0..nr_types), coloured through a 256-entry RGB table.
//
//   vz_strip   grid (items, n_sel).  A block of the strip is one contiguous run of 2h * ncol * w pixels, three bytes each.  A lane
//              takes four consecutive pixels of it and stores them as three dwords; the run starts `head` = (byte offset & 3) pixels
//              late so that every such store is dword-aligned whatever h, w and the block are, and the item after the last group
//              writes the head and the up to three pixels left at the end byte by byte.  The table is staged in LDS once per
//              workgroup.  A colourised pixel is the host's float32 sequence: clamp, subtract vmin, one correctly rounded divide by
//              float32(vmax - vmin), times 256, truncate, 256 -> 255; NaN -> (0, 0, 0).
// A pair of `sel` whose sample or block is out of range draws nothing; bytes outside the named blocks are never written.  Pixel
// indices inside a block are int32 (the caller bounds 2h * ncol * w by 2^30); byte offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define VZ_T 256

struct VzArgs {
    const uint8_t *img;
    const float *pred;
    const int32_t *np_map;
    const float *hv_map;
    const int32_t *tp_map;
    const int32_t *sel;
    const uint8_t *lut;
    uint8_t *out;
    int n, ih, iw, c, h, w, ncol, n_blocks, oy, ox;
    float tp_max;
};

// the table index of a value, or -1 for NaN
__device__ __forceinline__ int vz_index(float v, float vmin, float vmax)
{
    if (v != v) return -1;
    v = v > vmax ? vmax : v;
    v = v < vmin ? vmin : v;
    const float t = __fdiv_rn(v - vmin, vmax - vmin) * 256.0f;
    const int k = (int)t;
    return k > 255 ? 255 : k;
}

// the three bytes of pixel p of sample s's block, as r | g << 8 | b << 16
__device__ __forceinline__ uint32_t vz_pixel(const VzArgs &a, const uint8_t *lut, int s, int p)
{
    const int W = a.ncol * a.w;
    const int row = p / W, xx = p - row * W;
    const int col = xx / a.w, x = xx - col * a.w;
    const int pr = row >= a.h, y = pr ? row - a.h : row;
    if (col == 0) {
        const uint8_t *q = a.img + (((long)s * a.ih + (a.oy + y)) * a.iw + (a.ox + x)) * 3;
        return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    }
    const long m = ((long)s * a.h + y) * a.w + x;
    float v, vmin = -1.0f, vmax = 1.0f;
    if (col == 1) {
        vmin = 0.0f;
        v = pr ? a.pred[m * a.c + (a.c - 3)] : (float)a.np_map[m];
    } else if (col < 4) {
        v = pr ? a.pred[m * a.c + (a.c - 3) + (col - 1)] : a.hv_map[m * 2 + (col - 2)];
    } else {
        vmin = 0.0f;
        vmax = a.tp_max;
        v = pr ? a.pred[m * a.c] : (float)a.tp_map[m];
    }
    const int k = vz_index(v, vmin, vmax);
    if (k < 0) return 0u;
    return (uint32_t)lut[3 * k] | (uint32_t)lut[3 * k + 1] << 8 | (uint32_t)lut[3 * k + 2] << 16;
}

__global__ __launch_bounds__(VZ_T) void vz_strip(const VzArgs a)
{
    __shared__ uint8_t lut[768];
    for (int i = threadIdx.x; i < 768; i += VZ_T) lut[i] = a.lut[i];
    __syncthreads();
    const int s = a.sel[2 * blockIdx.y], b = a.sel[2 * blockIdx.y + 1];
    if (s < 0 || s >= a.n || b < 0 || b >= a.n_blocks) return;  // uniform over the workgroup
    const int P = 2 * a.h * a.ncol * a.w;
    const long base = (long)b * P * 3;                            // byte offset of the block in out
    uint8_t *dst = a.out + base;
    const int head = (int)(((uintptr_t)dst) & 3);                 // dst + 3 * head is dword-aligned: 3k = -k (mod 4)
    const int G = P > head ? (P - head) >> 2 : 0;
    const int g = blockIdx.x * VZ_T + threadIdx.x;
    if (g < G) {
        const int p = head + 4 * g;
        const uint32_t p0 = vz_pixel(a, lut, s, p), p1 = vz_pixel(a, lut, s, p + 1), p2 = vz_pixel(a, lut, s, p + 2), p3 = vz_pixel(a, lut, s, p + 3);
        uint32_t *d = (uint32_t *)(dst + (long)p * 3);
        d[0] = p0 | p1 << 24;
        d[1] = p1 >> 8 | p2 << 16;
        d[2] = p2 >> 16 | p3 << 8;
    } else if (g == G) {
        // the scalar ends: [0, head) and [head + 4G, P), each of at most three pixels
        for (int k = 0; k < 6; ++k) {
            const int p = k < 3 ? k : head + 4 * G + (k - 3);
            if (p >= P || (k < 3 && p >= head)) continue;
            const uint32_t v = vz_pixel(a, lut, s, p);
            dst[(long)p * 3] = (uint8_t)v;
            dst[(long)p * 3 + 1] = (uint8_t)(v >> 8);
            dst[(long)p * 3 + 2] = (uint8_t)(v >> 16);
        }
    }
}

int hvn_launch_viz_strip(const uint8_t *img, int n, int ih, int iw, const float *pred, int c, const int32_t *np_map, const float *hv_map,
                         const int32_t *tp_map, int h, int w, int nr_types, const int32_t *sel, int n_sel, const uint8_t *lut, uint8_t *out,
                         int n_blocks, hipStream_t stream)
{
    VzArgs a;
    a.img = img, a.pred = pred, a.np_map = np_map, a.hv_map = hv_map, a.tp_map = tp_map, a.sel = sel, a.lut = lut, a.out = out;
    a.n = n, a.ih = ih, a.iw = iw, a.c = c, a.h = h, a.w = w, a.n_blocks = n_blocks;
    a.ncol = nr_types > 0 && tp_map ? 5 : 4;
    a.oy = (ih - h) / 2, a.ox = (iw - w) / 2;                     // int((ih - h) * 0.5) for ih >= h
    a.tp_max = (float)nr_types;
    const long P = 2L * h * a.ncol * w;
    const long items = (P >> 2) + 1;                              // groups of four pixels, and the item of the scalar ends
    hipLaunchKernelGGL(vz_strip, dim3((unsigned)((items + VZ_T - 1) / VZ_T), (unsigned)n_sel), dim3(VZ_T), 0, stream, a);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

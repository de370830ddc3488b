// hvn_resample.hip -- one window of a slide resampled to the processing magnification on the device, bit-equal to
// hover_net_amd/resample.py (resize_window_host): OpenCV's scalar 8-bit fixed-point resize restated, 11 coefficient bits.
//
// Integer arithmetic only.  The float32 coefficient work is done on the host (resample.axis_table) and arrives as tables for the
// window's columns and rows: ofs (int32, in FULL-source coordinates) and coef (int16 [.][taps], taps = 4 cubic | 2 linear).  Tap k
// of an entry reads full-source index clamp(ofs + k - (taps == 4), 0, full - 1), which is then translated by the origin of the
// uploaded source box -- and clamped to the box once more, so that no table, however wrong, makes a launch read outside src (the
// caller checks that the box holds every tap: with a right table the second clamp never acts).
//
//   rs_resize   one workgroup per tile of RS_TH x RS_TW output pixels.  The rows of a tile are taken in groups whose source rows fit
//               RS_ROWS rows of LDS (one group for every factor >= 1/2; more for smaller factors).  Per group:
//                 horizontal pass: lane e < 3 * tile width owns output byte column e (pixel e / 3, channel e % 3) with its taps' byte
//                   offsets and coefficients in registers, and walks the group's source rows: hor[row][e] = sum src * coef, an
//                   exact int32, once per source row -- never per output row;
//                 vertical pass: one wave per output row, one lane per ALIGNED dword of the row's bytes: four bytes from LDS
//                   (cubic: (sum hor * coef + 2^21) >> 22 clamped; linear: the two-term form below), stored as one dword, or byte
//                   by byte in the head / tail dword of a row that does not start or end on a dword (rows are 3 * w bytes).
// Row bases are 64-bit; offsets within a row are 32-bit (the launcher bounds 3 * width).  Every loop is bounded by the tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define RS_T 256
#define RS_TH 16             // output rows per tile: about 11 source rows for f = 2
#define RS_TW 80             // output pixels per tile row = 240 bytes: 60 dwords, 61 when the row starts off a dword -- one wave
#define RS_NE (3 * RS_TW)
#define RS_ROWS 36           // source rows of the horizontal pass in LDS: 36 * 240 * 4 = 34 560 B (4 workgroups per CU); holds
                             // the 33 rows of a 16-row tile at f = 1/2

// window-local index of tap k: clamped against the full axis, translated, clamped against the box
template <int TAPS>
__device__ __forceinline__ int rs_tap(int ofs, int k, int full, int origin, int n)
{
    long long i = (long long)ofs + k - (TAPS == 4 ? 1 : 0);
    i = i < 0 ? 0 : (i > full - 1 ? full - 1 : i);
    i -= origin;
    return (int)(i < 0 ? 0 : (i > n - 1 ? n - 1 : i));
}

template <int TAPS>
__global__ __launch_bounds__(RS_T) void rs_resize(const uint8_t *__restrict__ src, int src_h, int src_w, int64_t pitch, int src_y0, int src_x0,
                                                  int full_h, int full_w, const int32_t *__restrict__ xofs, const int16_t *__restrict__ xcoef,
                                                  const int32_t *__restrict__ yofs, const int16_t *__restrict__ ycoef, uint8_t *__restrict__ dst,
                                                  int dst_h, int dst_w)
{
    __shared__ int32_t hor[RS_ROWS][RS_NE];
    const int t = threadIdx.x;
    const int tx0 = blockIdx.x * RS_TW, ty0 = blockIdx.y * RS_TH;
    const int tw = dst_w - tx0 < RS_TW ? dst_w - tx0 : RS_TW;
    const int ty1 = ty0 + RS_TH < dst_h ? ty0 + RS_TH : dst_h;
    const int ne = 3 * tw;  // bytes of a tile row

    int sx[TAPS], cx[TAPS];  // this lane's column: byte offsets of its taps in a source row, coefficients
    if (t < ne) {
        const int col = tx0 + t / 3, ch = t % 3;
        const int s = xofs[col];
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            sx[k] = 3 * rs_tap<TAPS>(s, k, full_w, src_x0, src_w) + ch;
            cx[k] = xcoef[col * TAPS + k];
        }
    }
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;

    for (int r = ty0; r < ty1;) {
        // the group [r, e): as many rows as keep the source rows [lo, hi] within RS_ROWS (one row needs at most TAPS)
        const int lo = rs_tap<TAPS>(yofs[r], 0, full_h, src_y0, src_h);
        int hi = rs_tap<TAPS>(yofs[r], TAPS - 1, full_h, src_y0, src_h);
        int e = r + 1;
        for (; e < ty1; ++e) {
            const int h2 = rs_tap<TAPS>(yofs[e], TAPS - 1, full_h, src_y0, src_h);
            if (h2 - lo + 1 > RS_ROWS) break;
            hi = h2 > hi ? h2 : hi;
        }
        const int nrows = hi - lo + 1;  // 1 .. RS_ROWS (tap TAPS - 1 >= tap 0: the clamps are monotone)

        if (t < ne) {
            const uint8_t *p = src + (int64_t)lo * pitch;
#pragma unroll 4
            for (int j = 0; j < nrows; ++j, p += pitch) {
                int acc = 0;
#pragma unroll
                for (int k = 0; k < TAPS; ++k) acc += (int)p[sx[k]] * cx[k];
                hor[j][t] = acc;
            }
        }
        __syncthreads();

        for (int y = r + wave; y < e; y += RS_T / 64) {
            int ry[TAPS], cy[TAPS];
            const int s = yofs[y];
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                const int j = rs_tap<TAPS>(s, k, full_h, src_y0, src_h) - lo;  // in [0, nrows) for a monotone table; bounded for any
                ry[k] = j < 0 ? 0 : (j > nrows - 1 ? nrows - 1 : j);
                cy[k] = ycoef[y * TAPS + k];
            }
            uint8_t *a0 = dst + (int64_t)y * (3 * (int64_t)dst_w) + 3 * tx0;  // first byte of the tile's part of row y
            const int mis = (int)((uintptr_t)a0 & 3);
            const int ndw = (mis + ne + 3) >> 2;                               // aligned dwords that hold a byte of it: <= 61
            if (lane < ndw) {
                const int e0 = 4 * lane - mis;                                 // tile byte of this dword's first byte
                uint32_t px[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    int el = e0 + b;
                    el = el < 0 ? 0 : (el > ne - 1 ? ne - 1 : el);
                    int v;
                    if (TAPS == 4) {
                        v = 0;
#pragma unroll
                        for (int k = 0; k < TAPS; ++k) v += hor[ry[k]][el] * cy[k];
                        v = (v + (1 << 21)) >> 22;
                        v = v < 0 ? 0 : (v > 255 ? 255 : v);
                    } else {
                        v = (((cy[0] * (hor[ry[0]][el] >> 4)) >> 16) + ((cy[1] * (hor[ry[1]][el] >> 4)) >> 16) + 2) >> 2;
                    }
                    px[b] = (uint32_t)v & 0xffu;
                }
                if (e0 >= 0 && e0 + 4 <= ne) {
                    *(uint32_t *)(a0 + e0) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (e0 + b >= 0 && e0 + b < ne) a0[e0 + b] = (uint8_t)px[b];
                }
            }
        }
        __syncthreads();  // the next group overwrites hor
        r = e;
    }
}

int hvn_launch_resize_window(const uint8_t *src, int src_h, int src_w, int64_t src_pitch, int src_y0, int src_x0, int full_h, int full_w,
                             const int32_t *xofs, const int16_t *xcoef, const int32_t *yofs, const int16_t *ycoef, int taps, uint8_t *dst,
                             int dst_h, int dst_w, hipStream_t stream)
{
    const dim3 grid((unsigned)((dst_w + RS_TW - 1) / RS_TW), (unsigned)((dst_h + RS_TH - 1) / RS_TH));
    if (grid.y > 65535u) return HVN_E_SIZE;
    if (taps == 4)
        hipLaunchKernelGGL(rs_resize<4>, grid, dim3(RS_T), 0, stream, src, src_h, src_w, src_pitch, src_y0, src_x0, full_h, full_w, xofs, xcoef,
                           yofs, ycoef, dst, dst_h, dst_w);
    else
        hipLaunchKernelGGL(rs_resize<2>, grid, dim3(RS_T), 0, stream, src, src_h, src_w, src_pitch, src_y0, src_x0, full_h, full_w, xofs, xcoef,
                           yofs, ycoef, dst, dst_h, dst_w);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

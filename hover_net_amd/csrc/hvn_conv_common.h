// hvn_conv_common.h -- what the matrix-pipe convolution kernels share (hvn_conv*.hip, hvn_wgrad_x3.hip, the bf16 helpers also with
// hvn_net_ops.hip): vector types, buffer / LDS-DMA wrappers, the bf16 split and pack helpers, and the host side of the implicit-GEMM
// launchers.  Every device helper is force-inlined and compiles to the instructions its per-file copies gave (tools/isa_diff.py,
// profiles/conv_common_isa_diff.txt).
// NOT here: the epilogue of hvn_conv_igemm_{x3, x3g, bf16, bf16g} (four copies that differ in element size and in x3g's two halves).  As one
// force-inlined template it kept registers and occupancy but never compiled to the same instructions as the copies -- LLVM orders phis,
// sinks selects and folds the tile addressing differently across the function boundary -- so each kernel keeps its own, and a change
// to the epilogue still has to be made in all four.  The same holds for the tile mapping, A-row decode and tap walk of the main loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: HIP's float4 struct copies lower to memcpy -> scratch
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void *lds_ptr_t;

// a byte offset at or beyond a descriptor's num_records (2^31 - 1): the load returns zeros, the store is dropped
#define HVN_OOB 0x80000000u

// raw buffer descriptor over everything from `ptr` on: address = ptr + soffset (SGPR) + voffset (VGPR)
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t hvn_buf(const void *ptr)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)ptr, 0, 0x7fffffff, 0x00020000);
}
static __device__ __forceinline__ f32x4 hvn_buf_load16(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
static __device__ __forceinline__ void hvn_buf_store16(f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, soff, 0);
}
// One LDS-DMA instruction: 64 lanes x 16 bytes from per-lane global offsets (voff + the wave-uniform soff; beyond num_records: zeros)
// to the 1 KiB at the wave-uniform LDS address `dst`, lane-linear.  (The builtin exists in the device pass only; hipcc's host pass
// silently drops a kernel whose body names it, and with it the kernel's launch stub.)
static __device__ __forceinline__ void hvn_dma16(__amdgpu_buffer_rsrc_t rsrc, lds_ptr_t dst, unsigned voff, int soff)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, 16, voff, soff, 0, 0);
#endif
}

// ---- bf16 ------------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ float hvn_bf16_lo(uint32_t v) { return __builtin_bit_cast(float, v << 16); }
static __device__ __forceinline__ float hvn_bf16_hi(uint32_t v) { return __builtin_bit_cast(float, v & 0xffff0000u); }
static __device__ __forceinline__ uint32_t hvn_bf16_pack(float a, float b)      // RNE (v_cvt_pk_bf16_f32)
{
    bf16x2 h = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, h);
}
// x = h + m + l exactly (RNE conversions; x - h and x - h - m are exact in fp32) for 2^-110 <= |x| < 3.38e38 and for 0: below, the low
// planes underflow bf16's denormal grid (absolute error < 2^-133); within 0.3 % of FLT_MAX h rounds to infinity -- a value no fp32
// accumulation of this network survives either (tests/test_x3_arithmetic.py pins both limits)
static __device__ __forceinline__ void hvn_split3(float x, __bf16 &h, __bf16 &m, __bf16 &l)
{
    h = (__bf16)x;
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}
// hvn_split3 over the 8 k-values a lane feeds one MFMA with
static __device__ __forceinline__ void hvn_split3x8(const f32x4 a, const f32x4 b, bf16x8 &h, bf16x8 &m, bf16x8 &l)
{
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 hh = (__bf16)x[e];
        const float r = x[e] - (float)hh;
        const __bf16 mm = (__bf16)r;
        h[e] = hh;
        m[e] = mm;
        l[e] = (__bf16)(r - (float)mm);
    }
}

// ---- host side of the launchers --------------------------------------------------------------------------------------------------
// The kernels index pixels with 32 bits and address x, x2 (and, with `out`, y and res) by 32-bit byte offsets from the sample of a
// tile's first row; 2^31 and beyond is the descriptors' "zeros" range.  A tile of bm rows reaches (HoWo + bm - 2) / HoWo samples ahead
// -- ONE when a sample holds a tile's worth of pixels, FOUR for a Winograd-domain product with 36 tiles per sample: with the arena's
// 0.5 GB sample stride that is beyond the reach, and rows would silently read zeros (round 4: the F(6x6,3x3) product of d3 in 'fast'
// mode).  Refused here instead.  m_margin: what the kernel adds to a pixel index at most (tile rows, rounded up by the launcher).
static inline bool hvn_conv_reach_ok(const ConvArgs &a, int bm, int elem_bytes, long m_margin, bool x2, bool out)
{
    if (a.M <= 0 || a.M >= (1L << 31) - m_margin) return false;
    const long howo = (long)a.Ho * a.Wo;
    if (howo <= 0) return false;
    const long ahead = (howo + bm - 2) / howo;
    const long span = ahead * a.xsn + (long)(a.H + a.KH) * a.xsy + (long)(a.W + a.KW) * a.xsx;
    if (span < 0 || span * elem_bytes >= (1L << 31)) return false;
    if (x2 && a.x2 && (ahead * a.x2sn + (long)a.H * a.x2sy * a.stride2) * elem_bytes >= (1L << 31)) return false;
    if (out) {
        if ((ahead * a.ysn + (long)(a.Ho + 1) * a.ysy + (long)a.Wo * a.ysx) * elem_bytes >= (1L << 31)) return false;
        if (a.res && (ahead * a.rsn + (long)(a.Ho + 1) * a.rsy + (long)a.Wo * a.rsx) * elem_bytes >= (1L << 31)) return false;
    }
    return true;
}
// "padded" = some tap of some output pixel falls outside the input window
static inline bool hvn_conv_padded(const ConvArgs &a)
{
    return a.pad_t > 0 || a.pad_l > 0 || (a.Ho - 1) * a.stride - a.pad_t + a.KH > a.H || (a.Wo - 1) * a.stride - a.pad_l + a.KW > a.W;
}
// tiles, the XCD-aware 1-D grid (8 x ceil(m_tiles / 8) x n_tiles; blockIdx.y = problem of a batched launch), the kernel's LDS attribute, launch
template <typename Kern>
static inline int hvn_conv_launch(Kern kern, ConvArgs p, int bm, int bn, int threads, size_t lds, int attr_lds,
                                  std::atomic<unsigned long long> &attr_done, hipStream_t stream)
{
    p.m_tiles = (p.M + bm - 1) / bm;
    p.n_tiles = (p.Cout + bn - 1) / bn;
    if (hvn_max_lds_once((const void *)kern, attr_lds, attr_done)) return HVN_E_LAUNCH;
    const long groups = (p.m_tiles + 7) / 8;
    const long grid = groups * 8 * p.n_tiles;
    if (grid <= 0 || grid > 0x7fffffffL) return HVN_E_ARG;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid, p.nbatch > 1 ? p.nbatch : 1), dim3(threads), lds, stream, p);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

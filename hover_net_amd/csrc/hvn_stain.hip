// hvn_stain.hip -- Macenko stain normalisation on the device (hover_net_amd/stain.py is the definition).
//
// The fit is a function of the multiset of RGB triples, and the device's share of it is that multiset in exact integers:
//   st_hist      adds the pixels of uint8 [rows][W][3] (optionally only those whose mask byte is non-zero) to 2^24 uint32 bins, bin =
//                r << 16 | g << 8 | b.  Equal keys are merged on chip before anything reaches memory: a lane carries (key, count) of
//                its current run across its loop (a run of background costs it nothing), and a finished run goes into a hash table of
//                ST_SLOTS (key, count) pairs in LDS -- one LDS atomic; lanes and waves of the workgroup that hold the same key meet
//                there.  A run that finds no slot within ST_PROBES probes goes to its bin directly.  At the end every occupied slot is
//                one global atomic.  Integer atomics only: the table is a function of the inputs alone.  Four pixels per lane as three
//                dwords where the row is dword-aligned; a byte form otherwise and for a row's last pixels.
//   st_count / st_scan / st_write   the non-empty bins as (key, count) pairs in ascending key order: counts per block of 4096 bins, an
//                exclusive scan of the 4096 block counts by one workgroup, then every block writes its pairs at its offset (a thread
//                owns 16 consecutive bins, so the order inside a block is the key order).  The layout is a function of the bins
//                alone.  Pairs past the list's capacity are not written; the status carries the true number.  With `clear` every
//                non-empty bin read is stored back as 0.
//   st_apply     y = the table form of Io * exp(-M . od): x = ((Io * T[c][0][r]) * T[c][1][g]) * T[c][2][b] in float64, in that order,
//                out = (uint8) (x < 255 ? x : 255) (NaN and +inf give 255).  The nine 256-entry tables sit in LDS (18 KB; Io is folded
//                into the first of each channel -- the same IEEE product).  The kernel only multiplies: no contraction or fast-math
//                setting can change a bit.  A thread reads its four pixels before it writes them, so y may be x itself.
// Rows: the launchers fold dense samples and dense rows into longer rows, so that a dense image is ONE row of batch * h * w pixels;
// row r of the folded grid lives at base + (r / R0) * sn + (r % R0) * sy.  Every index is bounded by the extents the caller validated
// (hvn_api.hip); byte offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvn_kernels.h"

#define ST_T 256
#define ST_SLOTS 2048        // LDS hash table of st_hist: 16 KB of (key, count)
#define ST_SLOT_BITS 11
#define ST_PROBES 4
#define ST_EMPTY 0xFFFFFFFFu // no key: keys are below 2^24
#define ST_BLOCKS 4096       // st_count / st_write: blocks of 4096 bins
#define ST_IO 240.0

struct StRows {
    long rows, R0, W;        // folded rows, rows per sample, pixels per row
    long sn, sy;             // byte strides of x
    long ysn, ysy;           // byte strides of y (apply)
};

// dense samples and rows folded into longer rows; `both`: y's strides have to allow the same folding
static StRows st_fold(int N, int H, int W, long xsn, long xsy, long ysn, long ysy, bool both)
{
    StRows r;
    r.rows = (long)N * H; r.R0 = H; r.W = W;
    r.sn = xsn; r.sy = xsy; r.ysn = ysn; r.ysy = ysy;
    if (xsy == 3L * W && (!both || ysy == 3L * W)) {                 // dense rows: a sample is one row
        r.rows = N; r.R0 = 1; r.W = (long)H * W;
        if (xsn == xsy * H && (!both || ysn == ysy * H)) {           // dense samples: the image is one row
            r.rows = 1; r.W = (long)N * H * W;
        }
    }
    return r;
}

static dim3 st_grid(const StRows &r)
{
    const long G = (r.W + 3) / 4;
    const long gx = (G + ST_T - 1) / ST_T < 2048 ? (G + ST_T - 1) / ST_T : 2048;
    long gy = 2048 / gx < 1 ? 1 : 2048 / gx;
    if (gy > r.rows) gy = r.rows;
    return dim3((unsigned)gx, (unsigned)gy, 1);
}

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void st_add(uint32_t *keys, uint32_t *cnts, uint32_t *__restrict__ bins, uint32_t key, uint32_t n)
{
    uint32_t s = (key * 2654435761u) >> (32 - ST_SLOT_BITS);
    for (int p = 0; p < ST_PROBES; ++p) {
        uint32_t old = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // a slot's key is written once
        if (old == ST_EMPTY) old = atomicCAS(keys + s, ST_EMPTY, key);
        if (old == ST_EMPTY || old == key) {
            atomicAdd(cnts + s, n);
            return;
        }
        s = (s + 1) & (ST_SLOTS - 1);
    }
    atomicAdd(bins + key, n);
}

__global__ __launch_bounds__(ST_T) void st_hist(const uint8_t *__restrict__ x, const uint8_t *__restrict__ mask, uint32_t *__restrict__ bins,
                                                const StRows a)
{
    __shared__ uint32_t keys[ST_SLOTS], cnts[ST_SLOTS];
    for (int s = threadIdx.x; s < ST_SLOTS; s += ST_T) {
        keys[s] = ST_EMPTY;
        cnts[s] = 0;
    }
    __syncthreads();
    uint32_t ck = ST_EMPTY, cn = 0;     // the lane's current run
    const long G = (a.W + 3) >> 2;
    for (long r = blockIdx.y; r < a.rows; r += gridDim.y) {
        const uint8_t *__restrict__ row = x + (r / a.R0) * a.sn + (r % a.R0) * a.sy;
        const uint8_t *__restrict__ mrow = mask ? mask + r * a.W : nullptr;
        const bool vec = (((uintptr_t)row) & 3) == 0;
        for (long g = (long)blockIdx.x * ST_T + threadIdx.x; g < G; g += (long)gridDim.x * ST_T) {
            const long p0 = g << 2;
            const int np = a.W - p0 >= 4 ? 4 : (int)(a.W - p0);
            uint32_t k[4];
            if (vec && np == 4) {
                const uint32_t *src = (const uint32_t *)(row + 3 * p0);
                const uint32_t u = src[0], v = src[1], w = src[2];
                k[0] = (u & 255u) << 16 | (u & 0xFF00u) | ((u >> 16) & 255u);
                k[1] = (u >> 24) << 16 | (v & 255u) << 8 | ((v >> 8) & 255u);
                k[2] = ((v >> 16) & 255u) << 16 | (v >> 24) << 8 | (w & 255u);
                k[3] = ((w >> 8) & 255u) << 16 | ((w >> 16) & 255u) << 8 | (w >> 24);
            } else {
                for (int i = 0; i < np; ++i) {
                    const uint8_t *px = row + 3 * (p0 + i);
                    k[i] = (uint32_t)px[0] << 16 | (uint32_t)px[1] << 8 | px[2];
                }
            }
            for (int i = 0; i < np; ++i) {
                if (mrow && !mrow[p0 + i]) continue;
                if (k[i] == ck) {
                    ++cn;
                } else {
                    if (cn) st_add(keys, cnts, bins, ck, cn);
                    ck = k[i];
                    cn = 1;
                }
            }
        }
    }
    if (cn) st_add(keys, cnts, bins, ck, cn);
    __syncthreads();
    for (int s = threadIdx.x; s < ST_SLOTS; s += ST_T)
        if (keys[s] != ST_EMPTY) atomicAdd(bins + keys[s], cnts[s]);
}

int hvn_launch_stain_hist(const StainHistArgs &a, hipStream_t stream)
{
    const StRows r = st_fold(a.N, a.H, a.W, a.xsn, a.xsy, 0, 0, false);
    hipLaunchKernelGGL(st_hist, st_grid(r), dim3(ST_T), 0, stream, a.x, a.mask, a.bins, r);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

// ---------------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup's 256 threads in thread order; total = the sum of all
__device__ __forceinline__ uint32_t st_block_scan(uint32_t v, uint32_t *wave_sums, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[wv] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (int i = 0; i < ST_T / 64; ++i) {
        if (i < wv) before += wave_sums[i];
        total += wave_sums[i];
    }
    __syncthreads();
    return before + inc - v;
}

// workspace: uint64 pixel sums [ST_BLOCKS], uint32 counts [ST_BLOCKS], uint32 offsets [ST_BLOCKS]
__global__ __launch_bounds__(ST_T) void st_count(const uint32_t *__restrict__ bins, uint64_t *__restrict__ ws_sum, uint32_t *__restrict__ ws_cnt)
{
    __shared__ uint32_t c_s[ST_T / 64];
    __shared__ uint64_t p_s[ST_T / 64];
    const uint4 *src = (const uint4 *)bins + (long)blockIdx.x * 1024;
    uint32_t c = 0;
    uint64_t p = 0;
    for (int i = 0; i < 4; ++i) {
        const uint4 v = src[i * ST_T + threadIdx.x];
        c += (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0);
        p += (uint64_t)v.x + v.y + v.z + v.w;
    }
    for (int d = 32; d > 0; d >>= 1) {
        c += __shfl_down(c, d, 64);
        p += __shfl_down(p, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        c_s[threadIdx.x >> 6] = c;
        p_s[threadIdx.x >> 6] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws_cnt[blockIdx.x] = c_s[0] + c_s[1] + c_s[2] + c_s[3];
        ws_sum[blockIdx.x] = p_s[0] + p_s[1] + p_s[2] + p_s[3];
    }
}

__global__ __launch_bounds__(ST_T) void st_scan(const uint64_t *__restrict__ ws_sum, const uint32_t *__restrict__ ws_cnt, uint32_t *__restrict__ ws_off,
                                                int64_t *__restrict__ status)
{
    __shared__ uint32_t wave_sums[ST_T / 64];
    __shared__ uint64_t p_s[ST_T / 64];
    const int per = ST_BLOCKS / ST_T;       // 16 consecutive blocks per thread
    uint32_t c[per], mine = 0;
    uint64_t p = 0;
    for (int i = 0; i < per; ++i) {
        c[i] = ws_cnt[threadIdx.x * per + i];
        mine += c[i];
        p += ws_sum[threadIdx.x * per + i];
    }
    uint32_t total;
    uint32_t off = st_block_scan(mine, wave_sums, total);
    for (int i = 0; i < per; ++i) {
        ws_off[threadIdx.x * per + i] = off;
        off += c[i];
    }
    for (int d = 32; d > 0; d >>= 1) p += __shfl_down(p, d, 64);
    if ((threadIdx.x & 63) == 0) p_s[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        status[0] = (int64_t)total;
        status[1] = (int64_t)(p_s[0] + p_s[1] + p_s[2] + p_s[3]);
    }
}

__global__ __launch_bounds__(ST_T) void st_write(uint32_t *__restrict__ bins, const uint32_t *__restrict__ ws_off, uint2 *__restrict__ list, uint32_t cap,
                                                 int clear)
{
    __shared__ uint32_t wave_sums[ST_T / 64];
    const uint32_t key0 = blockIdx.x * 4096u + threadIdx.x * 16u;    // this thread's 16 consecutive bins
    uint4 *src = (uint4 *)(bins + key0);
    uint32_t v[16], mine = 0;
    for (int i = 0; i < 4; ++i) {
        const uint4 q = src[i];
        v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
        if (clear && (q.x | q.y | q.z | q.w)) src[i] = make_uint4(0, 0, 0, 0);
    }
    for (int i = 0; i < 16; ++i) mine += v[i] != 0;
    uint32_t total;
    uint32_t at = ws_off[blockIdx.x] + st_block_scan(mine, wave_sums, total);
    for (int i = 0; i < 16; ++i) {
        if (!v[i]) continue;
        if (at < cap) list[at] = make_uint2(key0 + i, v[i]);
        ++at;
    }
}

int hvn_launch_stain_compact(uint32_t *bins, uint32_t *list, uint32_t cap, int64_t *status, void *workspace, int clear, hipStream_t stream)
{
    uint64_t *ws_sum = (uint64_t *)workspace;
    uint32_t *ws_cnt = (uint32_t *)(ws_sum + ST_BLOCKS), *ws_off = ws_cnt + ST_BLOCKS;
    hipLaunchKernelGGL(st_count, dim3(ST_BLOCKS), dim3(ST_T), 0, stream, bins, ws_sum, ws_cnt);
    hipLaunchKernelGGL(st_scan, dim3(1), dim3(ST_T), 0, stream, ws_sum, ws_cnt, ws_off, status);
    hipLaunchKernelGGL(st_write, dim3(ST_BLOCKS), dim3(ST_T), 0, stream, bins, ws_off, (uint2 *)list, cap, clear);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t st_level(const double *tab, uint32_t r, uint32_t g, uint32_t b)
{
    const double x = (tab[r] * tab[256 + g]) * tab[512 + b];
    return x < 255.0 ? (uint32_t)(int)x : 255u;       // NaN and +inf: 255
}

__device__ __forceinline__ uint32_t st_pixel(const double *tab, uint32_t r, uint32_t g, uint32_t b)
{
    return (st_level(tab, r, g, b) & 255u) | (st_level(tab + 768, r, g, b) & 255u) << 8 | (st_level(tab + 1536, r, g, b) & 255u) << 16;
}

__global__ __launch_bounds__(ST_T) void st_apply(const uint8_t *x, uint8_t *y, const double *__restrict__ tables, const StRows a)
{
    __shared__ double tab[9 * 256];
    for (int i = threadIdx.x; i < 9 * 256; i += ST_T) tab[i] = (i / 256) % 3 == 0 ? ST_IO * tables[i] : tables[i];
    __syncthreads();
    const long G = (a.W + 3) >> 2;
    for (long r = blockIdx.y; r < a.rows; r += gridDim.y) {
        const uint8_t *row = x + (r / a.R0) * a.sn + (r % a.R0) * a.sy;
        uint8_t *out = y + (r / a.R0) * a.ysn + (r % a.R0) * a.ysy;
        const bool vec = ((((uintptr_t)row) | ((uintptr_t)out)) & 3) == 0;
        for (long g = (long)blockIdx.x * ST_T + threadIdx.x; g < G; g += (long)gridDim.x * ST_T) {
            const long p0 = g << 2;
            const int np = a.W - p0 >= 4 ? 4 : (int)(a.W - p0);
            if (vec && np == 4) {
                const uint32_t *src = (const uint32_t *)(row + 3 * p0);
                const uint32_t u = src[0], v = src[1], w = src[2];
                const uint32_t q0 = st_pixel(tab, u & 255u, (u >> 8) & 255u, (u >> 16) & 255u);
                const uint32_t q1 = st_pixel(tab, u >> 24, v & 255u, (v >> 8) & 255u);
                const uint32_t q2 = st_pixel(tab, (v >> 16) & 255u, v >> 24, w & 255u);
                const uint32_t q3 = st_pixel(tab, (w >> 8) & 255u, (w >> 16) & 255u, w >> 24);
                uint32_t *dst = (uint32_t *)(out + 3 * p0);
                dst[0] = q0 | q1 << 24;
                dst[1] = q1 >> 8 | q2 << 16;
                dst[2] = q2 >> 16 | q3 << 8;
            } else {
                uint32_t q[4];
                for (int i = 0; i < np; ++i) {
                    const uint8_t *px = row + 3 * (p0 + i);
                    q[i] = st_pixel(tab, px[0], px[1], px[2]);
                }
                for (int i = 0; i < np; ++i) {
                    uint8_t *px = out + 3 * (p0 + i);
                    px[0] = (uint8_t)q[i];
                    px[1] = (uint8_t)(q[i] >> 8);
                    px[2] = (uint8_t)(q[i] >> 16);
                }
            }
        }
    }
}

int hvn_launch_stain_apply(const StainApplyArgs &a, hipStream_t stream)
{
    const StRows r = st_fold(a.N, a.H, a.W, a.xsn, a.xsy, a.ysn, a.ysy, true);
    hipLaunchKernelGGL(st_apply, st_grid(r), dim3(ST_T), 0, stream, a.x, a.y, a.tables, r);
    return hipGetLastError() == hipSuccess ? HVN_OK : HVN_E_LAUNCH;
}

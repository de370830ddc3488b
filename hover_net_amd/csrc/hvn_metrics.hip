// hvn_metrics.hip -- exact integer tables behind the instance-segmentation metrics of the reference's
// metrics/stats_utils.py (get_fast_pq, get_fast_aji, get_fast_aji_plus, get_dice_1, get_fast_dice_2, get_dice_2) and its
// remap_label.  Every score there is a function of one object per image: the count of pixels per distinct (true id, pred id)
// pair.  The kernels below build that table (and the label ranking of remap_label) with integer atomics only, so the set of
// triples is exact and identical from run to run; hover_net_amd/metrics.py does all floating-point arithmetic on the host.
//
// Pair table (one launch over all n images, blockIdx.y = image):
//   mt_pair_local   each workgroup reads MT_BLK pixels of both maps once (lanes on consecutive pixels), folds runs of equal keys
//                   inside a wave (ballot of the lanes whose key differs from the left neighbour's), and adds each run into a
//                   small open-addressing hash in LDS keyed by the 64-bit (t, p); a key that finds no slot within MT_PROBE probes
//                   goes straight to the global table.  The LDS table is then flushed: one global atomic per distinct pair.
//   global table    per image, capacity = next power of two >= 2 * h * w (an image has at most h * w distinct pairs, so the load
//                   factor stays <= 1/2, linear probing always ends and no retry path exists); the insert that claims a slot
//                   appends the slot's index to the image's triple list.
//   mt_pair_compact turns the first counts[i] list entries into (t, p, count) (order = claim order, not canonical).
//
// Label ranking (remap_label, by_size = False): a presence bitmap over [0, max_id] per image (atomicOr, one per run of equal ids
// inside a wave), a popcount prefix over its words (block sums, one scan per image, per-word exclusive prefix), then
// new id = prefix[word] + popcount(word's bits up to the id).  by_size = True adds an area histogram and a permutation gather.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/hvn.h"
#include "hvn_kernels.h"

#define MT_T 256                  // threads per workgroup (4 waves)
#define MT_PIX 16                 // pixels per thread per workgroup
#define MT_BLK (MT_T * MT_PIX)    // 4096 pixels per workgroup
#define MT_LCAP 1024              // LDS hash slots (8 KB keys + 4 KB counts)
#define MT_PROBE 16               // LDS probes before a key goes to the global table
#define RL_WORDS (MT_T * 16)      // bitmap words per prefix workgroup (16 per thread)

static size_t mt_align(size_t x) { return (x + 255) & ~(size_t)255; }

static long long mt_capacity(int h, int w)
{
    long long need = 2LL * h * w, c = 1;
    while (c < need) c <<= 1;
    return c;
}

__device__ __forceinline__ unsigned long long mt_hash(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// Slots go from 0 to a key exactly once and never change afterwards: a relaxed read that still sees 0 only costs a failed CAS.
__device__ void mt_global_add(unsigned long long *keys, unsigned *cnt, int32_t *list, int32_t *nk, unsigned long long mask,
                              unsigned long long key, unsigned c)
{
    unsigned long long s = mt_hash(key) & mask;
    for (;;) {
        unsigned long long k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            k = atomicCAS(&keys[s], 0ULL, key);
            if (k == 0) {
                atomicAdd(&cnt[s], c);
                const int i = atomicAdd(nk, 1);
                list[3 * (long)i] = (int32_t)s;        // mt_pair_compact replaces the slot index by the triple
                return;
            }
        }
        if (k == key) {
            atomicAdd(&cnt[s], c);
            return;
        }
        s = (s + 1) & mask;
    }
}

__device__ __forceinline__ bool mt_local_add(unsigned long long *lk, unsigned *lc, unsigned long long key, unsigned c)
{
    unsigned s = (unsigned)mt_hash(key) & (MT_LCAP - 1);
    for (int i = 0; i < MT_PROBE; ++i) {
        unsigned long long k = lk[s];
        if (k == 0) {
            k = atomicCAS(&lk[s], 0ULL, key);
            if (k == 0) k = key;
        }
        if (k == key) {
            atomicAdd(&lc[s], c);
            return true;
        }
        s = (s + 1) & (MT_LCAP - 1);
    }
    return false;
}

// Length of the run of equal values that starts at this lane (0 if the lane does not start one): brk = ballot of the lanes
// whose value differs from the left neighbour's (lane 0 always starts a run).
__device__ __forceinline__ unsigned mt_run_length(bool starts)
{
    const unsigned long long brk = __ballot(starts);
    const unsigned lane = __lane_id();
    if (!starts) return 0;
    const unsigned long long above = lane == 63 ? 0ULL : brk >> (lane + 1);
    return above ? (unsigned)__builtin_ctzll(above) + 1 : 64u - lane;
}

__global__ void __launch_bounds__(MT_T) mt_pair_local(const int32_t *__restrict__ tm, const int32_t *__restrict__ pm, long P,
                                                      unsigned long long *keys, unsigned *cnt, long long C, int32_t *triples,
                                                      int32_t *counts)
{
    __shared__ unsigned long long lk[MT_LCAP];
    __shared__ unsigned lc[MT_LCAP];
    const int img = blockIdx.y;
    for (int s = threadIdx.x; s < MT_LCAP; s += MT_T) {
        lk[s] = 0;
        lc[s] = 0;
    }
    __syncthreads();
    tm += (long)img * P;
    pm += (long)img * P;
    unsigned long long *gk = keys + (long long)img * C;
    unsigned *gc = cnt + (long long)img * C;
    int32_t *list = triples + (long)img * P * 3;
    int32_t *nk = counts + img;
    const unsigned long long mask = (unsigned long long)C - 1;
    const long base = (long)blockIdx.x * MT_BLK + threadIdx.x;
    for (int k = 0; k < MT_PIX; ++k) {
        const long i = base + (long)k * MT_T;
        unsigned long long key = 0;                       // (0, 0) and pixels past the end carry key 0 and are not counted
        if (i < P) key = ((unsigned long long)(uint32_t)tm[i] << 32) | (uint32_t)pm[i];
        const unsigned long long left = __shfl_up(key, 1);
        const unsigned run = mt_run_length(__lane_id() == 0 || left != key);
        if (run && key && !mt_local_add(lk, lc, key, run)) mt_global_add(gk, gc, list, nk, mask, key, run);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < MT_LCAP; s += MT_T)
        if (lk[s]) mt_global_add(gk, gc, list, nk, mask, lk[s], lc[s]);
}

__global__ void __launch_bounds__(MT_T) mt_pair_compact(const unsigned long long *keys, const unsigned *cnt, long long C, long P,
                                                        int32_t *triples, const int32_t *counts)
{
    const int img = blockIdx.y;
    const int K = counts[img];
    int32_t *tr = triples + (long)img * P * 3;
    for (long i = (long)blockIdx.x * MT_T + threadIdx.x; i < K; i += (long)gridDim.x * MT_T) {
        const long long s = (long long)img * C + tr[3 * i];
        const unsigned long long key = keys[s];
        tr[3 * i] = (int32_t)(key >> 32);
        tr[3 * i + 1] = (int32_t)(key & 0xffffffffULL);
        tr[3 * i + 2] = (int32_t)cnt[s];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// label range and ranking

__global__ void rl_range_init(int32_t *range, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        range[2 * i] = INT_MAX;
        range[2 * i + 1] = INT_MIN;
    }
}

__global__ void __launch_bounds__(MT_T) rl_range(const int32_t *__restrict__ map, long P, int32_t *range)
{
    const int img = blockIdx.y;
    map += (long)img * P;
    int lo = INT_MAX, hi = INT_MIN;
    const long base = (long)blockIdx.x * MT_BLK + threadIdx.x;
    for (int k = 0; k < MT_PIX; ++k) {
        const long i = base + (long)k * MT_T;
        if (i < P) {
            const int v = map[i];
            lo = min(lo, v);
            hi = max(hi, v);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if (__lane_id() == 0) {
        atomicMin(&range[2 * img], lo);
        atomicMax(&range[2 * img + 1], hi);
    }
}

__global__ void __launch_bounds__(MT_T) rl_mark(const int32_t *__restrict__ map, long P, int32_t max_id, unsigned *bits, long Wd)
{
    const int img = blockIdx.y;
    map += (long)img * P;
    bits += (long)img * Wd;
    const long base = (long)blockIdx.x * MT_BLK + threadIdx.x;
    for (int k = 0; k < MT_PIX; ++k) {
        const long i = base + (long)k * MT_T;
        const int v = i < P ? map[i] : 0;
        const int left = __shfl_up(v, 1);
        if ((__lane_id() == 0 || left != v) && v > 0 && v <= max_id) atomicOr(&bits[v >> 5], 1u << (v & 31));
    }
}

// Inclusive block scan of one value per thread (MT_T threads); returns the block total through *total.
__device__ __forceinline__ unsigned rl_block_scan(unsigned x, unsigned *total)
{
    __shared__ unsigned wsum[MT_T / 64];
    const unsigned lane = __lane_id(), wave = threadIdx.x / 64;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o);
        if (lane >= (unsigned)o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned off = 0, all = 0;
    for (unsigned j = 0; j < MT_T / 64; ++j) {
        if (j < wave) off += wsum[j];
        all += wsum[j];
    }
    __syncthreads();
    *total = all;
    return x + off;
}

__global__ void __launch_bounds__(MT_T) rl_block_sums(const unsigned *bits, long Wd, unsigned *bsum, int nbw)
{
    const int img = blockIdx.y;
    const uint4 *w4 = (const uint4 *)(bits + (long)img * Wd + (long)blockIdx.x * RL_WORDS + threadIdx.x * 16);
    unsigned s = 0;
    for (int j = 0; j < 4; ++j) {
        const uint4 q = w4[j];
        s += __popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w);
    }
    unsigned total;
    rl_block_scan(s, &total);
    if (threadIdx.x == 0) bsum[(long)img * nbw + blockIdx.x] = total;
}

// One workgroup per image: exclusive scan of the block sums in place; n_ids[img] = number of present non-zero ids.
__global__ void __launch_bounds__(MT_T) rl_scan_sums(unsigned *bsum, int nbw, int32_t *n_ids)
{
    const int img = blockIdx.x;
    unsigned *b = bsum + (long)img * nbw;
    unsigned carry = 0;
    for (int c0 = 0; c0 < nbw; c0 += MT_T) {
        const int i = c0 + threadIdx.x;
        const unsigned x = i < nbw ? b[i] : 0u;
        unsigned total;
        const unsigned inc = rl_block_scan(x, &total);
        if (i < nbw) b[i] = carry + inc - x;
        carry += total;
    }
    if (threadIdx.x == 0) n_ids[img] = (int32_t)carry;
}

__global__ void __launch_bounds__(MT_T) rl_word_prefix(const unsigned *bits, long Wd, const unsigned *bsum, int nbw, unsigned *prefix)
{
    const int img = blockIdx.y;
    const long w0 = (long)img * Wd + (long)blockIdx.x * RL_WORDS + threadIdx.x * 16;
    const uint4 *w4 = (const uint4 *)(bits + w0);
    unsigned v[16];
    for (int j = 0; j < 4; ++j) {
        const uint4 q = w4[j];
        v[4 * j] = __popc(q.x);
        v[4 * j + 1] = __popc(q.y);
        v[4 * j + 2] = __popc(q.z);
        v[4 * j + 3] = __popc(q.w);
    }
    unsigned s = 0;
    for (int j = 0; j < 16; ++j) s += v[j];
    unsigned total;
    unsigned run = rl_block_scan(s, &total) - s + bsum[(long)img * nbw + blockIdx.x];
    uint4 *p4 = (uint4 *)(prefix + w0);
    for (int j = 0; j < 4; ++j) {
        uint4 q;
        q.x = run; run += v[4 * j];
        q.y = run; run += v[4 * j + 1];
        q.z = run; run += v[4 * j + 2];
        q.w = run; run += v[4 * j + 3];
        p4[j] = q;
    }
}

__global__ void __launch_bounds__(MT_T) rl_relabel(const int32_t *__restrict__ map, long P, int32_t max_id, const unsigned *bits,
                                                   const unsigned *prefix, long Wd, int32_t *out)
{
    const int img = blockIdx.y;
    const long off = (long)img * P, wo = (long)img * Wd;
    const long base = (long)blockIdx.x * MT_BLK + threadIdx.x;
    for (int k = 0; k < MT_PIX; ++k) {
        const long i = base + (long)k * MT_T;
        if (i >= P) break;
        const int v = map[off + i];
        int r = 0;
        if (v > 0 && v <= max_id) {
            const long wd = wo + (v >> 5);
            const unsigned b = v & 31, m = b == 31 ? 0xffffffffu : ((2u << b) - 1u);
            r = (int)(prefix[wd] + __popc(bits[wd] & m));
        }
        out[off + i] = r;
    }
}

__global__ void __launch_bounds__(MT_T) rl_areas(const int32_t *__restrict__ map, long P, int32_t max_label, int32_t *areas)
{
    const int img = blockIdx.y;
    map += (long)img * P;
    areas += (long)img * ((long)max_label + 1);
    const long base = (long)blockIdx.x * MT_BLK + threadIdx.x;
    for (int k = 0; k < MT_PIX; ++k) {
        const long i = base + (long)k * MT_T;
        const int v = i < P ? map[i] : -1;
        const int left = __shfl_up(v, 1);
        const unsigned run = mt_run_length(__lane_id() == 0 || left != v);
        if (run && v >= 0 && v <= max_label) atomicAdd(&areas[v], (int)run);
    }
}

__global__ void __launch_bounds__(MT_T) rl_permute(int32_t *map, long P, int32_t max_label, const int32_t *perm)
{
    const int img = blockIdx.y;
    map += (long)img * P;
    perm += (long)img * ((long)max_label + 1);
    const long base = (long)blockIdx.x * MT_BLK + threadIdx.x;
    for (int k = 0; k < MT_PIX; ++k) {
        const long i = base + (long)k * MT_T;
        if (i >= P) break;
        const int v = map[i];
        if (v >= 0 && v <= max_label) map[i] = perm[v];
    }
}

static long rl_words(int32_t max_id) { return (((long)max_id / 32 + 1) + RL_WORDS - 1) / RL_WORDS * RL_WORDS; }

static bool mt_shape_ok(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (long long)h * w <= (1LL << 30) && n <= 65535; }
static int mt_bad_shape(const char *what, int n, int h)
{
    return hvn_fail(HVN_E_ARG, "%s: n outside [1, 65535], h or w < 1, or h * w > 2^30 (n = %d, h = %d)", what, n, h);
}

static dim3 mt_grid(int n, long P) { return dim3((unsigned)((P + MT_BLK - 1) / MT_BLK), (unsigned)n); }

extern "C" {

size_t hvn_pair_table_workspace_bytes(int n, int h, int w)
{
    if (!mt_shape_ok(n, h, w)) return 0;
    const size_t C = (size_t)mt_capacity(h, w);
    return mt_align((size_t)n * C * 8) + mt_align((size_t)n * C * 4);
}

int hvn_pair_table(const int32_t *true_map, const int32_t *pred_map, int n, int h, int w, int32_t *triples, int32_t *counts,
                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (!true_map || !pred_map || !triples || !counts) return hvn_fail(HVN_E_ARG, "pair_table: null pointer");
    if (!mt_shape_ok(n, h, w)) return mt_bad_shape("pair_table", n, h);
    if (!workspace || workspace_bytes < hvn_pair_table_workspace_bytes(n, h, w))
        return hvn_fail(HVN_E_SIZE, "pair_table: workspace NULL or smaller than hvn_pair_table_workspace_bytes (%zu bytes given)", workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const long long C = mt_capacity(h, w);
    const long P = (long)h * w;
    unsigned long long *keys = (unsigned long long *)workspace;
    unsigned *cnt = (unsigned *)((unsigned char *)workspace + mt_align((size_t)n * C * 8));
    if (hipMemsetAsync(workspace, 0, hvn_pair_table_workspace_bytes(n, h, w), s) != hipSuccess ||
        hipMemsetAsync(counts, 0, (size_t)n * 4, s) != hipSuccess)
        return hvn_fail(HVN_E_LAUNCH, "pair_table: hipMemsetAsync failed");
    hipLaunchKernelGGL(mt_pair_local, mt_grid(n, P), dim3(MT_T), 0, s, true_map, pred_map, P, keys, cnt, C, triples, counts);
    hipLaunchKernelGGL(mt_pair_compact, dim3(64, n), dim3(MT_T), 0, s, keys, cnt, C, P, triples, counts);
    return hvn_launched("pair_table");
}

int hvn_label_range(const int32_t *map, int n, int h, int w, int32_t *range, void *stream)
{
    if (!map || !range) return hvn_fail(HVN_E_ARG, "label_range: null pointer");
    if (!mt_shape_ok(n, h, w)) return mt_bad_shape("label_range", n, h);
    hipStream_t s = (hipStream_t)stream;
    const long P = (long)h * w;
    hipLaunchKernelGGL(rl_range_init, dim3((n + MT_T - 1) / MT_T), dim3(MT_T), 0, s, range, n);
    hipLaunchKernelGGL(rl_range, mt_grid(n, P), dim3(MT_T), 0, s, map, P, range);
    return hvn_launched("label_range");
}

size_t hvn_remap_label_workspace_bytes(int n, int h, int w, int32_t max_id)
{
    if (!mt_shape_ok(n, h, w) || max_id < 0) return 0;
    const long Wd = rl_words(max_id), nbw = Wd / RL_WORDS;
    return 2 * mt_align((size_t)n * Wd * 4) + mt_align((size_t)n * nbw * 4);
}

int hvn_remap_label(const int32_t *map, int n, int h, int w, int32_t max_id, int32_t *out, int32_t *n_ids, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    if (!map || !out || !n_ids) return hvn_fail(HVN_E_ARG, "remap_label: null pointer");
    if (!mt_shape_ok(n, h, w)) return mt_bad_shape("remap_label", n, h);
    if (max_id < 0) return hvn_fail(HVN_E_ARG, "remap_label: max_id %d < 0", max_id);
    if (!workspace || workspace_bytes < hvn_remap_label_workspace_bytes(n, h, w, max_id))
        return hvn_fail(HVN_E_SIZE, "remap_label: workspace NULL or smaller than hvn_remap_label_workspace_bytes (%zu bytes given)", workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const long P = (long)h * w, Wd = rl_words(max_id);
    const int nbw = (int)(Wd / RL_WORDS);
    unsigned *bits = (unsigned *)workspace;
    unsigned *prefix = (unsigned *)((unsigned char *)workspace + mt_align((size_t)n * Wd * 4));
    unsigned *bsum = (unsigned *)((unsigned char *)prefix + mt_align((size_t)n * Wd * 4));
    if (hipMemsetAsync(bits, 0, (size_t)n * Wd * 4, s) != hipSuccess) return hvn_fail(HVN_E_LAUNCH, "remap_label: hipMemsetAsync failed");
    hipLaunchKernelGGL(rl_mark, mt_grid(n, P), dim3(MT_T), 0, s, map, P, max_id, bits, Wd);
    hipLaunchKernelGGL(rl_block_sums, dim3(nbw, n), dim3(MT_T), 0, s, bits, Wd, bsum, nbw);
    hipLaunchKernelGGL(rl_scan_sums, dim3(n), dim3(MT_T), 0, s, bsum, nbw, n_ids);
    hipLaunchKernelGGL(rl_word_prefix, dim3(nbw, n), dim3(MT_T), 0, s, bits, Wd, bsum, nbw, prefix);
    hipLaunchKernelGGL(rl_relabel, mt_grid(n, P), dim3(MT_T), 0, s, map, P, max_id, bits, prefix, Wd, out);
    return hvn_launched("remap_label");
}

int hvn_label_areas(const int32_t *map, int n, int h, int w, int32_t max_label, int32_t *areas, void *stream)
{
    if (!map || !areas) return hvn_fail(HVN_E_ARG, "label_areas: null pointer");
    if (!mt_shape_ok(n, h, w)) return mt_bad_shape("label_areas", n, h);
    if (max_label < 0) return hvn_fail(HVN_E_ARG, "label_areas: max_label %d < 0", max_label);
    hipStream_t s = (hipStream_t)stream;
    const long P = (long)h * w;
    if (hipMemsetAsync(areas, 0, (size_t)n * ((size_t)max_label + 1) * 4, s) != hipSuccess) return hvn_fail(HVN_E_LAUNCH, "label_areas: hipMemsetAsync failed");
    hipLaunchKernelGGL(rl_areas, mt_grid(n, P), dim3(MT_T), 0, s, map, P, max_label, areas);
    return hvn_launched("label_areas");
}

int hvn_label_permute(int32_t *map, int n, int h, int w, int32_t max_label, const int32_t *perm, void *stream)
{
    if (!map || !perm) return hvn_fail(HVN_E_ARG, "label_permute: null pointer");
    if (!mt_shape_ok(n, h, w)) return mt_bad_shape("label_permute", n, h);
    if (max_label < 0) return hvn_fail(HVN_E_ARG, "label_permute: max_label %d < 0", max_label);
    hipStream_t s = (hipStream_t)stream;
    const long P = (long)h * w;
    hipLaunchKernelGGL(rl_permute, mt_grid(n, P), dim3(MT_T), 0, s, map, P, max_label, perm);
    return hvn_launched("label_permute");
}

}  // extern "C"

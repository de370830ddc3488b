// Internal launch interfaces shared by the .hip translation units of libhvn_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "hvn_env.h"
#include "hvn_error.h"   // the status enum of include/hvn.h and hvn_fail

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set it once per (kernel instantiation, device), from any
// host thread.  `done` = one bit per device ordinal (function-local static of the launcher).  Returns HVN_OK, or HVN_E_LAUNCH when the runtime refuses.
static inline int hvn_max_lds_once(const void *kern, int bytes, std::atomic<unsigned long long> &done)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return HVN_E_LAUNCH;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return HVN_OK;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return HVN_E_LAUNCH;
    done.fetch_or(bit, std::memory_order_release);
    return HVN_OK;
}

struct ConvArgs {
    const float *x;
    long xsn, xsy, xsx;
    int H, W, Cin;
    const float *w;
    const float *bias, *pre_s, *pre_b, *post_s, *post_b;
    const float *res;
    long rsn, rsy, rsx;
    float *y;
    long ysn, ysy, ysx;
    int N, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, relu;
    long M;
    long m_tiles;
    int n_tiles;
    int groups;
    const float *x2;      // optional second 1x1 input (channels appended to the reduction)
    long x2sn, x2sy, x2sx;
    int Cin2, stride2;
    int nbatch;           // > 1: blockIdx.y selects one of nbatch independent problems
    unsigned long long *dbg;  // optional: per-workgroup {start, k-loop end, epilogue end, HW_ID | LDS base << 32} (tools/conv_trace.py)
    long xb, wb, yb;      // element strides between them
};

int hvn_launch_conv(const ConvArgs &a, int tile_n, hipStream_t stream);

// Two chained 1x1 convs of a residual block in one launch (hvn_conv_chain.hip):
//   y  = [relu(. * post_s + post_b)]( W1 . x (+ W1b . x2) + res )        C channels        (a unit's conv3 + shortcut)
//   y2 = [relu]( W2 . a + bias2 ),  a = relu(y * pre_s + pre_b) or y     N2 channels       (the next unit's conv1)
// pixel tile of workgroup (xcd = blockIdx % 8, seq_m) of a convolution launch with `groups` = ceil(m_tiles / 8) tiles per XCD
static __device__ __forceinline__ int hvn_m_tile(int xcd, int seq_m, int groups, bool contiguous)
{
    return contiguous ? xcd * groups + seq_m : seq_m * 8 + xcd;
}

struct ChainArgs {
    const float *x;       // conv3 input view [N][Ho][Wo][K1]
    long xsn, xsy, xsx;
    int K1;
    const float *x2;      // optional second input (the strided 1x1 shortcut's), sampled at (oy * stride2, ox * stride2)
    long x2sn, x2sy, x2sx;
    int K1b, stride2;
    const float *w1;      // [C_pad][(K1 + K1b) / 32][1][32]
    const float *res;     // optional residual view (may alias y)
    long rsn, rsy, rsx;
    float *y;
    long ysn, ysy, ysx;
    int C;
    const float *post_s, *post_b, *pre_s, *pre_b;   // optional per-channel affines [C]
    const float *w2;      // [N2_pad][C / 32][1][32]
    const float *bias2;   // optional [N2]
    int relu2;
    float *y2;
    long y2sn, y2sy, y2sx;
    int N2;
    int N, Ho, Wo;
    long M;
    int bm;               // pixels per workgroup: 64, or anything else for 128
    unsigned long long *dbg;   // optional (HVN_CHAIN_TRACE): 10 cycle stamps per workgroup, see tools/chain_bench.py
};
int hvn_launch_conv_chain(const ChainArgs &a, hipStream_t stream);
int hvn_chain_supported(int c, int n2);
// the same chain for the bf16 path (hvn_conv_chain_bf16.hip): bf16 views (strides in elements), hvn_conv_bf16.hip's weight packing, 64 pixels per workgroup
int hvn_chain_bf16_supported(int k1, int k1b, int c, int n2);
int hvn_launch_conv_chain_bf16(const ChainArgs &a, hipStream_t stream);
// the same op with w1 / w2 = bf16 planes of the fp32 packings and both GEMMs' products on the bf16 matrix pipe (hvn_conv_chain_x3.hip)
int hvn_launch_conv_chain_x3(const ChainArgs &a, int terms, hipStream_t stream);
// the same op, same bits, conv3's input tile resident in registers and every other operand a chunk ahead in flight (hvn_conv_chain_x3r.hip);
// exists for K1 = 64 (+ K1b = 64 without a residual view and with N2 = 64)
int hvn_chain_x3r_supported(const ChainArgs &a);
int hvn_launch_conv_chain_x3r(const ChainArgs &a, int terms, hipStream_t stream);
int hvn_launch_conv_bf16(const ConvArgs &a, int tile_n, hipStream_t stream);   // x, res, y, x2, w are bf16; bias / scales fp32
// the same convolution (same packing, same bits) with both operands staged by LDS-DMA: bm = 256 | 128 pixels x 128 channels (hvn_conv_bf16g.hip)
int hvn_launch_conv_bf16g(const ConvArgs &a, int bm, hipStream_t stream);
// fp32 in / out; w = [cout_pad][k-step][3][32] bf16 planes of the fp32 weights; terms = 9 | 6 partial products (hvn_conv_x3.hip)
int hvn_launch_conv_x3(const ConvArgs &a, int tile_n, int terms, hipStream_t stream);
// the same convolution (same packing, same bits) with both operands staged by LDS-DMA, bm = 256 | 128 pixels x 128 channels (hvn_conv_x3g.hip)
int hvn_launch_conv_x3g(const ConvArgs &a, int bm, int terms, hipStream_t stream);
int hvn_conv_x3g_supported(const ConvArgs &a, int bm);
// fp32 packings ([...][32]-float granules) -> their bf16 planes [3][32] per granule (training: weights change every step)
int hvn_launch_split_x3(const float *src, uint16_t *dst, long granules, hipStream_t stream);

struct Conv0Args {
    const void *img;      // uint8 or float32
    long isn, isy, isx, isc;  // strides in elements
    int is_f32;
    int H, W;             // input extent
    const float *w;       // [7][7][3][64]
    const float *bias;    // [64]
    float *y;
    long ysn, ysy, ysx;
    int N, Ho, Wo, pad;
    int relu;             // 1: ReLU after the bias (inference, BN folded); 0: raw conv output (training)
    int out_bf16;         // y is bf16 (cfg 3) instead of fp32
};
int hvn_launch_conv0(const Conv0Args &a, hipStream_t stream);

struct UpAddArgs {
    const float *lo;
    long lsn, lsy, lsx;
    const float *skip;
    long ssn, ssy, ssx;
    float *y;
    long ysn, ysy, ysx;
    int N, H, W, C;  // output extent
    int bf16;        // all three tensors are bf16
};
int hvn_launch_upadd(const UpAddArgs &a, hipStream_t stream);

struct HeadArgs {
    const float *x;
    long xsn, xsy, xsx;
    const float *w;     // [cout][64]
    const float *bias;  // [cout]
    float *y;           // NCHW [N][cout][H][W]
    int N, H, W, Cout;
    int in_bf16;        // x is bf16 (the logits stay fp32)
};
int hvn_launch_head(const HeadArgs &a, hipStream_t stream);

int hvn_launch_extract_patches(const uint8_t *img, int H, int W, const int32_t *coords, int P, int win, int pad_t, int pad_l, uint8_t *out,
                               hipStream_t stream);

// hvn_resample.hip: arguments as hvn_resize_window (include/hvn.h), validated by the caller; HVN_OK, HVN_E_LAUNCH, HVN_E_SIZE = too many tile rows
int hvn_launch_resize_window(const uint8_t *src, int src_h, int src_w, int64_t src_pitch, int src_y0, int src_x0, int full_h, int full_w,
                             const int32_t *xofs, const int16_t *xcoef, const int32_t *yofs, const int16_t *ycoef, int taps, uint8_t *dst,
                             int dst_h, int dst_w, hipStream_t stream);

// hvn_tissue.hip: arguments as hvn_tissue_gray_hist / hvn_tissue_mask (include/hvn.h), validated by the caller; HVN_OK or HVN_E_LAUNCH
size_t hvn_tissue_workspace_bytes(int h, int w);
int hvn_launch_tissue_gray_hist(const uint8_t *rgb, int h, int w, uint8_t *gray, uint32_t *hist256, hipStream_t stream);
int hvn_launch_tissue_mask(const uint8_t *gray, int h, int w, int threshold, int min_obj, int max_hole, int radius, uint8_t *mask,
                           uint8_t *tap_objects, uint8_t *tap_holes, void *workspace, hipStream_t stream);

// hvn_viz.hip: arguments as hvn_viz_strip (include/hvn.h), validated by the caller (n_sel >= 1); HVN_OK or HVN_E_LAUNCH
int hvn_launch_viz_strip(const uint8_t *img, int n, int ih, int iw, const float *pred, int c, const int32_t *np_map, const float *hv_map,
                         const int32_t *tp_map, int h, int w, int nr_types, const int32_t *sel, int n_sel, const uint8_t *lut, uint8_t *out,
                         int n_blocks, hipStream_t stream);

struct PredMapArgs {
    const float *tp, *np, *hv;  // NCHW logits
    float *y;                   // [N][H][W][3|4]
    int N, H, W, nr_types;      // nr_types = 0: no type channel
};
int hvn_launch_predmap(const PredMapArgs &a, hipStream_t stream);

// hvn_tta.hip: test-time augmentation over the eight views k = r + 4 f of the square (flip left-right if f, then r quarter turns
// counter-clockwise); arguments validated by the caller (hvn_api.hip); HVN_OK or HVN_E_LAUNCH
struct ViewArgs {
    const uint8_t *x;           // [N][H][W][3]
    long xsn, xsy;              // byte strides of a sample and a row (pixels are 3 contiguous bytes)
    uint8_t *y;                 // view_k(x): [N][W][H][3] for odd r (H == W there), else [N][H][W][3]
    long ysn, ysy;
    int N, H, W, k;
};
int hvn_launch_view(const ViewArgs &a, hipStream_t stream);

struct TtaArgs {
    const float *tp, *np, *hv;  // NCHW logits of view k
    float *acc;                 // [N][H][W][3 + nr_types] = (p_np, h, v, p_0 ..) in the original orientation
    float *y;                   // last view: [N][H][W][3|4] as PREDMAP writes it
    int N, H, W, nr_types;      // H x W: the original orientation (a transposing view's planes are [W][H], H == W)
    int k, first, last, K;      // first: store the term instead of adding it; last: also write acc / K and the type to y
};
int hvn_launch_tta(const TtaArgs &a, hipStream_t stream);

// hvn_stain.hip: Macenko stain normalisation (hover_net_amd/stain.py); arguments validated by the caller (hvn_api.hip); HVN_OK or HVN_E_LAUNCH
struct StainHistArgs {
    const uint8_t *x;           // [N][H][W][3]
    long xsn, xsy;              // byte strides of a sample and a row (pixels are 3 contiguous bytes)
    const uint8_t *mask;        // dense [N][H][W], non-zero = count the pixel; NULL = all
    uint32_t *bins;             // [1 << 24], bin = r << 16 | g << 8 | b; the launch ADDS to it
    int N, H, W;
};
int hvn_launch_stain_hist(const StainHistArgs &a, hipStream_t stream);
#define HVN_STAIN_WORKSPACE_BYTES 65536      // of hvn_launch_stain_compact, 8-byte aligned
// list: uint32 [cap][2] = (key, count) of the non-empty bins, ascending; status: int64 {non-empty bins, pixels counted}
int hvn_launch_stain_compact(uint32_t *bins, uint32_t *list, uint32_t cap, int64_t *status, void *workspace, int clear, hipStream_t stream);
struct StainApplyArgs {
    const uint8_t *x;           // [N][H][W][3]
    long xsn, xsy;
    uint8_t *y;                 // same extents; may be x itself (same strides)
    long ysn, ysy;
    const double *tables;       // [3][3][256]: T[c][k][v]
    int N, H, W;
};
int hvn_launch_stain_apply(const StainApplyArgs &a, hipStream_t stream);

// hvn_neighbours.hip: fixed-radius neighbours of centroids (hover_net_amd/neighbours.py); arguments validated by the caller (hvn_api.hip); HVN_OK or HVN_E_LAUNCH
#define HVN_NBR_MAX_N (1L << 26)
#define HVN_NBR_MAX_AXIS 4096
#define HVN_NBR_MAX_CELLS (1L << 22)
// the one workspace of both ops, 8-byte aligned, in this order: x, y of the points in cell order (float64 [N] each), their positions and
// types (int32 [N] each), cell_start (int32 [cells + 1]), the cell counters / cursors (int32 [cells]), the scan's block sums (int32 [1024])
#define HVN_NBR_WORKSPACE_BYTES(N, cells) (24L * (N) + 4L * (2L * (cells) + 1) + 4096L)
struct NbrWorkspace {
    double *sx, *sy;
    int *spos, *stype, *cell_start, *cursor, *bsum;
};
// the carve-up of that workspace, for every launcher that reads it
static inline NbrWorkspace hvn_nbr_workspace(void *ws, long N, long cells)
{
    NbrWorkspace w;
    w.sx = (double *)ws;
    w.sy = w.sx + N;
    w.spos = (int *)(w.sy + N);
    w.stype = w.spos + N;
    w.cell_start = w.stype + N;
    w.cursor = w.cell_start + cells + 1;
    w.bsum = w.cursor + cells;
    return w;
}
#ifdef __HIPCC__
// the cell coordinate of v on one axis: the quotient is brought into [0, 4096] as a double BEFORE the conversion (a NaN compares false
// and becomes 0) and into [0, n) as an integer after it
__device__ __forceinline__ int hvn_nbr_axis(double v, double v0, double c, int n)
{
    double q = floor(__ddiv_rn(__dsub_rn(v, v0), c));
    q = q >= 0.0 ? q : 0.0;            // NaN and negatives
    q = q <= 4096.0 ? q : 4096.0;
    int i = (int)q;
    i = i < 0 ? 0 : i;
    return i > n - 1 ? n - 1 : i;
}
__device__ __forceinline__ int hvn_nbr_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }      // a cell_start value into [0, N]
__device__ __forceinline__ bool hvn_nbr_less(double d, int j, double D, int J) { return d < D || (d == D && j < J); }   // the total order (d2, j)
// d2 of a candidate (x, y) from (qx, qy): four float64 roundings, each named, so that nothing can be contracted (points.py: `d2_of`)
__device__ __forceinline__ double hvn_nbr_d2(double x, double y, double qx, double qy)
{
    const double dx = __dsub_rn(x, qx), dy = __dsub_rn(y, qy);
    return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
}
#endif
struct NbrGridArgs {
    const double *xy;           // [N][2] = (x, y)
    const int *types;           // [N] or NULL (all 0)
    const double *table;        // {x0, y0, c, r2}
    void *workspace;
    int N, ncy, ncx;
};
int hvn_launch_nbr_grid(const NbrGridArgs &a, hipStream_t stream);
struct NbrQueryArgs {
    const double *table;
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    int *count, *knn, *nearest; // [N][T], [N][k], [N][T]
    int N, ncy, ncx, T, k;
};
int hvn_launch_nbr_query(const NbrQueryArgs &a, hipStream_t stream);
// hvn_clusters.hip: DBSCAN over that grid (hover_net_amd/clusters.py); the second workspace, 8-byte aligned, by slot (the cell-ordered
// index): the union-find parent, the smallest position of a root's cores, the degree (int32 [N] each)
#define HVN_NBR_CLUSTER_MAX_MIN_PTS (1 << 26)
#define HVN_NBR_CLUSTER_WORKSPACE_BYTES(N) (12L * (N))
struct NbrClusterArgs {
    const double *table;
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    void *workspace2;           // HVN_NBR_CLUSTER_WORKSPACE_BYTES(N); every word read is written first
    int *label, *degree;        // [N] each, by position
    int N, ncy, ncx, min_pts;
    unsigned mask;              // bit t selects type t; 0xFFFFFFFF selects every point whatever its type
};
int hvn_launch_nbr_cluster(const NbrClusterArgs &a, hipStream_t stream);
// hvn_density.hip: typed counts within the radius of every node of a regular raster (hover_net_amd/density.py)
#define HVN_NBR_DENSITY_MAX_AXIS 16384
#define HVN_NBR_DENSITY_MAX_NODES (1L << 28)     // T * H * W
struct NbrDensityArgs {
    const double *table;        // {x0, y0, c, r2}, as for the grid
    const double *raster;       // {ox, oy, s}: node (u, v) is at (ox + u * s, oy + v * s)
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    int *count;                 // [T][H][W]; every element is written
    int N, ncy, ncx, T, H, W;
};
int hvn_launch_nbr_density(const NbrDensityArgs &a, hipStream_t stream);
// hvn_pairs.hip: typed pair counts by distance bin, the integers under Ripley's cross-type K (hover_net_amd/ripley.py)
#define HVN_NBR_PAIRS_MAX_R 32
#define HVN_NBR_PAIRS_MAX_BINS 4096              // T * T * R
struct NbrPairsArgs {
    const double *table;        // {x0, y0, c, r2_{R-1}}, as for the grid
    const double *rt;           // {wx0, wy0, wx1, wy1, r_0 .. r_{R-1}, r2_0 .. r2_{R-1}}: 4 + 2 R doubles
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    long long *acc;             // [2][T][T][R]; cleared in stream order, then every element is written
    int N, ncy, ncx, T, R;
};
int hvn_launch_nbr_pairs(const NbrPairsArgs &a, hipStream_t stream);
// what hvn_pairs.hip and hvn_pairs_sim.hip share: the workgroup, the staging tile and the flush interval
#define RP_T 256
#define RP_TILE 1024          // candidates per staging tile, as nb_query's NB_TILE
#define RP_FLUSH 32           // tiles between two flushes: 32 * 1024 * 256 = 2^23 tests
#define RP_NONE 0x7FFFFFFF
#ifdef __HIPCC__
// The wave's LDS adds have been carried out, not merely issued (lgkmcnt(0); the other counters are left alone).  It stands before every
// barrier that a flush follows: the compiler's own wait was missing in front of the barrier at the top of the tile loop, and a wave that
// passed it read and cleared the histogram while another wave's last adds -- 64 lanes on one word take the LDS a while -- were still on
// their way: 70 000 coincident points of one type lost 84 wave-adds of hx that way.
__device__ __forceinline__ void rp_adds_done() { __builtin_amdgcn_s_waitcnt(0xC07F); }
#endif
// hvn_pairs_sim.hip: the same counts under SB random relabellings of the points, the border-corrected plane only (ripley.py: `sims_host`)
#define HVN_NBR_PAIRS_SIM_MAX_SB 32
#define HVN_NBR_PAIRS_SIM_WORDS(SB) (((SB) + 3) / 4)        // 32-bit words of one point's labels, a byte per simulation
// dynamic LDS of the pair kernel: SB histograms of T T R words, and W label words per staged candidate and per lane; with its static
// arrays (the staged coordinates, 16672 bytes) a workgroup then stays within the 160 KiB of a CU
#define HVN_NBR_PAIRS_SIM_LDS_BYTES(SB, bins) (4L * (SB) * (bins) + 4L * (RP_TILE + RP_T) * HVN_NBR_PAIRS_SIM_WORDS(SB))
#define HVN_NBR_PAIRS_SIM_MAX_LDS (140L * 1024)
#define HVN_NBR_PAIRS_SIM_LABEL_BYTES(N, SB) (4L * (N) * HVN_NBR_PAIRS_SIM_WORDS(SB))
struct NbrPairsSimArgs {
    const double *table;        // {x0, y0, c, r2_{R-1}}, as for the grid
    const double *rt;           // as NbrPairsArgs::rt
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    const int *types;           // [N] by POSITION (the grid op's input) or NULL (all 0)
    const unsigned long long *keys;     // [SB][8] round keys
    unsigned *labels;           // HVN_NBR_PAIRS_SIM_LABEL_BYTES(N, SB): [N][W] words by slot; every word read is written first
    long long *out;             // [SB][T T R + T (R + 1)]: per simulation acc [T][T][R], then cnt [T][R + 1]; cleared in stream order
    int N, ncy, ncx, T, R, SB;
    int phase;                  // 0: both launches; 1: out cleared and the labels made only; 2: the pairs only, on the labels as they are
};
int hvn_launch_nbr_pairs_sim(const NbrPairsSimArgs &a, hipStream_t stream);
// hvn_regions.hip: exact point-in-polygon of the points against the canonical edges of G regions (hover_net_amd/regions.py)
#define HVN_NBR_REGIONS_MAX_G 4096
#define HVN_NBR_REGIONS_MAX_E (1 << 22)
#define HVN_NBR_REGIONS_MAX_ENTRIES(E, ncy) (8L * (E) + (ncy))      // the row lists' total length
struct NbrRegionsArgs {
    const double *table;        // {x0, y0, c, r2}, as for the grid (r2 is not read)
    const double *edges;        // [E][4] = (ax, ay, bx, by), ay < by
    const int *edge_region;     // [E], ascending
    const int *rows;            // row_start [ncy + 1], then the edge numbers of the row lists [M]
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    int *out;                   // first [N], hits [N], count [G][T]; count is cleared in stream order, then every element is written
    int N, ncy, ncx, T, G, E, M;
};
int hvn_launch_nbr_regions(const NbrRegionsArgs &a, hipStream_t stream);
// hvn_margins.hip: the points by distance to the boundary segments of G regions, in B bands (hover_net_amd/margins.py)
#define HVN_NBR_MARGINS_MAX_B 16
#define HVN_NBR_MARGINS_MAX_G 4096
#define HVN_NBR_MARGINS_MAX_S (1 << 22)
#define HVN_NBR_MARGINS_MAX_ENTRIES(S, ncy) (8L * (S) + (ncy))      // the row lists' total length
#define HVN_NBR_MARGINS_OUT_BYTES(N, G, B, T) (16L * (N) + 8L * (G) * (B) * (T))
struct NbrMarginsArgs {
    const double *table;        // {x0, y0, c, r2}, as for the grid (r2 is not read)
    const double *seg;          // [S][8] = (ax, ay, bx, by) with (ay, ax) <= (by, bx), then the box (x0, y0, x1, y1)
    const double *w2;           // [B] squared widths, ascending
    const int *seg_region;      // [S], ascending
    const int *rows;            // row_start [ncy + 1], then the segment numbers of the row lists [M]
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    void *out;                  // near_d2 double [N], then int near [N], near_inside [N], hist [G][2][B][T]; hist is cleared in
                                // stream order, then every element is written
    int N, ncy, ncx, T, G, S, M, B;
    int no_cull;                // != 0: the kernel form without the x-cull of the staged tile (same numbers; for measurements)
};
int hvn_launch_nbr_margins(const NbrMarginsArgs &a, hipStream_t stream);
// hvn_graph.hip: the Gabriel edges of length <= r among the points, as a CSR graph in two passes (hover_net_amd/graph.py)
#define HVN_NBR_GRAPH_LIST_CAP 512               // neighbours of one point that a wave keeps on chip; above it the slower exact path runs
#define HVN_NBR_GRAPH_MAX_E ((1L << 31) - 1)
#define HVN_NBR_GRAPH_MAX_WIDTH 64
struct NbrGraphArgs {
    const double *table;        // {x0, y0, c, r2}, as for the grid
    void *workspace;            // as hvn_launch_nbr_grid left it for the same N, ncy, ncx
    int *degree;                // count: [N] by position; every row with a point is written
    int *first;                 // count: NULL or [N][width] by position: the first `width` edges of every row as the wave finds them
    const long long *indptr;    // fill: [N + 1] by position, the exclusive running sum of degree
    int *indices;               // fill: [E]; row i's positions in any order
    long long E;                // fill: the length of indices
    int N, ncy, ncx;
    int width;                  // count with `first`: 1..HVN_NBR_GRAPH_MAX_WIDTH
    int fill;                   // 0: count, 1: fill
};
int hvn_launch_nbr_graph(const NbrGraphArgs &a, hipStream_t stream);
// hvn_forest.hip: the minimum spanning forest and the connected components of a CSR graph over the points, Boruvka rounds
// (hover_net_amd/forest.py).  The one workspace, 8-byte aligned, by position: best_d2 and best_pair (uint64 [N] each), parent, comp and
// minpos (int32 [N] each), then 64 control words: hooks[32], the rounds word, found[26]
#define HVN_NBR_FOREST_MAX_ROUNDS 26             // max(1, ceil(log2 N)) for N <= 2^26
#define HVN_NBR_FOREST_MAX_E ((1L << 31) - 1)
#define HVN_NBR_FOREST_WORKSPACE_BYTES(N) (28L * (N) + 256)
#define HVN_NBR_FOREST_ROUNDS_AT(N) (28L * (N) + 128)       // the byte offset of the int32 that counts the rounds that hooked anything
struct NbrForestArgs {
    const double *xy;           // [N][2] = (x, y) by position
    const long long *indptr;    // [N + 1]
    const int *indices;         // [E], NULL iff E = 0
    int *component;             // [N] out: the smallest position of i's connected component
    unsigned char *tree;        // [E] out: 1 for both directed entries of a forest edge, else 0; every element is written
    void *workspace;            // HVN_NBR_FOREST_WORKSPACE_BYTES(N); every word read is written first
    long long E;
    int N;
    int phase;                  // 0: the whole forest; 1: the start only; 2: round `round` only; 3: the end only (forest.py times them apart)
    int round;                  // phase 2: 0..HVN_NBR_FOREST_MAX_ROUNDS - 1 (not read otherwise)
    int no_filter;              // != 0: the kernel form whose atomicMin is not preceded by a read of the word (same numbers; for measurements)
};
int hvn_launch_nbr_forest(const NbrForestArgs &a, hipStream_t stream);

// hvn_texture.hip: per-nucleus grey-level co-occurrence counts over the label map (hover_net_amd/texture.py), one wave per record slot
struct InstTextureArgs {
    const uint8_t *image;       // [N][H][W][3] RGB, dense
    const int32_t *inst;        // [N][H][W]
    const hvn_inst_rec *rec;    // [N][max_inst]
    int32_t *out;               // [N][max_inst][HVN_TEX_WORDS]; every word is written
    int N, H, W, max_inst;
    int fixed;                  // 0: levels over the nucleus's own grey range; 1: over 0..255
    int merge;                  // 0: one LDS add per pair; 1: equal keys are merged on chip before the LDS add (the same numbers, slower)
};
int hvn_launch_inst_texture(const InstTextureArgs &a, hipStream_t stream);

struct WinoArgs {
    const float *x;       // WINO_IN: input view; WINO_OUT: M [n*n][tiles][C] per sample (n = m + 4)
    long xsn, xsy, xsx;
    float *y;             // WINO_IN: V [n*n][tiles][C] per sample; WINO_OUT: output view
    long ysn, ysy, ysx;
    const float *mat;     // B^T (n x n) or A^T (m x n)
    const float *bias;    // WINO_OUT only
    int N, H, W, C;       // WINO_IN: input window extent / channels; WINO_OUT: output extent / cout
    int ty, tx, pad, relu;
    int m;                // output tile edge: 2 or 4
    int r;                // filter edge: 5 or 3 (n = m + r - 1)
    int accum;            // WINO_OUT: y += result (data gradients accumulate)
    const float *lo;      // WINO_IN, optional: the input is nearest2x(lo) + x (net_utils.py:284-294 UpSample2x + the skip add), formed on
    long lsn, lsy, lsx;   // the fly: lo is the half-resolution view, x the full-resolution skip; nullptr = plain input
};
int hvn_launch_wino_in(const WinoArgs &a, hipStream_t stream);
int hvn_launch_wino_out(const WinoArgs &a, hipStream_t stream);

// ---- training step (hvn_train.hip) -------------------------------------------------------------
struct PackArgs {
    const float *src;     // parameter layout [cout][kh*kw][cin_g]
    float *dst;
    int cout, cin_g, groups, taps;
    int mode;             // 0 forward [lead_pad][cin/32][taps][32]; 1 dgrad [lead_pad][cout/32][taps][32] (transposed, taps flipped); 2 conv0
    int lead_pad;         // padded leading dimension (multiple of the conv kernel's column tile)
    const float *gmat;    // modes 3 / 4 (Winograd F(4x4,5x5) transforms U = G g G^T, forward / data-gradient): G [8][5]
};
int hvn_launch_pack_w(const PackArgs &a, hipStream_t stream);
// every mode 0 / 1 / 2 packing of a step in one launch: device table + first workgroup of each packing (first_block[n] = grid size)
int hvn_launch_pack_w_multi(const PackArgs *tbl, const int *first_block, int n, long blocks, hipStream_t stream);

struct WgradArgs {
    const float *x;       // conv input view
    long xsn, xsy, xsx;
    int H, W, Cin;
    const float *dy;      // output-gradient view
    long dsn, dsy, dsx;
    int Ho, Wo, Cout;
    float *dw;            // [Cout][KH*KW][Cin_g], accumulated with atomics
    int N, KH, KW, stride, pad_t, pad_l, groups, Cin_g;
    int tiles_m, tiles_n;
    unsigned rows_per_split;
    int nbatch;           // > 1: blockIdx.z selects one of nbatch independent problems
    long xb, db, wb;      // element strides of x, dy, dw between them
    int want_wgs;         // workgroups the K split aims at (0: the default)
    // deterministic reduce (hvn_run_train_plan_ws): split s of the pixel sum STORES its tile into copy s of the gradient tensor in
    // `part` (part_stride floats per copy, part_cap floats in all) and hvn_launch_reduce_parts adds the copies to dw in split order
    float *part;
    long part_stride, part_cap;
};
int hvn_launch_wgrad(const WgradArgs &a, hipStream_t stream);
// the K split both weight-gradient launchers make: -> number of splits, *rows_per_split (a multiple of 32)
long hvn_wgrad_split(const WgradArgs &a, long tiles, unsigned *rows_per_split);
// floats of `part` a launch of this shape needs (0: a single split, which needs none)
long hvn_wgrad_part_floats(const WgradArgs &a, int x3);
// dst[e] += part[0][e] + part[1][e] + ... in a fixed order (4 interleaved chains of ascending s, then chain 0 + 1 + 2 + 3)
int hvn_launch_reduce_parts(float *dst, const float *part, long elems, long nparts, long stride, hipStream_t stream);
// the same sum with its products on the bf16 matrix pipe from bf16x3 splits of both operands (hvn_wgrad_x3.hip): 128 x 128 channel tiles
int hvn_wgrad_x3_supported(const WgradArgs &a);
int hvn_launch_wgrad_x3(WgradArgs a, int terms, hipStream_t stream);
int hvn_launch_wino_dy(const struct WinoArgs &a, hipStream_t stream);
int hvn_launch_wino_dw(const float *du, float *dg, const float *gmat, int cout, int cin, hipStream_t stream);

#define HVN_BN_MAX_PARTS 256
struct BnArgs {
    const float *z;       // conv output (pre-normalisation)
    long zsn, zsy, zsx;
    const float *a;       // backward: the forward output relu(bn(z)) -- NOT READ since round 6 (the ReLU mask is recomputed from z, save[0..2C))
    float *a_out;         // forward: where it is written
    long asn, asy, asx;
    const float *da;      // backward: gradient of a
    long gsn, gsy, gsx;
    float *dz;            // backward: gradient of z (accumulated), may be null
    long dsn, dsy, dsx;
    double *ws;           // [HVN_BN_MAX_PARTS][2*C] partial sums (no initialisation needed)
    float *save;          // [4*C] scale, shift, mean, rstd
    float *coef;          // [3*C] backward coefficients
    const float *gamma, *beta;
    float *dgamma, *dbeta, *running_mean, *running_var;
    int N, H, W, C, lq, nparts;
    float eps, momentum;
    int dz_store;         // backward: dz = ... instead of dz += ... (the caller knows this launch is the first writer of dz in the step)
};
int hvn_launch_bn_forward(BnArgs a, hipStream_t stream);
int hvn_launch_bn_backward(BnArgs a, hipStream_t stream);

struct UpAddBwdArgs {
    const float *dy;
    long ysn, ysy, ysx;
    float *dlo;           // may be null
    long lsn, lsy, lsx;
    float *dskip;         // may be null
    long ssn, ssy, ssx;
    int N, H, W, C;       // extent of dy
};
int hvn_launch_upadd_bwd(const UpAddBwdArgs &a, hipStream_t stream);

struct HeadBwdArgs {
    const float *x;       // head input a [N][H][W][64] view
    long xsn, xsy, xsx;
    float *dx;            // its gradient (accumulated)
    long dsn, dsy, dsx;
    const float *dl;      // logit gradient NCHW [N][Cout][H][W]
    const float *w;       // [Cout][64]
    float *dw, *db;
    int N, H, W, Cout;
    float *part;          // deterministic reduce: [workgroups][Cout * 64 + Cout] partial sums (NULL: fp32 atomics)
    long part_cap;
};
int hvn_launch_head_bwd(const HeadBwdArgs &a, hipStream_t stream);
long hvn_head_bwd_part_floats(const HeadBwdArgs &a);

struct Conv0WgradArgs {
    const uint8_t *img;
    long isn, isy, isx;
    int H, W;
    const float *dy;
    long ysn, ysy, ysx;
    float *dw;            // [64][7][7][3]
    int N, Ho, Wo, pad;
    float *part;          // deterministic reduce: [workgroups][64 * 147] partial sums (NULL: fp32 atomics)
    long part_cap;
};
int hvn_launch_conv0_wgrad(const Conv0WgradArgs &a, hipStream_t stream);
long hvn_conv0_wgrad_part_floats(const Conv0WgradArgs &a);

struct LossArgs {
    const float *l_np, *l_hv, *l_tp;   // NCHW logits
    const int32_t *t_np, *t_tp;        // [N][H][W]
    const float *t_hv;                 // [N][H][W][2]
    float *d_np, *d_hv, *d_tp;         // logit gradients (stage 1)
    double *sums;                      // [64]
    float *gws;                        // [N][H][W][2] focus-weighted Sobel differences
    int N, H, W, T;
    double m_total;
    float wt[6];                       // np bce, np dice, hv mse, hv msge, tp bce, tp dice
    double *parts;                     // deterministic reduce: [workgroups][64] per-workgroup sums (NULL: double atomics into sums)
    long parts_cap;                    // doubles
};
long hvn_loss_part_doubles(int n, int h, int w);
int hvn_launch_loss(const LossArgs &a, int stage, hipStream_t stream);
int hvn_launch_adam(float *w, const float *g, float *m, float *v, long n, float b1, float b2, float eps, float step_size,
                    float inv_bc2_sqrt, hipStream_t stream);

int hvn_internal_run_one(const hvn_op *op, int batch, hipStream_t s);

// ---- validation statistics (hvn_valid.hip) ------------------------------------------------------
size_t hvn_valid_ws_bytes(long pixels);
int hvn_launch_valid_stats(const float *pred, const int32_t *np_map, const float *hv_map, const int32_t *tp_map, long pixels, int c, int nr_types,
                           long long *counts, double *hv_sse, void *ws, size_t ws_bytes, hipStream_t stream);

// ---- training targets (hvn_targets.hip) ---------------------------------------------------------
int hvn_launch_aug_shape(const uint8_t *img, const int32_t *ann, int h, int w, int c, const struct hvn_aug_sample *prm, int n, int oh, int ow,
                         uint8_t *oimg, int32_t *oann, hipStream_t stream);
int hvn_launch_aug_shape_images(const uint8_t *pix, const int32_t *ann, const struct hvn_image_rec *images, const struct hvn_patch_rec *patches,
                                int n_images, int n_patches, long total_pixels, int win_h, int win_w, int c, const struct hvn_aug_sample *prm, int n,
                                int oh, int ow, uint8_t *oimg, int32_t *oann, int32_t *status, hipStream_t stream);
int hvn_launch_aug_input(const uint8_t *src, const struct hvn_aug_sample *prm, const float *noise, int n, int h, int w, uint8_t *dst, hipStream_t stream);
size_t hvn_targets_ws_bytes(int n, int h, int w);
int hvn_launch_gen_targets(const int32_t *ann, int n, int h, int w, int ch, int cw, float *hv, int32_t *np_map, void *ws, size_t ws_bytes,
                           hipStream_t stream);

/*
 * hvn.h -- C ABI of libhvn_hip.so, the MI355X (gfx950) HoVer-Net hot path.
 *
 * The reference (vqdang/hover_net) is pure Python and has no FFI; its boundary for
 * this path is three duck-typed callables looked up by module name
 * (/root/reference/infer/base.py:56-78).  Each entry point below names the
 * reference interface it stands behind.  All pointers marked `dev` are device (HBM)
 * addresses owned by the caller; `stream` is a hipStream_t passed as void*; every
 * function returns 0 on success or a negative hvn_status and never throws.  One host
 * thread per stream.  See INTEGRATION.md for the ctypes binding.
 */
#ifndef HVN_H
#define HVN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVN_API __attribute__((visibility("default")))

typedef enum hvn_status {
    HVN_OK = 0,
    HVN_E_ARG = -1,      /* malformed descriptor (alignment, channel multiple, kind) */
    HVN_E_LAUNCH = -2,   /* hipLaunch / hipGetLastError failure */
    HVN_E_NOGPU = -3,    /* no gfx950 device visible */
    HVN_E_SIZE = -4      /* workspace too small */
} hvn_status;            /* every nonzero status comes with a text: hvn_last_error() */

/* Strided view: element (n,y,x,c) lives at base[n*sn + y*sy + x*sx + c*sc].  Every kernel but
 * CONV0 requires channels-last (sc = 1; 0 is read as 1). */
typedef struct hvn_view {
    void   *base;        /* dev */
    int64_t sn, sy, sx;  /* strides in elements */
    int32_t h, w, c;     /* window extent */
    int32_t sc;          /* channel stride in elements (CONV0 input only, e.g. h*w for NCHW) */
} hvn_view;

enum { HVN_OP_CONV0 = 1, HVN_OP_CONV = 2, HVN_OP_UPADD = 3, HVN_OP_HEAD = 4, HVN_OP_PREDMAP = 5, HVN_OP_WINO_IN = 6, HVN_OP_WINO_OUT = 7, HVN_OP_CHAIN = 8, HVN_OP_VIEW = 9, HVN_OP_TTA = 10,
       HVN_OP_STAIN_HIST = 11, HVN_OP_STAIN_COMPACT = 12, HVN_OP_STAIN_APPLY = 13, HVN_OP_NBR_GRID = 14, HVN_OP_NBR_QUERY = 15,
       HVN_OP_NBR_CLUSTER = 16, HVN_OP_NBR_DENSITY = 17, HVN_OP_NBR_PAIRS = 18, HVN_OP_NBR_REGIONS = 19,
       HVN_OP_NBR_PAIRS_SIM = 20, HVN_OP_NBR_MARGINS = 21, HVN_OP_NBR_GRAPH = 22,
       HVN_OP_NBR_FOREST = 23, HVN_OP_INST_TEXTURE = 24 };

#define HVN_TEX_LEVELS 8     /* grey levels of HVN_OP_INST_TEXTURE */
#define HVN_TEX_WORDS 276    /* int32 words per record slot of its output: 12 + HVN_TEX_LEVELS + 4 * HVN_TEX_LEVELS^2 */

/*
 * One fused launch of the network plan (hover_net_amd/plan.py lowers
 * /root/reference/models/hovernet/net_desc.py:101-145 to an array of these).
 *   CONV0   x = image, uint8 (x_dtype 0; infer_step hands NHWC bytes) or float32 0..255 (x_dtype 1;
 *           HoVerNet.forward's NCHW contract), w = [kh][kw][3][64] taps (1/255 and BN folded), bias, relu
 *   CONV    y = epi( conv( pro(x) ) ):  pro = relu(x*pre_scale+pre_shift) if pre_scale,
 *           w = [cout_pad][x.c/32][kh*kw][32] fp32 (cout_pad = multiple of tile_n; reduction order =
 *           32-channel slab, tap, channel); groups = 4 declares the block-diagonal packing of a grouped
 *           conv with 32 input / 8 output channels per group (dense-unit conv2, net_utils.py:114-125):
 *           the kernel then multiplies each slab only against its own group's output columns;
 *           x2 (1x1 convs): a second input tensor whose channels are appended to the reduction, read at
 *           (oy*s2, ox*s2) with s2 = `_rsv` -- y = W1.x + W2.x2 fuses a residual block's strided 1x1 shortcut
 *           (net_utils.py:229-230) into its first conv3, the weight rows being [x.c | x2.c] wide,
 *           epi = (+bias) (relu) (+res) (relu(.*post_scale+post_shift) if post_scale)
 *           nbatch > 1: `nbatch` independent problems in one launch; problem b reads x.base + b*batch_stride[0],
 *           w + b*batch_stride[1] and writes y.base + b*batch_stride[2] (elements) -- the n*n transform-domain
 *           products of a Winograd convolution,
 *   WINO_IN  Winograd F(m x m, r x r) input transform of a stride-1 conv: F(2,5) / F(4,5) for the 5x5 decoder convs
 *           (net_desc.py:45,52,59 conva), F(4,3) for the encoder's 3x3 convs (net_utils.py:186-196), n = m + r - 1:
 *           x = input view (zero padding pad_t/pad_l), y = V as [n*n][tiles][c] per sample (y.w = tiles),
 *           kh x kw = tile grid, w = B^T (n x n), stride = m, _rsv = r (both 0: r = 5 and m from y.h = 36 | 64),
 *           res (optional): a half-resolution view; the transformed input is then nearest2x(res) + x, i.e. the UpSample2x + skip add
 *           of net_utils.py:284-294 / net_desc.py:133-143 formed on the fly (x = the skip), bit-identical to UPADD followed by WINO_IN,
 *   WINO_OUT y = A^T M A (+bias)(relu): x = M as [n*n][tiles][cout] per sample, w = A^T (m x n), kh x kw = tile grid
 *           covering y (a partial last tile's surplus outputs are dropped); res = y: accumulate (y += ...),
 *   CHAIN   two chained 1x1 convs of a residual block (net_utils.py:250-266) in one launch, the second running on the first's
 *           output while it is still on chip:   y  = post( W.x (+ W'.x2) + res )      -- a unit's conv3 (+ fused shortcut), `cout` channels,
 *                                               y2 = relu( W2.a + bias2 ), a = relu(y*pre_scale+pre_shift) if pre_scale else y
 *           -- the next unit's pre-activation + conv1 (+ folded BN), `cout2` in {64, 128} channels; w / w2 packed like CONV
 *           ([cout_pad][(x.c + x2.c)/32][1][32] and [cout2_pad][cout/32][1][32]); NOTE pre_scale / pre_shift act on y here, not on x;
 *           res (optional, may alias y) must have y's strides; x.c + x2.c >= 64, cout % 64 == 0.  Bit-identical to the two CONV
 *           launches it replaces.  act_dtype 2 | 3: both GEMMs form their products on the bf16 matrix pipe from bf16x3 splits
 *           (csrc/hvn_conv_chain_x3.hip): w / w2 then hold the bf16 planes of the fp32 packings ([rows][k-step][3][32] bf16, see
 *           act_dtype below), 128 pixels per workgroup; bit-identical to the two CONV launches with the same act_dtype.  tile_n = 128 + 0x400
 *           (1152) of such a CHAIN selects the form with conv3's input tile resident in registers and every other operand a chunk
 *           ahead in flight (csrc/hvn_conv_chain_x3r.hip: x.c = 64, and x2.c = 64 with cout2 = 64 and no res; same bits; HVN_E_ARG otherwise).
 *   UPADD   y = nearest2x(x) + res
 *   HEAD    y.base = NCHW logits [n][cout][h][w];  w = [cout][64], bias[cout]
 *   PREDMAP y.base = [n][h][w][3|4] = [argmax(tp)?, softmax(np)[1], hv0, hv1]
 *           (run_desc.py:185-194); x.base = np logits, res.base = hv logits, w = tp logits or NULL,
 *           cout = nr_types (0 if none)
 *   VIEW    test-time augmentation (hover_net_amd/tta.py): y = view_k(x) on uint8 [n][h][w][3] patches (x_dtype 0 only), k = `_rsv` =
 *           r + 4 f in 0..7: view_k(a) = rot90(fliplr(a) if f else a, r) -- the left-right flip first, then r counter-clockwise quarter
 *           turns.  x and y have the same extents (c = 3) and are different buffers; odd r needs x.h == x.w; strides in bytes,
 *           sy / sn = 0: dense rows / samples; HVN_E_ARG otherwise
 *   TTA     PREDMAP for the logits of ONE view, folded into an accumulator: operands as PREDMAP (x.base = np logits, res.base = hv
 *           logits, w = tp logits or NULL, cout = nr_types, all in the view's orientation; y.h x y.w = the map in the ORIGINAL
 *           orientation, needed on every view), `_rsv` = view id k, y2.base = fp32 accumulator [n][h][w][3 + nr_types] = (p_np, h, v,
 *           p_0 ..), kh != 0: first view (the term is stored, else acc + term), kw != 0: last view, which also writes
 *           y.base = [n][h][w][3|4] = [first maximum of the mean type probabilities?, acc / K] with K = `stride` >= 1 (IEEE division).
 *           Per original pixel (i, j) the logits are read where view_k sends (i, j); p_np = softmax(np)[1] in PREDMAP's form,
 *           p_t = exp(l_t - m) / sum_j exp(l_j - m) (j ascending), (h, v) = M_k^T (h_k, v_k) with M_k = R^r F^f, F = diag(-1, 1),
 *           R = [[0, 1], [-1, 0]].  Sums run in call order, without atomics: the hv channels equal the same fp32 sum bit for bit, and
 *           one view (k = 0, K = 1) gives PREDMAP's np and hv bits.  HVN_E_ARG: k outside 0..7, h != w with odd r, no accumulator, a
 *           last view without y or with K < 1, y not 16-byte aligned (with types)
 *   STAIN_HIST / STAIN_COMPACT / STAIN_APPLY   Macenko stain normalisation (hover_net_amd/stain.py holds the definition; csrc/hvn_stain.hip).
 *           Never part of a plan.  Images are uint8 [n][h][w][3] (x_dtype 0 only, c = 3), strides in BYTES as VIEW (sy / sn = 0: dense
 *           rows / samples; sx 0 | 3), h * w <= 2^30, n <= 65535.  A refusal launches nothing and leaves every output untouched.
 *     STAIN_HIST     adds the pixels of x to the colour histogram y.base = uint32 [1 << 24], bin = r << 16 | g << 8 | b (4-byte aligned; the
 *           call ADDS: the caller clears the table, or lets STAIN_COMPACT do it, and bounds the pixels added to one table by 2^32 - 1);
 *           res.base = optional uint8 mask, dense [n][h][w]: non-zero = count the pixel, NULL = all.  Integer atomics only: the table is
 *           a function of the inputs alone.  No other field is read.
 *     STAIN_COMPACT  (batch must be 1) x.base = the bins (16-byte aligned); y.base = uint32 [cap][2] list (8-byte aligned), cap = y.h in
 *           [1, 2^24]: the non-empty bins as (key, count) pairs in ascending key order -- np.unique(return_counts=True) of the keys; a
 *           table of more non-empty bins than cap gives the first cap pairs; y2.base = int64 status [2] = { non-empty bins (the TRUE
 *           number, also past cap), pixels counted } (8-byte aligned); x2.base = 65536 bytes of device workspace (8-byte aligned);
 *           `_rsv` != 0: every non-empty bin read is also stored back as 0 (past cap too), which leaves the whole table clear for the
 *           next image.  The list's layout is a function of the bins alone.  HVN_E_SIZE: cap outside [1, 2^24].
 *     STAIN_APPLY    y = the normalised x: x and y have the same extents; y may be the very view x is (same base and strides: in place),
 *           any other overlap of the two is refused; w = float64 tables T[3][3][256] on the device (8-byte aligned; read as doubles
 *           whatever the pointer's declared type), T[c][k][v] = exp(-M[c][k] * od[v]) as stain.tables makes them.  Per channel c of a
 *           pixel (r, g, b): t = ((240.0 * T[c][0][r]) * T[c][1][g]) * T[c][2][b] in float64, multiplied in that order, and the byte is
 *           (uint8) (t < 255 ? t : 255), truncating (NaN and +inf give 255; entries are expected non-negative).  Only multiplications:
 *           equal to stain.apply_host bit for bit.
 *           HVN_E_ARG: a null pointer (the mask excepted), c != 3, x_dtype != 0, h or w < 1, a stride shorter than a row or a sample,
 *           a misaligned table / list / status / workspace, n > 65535, x and y of different extents or partly overlapping.
 *           HVN_E_SIZE: h * w > 2^30.
 *   NBR_GRID / NBR_QUERY   fixed-radius neighbours of N points (hover_net_amd/neighbours.py holds the definition; csrc/hvn_neighbours.hip).
 *           Never part of a plan; batch must be 1.  Shared by both: x.h = N in [1, 2^26]; kh x kw = ncy x ncx grid cells, each in
 *           [1, 4096], at most 2^22 in all; w = float64 table {x0, y0, c, r2} on the device (8-byte aligned; read as doubles whatever
 *           the pointer's declared type): the grid's origin, its cell side and the squared radius; x2.base = device workspace (8-byte
 *           aligned) of x2.sn BYTES >= 24 N + 4 (2 ncy ncx + 1) + 4096.  The cell of (x, y) is (floor((y - y0) / c), floor((x - x0) / c)),
 *           each clamped into the grid after the conversion (NaN -> 0): no input value indexes outside the workspace.  The caller chooses
 *           c so that two points with d2 <= r2 are at most one cell apart per axis (neighbours.grid: c = r (1 + 2^-20), wider where
 *           the caps demand it); the library does not check that.  A refusal launches nothing and leaves every output untouched.
 *     NBR_GRID       x.base = float64 [N][2] = (x, y) (8-byte aligned); res.base = int32 types [N] (4-byte aligned) or NULL = all 0.  Fills
 *           the workspace: cell_start [ncy ncx + 1] (integer atomics, then an exclusive scan) and the points' x, y, type and position in
 *           cell order.  The order inside a cell depends on atomic arrival.  No other field is read.
 *     NBR_QUERY      reads the workspace as NBR_GRID left it for the same N, kh, kw and table (x.base is not read); cout = T in 1..16,
 *           `_rsv` = k in 1..16; y.base = int32 count [N][T], y2.base = int32 knn [N][k], res.base = int32 nearest_of_type [N][T]
 *           (4-byte aligned).  With dx = xj - xi, dy = yj - yi, d2 = (dx * dx) + (dy * dy) in float64, one rounding per operation and
 *           no fused multiply-add, j is a neighbour of i when j != i and d2 <= r2: count[i][t] = neighbours of type t, knn[i] = the
 *           first k neighbours in ascending (d2, j), padded with -1, nearest[i][t] = the (d2, j)-smallest neighbour of type t or -1;
 *           i and j are positions in x.  A type outside [0, T) is counted in no column and still takes part in knn.  Integer sums and
 *           minima under a total order: the outputs are a function of the inputs alone, not of the order inside a cell.  Loops are
 *           bounded by cell_start values clamped to [0, N] and every output row by N: a workspace NBR_GRID did not fill gives wrong
 *           numbers, no access outside the arrays.
 *           HVN_E_ARG: a null pointer (types excepted), xy / table / workspace not 8-byte or an int32 array not 4-byte aligned, batch
 *           != 1, N < 1, k or T outside 1..16, kh or kw < 1.  HVN_E_SIZE: N > 2^26, kh or kw > 4096 or kh * kw > 2^22, x2.sn too small.
 *     NBR_CLUSTER    DBSCAN clusters over the same grid (hover_net_amd/clusters.py holds the definition; csrc/hvn_clusters.hip).  Runs
 *           after NBR_GRID on the same stream and reads the workspace as that op left it for the same N, kh, kw and table (x.base is
 *           not read); x.h, kh, kw, w, x2.base and x2.sn are the shared fields above.  cout = min_pts in [1, 2^26]; groups = the type
 *           mask: bit t selects type t, -1 selects every point whatever its type, and with any other mask a type outside [0, 16) is
 *           unselected; y.base = int32 label [N], y2.base = int32 degree [N] (4-byte aligned); res.base = a second device workspace of
 *           the op's own (8-byte aligned) of res.sn BYTES >= 12 N: per slot of the cell order the union-find parent, the smallest
 *           position among a root's cores and the degree (int32 [N] each).  The op writes every word of it that it reads: its content
 *           before the call does not matter.  With the neighbour relation of NBR_QUERY (d2 <= r2): degree[i] = 1 + the number of
 *           selected neighbours of a selected i, 0 for an unselected i; i is a core when degree[i] >= min_pts; a cluster is a connected
 *           component of the cores and label = the smallest position among them; a selected non-core with a core neighbour takes the
 *           label of its (d2, j)-smallest core neighbour j; every other point gets -1.  Integer sums, set unions and minima under a
 *           total order: the outputs are a function of the inputs alone.  No loop waits for another thread: a find steps only to a
 *           strictly smaller slot, a failed hook is retried only on a strictly smaller value, candidate loops are bounded by
 *           cell_start values clamped to [0, N] and every output row by N: a workspace NBR_GRID did not fill gives wrong numbers, no
 *           access outside the arrays and no loop without an end.
 *           HVN_E_ARG: a null pointer, label / degree not 4-byte or a table / workspace not 8-byte aligned, batch != 1, N < 1,
 *           min_pts < 1, a mask of 0, kh or kw < 1.  HVN_E_SIZE: min_pts > 2^26, N > 2^26, kh or kw > 4096 or kh * kw > 2^22, x2.sn
 *           or res.sn too small.
 *     NBR_DENSITY    typed counts within the radius of every NODE of a regular raster, over the same grid (hover_net_amd/density.py holds
 *           the definition; csrc/hvn_density.hip).  Runs after NBR_GRID on the same stream and reads the workspace as that op left it
 *           for the same N, kh, kw and table (x.base is not read); x.h, kh, kw, w, x2.base and x2.sn are the shared fields above.
 *           cout = T in 1..16; y.base = int32 count [T][H][W], contiguous (4-byte aligned), y.h = H and y.w = W, each in [1, 16384],
 *           T H W <= 2^28; bias = float64 table {ox, oy, s} on the device (8-byte aligned; read as doubles whatever the pointer's
 *           declared type, as w is).  Node (u, v) lies at px = ox + (u * s), py = oy + (v * s), computed in the kernel, never stored;
 *           with dx = xj - px, dy = yj - py, d2 = (dx * dx) + (dy * dy) in float64, one rounding per operation and no fused
 *           multiply-add, count[t][v][u] = the number of points j of type t with d2 <= r2.  A point exactly on a node counts (no j != i
 *           here: nodes are not points); a type outside [0, T) is counted in no plane.  A node's cell comes from NBR_GRID's formula and
 *           clamp, so nodes may lie anywhere, also far outside the points' extent.  EVERY element of count is written, whatever it held
 *           before: the caller clears nothing.  No atomics on the output, integer sums: a function of the inputs alone.  Loops are
 *           bounded by cell_start values clamped to [0, N] and by the grid's rows: a workspace NBR_GRID did not fill gives wrong
 *           numbers, no access outside the arrays and no loop without an end.
 *           HVN_E_ARG: a null pointer, count not 4-byte or a table / workspace not 8-byte aligned, batch != 1, N < 1, T outside
 *           1..16, H or W < 1, kh or kw < 1.  HVN_E_SIZE: H or W > 16384, T H W > 2^28, N > 2^26, kh or kw > 4096 or kh * kw > 2^22,
 *           x2.sn too small.
 *     NBR_PAIRS      typed pair counts by distance bin over the same grid: the integers under Ripley's cross-type K function
 *           (hover_net_amd/ripley.py holds the definition; csrc/hvn_pairs.hip).  Runs after NBR_GRID on the same stream and reads the
 *           workspace as that op left it for the same N, kh, kw and table (x.base is not read); x.h, kh, kw, w, x2.base and x2.sn are
 *           the shared fields above, and table[3] is r2 of the LARGEST radius.  cout = T in 1..16, `_rsv` = R in 1..32, T T R <= 4096;
 *           y.base = int64 acc [2][T][T][R], contiguous (8-byte aligned); bias = float64 table {wx0, wy0, wx1, wy1, r_0 .. r_{R-1},
 *           r2_0 .. r2_{R-1}} of 4 + 2 R doubles on the device (8-byte aligned; read as doubles whatever the pointer's declared type, as
 *           w is): the window, the ascending radii and their squares r2_k = r_k * r_k as the caller rounded them.  With d2 as in
 *           NBR_QUERY, kmin = the smallest k with d2 <= r2_k (none: the pair is not counted), b_i = min(x_i - wx0, wx1 - x_i, y_i -
 *           wy0, wy1 - y_i), each term one subtraction, and m_i = the number of k with r_k <= b_i, every ordered pair (i, j), j != i,
 *           of types (a, b) adds 1 to acc[0][a][b][kmin] and, only if kmin < m_i, 1 to acc[1][a][b][kmin] and -1 to acc[1][a][b][m_i]
 *           (the latter where m_i < R).  The running sums over the last axis are the pair counts within r_k, of all i (plane 0) and of
 *           the i that lie at least r_k inside the window (plane 1, the border method).  A type outside [0, T) lands in no bin, as i or
 *           as j.  EVERY element of acc is written, whatever it held before: the op clears it itself, in stream order.  Integer sums
 *           (32-bit in LDS, flushed into 64-bit global atomics before a word could pass 2^23): a function of the inputs alone.  Loops
 *           are bounded by cell_start values clamped to [0, N]: a workspace NBR_GRID did not fill gives wrong numbers, no access
 *           outside the arrays and no loop without an end.
 *           HVN_E_ARG: a null pointer, acc or a table / workspace not 8-byte aligned, batch != 1, N < 1, T outside 1..16, R outside
 *           1..32, kh or kw < 1.  HVN_E_SIZE: T T R > 4096, N > 2^26, kh or kw > 4096 or kh * kw > 2^22, x2.sn too small.
 *     NBR_REGIONS    exact point-in-polygon of the points against the canonical edges of G annotated regions: which regions hold which
 *           point, and the typed counts per region (hover_net_amd/regions.py holds the definition; csrc/hvn_regions.hip).  Runs after
 *           NBR_GRID on the same stream and reads the workspace as that op left it for the same N, kh, kw and table (x.base is not read;
 *           table[3] is not read either); x.h, kh, kw, w, x2.base and x2.sn are the shared fields above.  The extra tables take fields the
 *           family leaves free: cout = T in 1..16; `_rsv` = G in 1..4096; bias = float64 edges [E][4] = (ax, ay, bx, by) with ay < by on
 *           the device (8-byte aligned; read as doubles whatever the pointer's declared type, as w is); res.base = int32 edge_region [E]
 *           (4-byte aligned), ascending, and res.h = E in 1..2^22; y2.base = int32 rows (4-byte aligned): row_start [kh + 1] followed by
 *           the edge numbers of the row lists, and y2.sn = M, the lists' total length, in 1..8 E + kh: the edges of grid row k are
 *           rows[kh + 1 + j] for row_start[k] <= j < row_start[k + 1], and the caller lists an edge in every row from that of ay to that
 *           of by (NBR_GRID's row formula, which is monotone; an edge that no point can cross may be left out), the edges of one region
 *           adjacent and the regions ascending (the library
 *           does not check that); y.base = int32 out [2 N + G T], contiguous (4-byte aligned): first [N], hits [N], count [G][T].
 *           Point (px, py) crosses an edge when ay <= py, py < by and (px - ax) * (by - ay) < (bx - ax) * (py - ay), in float64, one
 *           rounding per operation, no fused multiply-add, the two products compared; it is inside region g when it crosses an odd
 *           number of g's edges.  first[i] = the smallest g with point i inside or -1, hits[i] = the number of such g, count[g][t] =
 *           the points of type t inside g; i is a position in NBR_GRID's x.  A type outside [0, T) is counted nowhere and the point
 *           still gets first / hits; a region id outside [0, G) is counted nowhere.  EVERY element of out is written, whatever it held
 *           before: the op clears count itself, in stream order.  Integer sums (wave ballots, summed per workgroup, global atomics): a function of the inputs
 *           alone.  Row starts are clamped to [0, M], edge numbers to [0, E), the walk of a workgroup's rows ends after 256 rounds:
 *           tables or a workspace the caller did not fill give wrong numbers, no access outside the arrays and no loop without an end.
 *           HVN_E_ARG: a null pointer, out / edge_region / rows not 4-byte or edges / table / workspace not 8-byte aligned, batch != 1,
 *           N < 1, T outside 1..16, G < 1, E < 1, M < 1, kh or kw < 1.  HVN_E_SIZE: G > 4096, E > 2^22, M > 8 E + kh, N > 2^26, kh or
 *           kw > 4096 or kh * kw > 2^22, x2.sn too small.
 *     NBR_MARGINS    the points by distance to the BOUNDARY of G annotated regions, in B bands: per point the nearest region within the
 *           largest width, the squared distance and the side; per (region, side, band, type) the ring counts (hover_net_amd/margins.py
 *           holds the definition; csrc/hvn_margins.hip).  Runs after NBR_GRID on the same stream and reads the workspace as that op left
 *           it for the same N, kh, kw and table (x.base is not read; table[3] is not read either); x.h, kh, kw, w, x2.base and x2.sn are
 *           the shared fields above.  The extra tables take fields the family leaves free: cout = T in 1..16; `_rsv` = G in 1..4096;
 *           cout2 = B in 1..16; w2 = float64 squared widths [B], ascending, on the device (8-byte aligned; read as doubles whatever the
 *           pointer's declared type, as w is); bias = float64 segments [S][8] on the device (8-byte aligned; read as doubles likewise):
 *           (ax, ay, bx, by) with (ay, ax) <= (by, bx), EVERY ring edge, horizontal ones included, then the segment's box (x0, y0, x1,
 *           y1) = (min(ax, bx) - W, ay - W, max(ax, bx) + W, by + W) as the caller rounded it, W the largest width; res.base = int32
 *           seg_region [S] (4-byte aligned), ascending, and res.h = S in 1..2^22; y2.base = int32 rows (4-byte aligned): row_start
 *           [kh + 1] followed by the segment numbers of the row lists, and y2.sn = M, the lists' total length, in 0..8 S + kh: the
 *           segments of grid row k are rows[kh + 1 + j] for row_start[k] <= j < row_start[k + 1], and the caller lists a segment in
 *           every row from that of y0 to that of y1 of its box (NBR_GRID's row formula, which is monotone; a segment that no point can be
 *           near or cross may be left out), the segments of one region adjacent and the regions ascending (the library does not check
 *           that); y.base = the output (8-byte aligned) of y.sn BYTES >= 16 N + 8 G B T: float64 near_d2 [N], then int32 near [N],
 *           near_inside [N], hist [G][2][B][T].  Point (px, py) crosses a segment by NBR_REGIONS' rule and is inside region g when it
 *           crosses an odd number of g's segments.  It is in a segment's box when x0 <= px <= x1 and y0 <= py <= y1; then, in float64,
 *           one rounding per operation, no fused multiply-add, with ux = bx - ax, uy = by - ay, vx = px - ax, vy = py - ay, dot =
 *           ux * vx + uy * vy, len2 = ux * ux + uy * uy: d2 = vx * vx + vy * vy if dot <= 0, (px - bx) * (px - bx) + (py - by) * (py -
 *           by) if dot >= len2, else (c * c) / len2 with c = ux * vy - uy * vx; the segment is near the point when d2 <= w2[B - 1], and
 *           dmin2(i, g) is the smallest d2 over g's segments near point i.  near[i] = the g with the smallest dmin2, ties to the smallest
 *           g, or -1; near_d2[i] = that dmin2 or +inf; near_inside[i] = 1 | 0 for that region or -1; hist[g][side][k][t] = the points of
 *           type t, inside (side 1) or outside (side 0) g, for which k is the smallest index with dmin2 <= w2[k] (the RING counts: the
 *           caller forms running sums over k); i is a position in NBR_GRID's x.  A type outside [0, T) is counted nowhere and the point
 *           still gets near; a region id outside [0, G) is committed nowhere.  EVERY element of the output is written, whatever it held
 *           before: the op clears hist itself, in stream order.  M = 0 is run like any other list: all -1 / +inf / 0.  stride != 0
 *           selects the kernel form that does not cull the staged segments by x (the same numbers; tools/margins_bench.py times the
 *           two against each other).  Integer sums and
 *           minima under a total order (a 32-bit LDS histogram per region run, flushed into global atomics): a function of the inputs
 *           alone.  Row starts are clamped to [0, M], segment numbers to [0, S), the walk of a workgroup's rows ends after 256 rounds:
 *           tables or a workspace the caller did not fill give wrong numbers, no access outside the arrays and no loop without an end.
 *           HVN_E_ARG: a null pointer, seg_region / rows not 4-byte or segments / widths / out / table / workspace not 8-byte aligned,
 *           batch != 1, N < 1, B or T outside 1..16, G < 1, S < 1, M < 0, kh or kw < 1.  HVN_E_SIZE: G > 4096, S > 2^22, M > 8 S + kh,
 *           y.sn too small, N > 2^26, kh or kw > 4096 or kh * kw > 2^22, x2.sn too small.
 *     NBR_PAIRS_SIM  the border-corrected counts of NBR_PAIRS under a BATCH of SB random relabellings of the points: the integers behind
 *           the random-labelling envelopes of Ripley's cross-type K (hover_net_amd/ripley.py holds the definition, `sims_host`;
 *           csrc/hvn_pairs_sim.hip).  Runs after NBR_GRID on the same stream and reads the workspace as that op left it for the same N,
 *           kh, kw and table (x.base is not read); x.h, kh, kw, w, x2.base and x2.sn are the shared fields above, table[3] is r2 of
 *           the LARGEST radius, and cout = T, `_rsv` = R and bias = the window and radius table are those of NBR_PAIRS.  The rest takes
 *           fields the family leaves free: nbatch = SB in 1..32 with 4 SB T T R + 5120 ceil(SB / 4) <= 143360, the bytes of LDS that a
 *           workgroup's SB histograms and staged labels take; res.base = the int32 types [N] in ORIGINAL order, as NBR_GRID's (4-byte
 *           aligned) or NULL = all 0; w2 = uint64 round keys [SB][8] on the device (8-byte aligned; read as 64-bit integers whatever the
 *           pointer's declared type), formed by the caller; y2.base = a label workspace of the op's own (4-byte aligned) of y2.sn
 *           BYTES >= 4 N ceil(SB / 4), which is at least N SB: per slot one byte per simulation in words of four.  The op writes every
 *           word of it that it reads.  y.base = int64 out [SB][T T R + T (R + 1)], contiguous (8-byte aligned): per simulation
 *           acc [T][T][R], then cnt [T][R + 1].  Simulation s labels the point at position p with types[pi_s(p)], where pi_s(p) is the
 *           first of F_s(p), F_s(F_s(p)), .. below N and F_s is the Feistel bijection of [0, 2^b), b = max(2, bit_length(N - 1)),
 *           hl = b / 2 low and hh = b - hl high bits, of eight rounds: hi ^= mix(lo + key[s][r]) & (2^hh - 1) for even r, lo ^=
 *           mix(hi + key[s][r]) & (2^hl - 1) for odd r, mix the splitmix64 finaliser, uint64 with wrap-around.  The walk ends after at
 *           most 2^b - N + 1 steps and the loop is bounded by that count.  With kmin and m_i as in NBR_PAIRS, every ordered pair (i, j),
 *           j != i, with kmin < m_i and labels (a, b) in simulation s adds 1 to acc[s][a][b][kmin] and -1 to acc[s][a][b][m_i] (the
 *           latter where m_i < R): plane 1 of NBR_PAIRS, whose running sum over the last axis the caller forms; every point i adds 1
 *           to cnt[s][a][m_i], and the points of type a at least r_k inside the window are the sum of cnt[s][a][m] over m > k.  A type
 *           outside [0, T) lands in no bin, as i or as j, wherever the permutation puts it.  The geometry of a pair is tested once for
 *           the whole batch.  EVERY element of out is written, whatever it held before: the op clears it itself, in stream order.
 *           stride = 0 is that op; 1 and 2 are its two halves, so that they can be timed apart (tools/ripley_sims_bench.py): 1 clears
 *           out and makes the labels and cnt only, 2 only adds the pairs into out, from the labels as the workspace holds them.
 *           Integer sums (signed 32-bit in LDS, flushed into 64-bit global atomics before a word could pass 2^23 in magnitude): a
 *           function of the inputs alone.  Loops are bounded by cell_start values clamped to [0, N], by SB and by the walk's count, and
 *           a position read from the workspace is clamped to [0, N): a workspace NBR_GRID did not fill gives wrong numbers, no access
 *           outside the arrays and no loop without an end.
 *           HVN_E_ARG: a null pointer (types excepted), out / keys / a table / workspace not 8-byte or types / labels not 4-byte
 *           aligned, batch != 1, N < 1, T outside 1..16, R outside 1..32, SB outside 1..32, stride outside 0..2, kh or kw < 1.  HVN_E_SIZE: T T R > 4096,
 *           the histograms and labels above 143360 bytes of LDS, y2.sn too small, N > 2^26, kh or kw > 4096 or kh * kw > 2^22, x2.sn
 *           too small.
 *     NBR_GRAPH      the cell graph of the points: the Gabriel edges of length <= r, as a CSR graph in two passes of one op
 *           (hover_net_amd/graph.py holds the definition; csrc/hvn_graph.hip).  Runs after NBR_GRID on the same stream and reads the
 *           workspace as that op left it for the same N, kh, kw and table (x.base is not read); x.h, kh, kw, w, x2.base and x2.sn are
 *           the shared fields above.  With the neighbour relation of NBR_QUERY (j != i and d2 <= r2) and dot(i, j, k) = ((xi - xk) *
 *           (xj - xk)) + ((yi - yk) * (yj - yk)) in float64, one rounding per operation and no fused multiply-add: k blocks (i, j)
 *           when k != i, k != j, k is a neighbour of i AND of j and dot(i, j, k) < 0; (i, j) is an edge when j is a neighbour of i and
 *           no k blocks it.  The relation is symmetric.  `_rsv` = the mode.  0, COUNT: y.base = int32 degree [N] (4-byte aligned),
 *           degree[i] = the number of edges of i, i a position in NBR_GRID's x; y.sn is not read; y2.base = NULL, or an int32 table
 *           first [N][W] (4-byte aligned) with W = `stride` in 1..64 (not read without the table): the positions of the first
 *           min(degree[i], W) graph neighbours of i that the kernel finds go to first[i][0 ..), the rest of the row is left as it
 *           was; a caller whose largest degree is at most W has the whole graph after this pass.  1, FILL: y2.base = int64
 *           indptr [N + 1] (8-byte aligned), the exclusive running sum of degree that the caller formed; y.base = int32 indices [E]
 *           (4-byte aligned) and y.sn = E in [1, 2^31): the positions of i's graph neighbours are written to indices[indptr[i] ..
 *           indptr[i + 1]); `stride` is not read.  Rows of the table and of indices are in NO particular order (the caller sorts a
 *           row; graph.py orders it by (d2, j)), so that no output depends on the order of the points inside a cell.  There is no cap
 *           on a degree or on the size of a neighbourhood: a wave keeps up to 512 neighbours of its point in LDS, and above that a
 *           slower path walks the candidate runs in global memory and gives the same integers.  Loops are bounded by cell_start
 *           values clamped to [0, N]; a point whose position in the workspace is outside [0, N) writes nothing; every store of the
 *           fill pass is bounded by its row's own end and by E, every store into the table by its row's W slots: a workspace NBR_GRID
 *           did not fill or an indptr that is not the count pass's gives wrong numbers, no access outside the arrays and no loop
 *           without an end.
 *           HVN_E_ARG: `_rsv` outside 0..1, a null pointer (degree in count; indices or indptr in fill), a table with W outside
 *           1..64, E < 1 in fill, degree / indices / the table not 4-byte or indptr / the grid's table / workspace not 8-byte
 *           aligned, batch != 1, N < 1, kh or kw < 1.  HVN_E_SIZE: E >= 2^31, N > 2^26, kh or kw > 4096 or kh * kw > 2^22, x2.sn
 *           too small.
 *     NBR_FOREST     the minimum spanning forest and the connected components of a symmetric CSR graph over the points, by Boruvka
 *           rounds (hover_net_amd/forest.py holds the definition; csrc/hvn_forest.hip).  It needs no grid and does not read NBR_GRID's
 *           workspace: x.base = float64 [N][2] = (x, y) by position (8-byte aligned), x.h = N in [1, 2^26]; w = int64 indptr [N + 1]
 *           on the device (8-byte aligned; read as 64-bit integers whatever the pointer's declared type); res.base = int32 indices [E]
 *           (4-byte aligned) and res.sn = E in [0, 2^31), NULL iff E = 0: the graph as NBR_GRAPH's caller holds it, rows in any order,
 *           symmetric, without self-loops and without a position twice in a row (the library does not check that); y.base = int32
 *           component [N] (4-byte aligned); y2.base = uint8 tree [E], NULL iff E = 0; x2.base = a workspace of the op's own (8-byte
 *           aligned) of x2.sn BYTES >= 28 N + 256.  The op writes every word of it that it reads.  The key of an undirected edge {i, j}
 *           is (d2(i, j), min(i, j), max(i, j)), compared lexicographically, d2 as NBR_QUERY forms it; {i, j} is in the forest when its
 *           ends are not connected by edges of strictly smaller key.  tree[e] = 1 for BOTH directed entries of a forest edge and 0 for
 *           every other entry; component[i] = the smallest position in i's connected component.  EVERY element of both is written,
 *           whatever it held before.  The int32 at byte 28 N + 128 of the workspace holds the number of rounds that joined anything.
 *           `_rsv` = 0 is that op, in stream order and without a readback: max(1, ceil(log2 N)) rounds of four launches, of which those
 *           after a round that joined nothing return at once.  1, 2 and 3 are its parts, so that they can be timed apart and a caller can
 *           read the workspace between them (tools/forest_bench.py): 1 the start, 2 the one round `stride` in 0..25 (the int32 at byte
 *           28 N + 4 stride of the workspace then counts what that round joined), 3 the end.  cout != 0 selects the kernel form whose
 *           atomic minima are not preceded by a read of the word (the same numbers).  kh, kw and every other field are not read.
 *           Integer minima under a strict total order: a function of the inputs alone.  Every indptr value is clamped into [0, E], an
 *           indices entry outside [0, N) is skipped, the walks are bounded by a row's length, by N and by the number of rounds: a graph
 *           that is not symmetric gives wrong numbers, no access outside the arrays and no loop without an end.
 *           HVN_E_ARG: `_rsv` outside 0..3, `stride` outside 0..25 with `_rsv` = 2, a null pointer (xy, indptr, component, the workspace;
 *           indices or tree with E > 0), N < 1, E < 0, batch != 1, xy / indptr / workspace not 8-byte or indices / component not 4-byte
 *           aligned.  HVN_E_SIZE: N > 2^26, E >= 2^31, x2.sn too small.
 *   INST_TEXTURE   per-nucleus grey-level co-occurrence counts: the integers under the chromatin texture features (hover_net_amd/texture.py
 *           holds the definition; csrc/hvn_texture.hip).  Never part of a plan; the third pass over a label map, next to
 *           hvn_instance_table and hvn_instance_features, whose inputs it reuses.  batch = n maps; x = the image view, uint8
 *           [n][h][w][3] RGB (x_dtype 0, c = 3, x.h = h, x.w = w), dense: strides in BYTES as VIEW, each 0 or the dense value (sx 0 | 3,
 *           sy 0 | 3 w, sn 0 | 3 h w); res.base = inst, int32 [n][h][w] (4-byte aligned); w = the records, hvn_inst_rec
 *           [n][max_inst] as hvn_instance_table left them (8-byte aligned; read as records whatever the pointer's declared type);
 *           cout = max_inst; y.base = the output, int32 [n][max_inst][HVN_TEX_WORDS] (8-byte aligned); `_rsv` = the scale mode, 0
 *           "range" | 1 "fixed"; `stride` = the accumulation form, 0 = one LDS add per pair, 1 = equal keys merged on chip before the
 *           LDS add (the same numbers, slower; tools/texture_bench.py times the two against each other).  No other field is read.
 *           The mask of a label is inst == label INSIDE the record's bbox clamped to the map, as in hvn_instance_features: any label
 *           map is valid, and a stale or foreign table cannot make the kernel read outside the map.  The grey value of a pixel is
 *           g = (77 R + 150 G + 29 B + 128) >> 8, its level q = ((g - lo) * 8) / span, span = hi - lo + 1, in 0..7, with (lo, hi) =
 *           the smallest and largest grey value of the mask in mode 0 and (0, 255) in mode 1.  The offsets (dx, dy), y down, are
 *           d = 0: (1, 0), 1: (1, 1), 2: (0, 1), 3: (-1, 1); glcm[d][a][b] = the mask pixels p of level a whose neighbour p + offset_d
 *           is a mask pixel of the same label and has level b: ORDERED pairs, not symmetrised, every unordered pair once.  A slot, in
 *           int32 words (slot j describes label j + 1, parallel to the records): 0..7 gsum = int64 [4], the sums of g, g^2, g^3, g^4
 *           over the mask (255^4 (2^31 - 1) < 2^63); 8 seen = the mask pixels found (== rec.area for a table made from this map);
 *           9, 10 = the nucleus's OWN smallest and largest grey value in BOTH modes (the mode only decides whether the level formula
 *           uses them or 0 and 255; both 0 when seen = 0); 11 = 0; 12..19 hist[8] = the mask pixels per level; 20..275 glcm[4][8][8].
 *           A slot with area <= 0 or an empty clamped bbox is 276 zero words.  EVERY word of every slot is written, whatever it held
 *           before: the caller clears nothing.  One wave per slot, the counts in a per-wave LDS block, no global atomics, no
 *           workspace, integer sums: a function of the inputs alone.  Every loop is bounded by the map extent.  A refusal launches
 *           nothing and leaves the output untouched.
 *           HVN_E_ARG: a null image, inst, records or output; n (batch), h, w or max_inst < 1; h * w >= 2^31; an image view that is
 *           not c = 3 uint8, or not dense; a scale mode other than 0 or 1; an accumulation form other than 0 or 1; output or records
 *           not 8-byte, inst not 4-byte aligned.  HVN_E_SIZE: n * max_inst >= 2^31.
 */
typedef struct hvn_op {
    int32_t kind, kh, kw, stride, pad_t, pad_l, relu, cout, tile_n, x_dtype, groups, _rsv;
    hvn_view x, res, y;
    hvn_view x2;         /* CONV, 1x1 only: optional second input (base NULL = none), sampled with spatial stride `_rsv` */
    const float *w, *bias, *pre_scale, *pre_shift, *post_scale, *post_shift; /* dev */
    int64_t batch_stride[3]; /* CONV with nbatch > 1: element strides of x, w, y between problems */
    int32_t nbatch;
    int32_t act_dtype;   /* 0: fp32 activations / weights; 1: bf16 activations (x, res, y, x2) and packed weights
                            ([cout_pad][ceil(x.c/64)][kh*kw][64] bf16, zero-filled past x.c), fp32 accumulation, fp32 bias /
                            scales; CONV0 (bf16 output), CONV, UPADD, HEAD (bf16 input, fp32 logits) honour it.
                            CONV only -- 2 | 3: fp32 activations, accumulation and outputs exactly as 0, but the products run on the
                            bf16 matrix pipe from exact three-way bf16 splits of the fp32 operands (csrc/hvn_conv_x3.hip): `w` then
                            holds the three bf16 planes of the fp32 packing, [cout_pad][k-step][3][32] bf16 (k-step = (x.c/32 slab,
                            tap), the fp32 packing's order) and batch_stride[1] counts bf16 elements; 2 = all nine partial
                            products (the fp32 dot product in another summation order), 3 = the six that carry more than 2^-24
                            of a product.  tile_n of such a CONV: 128 | 64 = 128 pixels x tile_n channels per workgroup
                            (hvn_conv_x3.hip); 128 + 0x300 (896) | 128 + 0x200 (640) = 256 | 128 pixels x 128 channels with both operands
                            staged by LDS-DMA (csrc/hvn_conv_x3g.hip; cout >= 128; same bits as the other forms); a CONV with act_dtype 1
                            takes the same two codes for the LDS-DMA form of the bf16 convolution (csrc/hvn_conv_bf16g.hip: no
                            prologue, cout >= 128, same bits as tile_n 128) */
    /* CHAIN only: the second conv's output view, packed weights, bias (or NULL) and channel count */
    hvn_view y2;
    const float *w2, *bias2; /* dev */
    int32_t cout2, _rsv2;
} hvn_op;

/* -- library ---------------------------------------------------------------------- */
HVN_API int         hvn_version(void);
HVN_API const char *hvn_build_id(void);   /* id of the sources the binary was compiled from; the Python binding refuses a stale library */
/* Text of the most recent call on this thread that returned a nonzero status, whichever entry point it was; it leads with that entry
 * point's name without hvn_ ("postproc: ..."; an op of a plan: "train op 7: wgrad: ...").  Every failing path writes it, so it never
 * repeats an earlier failure; a successful call leaves it alone. */
HVN_API const char *hvn_last_error(void);
HVN_API int         hvn_device_ok(void);  /* 1 if a gfx950 device is current */

/* -- network: HoVerNet.forward (net_desc.py:101-145) + infer_step epilogue (run_desc.py:171-197) */
HVN_API int hvn_run_plan(const hvn_op *ops, int n_ops, int batch, void *stream);
/* single launches, used by the per-kernel parity tests */
HVN_API int hvn_run_op(const hvn_op *op, int batch, void *stream);
/* per-launch timing of the CONV kernel: hvn_profile_enable(1) resets the tally and brackets every
 * CONV launch of the following hvn_run_plan / hvn_run_op calls with hipEvents on their stream;
 * hvn_profile_conv_ms() synchronises and returns the summed milliseconds (<0 if nothing was recorded) */
HVN_API int    hvn_profile_enable(int on);
HVN_API double hvn_profile_conv_ms(void);
HVN_API int    hvn_profile_conv_launches(void);
/* the same measurements one by one, in launch order: fills out[0..min(cap, launches)) and returns that count */
HVN_API int    hvn_profile_conv_ms_list(double *out, int cap);

/* -- patch extraction: infer/tile.py:46-94 _prepare_patching (numpy "reflect" padding) + dataloader/infer_loader.py:59-72
 * img: dev uint8 [h][w][3] (the UNPADDED source image); coords: dev int32 [n_patches][2] = (y, x) top-left corners in the
 * padded frame (patch_info[:, :2]); out: dev uint8 [n_patches][win][win][3]; pad_t / pad_l = (win - step) / 2. */
HVN_API int hvn_extract_patches(const uint8_t *img, int h, int w, const int32_t *coords, int n_patches, int win,
                                int pad_t, int pad_l, uint8_t *out, void *stream);

/* -- instance separation: post_proc.py:26-90 __proc_np_hv ---------------------------- */
/* bytes of device workspace needed for `n` maps of h x w */
HVN_API size_t hvn_postproc_workspace_bytes(int n, int h, int w);
/* pred: dev float32 [n][h][w][c] with [p, h, v] at channels c0..c0+2 (c0 = 1 when a type
 * channel leads, post_proc.py:109-114); inst: dev int32 [n][h][w].  Labels equal the
 * reference's (scipy raster-order numbering of the marker components). */
HVN_API int hvn_postproc(const float *pred, int n, int h, int w, int c, int c0,
                         int32_t *inst, void *workspace, size_t workspace_bytes, void *stream);
/* stage taps for tests (any may be NULL): blb int32, dist float64 (negated blur), marker int32 */
HVN_API int hvn_postproc_taps(const float *pred, int n, int h, int w, int c, int c0, int32_t *inst,
                              int32_t *blb, double *dist, int32_t *marker,
                              void *workspace, size_t workspace_bytes, void *stream);
/* which replay the marker-controlled watershed (post_proc.py:88) of the LAST hvn_postproc call on `workspace` took, summed over its
 * n maps (waits for `stream`): out[0] components that hold a marker, out[1] replayed on the small LDS window, out[2] on the bitmap
 * window, out[3] on the HBM window, out[4] handed to the one-lane heap by a mixed-label marker tie, out[5] by a full frontier,
 * out[6] component heap replays, out[7] WHOLE-TILE replays (a tie the component replay could not prove harmless), out[8] maps
 * flagged with such a tie, out[9] largest component bounding box. */
HVN_API int hvn_postproc_stats(const void *workspace, size_t workspace_bytes, int n, int h, int w, long long out[10], void *stream);

/* -- per-instance table: post_proc.py:119-181 process() (bbox, centroid, type vote) ----- */
typedef struct hvn_inst_rec {
    int32_t label;              /* value in the inst map */
    int32_t area;
    int32_t rmin, rmax, cmin, cmax; /* get_bounding_box semantics (misc/utils.py:18-28): max is exclusive */
    double  sum_x, sum_y;       /* cv2.moments m10, m01 over the bbox crop (offsets re-added): centroid = sum/area */
    int32_t type;               /* majority type, runner-up if 0 (post_proc.py:170-177); -1 if no type channel */
    int32_t type_count;         /* pixels of that type: type_prob = type_count / (area + 1e-6) */
} hvn_inst_rec;
/* records: dev [n][max_inst], slot j describes label j+1 (area 0 = label absent; labels above
 * max_inst are ignored); counts: dev int32 [n] = number of labels present; pred may be NULL when
 * nr_types == 0, else its channel 0 is the type map (post_proc.py:109-112). */
HVN_API size_t hvn_instance_table_workspace_bytes(int n, int max_inst, int nr_types);
HVN_API int hvn_instance_table(const int32_t *inst, const float *pred, int n, int h, int w, int c,
                               int nr_types, hvn_inst_rec *records, int32_t *counts, int max_inst,
                               void *workspace, size_t workspace_bytes, void *stream);

/* -- per-instance morphometric sums (csrc/hvn_features.hip): what regionprops-style shape and stain features are made of, as exact
 * integers; hover_net_amd/features.py derives the float features (axes, eccentricity, orientation, perimeter, circularity, mean and
 * std colour) on the host.  The mask of a label is inst == label INSIDE the record's bbox clamped to the map (for a table made
 * from this map: the whole label); everything else, other labels and the outside of the map included, is background.  Any label
 * map is valid (labels of several pieces, holes, other labels inside the bbox).
 * per[]: scikit-image's 4-neighbourhood perimeter estimator without floats.  A mask pixel is a border pixel when one of its
 * 4-neighbours is not in the mask; with n4 / nd = its 4- / diagonal neighbours that are border pixels of the same label,
 * per[0] counts (n4, nd) in {(2,0),(3,0),(2,1),(3,1),(2,2),(3,2)}, per[1] {(0,2),(1,3)}, per[2] {(1,1),(1,2)}; every other
 * combination counts nowhere.  perimeter = per[0] + per[1] * sqrt(2) + per[2] * (1 + sqrt(2)) / 2. */
typedef struct hvn_inst_feat {           /* slot j describes label j+1, parallel to hvn_inst_rec */
    int64_t sxx, syy, sxy;               /* sums of (x-cmin)^2, (y-rmin)^2, (x-cmin)(y-rmin) over the label's pixels */
    int32_t seen;                        /* pixels == label found inside the record's bbox (== rec.area for a table made from this map) */
    int32_t per[3];                      /* border-pixel class counts */
    int64_t csum[3], csq[3];             /* sums of c, c^2 per RGB channel over the label's pixels; 0 when image == NULL */
} hvn_inst_feat;
/* All pointers are device pointers; everything is enqueued on `stream`, nothing is allocated or synchronised.  inst: int32
 * [n][h][w]; image: uint8 [n][h][w][3] or NULL; records: hvn_instance_table's [n][max_inst]; feats: [n][max_inst], 8-byte
 * aligned.  A slot with area <= 0 (or a bbox that misses the map) gets an all-zero record; a stale or foreign table cannot make
 * the kernel read outside the map (the bbox is clamped) and shows as seen != area.  The workspace size is 0 (workspace may be
 * NULL).  HVN_E_ARG: a null pointer (image and workspace excepted), n, h, w or max_inst < 1, h * w >= 2^31, a misaligned pointer.
 * HVN_E_SIZE: n * max_inst >= 2^31. */
HVN_API size_t hvn_instance_features_workspace_bytes(int n, int h, int w, int max_inst);   /* may return 0 */
HVN_API int hvn_instance_features(const int32_t *inst, const uint8_t *image, int n, int h, int w, const hvn_inst_rec *records,
                                  int max_inst, hvn_inst_feat *feats, void *workspace, size_t workspace_bytes, void *stream);

/* -- instance-segmentation metrics: the exact integer tables behind metrics/stats_utils.py (get_fast_pq, get_fast_aji,
 * get_fast_aji_plus, get_dice_1, get_fast_dice_2, get_dice_2, remap_label); hover_net_amd/metrics.py does the float arithmetic.
 * All maps: dev int32 [n][h][w], h * w <= 2^30, n <= 65535.
 * Pair table: every distinct (t, p, count) over the pixels whose pair (true, pred) is not (0, 0), labels >= 0 and otherwise
 * arbitrary; triples: dev int32 [n][h * w][3], image i's first counts[i] rows in no canonical order; counts: dev int32 [n]. */
HVN_API size_t hvn_pair_table_workspace_bytes(int n, int h, int w);
HVN_API int hvn_pair_table(const int32_t *true_map, const int32_t *pred_map, int n, int h, int w, int32_t *triples, int32_t *counts,
                           void *workspace, size_t workspace_bytes, void *stream);
/* range: dev int32 [n][2] = (smallest, largest) label of each map. */
HVN_API int hvn_label_range(const int32_t *map, int n, int h, int w, int32_t *range, void *stream);
/* remap_label(by_size=False): out = 0 where map <= 0 or > max_id, else 1 + the number of distinct labels of the image in
 * (0, label); n_ids: dev int32 [n] = distinct labels in [1, max_id] per image.  out may alias map.  Workspace: two bits per
 * label value in [0, max_id] per image (512 MB per image at max_id = INT32_MAX). */
HVN_API size_t hvn_remap_label_workspace_bytes(int n, int h, int w, int32_t max_id);
HVN_API int hvn_remap_label(const int32_t *map, int n, int h, int w, int32_t max_id, int32_t *out, int32_t *n_ids, void *workspace,
                            size_t workspace_bytes, void *stream);
/* areas: dev int32 [n][max_label + 1] = pixels of each label in [0, max_label] (others are not counted). */
HVN_API int hvn_label_areas(const int32_t *map, int n, int h, int w, int32_t max_label, int32_t *areas, void *stream);
/* map = perm[image][map] in place where 0 <= map <= max_label; perm: dev int32 [n][max_label + 1]. */
HVN_API int hvn_label_permute(int32_t *map, int n, int h, int w, int32_t max_label, const int32_t *perm, void *stream);

/* -- whole-slide merge: infer/wsi.py:569-599 post_proc_normal_tile_callback, :602-677 post_proc_fixing_tile_callback and :51-60
 * _remove_inst on a DEVICE-resident int32 instance map [H][map_w] (tiles strictly in the reference's order: the id offset is the
 * running maximum id and the fix-up windows overlap).  pred_inst: dev int32 [h][w] local ids of the tile at (y0, x0).
 * normal:  window = pred_inst (+ off where > 0).
 * fixing:  old ids wholly inside the window (np.unique(roi)[1:] minus np.unique(edge)[1:] -- "[1:]" drops the smallest value as the
 *          reference does) are zeroed and listed in `removed` (count in counters[0]; counters[1] / [2] = smallest value on the window
 *          edge / in the window, counters[3] = smallest value of pred_inst: np.unique(pred_inst)[1:] drops it too); touching[i] = 1 for new ids i <= n_local that overlap a kept old instance (they are dropped); the
 *          other new ids are written with + off.  id_flags: dev int32 [2][cap] epoch-stamped tables (zeroed once; cap > every id in
 *          the map), epoch > 0 and increasing from call to call; removed: dev [removed_cap]; counters: dev [5] (counters[4] = window pixels whose id is >= cap, i.e. beyond the id tables: must be 0, the caller checks); touching: dev [n_local + 1]. */
HVN_API int hvn_wsi_merge_normal(int32_t *inst_map, int64_t map_w, int y0, int x0, int h, int w, const int32_t *pred_inst, int32_t off,
                                 void *stream);
HVN_API int hvn_wsi_merge_fixing(int32_t *inst_map, int64_t map_w, int y0, int x0, int h, int w, const int32_t *pred_inst, int32_t n_local,
                                 int32_t off, int32_t epoch, int32_t *id_flags, int64_t cap, int32_t *removed, int32_t removed_cap,
                                 int32_t *counters, uint8_t *touching, void *stream);

/* -- contours: cv2.findContours(crop, RETR_TREE, CHAIN_APPROX_SIMPLE)[0][0] of process() (post_proc.py:132-143)
 * HOST function (O(perimeter) per instance over its bbox crop): inst = host int32 [h][w]; recs = host records
 * (slots with area 0 are skipped); pts = host int32 [max_pts][2] as (x, y) in map coordinates;
 * offs = host int64 [n_rec + 1] prefix offsets into pts.  Returns the total number of points or <0. */
HVN_API long hvn_trace_contours(const int32_t *inst, int h, int w, const hvn_inst_rec *recs, int n_rec,
                                int32_t *pts, long max_pts, int64_t *offs);
/* DEVICE function, the batched form of the same arrays for maps in which EVERY LABEL IS ONE 8-CONNECTED PIECE (hvn_postproc's
 * output is; arbitrary maps go to hvn_trace_contours): then contours[0] is the outer border from the label's first raster pixel,
 * traced without marks in O(perimeter) steps, bit-equal to the host function (csrc/hvn_contour_dev.hip).  All pointers are device
 * pointers; everything is enqueued on `stream`, nothing is allocated or synchronised.  inst: int32 [n][h][w] (not written);
 * records: hvn_instance_table's [n][max_inst].  pts: int32 [max_pts][2] as (x, y) in map coordinates, 8-byte aligned;
 * offs: int64 [n * max_inst + 1]: the record at (map i, slot j) owns pts[offs[i * max_inst + j] : offs[i * max_inst + j + 1]],
 * slots in (map, slot) order (a prefix sum over the per-slot counts: the layout is a function of the input alone).
 * A record with area > 0 is FLAGGED and owns no points when its bbox is empty or leaves the map, row rmin holds no pixel of the
 * label inside the bbox, the walk exceeds 4 * area + 8 steps, or the walk's bounding box differs from the record's (a label of
 * several pieces -- unless a further piece lies inside the first piece's bbox, which is NOT detected -- or a stale table).
 * status: int32 [4] = { flagged records, 1 if offs[n * max_inst] > max_pts, smallest flagged i * max_inst + j or -1, 0 }.
 * offs is exact for all unflagged records even when status[1] is set; then the records whose range does not fit in max_pts are
 * not written and the caller sizes a second call from offs[n * max_inst]. */
HVN_API size_t hvn_contours_workspace_bytes(int n, int max_inst);
HVN_API int hvn_trace_contours_device(const int32_t *inst, int n, int h, int w, const hvn_inst_rec *records, int max_inst,
                                      int32_t *pts, int64_t max_pts, int64_t *offs, int32_t *status, void *workspace,
                                      size_t workspace_bytes, void *stream);

/* -- overlay: viz.visualize_instances_dict (closed contour polylines in the instance's colour, optional centroid dots) drawn on the
 * DEVICE, bit-equal to the host writer (csrc/hvn_overlay.hip).  All pointers are device pointers except dot_rgb (host, read during
 * the call); everything is enqueued on `stream`, nothing is allocated or synchronised.  image, overlay: uint8 [n][h][w][3], 4-byte
 * aligned; image == overlay (in place) is allowed.  pts: int32 [n_pts][2] as (x, y), 8-byte aligned, any int32 value (segments are
 * clipped pixel by pixel, at a cost bounded by the image size); offs: int64 [n * slots + 1], hvn_trace_contours_device's layout:
 * slot (i, j) of image i owns pts[offs[i * slots + j] : offs[i * slots + j + 1]] and is drawn into image i as the closed polyline
 * through its points (one point = one stamp, none = no contour), `thickness` (1..7) px wide: every pixel of a segment
 * (viz._segment_pixels) stamps the square of offsets -((thickness - 1) / 2) .. thickness / 2.  rgba: uint8 [n * slots][4] = r, g, b,
 * draw flag (0 = the slot draws nothing, neither contour nor dot).  centres: int32 [n * slots][2] as (x, y), 8-byte aligned: a
 * filled disc dx^2 + dy^2 <= dot_radius^2 (0..15) in dot_rgb per drawing slot; NULL = no dots.  Drawing order is the host's:
 * slot by slot, a slot's dot over its contour, later slots over earlier ones (an int32 owner map per pixel, largest key wins:
 * the result does not depend on scheduling).  A slot whose offs range is reversed or leaves [0, n_pts] draws nothing.
 * status: int32 [4] = { such slots, the smallest i * slots + j of them or -1, 0, 0 }.
 * HVN_E_SIZE: workspace smaller than hvn_overlay_workspace_bytes(n, h, w) (or not 16-byte aligned), thickness or dot_radius out of
 * range, n * slots >= 2^30 - 1 (the keys are int32). */
HVN_API size_t hvn_overlay_workspace_bytes(int n, int h, int w);
HVN_API int hvn_draw_overlay(const uint8_t *image, uint8_t *overlay, int n, int h, int w, const int32_t *pts, int64_t n_pts,
                             const int64_t *offs, int slots, const uint8_t *rgba, const int32_t *centres, int thickness,
                             int dot_radius, const uint8_t dot_rgb[3], int32_t *status, void *workspace, size_t workspace_bytes,
                             void *stream);

/* -- resample: one window of a slide resampled to the processing magnification (hover_net_amd/resample.py: OpenCV's scalar 8-bit
 * fixed-point resize restated, 11 coefficient bits), bit-equal to resample.resize_window_host (csrc/hvn_resample.hip).  All
 * pointers are device pointers; one launch on `stream`, nothing is allocated or synchronised; integer arithmetic only.
 * src: uint8 [src_h][src_w][3] with rows src_pitch bytes apart: the box of the FULL source [full_h][full_w] whose top-left is
 * (src_y0, src_x0).  dst: uint8 [dst_h][dst_w][3], contiguous, any alignment.  xofs int32 [dst_w], xcoef int16 [dst_w][taps],
 * yofs int32 [dst_h], ycoef int16 [dst_h][taps] (taps = 4 cubic | 2 linear): resample.axis_table's entries for the window's columns
 * and rows, ofs in FULL-source coordinates.  Tap k of an entry reads full-source index clamp(ofs + k - (taps == 4), 0, full - 1),
 * translated by the box origin.
 * The box must hold every such tap.  The tables are on the device, so the launcher cannot see their values: the CALLER checks the
 * taps of the first and last entries against the box before the call (resample.resize_window_device does), and the kernel clamps
 * the translated index into the box once more, so that no table makes a launch read outside src.
 * HVN_E_ARG: null or misaligned pointer, taps not 2 | 4, an empty extent, a row longer than 2^29 pixels, src_pitch < 3 * src_w, a box
 * that leaves the full source.  HVN_E_SIZE: dst_h > 16 * 65535. */
HVN_API int hvn_resize_window(const uint8_t *src, int src_h, int src_w, int64_t src_pitch, int src_y0, int src_x0, int full_h, int full_w,
                              const int32_t *xofs, const int16_t *xcoef, const int32_t *yofs, const int16_t *ycoef, int taps,
                              uint8_t *dst, int dst_h, int dst_w, void *stream);

/* -- tissue mask: the automatic mask of whole-slide mode (infer/wsi.py:486-500 simple_get_mask) on the device, bit-equal to
 * hover_net_amd/tissue_mask.py (csrc/hvn_tissue.hip).  All pointers are device pointers; everything is enqueued on `stream`, nothing
 * is allocated or synchronised; integer arithmetic and integer atomics only, so equal inputs give equal bytes.
 * hvn_tissue_gray_hist: rgb uint8 [h][w][3] -> gray uint8 [h][w] = (R*4899 + G*9617 + B*1868 + 8192) >> 14 and hist256, its 256
 * uint32 counters (cleared by the call).  The Otsu threshold is taken from the counters on the host (tissue_mask.otsu_from_hist).
 * hvn_tissue_mask: m0 = !(gray > threshold); objects = m0 without its 8-connected components of fewer than min_obj pixels; holes =
 * objects with every 4-connected component of its complement of fewer than max_hole pixels filled (border components included);
 * mask = holes dilated by the disk dy^2 + dx^2 <= radius^2.  mask, tap_objects, tap_holes: uint8 [h][w] of {0, 1}; the taps may be
 * NULL.  gray is only read; no two of the planes may overlap.
 * HVN_E_ARG: a null pointer (taps excepted), h or w < 1, radius outside [0, 32], a misaligned hist256 (4) or workspace (16).
 * HVN_E_SIZE: h * w > 2^30, workspace smaller than hvn_tissue_mask_workspace_bytes(h, w) (0 for an extent that is refused).
 * A refused call launches nothing and leaves its outputs untouched. */
HVN_API int hvn_tissue_gray_hist(const uint8_t *rgb, int h, int w, uint8_t *gray, uint32_t *hist256, void *stream);
HVN_API size_t hvn_tissue_mask_workspace_bytes(int h, int w);
HVN_API int hvn_tissue_mask(const uint8_t *gray, int h, int w, int threshold, int min_obj, int max_hole, int radius, uint8_t *mask,
                            uint8_t *tap_objects, uint8_t *tap_holes, void *workspace, size_t workspace_bytes, void *stream);

/* -- run-loop picture: models/hovernet/run_desc.py:201-256 viz_step_output on the device, bit-equal to hover_net_amd/viz.py
 * (csrc/hvn_viz.hip).  All pointers are device pointers; one launch on `stream`, nothing is allocated or synchronised; integer and
 * float32 work only, so equal inputs give equal bytes.
 * out is a strip of n_blocks blocks of 2h rows of ncol * w RGB pixels, ncol = 5 when nr_types > 0 and tp_map is not NULL (which
 * needs c == 4), else 4.  Each pair (sample, block) of `sel` draws one block: rows [2 * block * h, 2 * block * h + 2h), the truths
 * in the upper h rows and the predictions in the lower.  Column 0 of both is img[sample] cropped at (int((ih - h) * 0.5),
 * int((iw - w) * 0.5)); then np_map | p_nuc over 0..1, the two planes of hv_map | pred's h, v over -1..1, and tp_map | pred's
 * channel 0 over 0..nr_types.  A value v becomes lut[k], k = min(255, (int)(((clamp(v, vmin, vmax) - vmin) / (float)(vmax - vmin))
 * * 256)) with a correctly rounded float32 divide; NaN becomes (0, 0, 0).  Integer maps are converted to float32 first.
 * A pair whose sample is outside [0, n) or whose block is outside [0, n_blocks) draws nothing; bytes of out outside the named
 * blocks are never written; two pairs that name one block race (either may win, byte by byte).  n_sel == 0 launches nothing.
 * HVN_E_ARG (nothing launched, out untouched): a null pointer (tp_map excepted; sel only when n_sel > 0), n, h, w or n_blocks < 1,
 * n_sel < 0 or > 65535, ih < h, iw < w, c not 3 | 4, (nr_types > 0) != (c == 4), nr_types < 0 or > 16, a misaligned pred,
 * np_map, hv_map, tp_map or sel (4).  HVN_E_SIZE: 2h * 5w > 2^30. */
HVN_API int hvn_viz_strip(const uint8_t *img, int n, int ih, int iw, const float *pred, int c, const int32_t *np_map, const float *hv_map,
                          const int32_t *tp_map, int h, int w, int nr_types, const int32_t *sel, int n_sel, const uint8_t *lut,
                          uint8_t *out, int n_blocks, void *stream);


/* -- training step: run_desc.py:12-109 train_step (forward in train() mode, losses utils.py:54-172, backward, Adam) --
 * A training step is two hvn_top lists (forward, backward; hover_net_amd/train_plan.py lowers the network to them)
 * around the two loss stages.  Weights live in the parameter layout [cout][kh*kw][cin_g] (torch channels_last);
 * gradients are ACCUMULATED into their destinations (the caller zeroes the gradient arena once per step).
 *   NET          net = one forward-plan op (CONV0 / CONV / UPADD / HEAD); convolutions of the forward pass and the
 *                data gradients (stride-1 conv of the -- possibly dilated -- output gradient, res = y to accumulate)
 *   PACK_W       p[0] = weights, p[1] = packed copy for the conv kernel; mode 0 forward ([lead_pad][cin/32][taps][32],
 *                groups expanded block-diagonally), 1 data-gradient (transposed, taps flipped:
 *                [lead_pad][cout/32][taps][32]), 2 conv0 ([7][7][3][64] x 1/255); 3 / 4 Winograd F(4x4,5x5) transform
 *                U = G g G^T of a 5x5 conv for the forward / data-gradient pass ([64][lead_pad][k/32][32], p[2] = G
 *                [8][5]); cout, cin_g, groups, kh, kw
 *   BN_FWD       a = relu(batchnorm_train(z)): x = z, y = a; p[0] = double ws[256][2c] (scratch for the partial sums),
 *                p[1] = save[4c] (scale, shift, mean, rstd), p[2] = gamma, p[3] = beta, p[4] = running_mean,
 *                p[5] = running_var (updated: momentum, unbiased variance); eps, momentum
 *   BN_BWD       x = z, y = a (not read: the ReLU mask a > 0 is recomputed from z and save's scale / shift with the forward's own
 *                instruction), dy = grad a, dx = grad z (+=; mode & 1: = -- the caller knows this launch is the first writer of
 *                grad z in the step; base NULL: none); p[0] = ws, p[1] = save (as the BN_FWD of this step left it), p[2] = gamma,
 *                p[3] = grad gamma (+=), p[4] = grad beta (+=), p[5] = coef[3c] scratch
 *   WGRAD        p[0][cout][kh*kw][cin_g] += sum_pixels dy (x) x: x = conv input view, dy = output-gradient view;
 *                kh, kw, stride, pad_t, pad_l, groups; mode = workgroups the split of the pixel sum aims at (0: default;
 *                a tuning hint, the result is the same sum in another order); `_pad` = 6 | 9: the products run on the bf16 matrix
 *                pipe from exact three-way bf16 splits of both fp32 operands (csrc/hvn_wgrad_x3.hip; 9 = every partial product, 6 =
 *                those above 2^-24 of a product) where the shape has that form (ungrouped, cout >= 128, x.c % 128 == 0), 0 = fp32 pipe
 *   CONV0_WGRAD  x = uint8 image view, dy = grad of the conv0 output, p[0] = grad [64][7][7][3] (+=); pad_t
 *   UPADD_BWD    dy = grad of nearest2x(lo) + skip; dx = grad lo (+= 2x2 sums, nullable), y = grad skip (+=, nullable)
 *   HEAD_BWD     x = head input [h][w][64], dx = its grad (+=), p[0] = logit grad NCHW, p[1] = W [cout][64],
 *                p[2] = grad W (+=), p[3] = grad bias (+=); cout
 *   WGRAD with nbatch > 1: nbatch independent problems, problem b at x.base + b*batch_stride[0], dy.base +
 *                b*batch_stride[1], p[0] + b*batch_stride[2] (elements) -- the 64 transform positions of the
 *                Winograd-domain weight gradient of a 5x5 conv:
 *   WINO_DY      dM = A dY A^T per 4x4 tile of the output gradient: x = dy view, y = dM as [64][tiles][c] per sample,
 *                p[0] = A^T [4][8], kh x kw = tile grid
 *   WINO_DW      grad g [cout][25][cin] (p[1]) += G^T dU G of dU [64][cout][cin] (p[0]), p[2] = G [8][5]; cout, cin_g
 *   PACK_MULTI   every mode 0 / 1 / 2 PACK_W of a step in one launch: p[0] = dev table of hvn_pack_desc [cout], p[1] = dev int32
 *                [cout + 1] first workgroup (of 256 outputs) of each packing, batch_stride[0] = workgroups in total.  The table lives
 *                in device memory, so PACK_W's shape checks (cin % 32 / cout % 32, lead_pad >= rows, non-null pointers) cannot be
 *                made at the call: the CALLER makes them when it builds the table (train_engine._pack_ops raises on a bad entry)
 *   SPLIT_X3     p[0] = fp32 weight packings (batch_stride[0] granules of 32 floats, any concatenation of PACK_W outputs), p[1] = their
 *                three bf16 planes, [3][32] bf16 per granule: what a CONV with act_dtype 2 | 3 reads (the weights of a training step
 *                change every step, so the planes are made on the device after the PACK_W ops)
 * Extent rules (checked over the WHOLE list before its first op is launched: a list with a descriptor that breaks one, at any index,
 * is refused with HVN_E_ARG and the rule's own text and nothing runs; the kernels take N, H, W, C from ONE view and walk the others
 * with them):
 *   BN_FWD / BN_BWD  (h, w, c) come from x = z; y, and for BN_BWD dy and a non-NULL dx, must have exactly that (h, w, c).
 *                BN_FWD needs batch * h * w >= 2: the running variance is the unbiased one, which one value per channel does not
 *                have (torch.nn.BatchNorm2d raises for it in train() mode)
 *   UPADD_BWD    (h, w, c) come from dy, h and w even; a non-NULL dx must be (h / 2, w / 2, c), a non-NULL y (h, w, c); dx and y both
 *                NULL is refused (nothing to do)
 *   HEAD_BWD     (h, w) come from x (c = 64, h and w positive); dx must be (h, w, 64)
 */
enum { HVN_T_NET = 1, HVN_T_PACK_W = 2, HVN_T_BN_FWD = 3, HVN_T_BN_BWD = 4, HVN_T_WGRAD = 5, HVN_T_CONV0_WGRAD = 6,
       HVN_T_UPADD_BWD = 7, HVN_T_HEAD_BWD = 8, HVN_T_WINO_DY = 9, HVN_T_WINO_DW = 10, HVN_T_SPLIT_X3 = 11, HVN_T_PACK_MULTI = 12 };
typedef struct hvn_pack_desc {   /* one entry of PACK_MULTI's table = the fields of a PACK_W op */
    const float *src;            /* parameter [cout][kh*kw][cin_g] (dev) */
    float *dst;                  /* packing (dev) */
    int32_t cout, cin_g, groups, taps, mode, lead_pad;
    const float *gmat;           /* unused by modes 0 / 1 / 2 */
} hvn_pack_desc;
typedef struct hvn_top {
    int32_t kind, kh, kw, stride, pad_t, pad_l, groups, cout, cin_g, mode, lead_pad, _pad;
    hvn_view x, y, dx, dy;
    void *p[6];          /* dev */
    float eps, momentum;
    const hvn_op *net;   /* host */
    int64_t batch_stride[3]; /* WGRAD with nbatch > 1 */
    int32_t nbatch, _pad2;
} hvn_top;
HVN_API int hvn_run_train_plan(const hvn_top *ops, int n_ops, int batch, void *stream);
/* The same list with DETERMINISTIC cross-workgroup sums (reference: torch.use_deterministic_algorithms for run_desc.py:84-88's
 * loss.backward()).  hvn_run_train_plan ends WGRAD's split of the pixel sum, CONV0_WGRAD and HEAD_BWD in fp32 atomics, whose order the
 * hardware scheduler picks: the same step run twice differs in the last bits of its weight gradients.  With a workspace every such
 * workgroup STORES its partial tile into its own copy and a second launch adds the copies in a fixed order: bit-identical gradients
 * run to run (and box to box for equal `mode` hints).  workspace: dev, 16-byte aligned, >= hvn_train_workspace_bytes(ops, n_ops,
 * batch) bytes (HVN_E_SIZE otherwise), shared by all ops of the list (they run in stream order); NULL = hvn_run_train_plan. */
HVN_API int hvn_run_train_plan_ws(const hvn_top *ops, int n_ops, int batch, void *stream, void *workspace, size_t workspace_bytes);
HVN_API size_t hvn_train_workspace_bytes(const hvn_top *ops, int n_ops, int batch);
HVN_API const char *hvn_train_last_error(void);   /* = hvn_last_error(): an alias kept for existing callers */

/* Losses of run_desc.py:40-82 with opt.py:47-51 weights (np: bce + dice, hv: mse + msge, tp: bce + dice).
 * logits_* / grad_*: dev float32 NCHW [n][c][h][w] (c = 2, 2, nr_types); true_np / true_tp: dev int32 [n][h][w];
 * true_hv: dev float32 [n][h][w][2]; sums: dev double[64], zero before hvn_loss_forward, which adds this rank's
 * partial sums ([0] bce_np [1] bce_tp [2] mse [3] msge numerator [4] focus sum; [8+c] [10+c] [12+c] dice np
 * inse/l/r; [16+c] [32+c] [48+c] dice tp); the caller may SUM-all-reduce it over ranks, sets total_pixels to the
 * pixel count of the whole batch (all ranks), and hvn_loss_backward writes the logit gradients of this rank's
 * pixels.  sobel_ws: dev float32 [n][h][w][2] scratch carried from forward to backward. */
typedef struct hvn_loss {
    const float *logits_np, *logits_hv, *logits_tp;
    const int32_t *true_np, *true_tp;
    const float *true_hv;
    float *grad_np, *grad_hv, *grad_tp;
    double *sums;
    float *sobel_ws;
    int32_t n, h, w, nr_types;   /* nr_types = 0: no tp branch */
    double total_pixels;
    /* loss weights of run_desc.py:66-82 (`loss += loss_weight * term_loss`, table opt.py:47-51): np bce, np dice, hv mse,
     * hv msge, tp bce, tp dice; 0 = term absent from the table.  They scale the logit gradients (hvn_loss_backward); the
     * partial sums of hvn_loss_forward are the unweighted terms, which is what the reference tracks per term. */
    float weight[6];
    /* deterministic sums: dev double [partials_cap >= hvn_loss_partials_count(n, h, w)]; every workgroup of hvn_loss_forward stores
     * its 64 sums there and a second launch adds them to `sums` in a fixed order.  NULL: double atomics into `sums` (their order, and
     * with it the 16th digit of the sums, varies run to run). */
    double *partials;
    int64_t partials_cap;
} hvn_loss;
HVN_API int64_t hvn_loss_partials_count(int n, int h, int w);
HVN_API int hvn_loss_forward(const hvn_loss *l, void *stream);
HVN_API int hvn_loss_backward(const hvn_loss *l, void *stream);

/* Validation statistics: the scalar half of run_desc.py:262-333 proc_valid_step_output, accumulated on the device (added to the ABI
 * without a version step: hvn_version() stays 104, the binding resolves every export by name at load time).
 * pred: dev float32 [n][h][w][c], c = 3 | 4 = [type?, p_nuc, h, v] as PREDMAP writes it (16-byte aligned, read in place); np_map: dev
 * int32 [n][h][w]; hv_map: dev float32 [n][h][w][2]; tp_map: dev int32 [n][h][w] with c = 4 and 0 < nr_types <= 16, NULL with c = 3 and
 * nr_types = 0 (anything else is refused).  The call ADDS this batch to the caller's state, in stream order and with no host sync:
 *   counts: dev int64 [4 + 2 * nr_types] = pixels, np_correct (count of (p_nuc > 0.5) == np_map; exactly 0.5 and NaN are not nucleus),
 *           np_inter, np_total for label 1 (total = count(true == 1) + count(pred == 1)), then (tp_inter_t, tp_total_t) for t = 0 ..
 *           nr_types - 1: the float type channel compared to the integer label; a label no t equals is counted by nobody;
 *   hv_sse: dev float64 [1] += sum over both HV channels of (double(pred) - double(true))^2, each term a rounded product.
 * The counts are exact integers; the float64 sum is a fixed function of the inputs and the call sequence (a fixed tree per workgroup,
 * one partial per workgroup of 1024 pixels stored to the workspace, added in workgroup order; no atomics). */
HVN_API size_t hvn_valid_stats_workspace_bytes(int n, int h, int w);
HVN_API int hvn_valid_stats(const float *pred, const int32_t *np_map, const float *hv_map, const int32_t *tp_map, int n, int h, int w, int c,
                            int nr_types, int64_t *counts, double *hv_sse, void *workspace, size_t workspace_bytes, void *stream);

/* Training targets: models/hovernet/targets.py:100-116 gen_targets (gen_instance_hv_map :17-96 with fix_mirror_padding,
 * remove_small_objects(30) on the crop, the unclamped 2-px box widening and its skip-at-the-near-border consequence).
 * ann: dev int32 [n][h][w] instance ids (0 = background); hv_map: dev float32 [n][crop_h][crop_w][2] = (x, y) offsets in
 * [-1, 1]; np_map: dev int32 [n][crop_h][crop_w] in {0, 1}.  Bit-exact with the reference. */
HVN_API size_t hvn_gen_targets_workspace_bytes(int n, int h, int w);
HVN_API int hvn_gen_targets(const int32_t *ann, int n, int h, int w, int crop_h, int crop_w, float *hv_map, int32_t *np_map,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Training-time augmentation of a RESIDENT patch set: dataloader/train_loader.py:76-199 (FileLoader.__getitem__ + __get_augmentation)
 * and the image functions of dataloader/augs.py:36-113.  One record per OUTPUT sample, drawn on the host:
 *   shape part (image + annotation): out(y, x) = in[src](round_half_up(inv * (x', y', 1))) or 0 outside, where (x', y') is the
 *   output pixel after the flips, offset to the centre-crop window of the source patch (CropToFixedSize / cropping_center);
 *   input part (image only): kind 0 = cv2.GaussianBlur((p0, p1), 0) | 1 = cv2.medianBlur(p0) | 2 = additive Gaussian noise
 *   (noise_scale * z, z from the caller's N(0,1) buffer, one plane if !per_channel) | 3 = none; then order[0..3] in turn:
 *   0 = add_to_hue(hue), 1 = add_to_saturation(sat = 1 + draw), 2 = add_to_brightness(bright), 3 = add_to_contrast (returns its
 *   input unchanged in the reference, augs.py:96-97), < 0 = skip. */
typedef struct hvn_aug_sample {
    double  inv[6];            /* destination -> source affine: x_s = inv[0] x + inv[1] y + inv[2], y_s = inv[3] x + inv[4] y + inv[5] */
    int32_t src;               /* index of the source patch in the resident set */
    int32_t flip_lr, flip_ud;
    int32_t kind, p0, p1;
    int32_t per_channel;
    float   noise_scale;
    int32_t order[4];
    double  hue, sat, bright, contrast;
} hvn_aug_sample;
/* img: dev uint8 [P][h][w][3], ann: dev int32 [P][h][w][c] (c = 1 or 2: instance ids, types); out_img: dev uint8 [n][oh][ow][3],
 * out_ann: dev int32 [n][oh][ow][c]; prm: dev hvn_aug_sample[n] with 0 <= src < P. */
HVN_API int hvn_augment_shape(const uint8_t *img, const int32_t *ann, int n_resident, int h, int w, int c, const hvn_aug_sample *prm, int n,
                              int out_h, int out_w, uint8_t *out_img, int32_t *out_ann, void *stream);
/* The same gather over WHOLE images instead of an extracted patch set (extract_patches.py + misc/patch_extractor.py:58-133 folded in).
 * pixels: dev uint8 [total_pixels][3] and ann: dev int32 [total_pixels][c], the images back to back, row-major; images: dev
 * hvn_image_rec[n_images] (offset in pixels; offset + h * w <= total_pixels); patches: dev hvn_patch_rec[n_patches], the window
 * [row, row + win_h) x [col, col + win_w) of image `image` in UNPADDED coordinates (negative / past the edge = the mirror pad).
 * Patch frame arithmetic is hvn_augment_shape's with h = win_h, w = win_w; the pixel then comes from image row refl(row + fy, h_i),
 * column refl(col + fx, w_i), refl = numpy "reflect" as an index map (period 2(n - 1); n == 1 -> 0).  prm[k].src indexes `patches`.
 * The kernel checks 0 <= src < n_patches, 0 <= image < n_images, h, w > 0 and the image's extent against total_pixels before it
 * reads through them: a sample that fails is written as zeros and, when status != NULL, adds 1 to status[0] (dev int32, zeroed by
 * the caller). */
typedef struct hvn_image_rec {
    int64_t offset;            /* first pixel of the image in `pixels` / `ann` */
    int32_t h, w;
} hvn_image_rec;
typedef struct hvn_patch_rec {
    int32_t image, row, col;
} hvn_patch_rec;
HVN_API int hvn_augment_shape_images(const uint8_t *pixels, const int32_t *ann, const hvn_image_rec *images, const hvn_patch_rec *patches,
                                     int n_images, int n_patches, int64_t total_pixels, int win_h, int win_w, int c, const hvn_aug_sample *prm,
                                     int n, int out_h, int out_w, uint8_t *out_img, int32_t *out_ann, int32_t *status, void *stream);
/* src / dst: dev uint8 [n][h][w][3] (must not alias: the blurs read neighbours); noise: dev float32 [n][h][w][3] standard normal samples
 * (may be NULL when no record has kind 2). */
HVN_API int hvn_augment_input(const uint8_t *src, const hvn_aug_sample *prm, const float *noise, int n, int h, int w, uint8_t *dst, void *stream);

/* torch.optim.Adam (opt.py:38-44: lr 1e-4, betas (0.9, 0.999), eps 1e-8, no weight decay) over flat dev slabs;
 * step = 1 for the first update. */
HVN_API int hvn_adam_step(float *w, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2,
                          float eps, int step, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HVN_H */

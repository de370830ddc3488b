// hvn_api.hip -- the C ABI (include/hvn.h) over the kernels: descriptor validation,
// plan execution, the error text of the whole library (hvn_error.h), optional per-launch timing of the conv kernel.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hvn_kernels.h"

static thread_local char g_err[512] = "";   // the library's one error text (hvn_error.h)

int hvn_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hvn_launch_status(int rc, const char *what)
{
    return rc ? hvn_fail(rc, "%s: %s", what, rc == HVN_E_LAUNCH ? "launch failed" : "the launcher refused these arguments") : HVN_OK;
}

int hvn_fail_in_op(int code, const char *plan, int i)
{
    char text[sizeof(g_err)];
    snprintf(text, sizeof(text), "%s", g_err);
    return hvn_fail(code, "%s op %d: %s", plan, i, text);
}

int hvn_launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HVN_OK : hvn_fail(HVN_E_LAUNCH, "%s: launch failed: %s", what, hipGetErrorString(e));
}

extern "C" {

int hvn_version(void) { return 104; }   // 1.04: + CONV act_dtype 2 | 3 (bf16x3 products), PACK_MULTI / SPLIT_X3 training ops, wsi_merge counters[5]; 1.02: + CHAIN op

#ifndef HVN_BUILD_ID
#define HVN_BUILD_ID "unstamped"
#endif
static const char hvn_build_tag[] = "hvn-build-id:" HVN_BUILD_ID;     // findable in the file's bytes without loading it
const char *hvn_build_id(void) { return hvn_build_tag + 13; }   // hash of the sources this binary was compiled from (hover_net_amd/lib.py:source_id)

const char *hvn_last_error(void) { return g_err; }

int hvn_device_ok(void)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

// ---- profiling of CONV launches (bench.py's roofline leg) -------------------------------
static bool g_prof = false;
static std::vector<hipEvent_t> g_ev;   // pairs
static size_t g_ev_used = 0;

int hvn_profile_enable(int on)
{
    g_prof = on != 0;
    g_ev_used = 0;
    return 0;
}

static void prof_mark(hipStream_t s)
{
    if (g_ev_used == g_ev.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        g_ev.push_back(e);
    }
    hipEventRecord(g_ev[g_ev_used++], s);
}

double hvn_profile_conv_ms(void)
{
    if (g_ev_used < 2) return -1.0;
    hipEventSynchronize(g_ev[g_ev_used - 1]);
    double total = 0.0;
    for (size_t i = 0; i + 1 < g_ev_used; i += 2) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, g_ev[i], g_ev[i + 1]);
        total += ms;
    }
    return total;
}

int hvn_profile_conv_launches(void) { return (int)(g_ev_used / 2); }

int hvn_profile_conv_ms_list(double *out, int cap)
{
    if (g_ev_used < 2) return 0;
    hipEventSynchronize(g_ev[g_ev_used - 1]);
    int n = 0;
    for (size_t i = 0; i + 1 < g_ev_used && n < cap; i += 2, ++n) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, g_ev[i], g_ev[i + 1]);
        out[n] = ms;
    }
    return n;
}

}  // extern "C"

// ---- one op (also a HVN_T_NET op of a training plan: hvn_train_api.hip) ---------------------
static bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
// base and strides of a view into a launcher's argument struct
template <class T> static inline void set_view(const hvn_view &v, T *&p, long &sn, long &sy, long &sx) { p = (T *)v.base; sn = v.sn; sy = v.sy; sx = v.sx; }
// every stride a multiple of mask + 1 elements (3: 16 bytes of fp32, 7: 16 bytes of bf16)
static inline bool strides_ok(const hvn_view &v, long mask) { return ((v.sn | v.sy | v.sx) & mask) == 0; }

// the image view of a STAIN op: uint8 [batch][h][w][3], byte strides (0 = dense); 0 = accepted, sn / sy resolved
static int stain_image(const char *what, const hvn_op *op, const hvn_view &v, int batch, long &sn, long &sy)
{
    if (!v.base) return hvn_fail(HVN_E_ARG, "%s: null pointer", what);
    if (op->x_dtype != 0) return hvn_fail(HVN_E_ARG, "%s: uint8 pixels only (x_dtype %d)", what, op->x_dtype);
    if (v.h < 1 || v.w < 1 || v.c != 3) return hvn_fail(HVN_E_ARG, "%s: h, w >= 1 and three channels (c = %d)", what, v.c);
    if ((int64_t)v.h * v.w > ((int64_t)1 << 30)) return hvn_fail(HVN_E_SIZE, "%s: h * w > 2^30 (h = %d)", what, v.h);
    if (batch > 65535) return hvn_fail(HVN_E_ARG, "%s: batch %d above 65535", what, batch);
    if ((v.sx && v.sx != 3) || v.sc > 1) return hvn_fail(HVN_E_ARG, "%s: pixels are three contiguous bytes", what);
    sy = v.sy ? v.sy : 3L * v.w;
    sn = v.sn ? v.sn : sy * v.h;
    if (sy < 3L * v.w || sn < sy * v.h) return hvn_fail(HVN_E_ARG, "%s: a stride shorter than a row or a sample", what);
    return 0;
}

// what the NBR ops share: the table, the workspace, N and the grid; 0 = accepted
static int nbr_common(const char *what, const hvn_op *op, int batch)
{
    const int N = op->x.h;
    if (!op->w || !op->x2.base) return hvn_fail(HVN_E_ARG, "%s: null pointer", what);
    if (batch != 1) return hvn_fail(HVN_E_ARG, "%s: batch %d, not 1", what, batch);
    if (((uintptr_t)op->w & 7) || ((uintptr_t)op->x2.base & 7)) return hvn_fail(HVN_E_ARG, "%s: misaligned table or workspace (8)", what);
    if (N < 1) return hvn_fail(HVN_E_ARG, "%s: N = %d, fewer than one point", what, N);
    if (op->kh < 1 || op->kw < 1) return hvn_fail(HVN_E_ARG, "%s: a grid of %d x %d cells", what, op->kh, op->kw);
    if (N > HVN_NBR_MAX_N) return hvn_fail(HVN_E_SIZE, "%s: N = %d above 2^26", what, N);
    const long cells = (long)op->kh * op->kw;
    if (op->kh > HVN_NBR_MAX_AXIS || op->kw > HVN_NBR_MAX_AXIS || cells > HVN_NBR_MAX_CELLS)
        return hvn_fail(HVN_E_SIZE, "%s: a grid of %d x %d cells, more than 4096 per axis or 2^22 in all", what, op->kh, op->kw);
    if ((long)op->x2.sn < HVN_NBR_WORKSPACE_BYTES(N, cells))
        return hvn_fail(HVN_E_SIZE, "%s: workspace of %ld bytes, %ld needed", what, (long)op->x2.sn, HVN_NBR_WORKSPACE_BYTES(N, cells));
    return 0;
}

int hvn_internal_run_one(const hvn_op *op, int batch, hipStream_t s)
{
    switch (op->kind) {
    case HVN_OP_CONV0: {
        Conv0Args a;
        set_view(op->x, a.img, a.isn, a.isy, a.isx);
        a.isc = op->x.sc ? op->x.sc : 1;
        a.is_f32 = op->x_dtype;
        a.H = op->x.h; a.W = op->x.w;
        a.w = op->w; a.bias = op->bias;
        set_view(op->y, a.y, a.ysn, a.ysy, a.ysx);
        a.N = batch; a.Ho = op->y.h; a.Wo = op->y.w; a.pad = op->pad_t; a.relu = op->relu; a.out_bf16 = op->act_dtype == 1;
        if (op->kh != 7 || op->kw != 7 || op->x.c != 3 || op->y.c != 64 || !op->w || !op->bias || !op->x.base || !op->y.base)
            return hvn_fail(HVN_E_ARG, "conv0: expects 7x7x3->64 with bias, a non-null image and output");
        if (!aligned16(a.y) || !strides_ok(op->y, 3)) return hvn_fail(HVN_E_ARG, "conv0: output view not 16-byte aligned");
        return hvn_launch_status(hvn_launch_conv0(a, s), "conv0");
    }
    case HVN_OP_CONV: {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        set_view(op->x, a.x, a.xsn, a.xsy, a.xsx);
        a.H = op->x.h; a.W = op->x.w; a.Cin = op->x.c;
        a.w = op->w; a.bias = op->bias;
        a.pre_s = op->pre_scale; a.pre_b = op->pre_shift;
        a.post_s = op->post_scale; a.post_b = op->post_shift;
        set_view(op->res, a.res, a.rsn, a.rsy, a.rsx);
        set_view(op->y, a.y, a.ysn, a.ysy, a.ysx);
        a.N = batch; a.Ho = op->y.h; a.Wo = op->y.w; a.Cout = op->cout;
        a.KH = op->kh; a.KW = op->kw; a.stride = op->stride; a.pad_t = op->pad_t; a.pad_l = op->pad_l;
        a.relu = op->relu;
        a.groups = op->groups > 1 ? op->groups : 1;
        set_view(op->x2, a.x2, a.x2sn, a.x2sy, a.x2sx);
        a.Cin2 = a.x2 ? op->x2.c : 0;
        a.stride2 = op->_rsv > 0 ? op->_rsv : 1;
        if (a.x2 && (op->kh != 1 || op->kw != 1 || a.stride != 1 || a.Cin2 % 32 || !aligned16(a.x2) || !strides_ok(op->x2, 3) ||
                     a.pre_s || (long)(a.Ho - 1) * a.stride2 >= op->x2.h || (long)(a.Wo - 1) * a.stride2 >= op->x2.w))
            return hvn_fail(HVN_E_ARG, "conv: second input needs a 1x1 stride-1 op without prologue and a view that covers the output grid");
        a.M = (long)batch * a.Ho * a.Wo;
        if (!a.x || !a.w || !a.y) return hvn_fail(HVN_E_ARG, "conv: null pointer");
        if (a.Cin % 32) return hvn_fail(HVN_E_ARG, "conv: input channels must be a multiple of 32 (got %d)", a.Cin);
        if (!aligned16(a.x) || !aligned16(a.w) || !strides_ok(op->x, 3))
            return hvn_fail(HVN_E_ARG, "conv: input view / weights not 16-byte aligned");
        if ((a.pre_s && !aligned16(a.pre_s)) || (a.pre_b && !aligned16(a.pre_b)) || (!a.pre_s != !a.pre_b))
            return hvn_fail(HVN_E_ARG, "conv: prologue vectors must be 16-byte aligned and come in pairs");
        if (!a.post_s != !a.post_b) return hvn_fail(HVN_E_ARG, "conv: epilogue affine must come in pairs");
        if (op->y.c != op->cout) return hvn_fail(HVN_E_ARG, "conv: output view channels != cout");
        a.nbatch = op->nbatch > 1 ? op->nbatch : 1;
        a.xb = op->batch_stride[0]; a.wb = op->batch_stride[1]; a.yb = op->batch_stride[2];
        if (a.nbatch > 1 && ((a.xb | a.wb | a.yb) & 3)) return hvn_fail(HVN_E_ARG, "conv: batch strides must keep 16-byte alignment");
        const bool bf16 = op->act_dtype == 1;
        if (bf16 && (!strides_ok(op->x, 7) || (a.x2 && !strides_ok(op->x2, 7)) || a.nbatch > 1))
            return hvn_fail(HVN_E_ARG, "conv(bf16): input strides must be multiples of 8 elements; no batched launch");
        if (g_prof) prof_mark(s);
        const bool x3 = op->act_dtype == 2 || op->act_dtype == 3;
        if (x3 && (a.groups > 1 || (a.nbatch > 1 && (a.wb & 7)))) return hvn_fail(HVN_E_ARG, "conv(bf16x3): no grouped convs; batch stride of the planes must keep 16-byte alignment");
        int rc;
        if (bf16 && (op->tile_n == 896 || op->tile_n == 640))            // LDS-DMA form of the bf16 convolution (hvn_conv_bf16g.hip)
            rc = hvn_launch_conv_bf16g(a, op->tile_n == 896 ? 256 : 128, s);
        else if (bf16)
            rc = hvn_launch_conv_bf16(a, op->tile_n, s);
        else if (x3 && (op->tile_n == 896 || op->tile_n == 640))      // LDS-DMA form, 256 | 128 pixels x 128 channels (hvn_conv_x3g.hip)
            rc = hvn_launch_conv_x3g(a, op->tile_n == 896 ? 256 : 128, op->act_dtype == 3 ? 6 : 9, s);
        else
            rc = x3 ? hvn_launch_conv_x3(a, op->tile_n, op->act_dtype == 3 ? 6 : 9, s) : hvn_launch_conv(a, op->tile_n, s);
        if (g_prof) prof_mark(s);
        if (rc) return hvn_fail(rc, "conv: launch failed (tile_n=%d)", op->tile_n);
        return HVN_OK;
    }
    case HVN_OP_CHAIN: {
        ChainArgs a;
        memset(&a, 0, sizeof(a));
        set_view(op->x, a.x, a.xsn, a.xsy, a.xsx);
        a.K1 = op->x.c;
        set_view(op->x2, a.x2, a.x2sn, a.x2sy, a.x2sx);
        a.K1b = a.x2 ? op->x2.c : 0;
        a.stride2 = op->_rsv > 0 ? op->_rsv : 1;
        a.w1 = op->w;
        set_view(op->res, a.res, a.rsn, a.rsy, a.rsx);
        set_view(op->y, a.y, a.ysn, a.ysy, a.ysx);
        a.C = op->cout;
        a.post_s = op->post_scale; a.post_b = op->post_shift;
        a.pre_s = op->pre_scale; a.pre_b = op->pre_shift;
        a.w2 = op->w2; a.bias2 = op->bias2; a.relu2 = 1;
        set_view(op->y2, a.y2, a.y2sn, a.y2sy, a.y2sx);
        a.N2 = op->cout2;
        a.N = batch; a.Ho = op->y.h; a.Wo = op->y.w;
        a.M = (long)batch * a.Ho * a.Wo;
        a.bm = op->tile_n == 64 ? 64 : 128;      // CHAIN: tile_n = pixels per workgroup (0 / 128: 128)
        const bool cx3 = op->act_dtype == 2 || op->act_dtype == 3;       // products on the bf16 pipe from bf16x3 splits: w / w2 = plane packings
        const bool cbf = op->act_dtype == 1;                             // bf16 activations and weights (hvn_conv_chain_bf16.hip)
        if (op->act_dtype != 0 && !cx3 && !cbf) return hvn_fail(HVN_E_ARG, "chain: act_dtype 0 (fp32), 1 (bf16) or 2 | 3 (fp32 with bf16x3 products)");
        // the bf16 form differs from the fp32 / bf16x3 forms in three things: the channel counts it exists for, the stride multiple, the launcher
        const char *form = cbf ? " (bf16)" : "";
        const bool channels_ok = cbf ? hvn_chain_bf16_supported(a.K1, a.K1b, a.C, a.N2) != 0
                                     : hvn_chain_supported(a.C, a.N2) && !(a.K1 % 32 || a.K1b % 32 || a.K1 + a.K1b < 64);
        const long stride_mask = cbf ? 7 : 3;
        if (!a.x || !a.w1 || !a.y || !a.w2 || !a.y2) return hvn_fail(HVN_E_ARG, "chain: null pointer");
        if (op->kh != 1 || op->kw != 1 || op->stride != 1 || op->pad_t || op->pad_l || op->relu || op->bias)
            return hvn_fail(HVN_E_ARG, "chain: the first conv is a plain 1x1 (no bias / relu of its own)");
        if (!channels_ok || op->y.c != a.C || op->y2.c != a.N2)
            return hvn_fail(HVN_E_ARG, "chain%s: needs %s, cout2 in {64, 128} (cout2 = %d)", form,
                            cbf ? "input channels in slabs of 64 (64 or 128 in all), cout % 256 == 0" : "input channels in slabs of 32 (>= 64), cout % 64 == 0", a.N2);
        if (op->x.h != a.Ho || op->x.w != a.Wo || op->y2.h != a.Ho || op->y2.w != a.Wo ||
            (a.x2 && ((long)(a.Ho - 1) * a.stride2 >= op->x2.h || (long)(a.Wo - 1) * a.stride2 >= op->x2.w)))
            return hvn_fail(HVN_E_ARG, "chain: views do not cover the output grid");
        if (a.res && (a.rsn != a.ysn || a.rsy != a.ysy || a.rsx != a.ysx || op->res.c != a.C))
            return hvn_fail(HVN_E_ARG, "chain: the residual view must have the output's strides");
        if (!aligned16(a.x) || !aligned16(a.w1) || !aligned16(a.w2) || !aligned16(a.y) || !aligned16(a.y2) || (a.res && !aligned16(a.res)) ||
            (a.x2 && !aligned16(a.x2)) || !strides_ok(op->x, stride_mask) || !strides_ok(op->y, stride_mask) || !strides_ok(op->y2, stride_mask) ||
            !strides_ok(op->x2, stride_mask))
            return hvn_fail(HVN_E_ARG, "chain%s: views / weights not 16-byte aligned", form);
        if ((!a.pre_s != !a.pre_b) || (!a.post_s != !a.post_b) || (a.pre_s && (!aligned16(a.pre_s) || !aligned16(a.pre_b))) ||
            (a.post_s && (!aligned16(a.post_s) || !aligned16(a.post_b))) || (a.bias2 && !aligned16(a.bias2)))
            return hvn_fail(HVN_E_ARG, "chain: per-channel vectors must be 16-byte aligned and come in pairs");
        if (g_prof) prof_mark(s);
        int rc;
        if (cbf)
            rc = hvn_launch_conv_chain_bf16(a, s);
        else if (cx3 && op->tile_n == 1152)      // input tile resident in registers, operands a chunk ahead (hvn_conv_chain_x3r.hip)
            rc = hvn_launch_conv_chain_x3r(a, op->act_dtype == 3 ? 6 : 9, s);
        else
            rc = cx3 ? hvn_launch_conv_chain_x3(a, op->act_dtype == 3 ? 6 : 9, s) : hvn_launch_conv_chain(a, s);
        if (g_prof) prof_mark(s);
        if (rc) return hvn_fail(rc, "chain%s: launch failed (cout2=%d)", form, a.N2);
        return HVN_OK;
    }
    case HVN_OP_WINO_IN:
    case HVN_OP_WINO_OUT: {
        WinoArgs a;
        const bool in = op->kind == HVN_OP_WINO_IN;
        set_view(op->x, a.x, a.xsn, a.xsy, a.xsx);
        set_view(op->y, a.y, a.ysn, a.ysy, a.ysx);
        a.mat = op->w; a.bias = op->bias;
        a.N = batch; a.H = in ? op->x.h : op->y.h; a.W = in ? op->x.w : op->y.w; a.C = in ? op->x.c : op->y.c;
        a.ty = op->kh; a.tx = op->kw; a.pad = op->pad_t; a.relu = op->relu;
        a.accum = (!in && op->res.base != nullptr) ? 1 : 0;
        a.lo = nullptr; a.lsn = a.lsy = a.lsx = 0;
        if (in && op->res.base) {       // WINO_IN with res: the input is nearest2x(res) + x, formed on the fly (UPADD fused into the transform)
            set_view(op->res, a.lo, a.lsn, a.lsy, a.lsx);
            if (op->res.h * 2 != op->x.h || op->res.w * 2 != op->x.w || op->res.c != op->x.c || !aligned16(a.lo) || !strides_ok(op->res, 3))
                return hvn_fail(HVN_E_ARG, "wino_in: the half-resolution input must be x.h/2 x x.w/2 x x.c and 16-byte aligned");
        }
        if (a.accum && op->res.base != op->y.base) return hvn_fail(HVN_E_ARG, "wino_out: res must alias y (accumulate in place)");
        const int n2 = in ? op->y.h : op->x.h;       // transform positions (m + r - 1)^2
        if (op->stride > 1 && op->_rsv > 1) {         // explicit F(m x m, r x r): stride = m, _rsv = r
            a.m = op->stride; a.r = op->_rsv;
        } else {                                     // legacy encoding by the number of positions: 5x5 filters
            a.m = n2 == 36 ? 2 : n2 == 64 ? 4 : n2 == 100 ? 6 : 0; a.r = 5;
        }
        if (!a.m || (a.m + a.r - 1) * (a.m + a.r - 1) != n2 || !((a.m == 2 && a.r == 5) || ((a.m == 4 || a.m == 6) && (a.r == 5 || a.r == 3))))
            return hvn_fail(HVN_E_ARG, "winograd transform: %d transform positions do not match F(2,5) / F(4,5) / F(4,3) / F(6,3) / F(6,5)", n2);
        if (!a.x || !a.y || !a.mat || a.ty <= 0 || a.tx <= 0 || (a.C & 3)) return hvn_fail(HVN_E_ARG, "winograd transform: bad descriptor");
        if (!aligned16(a.x) || !aligned16(a.y) || !strides_ok(op->x, 3) || !strides_ok(op->y, 3))
            return hvn_fail(HVN_E_ARG, "winograd transform: views not 16-byte aligned");
        if (in && (op->y.w != a.ty * a.tx || op->y.c != a.C)) return hvn_fail(HVN_E_ARG, "wino_in: V must be [n*n][tiles][c]");
        if (!in && (op->x.w != a.ty * a.tx || op->y.h > a.m * a.ty || op->y.h <= a.m * (a.ty - 1) || op->y.w > a.m * a.tx ||
                    op->y.w <= a.m * (a.tx - 1) || op->x.c != a.C))
            return hvn_fail(HVN_E_ARG, "wino_out: M must be [n*n][tiles][cout] and the tiles must cover y");
        if (g_prof) prof_mark(s);
        int rc = in ? hvn_launch_wino_in(a, s) : hvn_launch_wino_out(a, s);
        if (g_prof) prof_mark(s);
        return hvn_launch_status(rc, in ? "wino_in" : "wino_out");
    }
    case HVN_OP_UPADD: {
        UpAddArgs a;
        set_view(op->x, a.lo, a.lsn, a.lsy, a.lsx);
        set_view(op->res, a.skip, a.ssn, a.ssy, a.ssx);
        set_view(op->y, a.y, a.ysn, a.ysy, a.ysx);
        a.N = batch; a.H = op->y.h; a.W = op->y.w; a.C = op->y.c; a.bf16 = op->act_dtype == 1;
        if (a.bf16 && !(strides_ok(op->x, 7) && strides_ok(op->res, 7) && strides_ok(op->y, 7)))
            return hvn_fail(HVN_E_ARG, "upadd(bf16): strides must be multiples of 8 elements");
        if (!a.lo || !a.skip || !a.y) return hvn_fail(HVN_E_ARG, "upadd: null pointer");
        if (op->x.h * 2 != a.H || op->x.w * 2 != a.W || op->res.h != a.H || op->res.w != a.W || op->x.c != a.C || op->res.c != a.C)
            return hvn_fail(HVN_E_ARG, "upadd: shape mismatch");
        if (a.C <= 0 || a.C % (a.bf16 ? 8 : 4))     // one thread moves 16 bytes: the launcher would refuse without a text of its own
            return hvn_fail(HVN_E_ARG, "upadd: channels must be a multiple of 4 (fp32) or 8 (bf16) (got %d)", a.C);
        if (!aligned16(a.lo) || !aligned16(a.skip) || !aligned16(a.y) || !(strides_ok(op->x, 3) && strides_ok(op->res, 3) && strides_ok(op->y, 3)))
            return hvn_fail(HVN_E_ARG, "upadd: views not 16-byte aligned");
        return hvn_launch_status(hvn_launch_upadd(a, s), "upadd");
    }
    case HVN_OP_HEAD: {
        HeadArgs a;
        set_view(op->x, a.x, a.xsn, a.xsy, a.xsx);
        a.w = op->w; a.bias = op->bias;
        a.y = (float *)op->y.base;
        a.N = batch; a.H = op->x.h; a.W = op->x.w; a.Cout = op->cout; a.in_bf16 = op->act_dtype == 1;
        if (a.in_bf16 && !strides_ok(op->x, 7)) return hvn_fail(HVN_E_ARG, "head(bf16): strides must be multiples of 8 elements");
        if (op->x.c != 64 || !a.w || !a.bias || !a.x || !a.y) return hvn_fail(HVN_E_ARG, "head: expects 64 input channels, weights and bias");
        if (!aligned16(a.x) || !strides_ok(op->x, 3)) return hvn_fail(HVN_E_ARG, "head: input view not 16-byte aligned");
        return hvn_launch_status(hvn_launch_head(a, s), "head");
    }
    case HVN_OP_PREDMAP: {
        PredMapArgs a;
        a.np = (const float *)op->x.base;
        a.hv = (const float *)op->res.base;
        a.tp = op->w;
        a.y = (float *)op->y.base;
        a.N = batch; a.H = op->y.h; a.W = op->y.w; a.nr_types = op->cout;
        if (!a.np || !a.hv || !a.y || (a.nr_types > 0 && !a.tp)) return hvn_fail(HVN_E_ARG, "predmap: null pointer");
        if (a.nr_types > 0 && !aligned16(a.y)) return hvn_fail(HVN_E_ARG, "predmap: output not 16-byte aligned");
        return hvn_launch_status(hvn_launch_predmap(a, s), "predmap");
    }
    case HVN_OP_VIEW: {
        ViewArgs a;
        a.x = (const uint8_t *)op->x.base;
        a.y = (uint8_t *)op->y.base;
        a.N = batch; a.H = op->x.h; a.W = op->x.w; a.k = op->_rsv;
        if (a.k < 0 || a.k > 7) return hvn_fail(HVN_E_ARG, "view: view id %d outside 0..7", a.k);
        if (op->x_dtype != 0) return hvn_fail(HVN_E_ARG, "view: uint8 patches only (x_dtype %d)", op->x_dtype);
        if (!a.x || !a.y || a.x == a.y) return hvn_fail(HVN_E_ARG, "view: null pointer, or x and y are the same buffer");
        if (a.H < 1 || a.W < 1 || op->x.c != 3 || op->y.h != a.H || op->y.w != a.W || op->y.c != 3)
            return hvn_fail(HVN_E_ARG, "view: x and y must have the same extents, three channels (x.h = %d)", a.H);
        if ((a.k & 1) && a.H != a.W) return hvn_fail(HVN_E_ARG, "view: a quarter turn needs square patches (view %d)", a.k);
        if (batch > 65535) return hvn_fail(HVN_E_ARG, "view: batch %d above 65535", batch);
        if ((op->x.sx && op->x.sx != 3) || (op->y.sx && op->y.sx != 3) || op->x.sc > 1 || op->y.sc > 1)
            return hvn_fail(HVN_E_ARG, "view: pixels are three contiguous bytes");
        // 0 = dense; a view's rows are x.h long for odd r, which is x.w there
        a.xsy = op->x.sy ? op->x.sy : 3L * a.W; a.xsn = op->x.sn ? op->x.sn : a.xsy * a.H;
        a.ysy = op->y.sy ? op->y.sy : 3L * a.W; a.ysn = op->y.sn ? op->y.sn : a.ysy * a.H;
        if (a.xsy < 3L * a.W || a.ysy < 3L * a.W || a.xsn < a.xsy * a.H || a.ysn < a.ysy * a.H)
            return hvn_fail(HVN_E_ARG, "view: a stride shorter than a row or a sample");
        return hvn_launch_status(hvn_launch_view(a, s), "view");
    }
    case HVN_OP_TTA: {
        TtaArgs a;
        a.np = (const float *)op->x.base;
        a.hv = (const float *)op->res.base;
        a.tp = op->w;
        a.acc = (float *)op->y2.base;
        a.y = (float *)op->y.base;
        a.N = batch; a.H = op->y.h; a.W = op->y.w; a.nr_types = op->cout;
        a.k = op->_rsv; a.first = op->kh != 0; a.last = op->kw != 0; a.K = op->stride;
        if (a.k < 0 || a.k > 7) return hvn_fail(HVN_E_ARG, "tta: view id %d outside 0..7", a.k);
        if (a.H < 1 || a.W < 1 || a.nr_types < 0) return hvn_fail(HVN_E_ARG, "tta: empty map or negative nr_types (y.h = %d)", a.H);
        if ((a.k & 1) && a.H != a.W) return hvn_fail(HVN_E_ARG, "tta: a quarter turn needs square maps (view %d)", a.k);
        if (!a.np || !a.hv || (a.nr_types > 0 && !a.tp)) return hvn_fail(HVN_E_ARG, "tta: null pointer");
        if (!a.acc || ((uintptr_t)a.acc & 3)) return hvn_fail(HVN_E_ARG, "tta: null or misaligned accumulator (y2)");
        if (a.last && !a.y) return hvn_fail(HVN_E_ARG, "tta: the last view needs an output (y)");
        if (a.last && a.K < 1) return hvn_fail(HVN_E_ARG, "tta: the last view needs the number of views (stride = %d)", a.K);
        if (a.last && a.y == a.acc) return hvn_fail(HVN_E_ARG, "tta: y and the accumulator are the same buffer");
        if (a.last && (a.nr_types > 0 ? !aligned16(a.y) : (((uintptr_t)a.y & 3) != 0))) return hvn_fail(HVN_E_ARG, "tta: output not 16-byte aligned");
        if (batch > 65535) return hvn_fail(HVN_E_ARG, "tta: batch %d above 65535", batch);
        return hvn_launch_status(hvn_launch_tta(a, s), "tta");
    }
    case HVN_OP_STAIN_HIST: {
        StainHistArgs a;
        a.x = (const uint8_t *)op->x.base;
        a.mask = (const uint8_t *)op->res.base;
        a.bins = (uint32_t *)op->y.base;
        a.N = batch; a.H = op->x.h; a.W = op->x.w;
        if (!a.bins) return hvn_fail(HVN_E_ARG, "stain_hist: null pointer");
        if (int rc = stain_image("stain_hist", op, op->x, batch, a.xsn, a.xsy)) return rc;
        if ((uintptr_t)a.bins & 3) return hvn_fail(HVN_E_ARG, "stain_hist: misaligned bins");
        return hvn_launch_status(hvn_launch_stain_hist(a, s), "stain_hist");
    }
    case HVN_OP_STAIN_COMPACT: {
        uint32_t *bins = (uint32_t *)op->x.base, *list = (uint32_t *)op->y.base;
        int64_t *status = (int64_t *)op->y2.base;
        void *ws = op->x2.base;
        if (!bins || !list || !status || !ws) return hvn_fail(HVN_E_ARG, "stain_compact: null pointer");
        if (batch != 1) return hvn_fail(HVN_E_ARG, "stain_compact: batch %d, not 1", batch);
        if (((uintptr_t)bins & 15) || ((uintptr_t)list & 7) || ((uintptr_t)status & 7) || ((uintptr_t)ws & 7))
            return hvn_fail(HVN_E_ARG, "stain_compact: misaligned bins (16), list, status or workspace (8)");
        if (op->y.h < 1 || op->y.h > (1 << 24)) return hvn_fail(HVN_E_SIZE, "stain_compact: list capacity %d outside [1, 2^24]", op->y.h);
        return hvn_launch_status(hvn_launch_stain_compact(bins, list, (uint32_t)op->y.h, status, ws, op->_rsv != 0, s), "stain_compact");
    }
    case HVN_OP_STAIN_APPLY: {
        StainApplyArgs a;
        a.x = (const uint8_t *)op->x.base;
        a.y = (uint8_t *)op->y.base;
        a.tables = (const double *)op->w;
        a.N = batch; a.H = op->x.h; a.W = op->x.w;
        if (!a.y || !a.tables) return hvn_fail(HVN_E_ARG, "stain_apply: null pointer");
        if (int rc = stain_image("stain_apply", op, op->x, batch, a.xsn, a.xsy)) return rc;
        if (op->y.h != a.H || op->y.w != a.W) return hvn_fail(HVN_E_ARG, "stain_apply: x and y must have the same extents (y.h = %d)", op->y.h);
        if (int rc = stain_image("stain_apply", op, op->y, batch, a.ysn, a.ysy)) return rc;
        if ((uintptr_t)a.tables & 7) return hvn_fail(HVN_E_ARG, "stain_apply: misaligned tables");
        if (!((const uint8_t *)a.y == a.x && a.ysn == a.xsn && a.ysy == a.xsy)) {       // y is x itself, or the two do not meet
            const uintptr_t x0 = (uintptr_t)a.x, x1 = x0 + (uintptr_t)((batch - 1) * a.xsn + (a.H - 1) * a.xsy + 3L * a.W);
            const uintptr_t y0 = (uintptr_t)a.y, y1 = y0 + (uintptr_t)((batch - 1) * a.ysn + (a.H - 1) * a.ysy + 3L * a.W);
            if (x0 < y1 && y0 < x1) return hvn_fail(HVN_E_ARG, "stain_apply: x and y overlap without being the same view");
        }
        return hvn_launch_status(hvn_launch_stain_apply(a, s), "stain_apply");
    }
    case HVN_OP_NBR_GRID: {
        NbrGridArgs a;
        a.xy = (const double *)op->x.base;
        a.types = (const int *)op->res.base;
        a.table = (const double *)op->w;
        a.workspace = op->x2.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw;
        if (!a.xy || !a.workspace) return hvn_fail(HVN_E_ARG, "nbr_grid: null pointer");
        if (int rc = nbr_common("nbr_grid", op, batch)) return rc;
        if (((uintptr_t)a.xy & 7) || ((uintptr_t)a.types & 3)) return hvn_fail(HVN_E_ARG, "nbr_grid: misaligned xy (8) or types (4)");
        return hvn_launch_status(hvn_launch_nbr_grid(a, s), "nbr_grid");
    }
    case HVN_OP_NBR_QUERY: {
        NbrQueryArgs a;
        a.table = (const double *)op->w;
        a.workspace = op->x2.base;
        a.count = (int *)op->y.base; a.knn = (int *)op->y2.base; a.nearest = (int *)op->res.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw; a.T = op->cout; a.k = op->_rsv;
        if (!a.workspace || !a.count || !a.knn || !a.nearest) return hvn_fail(HVN_E_ARG, "nbr_query: null pointer");
        if (a.k < 1 || a.k > 16) return hvn_fail(HVN_E_ARG, "nbr_query: k = %d outside 1..16", a.k);
        if (a.T < 1 || a.T > 16) return hvn_fail(HVN_E_ARG, "nbr_query: %d types outside 1..16", a.T);
        if (int rc = nbr_common("nbr_query", op, batch)) return rc;
        if (((uintptr_t)a.count | (uintptr_t)a.knn | (uintptr_t)a.nearest) & 3) return hvn_fail(HVN_E_ARG, "nbr_query: misaligned count, knn or nearest (4)");
        return hvn_launch_status(hvn_launch_nbr_query(a, s), "nbr_query");
    }
    case HVN_OP_NBR_CLUSTER: {
        NbrClusterArgs a;
        a.table = (const double *)op->w;
        a.workspace = op->x2.base;
        a.workspace2 = op->res.base;
        a.label = (int *)op->y.base; a.degree = (int *)op->y2.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw; a.min_pts = op->cout; a.mask = (unsigned)op->groups;
        if (!a.workspace || !a.workspace2 || !a.label || !a.degree) return hvn_fail(HVN_E_ARG, "nbr_cluster: null pointer");
        if (a.min_pts < 1) return hvn_fail(HVN_E_ARG, "nbr_cluster: min_pts = %d, below 1", a.min_pts);
        if (a.mask == 0) return hvn_fail(HVN_E_ARG, "nbr_cluster: a type mask of 0 selects no point");
        if (a.min_pts > HVN_NBR_CLUSTER_MAX_MIN_PTS) return hvn_fail(HVN_E_SIZE, "nbr_cluster: min_pts = %d above 2^26", a.min_pts);
        if (int rc = nbr_common("nbr_cluster", op, batch)) return rc;
        if (((uintptr_t)a.label | (uintptr_t)a.degree) & 3) return hvn_fail(HVN_E_ARG, "nbr_cluster: misaligned label or degree (4)");
        if ((uintptr_t)a.workspace2 & 7) return hvn_fail(HVN_E_ARG, "nbr_cluster: misaligned second workspace (8)");
        if ((long)op->res.sn < HVN_NBR_CLUSTER_WORKSPACE_BYTES(a.N))
            return hvn_fail(HVN_E_SIZE, "nbr_cluster: second workspace of %ld bytes, %ld needed", (long)op->res.sn, HVN_NBR_CLUSTER_WORKSPACE_BYTES(a.N));
        return hvn_launch_status(hvn_launch_nbr_cluster(a, s), "nbr_cluster");
    }
    case HVN_OP_NBR_DENSITY: {
        NbrDensityArgs a;
        a.table = (const double *)op->w;
        a.raster = (const double *)op->bias;
        a.workspace = op->x2.base;
        a.count = (int *)op->y.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw; a.T = op->cout; a.H = op->y.h; a.W = op->y.w;
        if (!a.workspace || !a.count || !a.raster) return hvn_fail(HVN_E_ARG, "nbr_density: null pointer");
        if (a.T < 1 || a.T > 16) return hvn_fail(HVN_E_ARG, "nbr_density: %d types outside 1..16", a.T);
        if (a.H < 1 || a.W < 1) return hvn_fail(HVN_E_ARG, "nbr_density: a raster of %d x %d nodes", a.H, a.W);
        if (a.H > HVN_NBR_DENSITY_MAX_AXIS || a.W > HVN_NBR_DENSITY_MAX_AXIS || (long)a.T * a.H * a.W > HVN_NBR_DENSITY_MAX_NODES)
            return hvn_fail(HVN_E_SIZE, "nbr_density: %d planes of %d x %d nodes, more than 16384 per axis or 2^28 in all", a.T, a.H, a.W);
        if (int rc = nbr_common("nbr_density", op, batch)) return rc;
        if ((uintptr_t)a.count & 3) return hvn_fail(HVN_E_ARG, "nbr_density: misaligned count (4)");
        if ((uintptr_t)a.raster & 7) return hvn_fail(HVN_E_ARG, "nbr_density: misaligned raster table (8)");
        return hvn_launch_status(hvn_launch_nbr_density(a, s), "nbr_density");
    }
    case HVN_OP_NBR_PAIRS: {
        NbrPairsArgs a;
        a.table = (const double *)op->w;
        a.rt = (const double *)op->bias;
        a.workspace = op->x2.base;
        a.acc = (long long *)op->y.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw; a.T = op->cout; a.R = op->_rsv;
        if (!a.workspace || !a.acc || !a.rt) return hvn_fail(HVN_E_ARG, "nbr_pairs: null pointer");
        if (a.T < 1 || a.T > 16) return hvn_fail(HVN_E_ARG, "nbr_pairs: %d types outside 1..16", a.T);
        if (a.R < 1 || a.R > HVN_NBR_PAIRS_MAX_R) return hvn_fail(HVN_E_ARG, "nbr_pairs: %d radii outside 1..32", a.R);
        if (a.T * a.T * a.R > HVN_NBR_PAIRS_MAX_BINS) return hvn_fail(HVN_E_SIZE, "nbr_pairs: %d x %d types and %d radii, more than 4096 bins", a.T, a.T, a.R);
        if (int rc = nbr_common("nbr_pairs", op, batch)) return rc;
        if ((uintptr_t)a.acc & 7) return hvn_fail(HVN_E_ARG, "nbr_pairs: misaligned acc (8)");
        if ((uintptr_t)a.rt & 7) return hvn_fail(HVN_E_ARG, "nbr_pairs: misaligned window and radius table (8)");
        return hvn_launch_status(hvn_launch_nbr_pairs(a, s), "nbr_pairs");
    }
    case HVN_OP_NBR_PAIRS_SIM: {
        NbrPairsSimArgs a;
        a.table = (const double *)op->w;
        a.rt = (const double *)op->bias;
        a.workspace = op->x2.base;
        a.types = (const int *)op->res.base;
        a.keys = (const unsigned long long *)op->w2;
        a.labels = (unsigned *)op->y2.base;
        a.out = (long long *)op->y.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw; a.T = op->cout; a.R = op->_rsv; a.SB = op->nbatch; a.phase = op->stride;
        if (!a.workspace || !a.out || !a.rt || !a.keys || !a.labels) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: null pointer");
        if (a.T < 1 || a.T > 16) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: %d types outside 1..16", a.T);
        if (a.R < 1 || a.R > HVN_NBR_PAIRS_MAX_R) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: %d radii outside 1..32", a.R);
        if (a.SB < 1 || a.SB > HVN_NBR_PAIRS_SIM_MAX_SB) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: a batch of %d simulations outside 1..32", a.SB);
        if (a.phase < 0 || a.phase > 2) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: stride = %d is no phase (0: both, 1: labels, 2: pairs)", a.phase);
        if (a.T * a.T * a.R > HVN_NBR_PAIRS_MAX_BINS)
            return hvn_fail(HVN_E_SIZE, "nbr_pairs_sim: %d x %d types and %d radii, more than 4096 bins", a.T, a.T, a.R);
        if (HVN_NBR_PAIRS_SIM_LDS_BYTES(a.SB, a.T * a.T * a.R) > HVN_NBR_PAIRS_SIM_MAX_LDS)
            return hvn_fail(HVN_E_SIZE, "nbr_pairs_sim: %d histograms of %d bins need %ld bytes of LDS, more than %ld", a.SB, a.T * a.T * a.R,
                            HVN_NBR_PAIRS_SIM_LDS_BYTES(a.SB, a.T * a.T * a.R), HVN_NBR_PAIRS_SIM_MAX_LDS);
        if (int rc = nbr_common("nbr_pairs_sim", op, batch)) return rc;
        if ((long)op->y2.sn < HVN_NBR_PAIRS_SIM_LABEL_BYTES(a.N, a.SB))
            return hvn_fail(HVN_E_SIZE, "nbr_pairs_sim: label workspace of %ld bytes, %ld needed", (long)op->y2.sn, HVN_NBR_PAIRS_SIM_LABEL_BYTES(a.N, a.SB));
        if (((uintptr_t)a.out | (uintptr_t)a.keys) & 7) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: misaligned out or key table (8)");
        if ((uintptr_t)a.rt & 7) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: misaligned window and radius table (8)");
        if (((uintptr_t)a.types | (uintptr_t)a.labels) & 3) return hvn_fail(HVN_E_ARG, "nbr_pairs_sim: misaligned types or label workspace (4)");
        return hvn_launch_status(hvn_launch_nbr_pairs_sim(a, s), "nbr_pairs_sim");
    }
    case HVN_OP_NBR_REGIONS: {
        NbrRegionsArgs a;
        a.table = (const double *)op->w;
        a.edges = (const double *)op->bias;
        a.edge_region = (const int *)op->res.base;
        a.rows = (const int *)op->y2.base;
        a.workspace = op->x2.base;
        a.out = (int *)op->y.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw; a.T = op->cout; a.G = op->_rsv; a.E = op->res.h;
        if (!a.workspace || !a.out || !a.edges || !a.edge_region || !a.rows) return hvn_fail(HVN_E_ARG, "nbr_regions: null pointer");
        if (a.T < 1 || a.T > 16) return hvn_fail(HVN_E_ARG, "nbr_regions: %d types outside 1..16", a.T);
        if (a.G < 1) return hvn_fail(HVN_E_ARG, "nbr_regions: %d regions, fewer than one", a.G);
        if (a.E < 1) return hvn_fail(HVN_E_ARG, "nbr_regions: %d edges, fewer than one", a.E);
        if (op->y2.sn < 1) return hvn_fail(HVN_E_ARG, "nbr_regions: row lists of %ld entries, fewer than one", (long)op->y2.sn);
        if (a.G > HVN_NBR_REGIONS_MAX_G) return hvn_fail(HVN_E_SIZE, "nbr_regions: %d regions above 4096", a.G);
        if (a.E > HVN_NBR_REGIONS_MAX_E) return hvn_fail(HVN_E_SIZE, "nbr_regions: %d edges above 2^22", a.E);
        if (int rc = nbr_common("nbr_regions", op, batch)) return rc;
        if ((long)op->y2.sn > HVN_NBR_REGIONS_MAX_ENTRIES(a.E, a.ncy))
            return hvn_fail(HVN_E_SIZE, "nbr_regions: row lists of %ld entries, more than 8 E + kh = %ld", (long)op->y2.sn, HVN_NBR_REGIONS_MAX_ENTRIES(a.E, a.ncy));
        a.M = (int)op->y2.sn;
        if (((uintptr_t)a.out | (uintptr_t)a.edge_region | (uintptr_t)a.rows) & 3) return hvn_fail(HVN_E_ARG, "nbr_regions: misaligned out, edge_region or rows (4)");
        if ((uintptr_t)a.edges & 7) return hvn_fail(HVN_E_ARG, "nbr_regions: misaligned edge table (8)");
        return hvn_launch_status(hvn_launch_nbr_regions(a, s), "nbr_regions");
    }
    case HVN_OP_NBR_MARGINS: {
        NbrMarginsArgs a;
        a.table = (const double *)op->w;
        a.seg = (const double *)op->bias;
        a.w2 = (const double *)op->w2;
        a.seg_region = (const int *)op->res.base;
        a.rows = (const int *)op->y2.base;
        a.workspace = op->x2.base;
        a.out = op->y.base;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw; a.T = op->cout; a.G = op->_rsv; a.S = op->res.h; a.B = op->cout2; a.no_cull = op->stride != 0;
        if (!a.workspace || !a.out) return hvn_fail(HVN_E_ARG, "nbr_margins: null pointer");
        if (!a.seg) return hvn_fail(HVN_E_ARG, "nbr_margins: null segment table (bias)");
        if (!a.w2) return hvn_fail(HVN_E_ARG, "nbr_margins: null table of squared widths (w2)");
        if (!a.seg_region) return hvn_fail(HVN_E_ARG, "nbr_margins: null table of segment regions (res)");
        if (!a.rows) return hvn_fail(HVN_E_ARG, "nbr_margins: null row lists (y2)");
        if (a.B < 1 || a.B > HVN_NBR_MARGINS_MAX_B) return hvn_fail(HVN_E_ARG, "nbr_margins: %d widths outside 1..16", a.B);
        if (a.T < 1 || a.T > 16) return hvn_fail(HVN_E_ARG, "nbr_margins: %d types outside 1..16", a.T);
        if (a.G < 1 || a.G > HVN_NBR_MARGINS_MAX_G) return hvn_fail(a.G < 1 ? HVN_E_ARG : HVN_E_SIZE, "nbr_margins: %d regions outside 1..4096", a.G);
        if (a.S < 1) return hvn_fail(HVN_E_ARG, "nbr_margins: %d segments, fewer than one", a.S);
        if (a.S > HVN_NBR_MARGINS_MAX_S) return hvn_fail(HVN_E_SIZE, "nbr_margins: %d segments above 2^22", a.S);
        if (op->y2.sn < 0) return hvn_fail(HVN_E_ARG, "nbr_margins: row lists of %ld entries, fewer than none", (long)op->y2.sn);
        if (int rc = nbr_common("nbr_margins", op, batch)) return rc;
        if ((long)op->y2.sn > HVN_NBR_MARGINS_MAX_ENTRIES(a.S, a.ncy))
            return hvn_fail(HVN_E_SIZE, "nbr_margins: row lists of %ld entries, more than 8 S + kh = %ld", (long)op->y2.sn, HVN_NBR_MARGINS_MAX_ENTRIES(a.S, a.ncy));
        a.M = (int)op->y2.sn;
        if ((long)op->y.sn < HVN_NBR_MARGINS_OUT_BYTES(a.N, a.G, a.B, a.T))
            return hvn_fail(HVN_E_SIZE, "nbr_margins: output of %ld bytes, %ld needed", (long)op->y.sn, HVN_NBR_MARGINS_OUT_BYTES(a.N, a.G, a.B, a.T));
        if (((uintptr_t)a.seg_region | (uintptr_t)a.rows) & 3) return hvn_fail(HVN_E_ARG, "nbr_margins: misaligned seg_region or rows (4)");
        if (((uintptr_t)a.seg | (uintptr_t)a.w2 | (uintptr_t)a.out) & 7) return hvn_fail(HVN_E_ARG, "nbr_margins: misaligned segment table, widths or out (8)");
        return hvn_launch_status(hvn_launch_nbr_margins(a, s), "nbr_margins");
    }
    case HVN_OP_NBR_GRAPH: {
        NbrGraphArgs a;
        a.table = (const double *)op->w;
        a.workspace = op->x2.base;
        a.fill = op->_rsv;
        a.degree = a.fill ? nullptr : (int *)op->y.base;
        a.indices = a.fill ? (int *)op->y.base : nullptr;
        a.indptr = a.fill ? (const long long *)op->y2.base : nullptr;
        a.first = a.fill ? nullptr : (int *)op->y2.base;
        a.width = op->stride;
        a.E = (long long)op->y.sn;
        a.N = op->x.h; a.ncy = op->kh; a.ncx = op->kw;
        if (a.fill != 0 && a.fill != 1) return hvn_fail(HVN_E_ARG, "nbr_graph: `_rsv` = %d is no mode (0: count, 1: fill)", a.fill);
        if (!a.workspace) return hvn_fail(HVN_E_ARG, "nbr_graph: null pointer");
        if (!a.fill && !a.degree) return hvn_fail(HVN_E_ARG, "nbr_graph: null degree (y) of the count pass");
        if (a.first && (a.width < 1 || a.width > HVN_NBR_GRAPH_MAX_WIDTH))
            return hvn_fail(HVN_E_ARG, "nbr_graph: a table (y2) of %d slots per point outside 1..64 (stride)", a.width);
        if (a.fill && !a.indices) return hvn_fail(HVN_E_ARG, "nbr_graph: null indices (y) of the fill pass");
        if (a.fill && !a.indptr) return hvn_fail(HVN_E_ARG, "nbr_graph: null indptr (y2) of the fill pass");
        if (a.fill && a.E < 1) return hvn_fail(HVN_E_ARG, "nbr_graph: indices of %ld entries, fewer than one", (long)a.E);
        if (a.fill && a.E > HVN_NBR_GRAPH_MAX_E) return hvn_fail(HVN_E_SIZE, "nbr_graph: indices of %ld entries reach 2^31", (long)a.E);
        if (int rc = nbr_common("nbr_graph", op, batch)) return rc;
        if ((uintptr_t)op->y.base & 3) return hvn_fail(HVN_E_ARG, "nbr_graph: misaligned degree or indices (4)");
        if (a.fill && ((uintptr_t)a.indptr & 7)) return hvn_fail(HVN_E_ARG, "nbr_graph: misaligned indptr (8)");
        if ((uintptr_t)a.first & 3) return hvn_fail(HVN_E_ARG, "nbr_graph: misaligned table (y2) of the count pass (4)");
        return hvn_launch_status(hvn_launch_nbr_graph(a, s), "nbr_graph");
    }
    case HVN_OP_NBR_FOREST: {
        NbrForestArgs a;
        a.xy = (const double *)op->x.base;
        a.indptr = (const long long *)op->w;
        a.indices = (const int *)op->res.base;
        a.component = (int *)op->y.base;
        a.tree = (unsigned char *)op->y2.base;
        a.workspace = op->x2.base;
        a.E = (long long)op->res.sn;
        a.N = op->x.h; a.phase = op->_rsv; a.round = op->stride; a.no_filter = op->cout != 0;
        if (a.phase < 0 || a.phase > 3) return hvn_fail(HVN_E_ARG, "nbr_forest: `_rsv` = %d is no phase (0: all, 1: start, 2: one round, 3: end)", a.phase);
        if (a.phase == 2 && (a.round < 0 || a.round >= HVN_NBR_FOREST_MAX_ROUNDS))
            return hvn_fail(HVN_E_ARG, "nbr_forest: round %d outside 0..25 (stride)", a.round);
        if (!a.xy) return hvn_fail(HVN_E_ARG, "nbr_forest: null xy (x)");
        if (!a.indptr) return hvn_fail(HVN_E_ARG, "nbr_forest: null indptr (w)");
        if (!a.component) return hvn_fail(HVN_E_ARG, "nbr_forest: null component (y)");
        if (!a.workspace) return hvn_fail(HVN_E_ARG, "nbr_forest: null workspace (x2)");
        if (a.N < 1) return hvn_fail(HVN_E_ARG, "nbr_forest: N = %d, fewer than one point", a.N);
        if (a.N > HVN_NBR_MAX_N) return hvn_fail(HVN_E_SIZE, "nbr_forest: N = %d above 2^26", a.N);
        if (a.E < 0) return hvn_fail(HVN_E_ARG, "nbr_forest: indices of %ld entries, fewer than none", (long)a.E);
        if (a.E > HVN_NBR_FOREST_MAX_E) return hvn_fail(HVN_E_SIZE, "nbr_forest: indices of %ld entries reach 2^31", (long)a.E);
        if (a.E > 0 && !a.indices) return hvn_fail(HVN_E_ARG, "nbr_forest: null indices (res) of %ld entries", (long)a.E);
        if (a.E > 0 && !a.tree) return hvn_fail(HVN_E_ARG, "nbr_forest: null tree (y2) of %ld entries", (long)a.E);
        if (batch != 1) return hvn_fail(HVN_E_ARG, "nbr_forest: batch %d, not 1", batch);
        if ((long)op->x2.sn < HVN_NBR_FOREST_WORKSPACE_BYTES(a.N))
            return hvn_fail(HVN_E_SIZE, "nbr_forest: workspace of %ld bytes, %ld needed", (long)op->x2.sn, HVN_NBR_FOREST_WORKSPACE_BYTES(a.N));
        if ((uintptr_t)a.xy & 7) return hvn_fail(HVN_E_ARG, "nbr_forest: misaligned xy (8)");
        if ((uintptr_t)a.indptr & 7) return hvn_fail(HVN_E_ARG, "nbr_forest: misaligned indptr (8)");
        if ((uintptr_t)a.workspace & 7) return hvn_fail(HVN_E_ARG, "nbr_forest: misaligned workspace (8)");
        if ((uintptr_t)a.indices & 3) return hvn_fail(HVN_E_ARG, "nbr_forest: misaligned indices (4)");
        if ((uintptr_t)a.component & 3) return hvn_fail(HVN_E_ARG, "nbr_forest: misaligned component (4)");
        return hvn_launch_status(hvn_launch_nbr_forest(a, s), "nbr_forest");
    }
    case HVN_OP_INST_TEXTURE: {
        InstTextureArgs a;
        a.image = (const uint8_t *)op->x.base;
        a.inst = (const int32_t *)op->res.base;
        a.rec = (const hvn_inst_rec *)op->w;
        a.out = (int32_t *)op->y.base;
        a.N = batch; a.H = op->x.h; a.W = op->x.w; a.max_inst = op->cout;
        a.fixed = op->_rsv; a.merge = op->stride;
        if (!a.image) return hvn_fail(HVN_E_ARG, "inst_texture: null image (x)");
        if (!a.inst) return hvn_fail(HVN_E_ARG, "inst_texture: null inst (res)");
        if (!a.rec) return hvn_fail(HVN_E_ARG, "inst_texture: null records (w)");
        if (!a.out) return hvn_fail(HVN_E_ARG, "inst_texture: null output (y)");
        if (a.H < 1 || a.W < 1 || a.max_inst < 1) return hvn_fail(HVN_E_ARG, "inst_texture: n, h, w or max_inst < 1 (h = %d, w = %d, max_inst = %d)", a.H, a.W, a.max_inst);
        if ((long)a.H * a.W >= (1L << 31)) return hvn_fail(HVN_E_ARG, "inst_texture: h * w >= 2^31 (h = %d)", a.H);
        if (op->x.c != 3 || op->x_dtype != 0) return hvn_fail(HVN_E_ARG, "inst_texture: the image view is not c = 3 uint8 (c = %d, x_dtype = %d)", op->x.c, op->x_dtype);
        // strides in bytes as VIEW; 0 = dense, and dense is the only form this op reads
        if ((op->x.sx != 0 && op->x.sx != 3) || (op->x.sy != 0 && op->x.sy != 3L * a.W) || (op->x.sn != 0 && op->x.sn != 3L * a.H * a.W))
            return hvn_fail(HVN_E_ARG, "inst_texture: the image view is not dense (sy = %ld)", (long)op->x.sy);
        if (a.fixed != 0 && a.fixed != 1) return hvn_fail(HVN_E_ARG, "inst_texture: `_rsv` = %d is no scale mode (0: range, 1: fixed)", a.fixed);
        if (a.merge != 0 && a.merge != 1) return hvn_fail(HVN_E_ARG, "inst_texture: `stride` = %d is no accumulation form (0: plain, 1: merged)", a.merge);
        if (((uintptr_t)a.out & 7) || ((uintptr_t)a.rec & 7)) return hvn_fail(HVN_E_ARG, "inst_texture: misaligned output or records (8)");
        if ((uintptr_t)a.inst & 3) return hvn_fail(HVN_E_ARG, "inst_texture: misaligned inst (4)");
        if ((long)a.N * a.max_inst >= (1L << 31)) return hvn_fail(HVN_E_SIZE, "inst_texture: n * max_inst >= 2^31 (%ld slots)", (long)a.N * a.max_inst);
        return hvn_launch_status(hvn_launch_inst_texture(a, s), "inst_texture");
    }
    default:
        return hvn_fail(HVN_E_ARG, "unknown op kind %d", op->kind);
    }
}

extern "C" {

int hvn_run_op(const hvn_op *op, int batch, void *stream)
{
    if (!op || batch <= 0) return hvn_fail(HVN_E_ARG, "run_op: bad arguments");
    return hvn_internal_run_one(op, batch, (hipStream_t)stream);     // its refusals lead with the op's name ("conv: ...")
}

int hvn_extract_patches(const uint8_t *img, int h, int w, const int32_t *coords, int n_patches, int win, int pad_t, int pad_l,
                        uint8_t *out, void *stream)
{
    if (!img || !coords || !out || h <= 0 || w <= 0 || n_patches <= 0 || win <= 0 || pad_t < 0 || pad_l < 0)
        return hvn_fail(HVN_E_ARG, "extract_patches: bad arguments");
    int rc = hvn_launch_extract_patches(img, h, w, coords, n_patches, win, pad_t, pad_l, out, (hipStream_t)stream);
    if (rc) return hvn_fail(HVN_E_LAUNCH, "extract_patches: launch failed");
    return 0;
}

int hvn_resize_window(const uint8_t *src, int src_h, int src_w, int64_t src_pitch, int src_y0, int src_x0, int full_h, int full_w,
                      const int32_t *xofs, const int16_t *xcoef, const int32_t *yofs, const int16_t *ycoef, int taps, uint8_t *dst, int dst_h,
                      int dst_w, void *stream)
{
    if (!src || !xofs || !xcoef || !yofs || !ycoef || !dst) return hvn_fail(HVN_E_ARG, "resize_window: null pointer");
    if (taps != 2 && taps != 4) return hvn_fail(HVN_E_ARG, "resize_window: taps = %d (2 = linear, 4 = cubic)", taps);
    if (((uintptr_t)xofs & 3) || ((uintptr_t)yofs & 3) || ((uintptr_t)xcoef & 1) || ((uintptr_t)ycoef & 1))
        return hvn_fail(HVN_E_ARG, "resize_window: misaligned table");
    if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0 || full_h <= 0 || full_w <= 0)
        return hvn_fail(HVN_E_ARG, "resize_window: empty source, window or destination");
    // offsets within a row are 32-bit: 3 * width (and taps * width, the coefficient index) must fit
    if (src_w > (1 << 29) || dst_w > (1 << 29) || dst_h > (1 << 29)) return hvn_fail(HVN_E_ARG, "resize_window: a row longer than 2^29 pixels");
    if (src_pitch < 3 * (int64_t)src_w) return hvn_fail(HVN_E_ARG, "resize_window: src_pitch %ld is shorter than a source row", (long)src_pitch);
    // the uploaded box must lie in the full source: taps are clamped against the full source, then translated into the box
    if (src_y0 < 0 || src_x0 < 0 || (int64_t)src_y0 + src_h > full_h || (int64_t)src_x0 + src_w > full_w)
        return hvn_fail(HVN_E_ARG, "resize_window: the uploaded source box leaves the full source");
    int rc = hvn_launch_resize_window(src, src_h, src_w, src_pitch, src_y0, src_x0, full_h, full_w, xofs, xcoef, yofs, ycoef, taps, dst, dst_h,
                                      dst_w, (hipStream_t)stream);
    if (rc == HVN_E_SIZE) return hvn_fail(HVN_E_SIZE, "resize_window: %d output rows are more than one launch takes (16 * 65535)", dst_h);
    if (rc) return hvn_fail(HVN_E_LAUNCH, "resize_window: launch failed");
    return 0;
}

// the tissue mask's common refusals: 0 = the extent is one the kernels index with int32
static int tissue_extent(const char *what, int h, int w)
{
    if (h < 1 || w < 1) return hvn_fail(HVN_E_ARG, "%s: h or w < 1 (h = %d)", what, h);
    if ((int64_t)h * w > ((int64_t)1 << 30)) return hvn_fail(HVN_E_SIZE, "%s: h * w > 2^30 (h = %d)", what, h);
    return 0;
}

int hvn_tissue_gray_hist(const uint8_t *rgb, int h, int w, uint8_t *gray, uint32_t *hist256, void *stream)
{
    if (!rgb || !gray || !hist256) return hvn_fail(HVN_E_ARG, "tissue_gray_hist: null pointer");
    if ((uintptr_t)hist256 & 3) return hvn_fail(HVN_E_ARG, "tissue_gray_hist: misaligned hist256");
    if (int rc = tissue_extent("tissue_gray_hist", h, w)) return rc;
    if (hvn_launch_tissue_gray_hist(rgb, h, w, gray, hist256, (hipStream_t)stream)) return hvn_fail(HVN_E_LAUNCH, "tissue_gray_hist: launch failed");
    return 0;
}

size_t hvn_tissue_mask_workspace_bytes(int h, int w)
{
    if (h < 1 || w < 1 || (int64_t)h * w > ((int64_t)1 << 30)) return 0;
    return hvn_tissue_workspace_bytes(h, w);
}

int hvn_tissue_mask(const uint8_t *gray, int h, int w, int threshold, int min_obj, int max_hole, int radius, uint8_t *mask,
                    uint8_t *tap_objects, uint8_t *tap_holes, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!gray || !mask || !workspace) return hvn_fail(HVN_E_ARG, "tissue_mask: null pointer");
    if (int rc = tissue_extent("tissue_mask", h, w)) return rc;
    if (radius < 0 || radius > 32) return hvn_fail(HVN_E_ARG, "tissue_mask: radius %d outside [0, 32]", radius);
    if ((uintptr_t)workspace & 15) return hvn_fail(HVN_E_ARG, "tissue_mask: workspace is not 16-byte aligned");
    if (workspace_bytes < hvn_tissue_workspace_bytes(h, w))
        return hvn_fail(HVN_E_SIZE, "tissue_mask: workspace smaller than hvn_tissue_mask_workspace_bytes (%zu bytes given)", workspace_bytes);
    if (hvn_launch_tissue_mask(gray, h, w, threshold, min_obj, max_hole, radius, mask, tap_objects, tap_holes, workspace, (hipStream_t)stream))
        return hvn_fail(HVN_E_LAUNCH, "tissue_mask: launch failed");
    return 0;
}

int hvn_viz_strip(const uint8_t *img, int n, int ih, int iw, const float *pred, int c, const int32_t *np_map, const float *hv_map,
                  const int32_t *tp_map, int h, int w, int nr_types, const int32_t *sel, int n_sel, const uint8_t *lut, uint8_t *out,
                  int n_blocks, void *stream)
{
    if (!img || !pred || !np_map || !hv_map || !lut || !out || (n_sel > 0 && !sel)) return hvn_fail(HVN_E_ARG, "viz_strip: null pointer");
    if (n < 1 || h < 1 || w < 1 || n_blocks < 1) return hvn_fail(HVN_E_ARG, "viz_strip: n, h, w or n_blocks < 1 (h = %d)", h);
    if (n_sel < 0 || n_sel > 65535) return hvn_fail(HVN_E_ARG, "viz_strip: n_sel %d outside [0, 65535]", n_sel);
    if (ih < h || iw < w) return hvn_fail(HVN_E_ARG, "viz_strip: the image is smaller than the maps (ih = %d)", ih);
    if (c != 3 && c != 4) return hvn_fail(HVN_E_ARG, "viz_strip: c = %d, not 3 or 4", c);
    if (nr_types < 0 || nr_types > 16) return hvn_fail(HVN_E_ARG, "viz_strip: nr_types %d outside [0, 16]", nr_types);
    if ((nr_types > 0) != (c == 4)) return hvn_fail(HVN_E_ARG, "viz_strip: nr_types > 0 goes with c == 4 and nr_types == 0 with c == 3 (c = %d)", c);
    if (((uintptr_t)pred | (uintptr_t)np_map | (uintptr_t)hv_map | (uintptr_t)tp_map | (uintptr_t)sel) & 3)
        return hvn_fail(HVN_E_ARG, "viz_strip: misaligned pred, map or sel");
    if ((int64_t)2 * h * 5 * w > ((int64_t)1 << 30)) return hvn_fail(HVN_E_SIZE, "viz_strip: 2h * 5w > 2^30 (h = %d)", h);
    if (n_sel == 0) return 0;
    if (hvn_launch_viz_strip(img, n, ih, iw, pred, c, np_map, hv_map, tp_map, h, w, nr_types, sel, n_sel, lut, out, n_blocks, (hipStream_t)stream))
        return hvn_fail(HVN_E_LAUNCH, "viz_strip: launch failed");
    return 0;
}

int hvn_run_plan(const hvn_op *ops, int n_ops, int batch, void *stream)
{
    if (!ops || n_ops <= 0 || batch <= 0) return hvn_fail(HVN_E_ARG, "run_plan: bad arguments");
    for (int i = 0; i < n_ops; ++i) {
        int rc = hvn_internal_run_one(&ops[i], batch, (hipStream_t)stream);
        if (rc) return hvn_fail_in_op(rc, "run_plan", i);
    }
    return 0;
}

}  // extern "C"

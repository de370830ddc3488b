// hvn_train_api.hip -- C ABI of the training step (include/hvn.h, "training" section): descriptor validation and
// dispatch of hvn_top lists, the loss stages and the Adam update.  Refusals go through hvn_fail (hvn_error.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include "hvn_kernels.h"

// PACK_MULTI's device table is written by the host as hvn_pack_desc (include/hvn.h) and read by the kernel as PackArgs
static_assert(sizeof(hvn_pack_desc) == sizeof(PackArgs) && offsetof(hvn_pack_desc, gmat) == offsetof(PackArgs, gmat) &&
              offsetof(hvn_pack_desc, lead_pad) == offsetof(PackArgs, lead_pad) && offsetof(hvn_pack_desc, cout) == offsetof(PackArgs, cout),
              "hvn_pack_desc must mirror PackArgs");

static inline bool al16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
static inline bool view_ok(const hvn_view &v) { return v.base && al16(v.base) && ((v.sn | v.sy | v.sx) & 3) == 0 && (v.c & 3) == 0; }
// The kernels of BN, UPADD_BWD and HEAD_BWD take N, H, W, C from ONE view and walk the others with them: every other view must
// have the extent that view implies (include/hvn.h, "extent rules"), or the kernel would read and write outside it.
static inline bool same_extent(const hvn_view &v, int h, int w, int c) { return v.h == h && v.w == w && v.c == c; }

// The arguments of the three op kinds that end in a cross-workgroup sum, filled from the descriptor (shared by the launch path and by
// hvn_train_workspace_bytes, so that both see the same launch shape).
static int wgrad_args(const hvn_top *t, int batch, WgradArgs &a)
{
    memset(&a, 0, sizeof(a));
    if (!view_ok(t->x) || !view_ok(t->dy) || !t->p[0]) return HVN_E_ARG;
    a.x = (const float *)t->x.base; a.xsn = t->x.sn; a.xsy = t->x.sy; a.xsx = t->x.sx; a.H = t->x.h; a.W = t->x.w; a.Cin = t->x.c;
    a.dy = (const float *)t->dy.base; a.dsn = t->dy.sn; a.dsy = t->dy.sy; a.dsx = t->dy.sx; a.Ho = t->dy.h; a.Wo = t->dy.w; a.Cout = t->dy.c;
    a.dw = (float *)t->p[0];
    a.N = batch; a.KH = t->kh; a.KW = t->kw; a.stride = t->stride; a.pad_t = t->pad_t; a.pad_l = t->pad_l;
    a.groups = t->groups > 1 ? t->groups : 1; a.Cin_g = a.Cin / a.groups;
    a.nbatch = t->nbatch > 1 ? t->nbatch : 1;
    a.xb = t->batch_stride[0]; a.db = t->batch_stride[1]; a.wb = t->batch_stride[2];
    a.want_wgs = t->mode > 0 ? t->mode : 0;
    return 0;
}
static int conv0_wgrad_args(const hvn_top *t, int batch, Conv0WgradArgs &a)
{
    memset(&a, 0, sizeof(a));
    if (!t->x.base || !view_ok(t->dy) || !t->p[0] || t->dy.c != 64 || t->x.c != 3) return HVN_E_ARG;
    a.img = (const uint8_t *)t->x.base; a.isn = t->x.sn; a.isy = t->x.sy; a.isx = t->x.sx; a.H = t->x.h; a.W = t->x.w;
    a.dy = (const float *)t->dy.base; a.ysn = t->dy.sn; a.ysy = t->dy.sy; a.ysx = t->dy.sx;
    a.dw = (float *)t->p[0];
    a.N = batch; a.Ho = t->dy.h; a.Wo = t->dy.w; a.pad = t->pad_t;
    return 0;
}
static int head_bwd_args(const hvn_top *t, int batch, HeadBwdArgs &a)
{
    memset(&a, 0, sizeof(a));
    if (!view_ok(t->x) || !view_ok(t->dx) || t->x.c != 64 || !t->p[0] || !t->p[1] || !t->p[2] || !t->p[3]) return HVN_E_ARG;
    a.x = (const float *)t->x.base; a.xsn = t->x.sn; a.xsy = t->x.sy; a.xsx = t->x.sx;
    a.dx = (float *)t->dx.base; a.dsn = t->dx.sn; a.dsy = t->dx.sy; a.dsx = t->dx.sx;
    a.dl = (const float *)t->p[0]; a.w = (const float *)t->p[1]; a.dw = (float *)t->p[2]; a.db = (float *)t->p[3];
    a.N = batch; a.H = t->x.h; a.W = t->x.w; a.Cout = t->cout;
    return 0;
}

// The extent rules of include/hvn.h for one op.  hvn_run_train_plan_ws applies them to EVERY op of the list before it launches the
// first one, so that a list with a bad descriptor anywhere leaves the device untouched.
static int extent_rules(const hvn_top *t, int batch)
{
    switch (t->kind) {
    case HVN_T_BN_FWD:
    case HVN_T_BN_BWD: {
        const int h = t->x.h, w = t->x.w, c = t->x.c;
        if (h <= 0 || w <= 0 || c <= 0) return hvn_fail(HVN_E_ARG, "bn: z has an empty extent (h = %d, w = %d, c = %d)", h, w, c);
        if (!same_extent(t->y, h, w, c))
            return hvn_fail(HVN_E_ARG, "bn: the a view's extent (%d, %d, %d) differs from z's (%d, %d, %d)", t->y.h, t->y.w, t->y.c, h, w, c);
        if (t->kind == HVN_T_BN_FWD) {
            if ((long)batch * h * w < 2)
                return hvn_fail(HVN_E_ARG, "bn forward: one value per channel has no unbiased variance (batch * h * w = %ld < 2)", (long)batch * h * w);
            return HVN_OK;
        }
        if (!same_extent(t->dy, h, w, c))
            return hvn_fail(HVN_E_ARG, "bn backward: the da view's extent (%d, %d, %d) differs from z's (%d, %d, %d)", t->dy.h, t->dy.w, t->dy.c, h, w, c);
        if (t->dx.base && !same_extent(t->dx, h, w, c))
            return hvn_fail(HVN_E_ARG, "bn backward: the dz view's extent (%d, %d, %d) differs from z's (%d, %d, %d)", t->dx.h, t->dx.w, t->dx.c, h, w, c);
        return HVN_OK;
    }
    case HVN_T_UPADD_BWD: {
        const int h = t->dy.h, w = t->dy.w, c = t->dy.c;
        if (!t->dx.base && !t->y.base) return hvn_fail(HVN_E_ARG, "upadd backward: both dlo and dskip are NULL");
        if (h <= 0 || w <= 0 || c <= 0 || (h | w) & 1) return hvn_fail(HVN_E_ARG, "upadd backward: extent must be even (dy is %d x %d x %d)", h, w, c);
        if (t->dx.base && !same_extent(t->dx, h / 2, w / 2, c))
            return hvn_fail(HVN_E_ARG, "upadd backward: dlo must be (h / 2, w / 2, c) of dy (dlo is %d x %d x %d, dy %d x %d x %d)", t->dx.h, t->dx.w,
                            t->dx.c, h, w, c);
        if (t->y.base && !same_extent(t->y, h, w, c))
            return hvn_fail(HVN_E_ARG, "upadd backward: dskip must be (h, w, c) of dy (dskip is %d x %d x %d, dy %d x %d x %d)", t->y.h, t->y.w, t->y.c,
                            h, w, c);
        return HVN_OK;
    }
    case HVN_T_HEAD_BWD:
        if (t->x.h <= 0 || t->x.w <= 0) return hvn_fail(HVN_E_ARG, "head backward: x has an empty extent (h = %d, w = %d)", t->x.h, t->x.w);
        if (!same_extent(t->dx, t->x.h, t->x.w, t->x.c))
            return hvn_fail(HVN_E_ARG, "head backward: the dx view's extent (%d, %d, %d) differs from x's (%d, %d, %d)", t->dx.h, t->dx.w, t->dx.c, t->x.h,
                            t->x.w, t->x.c);
        return HVN_OK;
    default:
        return HVN_OK;
    }
}

// ws / ws_floats: the deterministic-reduce workspace of hvn_run_train_plan_ws (NULL: atomics)
static int run_top(const hvn_top *t, int batch, hipStream_t s, float *ws, long ws_floats)
{
    switch (t->kind) {
    case HVN_T_NET:
        if (!t->net) return hvn_fail(HVN_E_ARG, "null net op");
        return hvn_internal_run_one(t->net, batch, s);       // leaves its own text
    case HVN_T_PACK_W: {
        PackArgs a;
        a.src = (const float *)t->p[0]; a.dst = (float *)t->p[1];
        a.cout = t->cout; a.cin_g = t->cin_g; a.groups = t->groups > 1 ? t->groups : 1; a.taps = t->kh * t->kw;
        a.mode = t->mode; a.lead_pad = t->lead_pad; a.gmat = (const float *)t->p[2];
        if (!a.src || !a.dst) return hvn_fail(HVN_E_ARG, "pack: null pointer");
        if ((a.mode == 3 || a.mode == 4) && (!a.gmat || a.taps != 25 || a.groups != 1 || (a.mode == 3 ? a.cin_g : a.cout) % 32))
            return hvn_fail(HVN_E_ARG, "pack: Winograd transform needs a 5x5 ungrouped conv, G and k %% 32 == 0");
        if (a.mode == 0 && ((a.cin_g * a.groups) % 32 || a.lead_pad < a.cout)) return hvn_fail(HVN_E_ARG, "pack: forward needs cin %% 32 == 0");
        if (a.mode == 1 && (a.cout % 32 || a.lead_pad < a.cin_g * a.groups)) return hvn_fail(HVN_E_ARG, "pack: dgrad needs cout %% 32 == 0");
        return hvn_launch_status(hvn_launch_pack_w(a, s), "pack");
    }
    case HVN_T_BN_FWD:
    case HVN_T_BN_BWD: {
        BnArgs a;
        memset(&a, 0, sizeof(a));
        const bool fwd = t->kind == HVN_T_BN_FWD;
        if (!view_ok(t->x) || !view_ok(t->y)) return hvn_fail(HVN_E_ARG, "bn: bad z / a view");
        a.z = (const float *)t->x.base; a.zsn = t->x.sn; a.zsy = t->x.sy; a.zsx = t->x.sx;
        a.a = (const float *)t->y.base; a.a_out = (float *)t->y.base; a.asn = t->y.sn; a.asy = t->y.sy; a.asx = t->y.sx;
        a.N = batch; a.H = t->x.h; a.W = t->x.w; a.C = t->x.c;
        a.ws = (double *)t->p[0]; a.save = (float *)t->p[1]; a.gamma = (const float *)t->p[2];
        a.eps = t->eps; a.momentum = t->momentum;
        if (!a.ws || !a.save || !a.gamma) return hvn_fail(HVN_E_ARG, "bn: null pointer");
        if (fwd) {
            a.beta = (const float *)t->p[3]; a.running_mean = (float *)t->p[4]; a.running_var = (float *)t->p[5];
            if (!a.beta || !a.running_mean || !a.running_var) return hvn_fail(HVN_E_ARG, "bn forward: null pointer");
            return hvn_launch_status(hvn_launch_bn_forward(a, s), "bn forward");
        }
        if (!view_ok(t->dy)) return hvn_fail(HVN_E_ARG, "bn backward: bad da view");
        a.da = (const float *)t->dy.base; a.gsn = t->dy.sn; a.gsy = t->dy.sy; a.gsx = t->dy.sx;
        if (t->dx.base) {
            if (!view_ok(t->dx)) return hvn_fail(HVN_E_ARG, "bn backward: bad dz view");
            a.dz = (float *)t->dx.base; a.dsn = t->dx.sn; a.dsy = t->dx.sy; a.dsx = t->dx.sx;
        }
        a.dz_store = t->mode & 1;
        a.dgamma = (float *)t->p[3]; a.dbeta = (float *)t->p[4]; a.coef = (float *)t->p[5];
        if (!a.dgamma || !a.dbeta || !a.coef) return hvn_fail(HVN_E_ARG, "bn backward: null pointer");
        return hvn_launch_status(hvn_launch_bn_backward(a, s), "bn backward");
    }
    case HVN_T_WGRAD: {
        WgradArgs a;
        if (wgrad_args(t, batch, a)) return hvn_fail(HVN_E_ARG, "wgrad: bad view");
        if ((long)batch * a.Ho * a.Wo >= (1L << 31)) return hvn_fail(HVN_E_ARG, "wgrad: too many rows");
        const int x3 = t->_pad;     // 6 | 9: products on the bf16 pipe (bf16x3 splits of both operands) where the shape has that form
        if (x3 != 0 && x3 != 6 && x3 != 9) return hvn_fail(HVN_E_ARG, "wgrad: _pad selects the bf16x3 form with 6 or 9 partial products (0: fp32 pipe)");
        a.part = ws; a.part_cap = ws_floats;
        int rc = (x3 && hvn_wgrad_x3_supported(a)) ? hvn_launch_wgrad_x3(a, x3, s) : hvn_launch_wgrad(a, s);
        if (rc == HVN_E_ARG) return hvn_fail(rc, "wgrad: unsupported channel counts");
        if (rc == HVN_E_SIZE) return hvn_fail(rc, "wgrad: workspace smaller than hvn_train_workspace_bytes");
        return hvn_launch_status(rc, "wgrad");
    }
    case HVN_T_CONV0_WGRAD: {
        Conv0WgradArgs a;
        if (conv0_wgrad_args(t, batch, a)) return hvn_fail(HVN_E_ARG, "conv0 wgrad: bad arguments");
        a.part = ws; a.part_cap = ws_floats;
        int rc = hvn_launch_conv0_wgrad(a, s);
        if (rc == HVN_E_SIZE) return hvn_fail(rc, "conv0 wgrad: workspace smaller than hvn_train_workspace_bytes");
        return hvn_launch_status(rc, "conv0 wgrad");
    }
    case HVN_T_UPADD_BWD: {
        UpAddBwdArgs a;
        memset(&a, 0, sizeof(a));
        if (!view_ok(t->dy)) return hvn_fail(HVN_E_ARG, "upadd backward: bad dy view");
        a.dy = (const float *)t->dy.base; a.ysn = t->dy.sn; a.ysy = t->dy.sy; a.ysx = t->dy.sx;
        if (t->dx.base) {
            if (!view_ok(t->dx)) return hvn_fail(HVN_E_ARG, "upadd backward: bad dlo view");
            a.dlo = (float *)t->dx.base; a.lsn = t->dx.sn; a.lsy = t->dx.sy; a.lsx = t->dx.sx;
        }
        if (t->y.base) {
            if (!view_ok(t->y)) return hvn_fail(HVN_E_ARG, "upadd backward: bad dskip view");
            a.dskip = (float *)t->y.base; a.ssn = t->y.sn; a.ssy = t->y.sy; a.ssx = t->y.sx;
        }
        a.N = batch; a.H = t->dy.h; a.W = t->dy.w; a.C = t->dy.c;
        int rc = hvn_launch_upadd_bwd(a, s);
        if (rc == HVN_E_ARG) return hvn_fail(rc, "upadd backward: extent must be even");
        return hvn_launch_status(rc, "upadd backward");
    }
    case HVN_T_HEAD_BWD: {
        HeadBwdArgs a;
        if (head_bwd_args(t, batch, a)) return hvn_fail(HVN_E_ARG, "head backward: bad arguments");
        a.part = ws; a.part_cap = ws_floats;
        int rc = hvn_launch_head_bwd(a, s);
        if (rc == HVN_E_ARG) return hvn_fail(rc, "head backward: 1..16 output channels");
        if (rc == HVN_E_SIZE) return hvn_fail(rc, "head backward: workspace smaller than hvn_train_workspace_bytes");
        return hvn_launch_status(rc, "head backward");
    }
    case HVN_T_WINO_DY: {
        WinoArgs a;
        memset(&a, 0, sizeof(a));
        if (!view_ok(t->x) || !t->y.base || !al16(t->y.base) || !t->p[0]) return hvn_fail(HVN_E_ARG, "wino_dy: bad arguments");
        a.x = (const float *)t->x.base; a.xsn = t->x.sn; a.xsy = t->x.sy; a.xsx = t->x.sx;
        a.y = (float *)t->y.base; a.ysn = t->y.sn; a.ysy = t->y.sy; a.ysx = t->y.sx;
        a.mat = (const float *)t->p[0];
        a.N = batch; a.H = t->x.h; a.W = t->x.w; a.C = t->x.c; a.ty = t->kh; a.tx = t->kw; a.m = 4;
        if (t->y.h != 64 || t->y.w != a.ty * a.tx || t->y.c != a.C || 4 * a.ty < a.H || 4 * a.tx < a.W)
            return hvn_fail(HVN_E_ARG, "wino_dy: dM must be [64][tiles][c] and the tiles must cover dy");
        return hvn_launch_status(hvn_launch_wino_dy(a, s), "wino_dy");
    }
    case HVN_T_PACK_MULTI:
        if (!t->p[0] || !t->p[1] || t->cout <= 0 || t->batch_stride[0] <= 0) return hvn_fail(HVN_E_ARG, "pack_multi: bad arguments");
        if (hvn_launch_pack_w_multi((const PackArgs *)t->p[0], (const int *)t->p[1], t->cout, (long)t->batch_stride[0], s))
            return hvn_fail(HVN_E_ARG, "pack_multi: launch refused");
        return 0;
    case HVN_T_SPLIT_X3:
        if (!t->p[0] || !t->p[1] || t->batch_stride[0] <= 0) return hvn_fail(HVN_E_ARG, "split_x3: bad arguments");
        if (hvn_launch_split_x3((const float *)t->p[0], (uint16_t *)t->p[1], (long)t->batch_stride[0], s)) return hvn_fail(HVN_E_ARG, "split_x3: launch refused");
        return 0;
    case HVN_T_WINO_DW:
        if (!t->p[0] || !t->p[1] || !t->p[2] || t->cout <= 0 || t->cin_g <= 0) return hvn_fail(HVN_E_ARG, "wino_dw: bad arguments");
        return hvn_launch_status(hvn_launch_wino_dw((const float *)t->p[0], (float *)t->p[1], (const float *)t->p[2], t->cout, t->cin_g, s), "wino_dw");
    default:
        return hvn_fail(HVN_E_ARG, "unknown kind %d", t->kind);
    }
}

extern "C" {

const char *hvn_train_last_error(void) { return hvn_last_error(); }      // an alias kept for existing callers

int hvn_run_train_plan_ws(const hvn_top *ops, int n_ops, int batch, void *stream, void *workspace, size_t workspace_bytes)
{
    if (!ops || n_ops <= 0 || batch <= 0) return hvn_fail(HVN_E_ARG, "run_train_plan_ws: ops NULL, or n_ops or batch < 1");
    if (workspace && !al16(workspace)) return hvn_fail(HVN_E_ARG, "run_train_plan_ws: workspace must be 16-byte aligned");
    for (int i = 0; i < n_ops; ++i)          // every extent rule, over the whole list, before the first launch
        if (int rc = extent_rules(&ops[i], batch)) return hvn_fail_in_op(rc, "train", i);
    for (int i = 0; i < n_ops; ++i) {
        int rc = run_top(&ops[i], batch, (hipStream_t)stream, (float *)workspace, workspace ? (long)(workspace_bytes / sizeof(float)) : 0);
        if (rc) return hvn_fail_in_op(rc, "train", i);
    }
    return HVN_OK;
}

int hvn_run_train_plan(const hvn_top *ops, int n_ops, int batch, void *stream) { return hvn_run_train_plan_ws(ops, n_ops, batch, stream, NULL, 0); }

size_t hvn_train_workspace_bytes(const hvn_top *ops, int n_ops, int batch)
{
    long need = 0;
    if (!ops || batch <= 0) return 0;
    for (int i = 0; i < n_ops; ++i) {
        const hvn_top *t = &ops[i];
        long f = 0;
        if (t->kind == HVN_T_WGRAD) {
            WgradArgs a;
            if (!wgrad_args(t, batch, a)) f = hvn_wgrad_part_floats(a, t->_pad);
        } else if (t->kind == HVN_T_CONV0_WGRAD) {
            Conv0WgradArgs a;
            if (!conv0_wgrad_args(t, batch, a)) f = hvn_conv0_wgrad_part_floats(a);
        } else if (t->kind == HVN_T_HEAD_BWD) {
            HeadBwdArgs a;
            if (!head_bwd_args(t, batch, a) && a.Cout >= 1 && a.Cout <= 16) f = hvn_head_bwd_part_floats(a);
        }
        if (f > need) need = f;
    }
    return (size_t)need * sizeof(float);
}

// what: the entry point's name in the refusal's text
static int loss_common(const char *what, const hvn_loss *l, LossArgs &a)
{
    if (!l) return hvn_fail(HVN_E_ARG, "%s: null descriptor", what);
    if (!l->logits_np || !l->logits_hv || !l->true_np || !l->true_hv || !l->sums || !l->sobel_ws)
        return hvn_fail(HVN_E_ARG, "%s: null np / hv logits or targets, sums or sobel_ws", what);
    if (l->nr_types > 0 && (!l->logits_tp || !l->true_tp)) return hvn_fail(HVN_E_ARG, "%s: nr_types > 0 needs logits_tp and true_tp", what);
    if (l->nr_types < 0 || l->nr_types > 16 || l->n <= 0 || l->h <= 0 || l->w <= 0)
        return hvn_fail(HVN_E_ARG, "%s: nr_types outside [0, 16], or n, h or w < 1 (nr_types = %d)", what, l->nr_types);
    memset(&a, 0, sizeof(a));
    a.l_np = l->logits_np; a.l_hv = l->logits_hv; a.l_tp = l->logits_tp;
    a.t_np = l->true_np; a.t_tp = l->true_tp; a.t_hv = l->true_hv;
    a.d_np = l->grad_np; a.d_hv = l->grad_hv; a.d_tp = l->grad_tp;
    a.sums = l->sums; a.gws = l->sobel_ws;
    a.N = l->n; a.H = l->h; a.W = l->w; a.T = l->nr_types;
    a.m_total = l->total_pixels;
    for (int i = 0; i < 6; ++i) {
        if (!(l->weight[i] >= 0.f)) return hvn_fail(HVN_E_ARG, "%s: weight[%d] is negative or NaN", what, i);
        a.wt[i] = l->weight[i];
    }
    a.parts = l->partials;
    a.parts_cap = l->partials ? (long)l->partials_cap : 0;
    return HVN_OK;
}

int hvn_loss_forward(const hvn_loss *l, void *stream)
{
    LossArgs a;
    if (int rc = loss_common("loss_forward", l, a)) return rc;
    int rc = hvn_launch_loss(a, 0, (hipStream_t)stream);
    if (rc == HVN_E_SIZE) return hvn_fail(rc, "loss_forward: partials smaller than hvn_loss_partials_count doubles");
    return hvn_launch_status(rc, "loss_forward");
}

int hvn_loss_backward(const hvn_loss *l, void *stream)
{
    LossArgs a;
    if (int rc = loss_common("loss_backward", l, a)) return rc;
    if (!l->grad_np || !l->grad_hv || (l->nr_types > 0 && !l->grad_tp)) return hvn_fail(HVN_E_ARG, "loss_backward: null gradient pointer");
    if (!(l->total_pixels > 0)) return hvn_fail(HVN_E_ARG, "loss_backward: total_pixels must be positive");
    return hvn_launch_status(hvn_launch_loss(a, 1, (hipStream_t)stream), "loss_backward");
}

int64_t hvn_loss_partials_count(int n, int h, int w) { return (n > 0 && h > 0 && w > 0) ? (int64_t)hvn_loss_part_doubles(n, h, w) : 0; }

size_t hvn_gen_targets_workspace_bytes(int n, int h, int w) { return (n > 0 && h > 0 && w > 0) ? hvn_targets_ws_bytes(n, h, w) : 0; }

int hvn_gen_targets(const int32_t *ann, int n, int h, int w, int crop_h, int crop_w, float *hv_map, int32_t *np_map, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    if (!ann || !hv_map || !np_map || !workspace) return hvn_fail(HVN_E_ARG, "gen_targets: null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || (long)h * w >= (1L << 31)) return hvn_fail(HVN_E_ARG, "gen_targets: n, h or w < 1, or h * w >= 2^31 (h = %d)", h);
    if (crop_h <= 0 || crop_w <= 0 || crop_h > h || crop_w > w) return hvn_fail(HVN_E_ARG, "gen_targets: the crop must lie in the map (crop_h = %d)", crop_h);
    int rc = hvn_launch_gen_targets(ann, n, h, w, crop_h, crop_w, hv_map, np_map, workspace, workspace_bytes, (hipStream_t)stream);
    if (rc == HVN_E_SIZE) return hvn_fail(rc, "gen_targets: workspace smaller than hvn_gen_targets_workspace_bytes (%zu bytes given)", workspace_bytes);
    return hvn_launch_status(rc, "gen_targets");
}

static bool valid_shape_ok(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (long long)n * h * w <= (1LL << 36); }

size_t hvn_valid_stats_workspace_bytes(int n, int h, int w) { return valid_shape_ok(n, h, w) ? hvn_valid_ws_bytes((long)n * h * w) : 0; }

int hvn_valid_stats(const float *pred, const int32_t *np_map, const float *hv_map, const int32_t *tp_map, int n, int h, int w, int c,
                    int nr_types, int64_t *counts, double *hv_sse, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!pred || !np_map || !hv_map || !counts || !hv_sse) return hvn_fail(HVN_E_ARG, "valid_stats: null pointer");
    if (!valid_shape_ok(n, h, w)) return hvn_fail(HVN_E_ARG, "valid_stats: n, h, w must be positive (at most 2^36 pixels)");
    if (c != 3 && c != 4) return hvn_fail(HVN_E_ARG, "valid_stats: the prediction map has 3 or 4 channels (c = %d)", c);
    if (nr_types < 0 || nr_types > 16) return hvn_fail(HVN_E_ARG, "valid_stats: nr_types %d outside [0, 16]", nr_types);
    if (c == 3 && (tp_map || nr_types > 0)) return hvn_fail(HVN_E_ARG, "valid_stats: a 3-channel map has no type channel (tp_map NULL, nr_types 0)");
    if (c == 4 && (!tp_map || nr_types == 0)) return hvn_fail(HVN_E_ARG, "valid_stats: a 4-channel map needs tp_map and nr_types > 0");
    if (!al16(pred) || (((uintptr_t)hv_map) & 7) || (((uintptr_t)np_map | (uintptr_t)tp_map) & 3) || (((uintptr_t)counts | (uintptr_t)hv_sse) & 7))
        return hvn_fail(HVN_E_ARG, "valid_stats: pred must be 16-byte, hv_map / counts / hv_sse 8-byte, np_map / tp_map 4-byte aligned");
    if (!workspace || workspace_bytes < hvn_valid_stats_workspace_bytes(n, h, w))
        return hvn_fail(HVN_E_SIZE, "valid_stats: workspace NULL or smaller than hvn_valid_stats_workspace_bytes (%zu bytes given)", workspace_bytes);
    int rc = hvn_launch_valid_stats(pred, np_map, hv_map, tp_map, (long)n * h * w, c, nr_types, (long long *)counts, hv_sse, workspace,
                                    workspace_bytes, (hipStream_t)stream);
    if (rc == HVN_E_SIZE) return hvn_fail(rc, "valid_stats: workspace too small");
    return hvn_launch_status(rc, "valid_stats");
}

int hvn_augment_shape(const uint8_t *img, const int32_t *ann, int n_resident, int h, int w, int c, const hvn_aug_sample *prm, int n, int out_h,
                      int out_w, uint8_t *out_img, int32_t *out_ann, void *stream)
{
    if (!img || !ann || !prm || !out_img || !out_ann) return hvn_fail(HVN_E_ARG, "augment_shape: null pointer");
    if (n_resident <= 0 || n <= 0 || h <= 0 || w <= 0 || c < 1 || c > 4 || (long)n_resident * h * w >= (1L << 40))
        return hvn_fail(HVN_E_ARG, "augment_shape: n_resident, n, h or w < 1, c outside [1, 4], or 2^40 resident pixels (h = %d, c = %d)", h, c);
    if (out_h <= 0 || out_w <= 0 || out_h > h || out_w > w) return hvn_fail(HVN_E_ARG, "augment_shape: the output must be no larger than a patch (out_h = %d)", out_h);
    int rc = hvn_launch_aug_shape(img, ann, h, w, c, prm, n, out_h, out_w, out_img, out_ann, (hipStream_t)stream);
    return rc ? hvn_fail(HVN_E_LAUNCH, "augment_shape: launch failed") : HVN_OK;
}

int hvn_augment_shape_images(const uint8_t *pixels, const int32_t *ann, const hvn_image_rec *images, const hvn_patch_rec *patches, int n_images,
                             int n_patches, int64_t total_pixels, int win_h, int win_w, int c, const hvn_aug_sample *prm, int n, int out_h, int out_w,
                             uint8_t *out_img, int32_t *out_ann, int32_t *status, void *stream)
{
    if (!pixels || !ann || !images || !patches || !prm || !out_img || !out_ann) return hvn_fail(HVN_E_ARG, "augment_shape_images: null pointer");
    if (n_images <= 0 || n_patches <= 0 || total_pixels <= 0 || total_pixels >= (1LL << 40) || n <= 0 || win_h <= 0 || win_w <= 0 || c < 1 || c > 4)
        return hvn_fail(HVN_E_ARG, "augment_shape_images: n_images, n_patches, n, win_h or win_w < 1, c outside [1, 4], or total_pixels outside (0, 2^40) (c = %d)", c);
    if (out_h <= 0 || out_w <= 0 || out_h > win_h || out_w > win_w)
        return hvn_fail(HVN_E_ARG, "augment_shape_images: the output must be no larger than the window (out_h = %d)", out_h);
    if ((((uintptr_t)images) & 7) || (((uintptr_t)patches | (uintptr_t)status) & 3))
        return hvn_fail(HVN_E_ARG, "augment_shape_images: images must be 8-byte, patches and status 4-byte aligned");
    int rc = hvn_launch_aug_shape_images(pixels, ann, images, patches, n_images, n_patches, (long)total_pixels, win_h, win_w, c, prm, n, out_h, out_w,
                                         out_img, out_ann, status, (hipStream_t)stream);
    return rc ? hvn_fail(HVN_E_LAUNCH, "augment_shape_images: launch failed") : HVN_OK;
}

int hvn_augment_input(const uint8_t *src, const hvn_aug_sample *prm, const float *noise, int n, int h, int w, uint8_t *dst, void *stream)
{
    if (!src || !prm || !dst || src == dst) return hvn_fail(HVN_E_ARG, "augment_input: null pointer, or src and dst are the same buffer");
    if (n <= 0 || h <= 0 || w <= 0) return hvn_fail(HVN_E_ARG, "augment_input: n, h or w < 1 (h = %d)", h);
    int rc = hvn_launch_aug_input(src, prm, noise, n, h, w, dst, (hipStream_t)stream);
    return rc ? hvn_fail(HVN_E_LAUNCH, "augment_input: launch failed") : HVN_OK;
}

int hvn_adam_step(float *w, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2, float eps, int step,
                  void *stream)
{
    if (!w || !g || !m || !v || !al16(w) || !al16(g) || !al16(m) || !al16(v)) return hvn_fail(HVN_E_ARG, "adam_step: w, g, m and v must be non-null and 16-byte aligned");
    if (n <= 0 || step < 1) return hvn_fail(HVN_E_ARG, "adam_step: n or step < 1 (step = %d)", step);
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    int rc = hvn_launch_adam(w, g, m, v, (long)n, beta1, beta2, eps, (float)((double)lr / bc1), (float)(1.0 / sqrt(bc2)), (hipStream_t)stream);
    return hvn_launch_status(rc, "adam_step");
}

}  // extern "C"

"""Helpers for the -m gpu parity tests: tiny hand-made plans run through the real
libhvn_hip.so via hover_net_amd.engine.Engine, compared with tests/plan_interp.py."""
import numpy as np
import torch

from hover_net_amd import plan as PL


class MiniPlan(PL.Plan):
    def __init__(self):
        self.mode, self.nr_types = "mini", None
        self.geo = {"inp": 0, "out": 0}
        self.ops, self.bufs, self.logits, self.pred_map = [], [], {}, None
        self.image = PL.Buf("image", 1, 1, 3, "u8")
        self.arena_per_sample = 0


def rand_conv_weight(rng, cout, cin_g, k):
    return rng.normal(0.0, np.sqrt(2.0 / (cin_g * k * k)), (cout, cin_g, k, k))


def run_conv_case(n, xbuf_shape, xview, ybuf_shape, yview, wt, *, stride=1, pad=(0, 0), groups=1, bn=False, relu=0, pre=False,
                  res=False, post=False, seed=0, inplace_res=False, dtype="fp32", force_tile=None, x3=0):
    """Builds one CONV op over strided views, runs it on the GPU and with the torch
    interpreter.  xview / yview = (y0, x0, h, w, c0, c).  Returns (got, want) NHWC tensors of the
    WHOLE output buffer (so writes outside the view would be caught)."""
    from hover_net_amd.engine import Engine
    import plan_interp

    rng = np.random.default_rng(seed)
    P = MiniPlan()
    xb = P.buf("x", *xbuf_shape)
    yb = xb if ybuf_shape is None else P.buf("y", *ybuf_shape)
    xv = PL.View(xb, *xview)
    yv = PL.View(yb, *yview)
    cout = wt.shape[0]
    kw = {}
    if bn:
        kw["bn"] = (rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.2, cout))
    if pre:
        kw["pre"] = (rng.uniform(0.5, 1.5, xv.c), rng.normal(0, 0.3, xv.c))
    if post:
        kw["post"] = (rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.3, cout))
    rv = None
    if res:
        if inplace_res:
            rv = yv
        else:
            rb = P.buf("r", yb.h, yb.w, yb.c)
            rv = PL.View(rb, *yview)
        kw["res"] = rv
    op = P.conv("case", xv, yv, wt, stride=stride, pad=pad, groups=groups, relu=relu, **kw)
    if x3:
        assert op.tile_n in (128, 64) and groups == 1
        op.extra["x3"] = x3          # products on the bf16 matrix pipe from exact bf16x3 splits (csrc/hvn_conv_x3.hip)
    P.pack()
    eng = Engine(P, max_batch=n, dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    if dtype == "bf16":
        # bf16 path: the arena holds bf16; the reference sees the same (rounded) inputs and bf16-rounded weights, so
        # what is left is the accumulation order and the rounding of the output to bf16
        eng.arena.view(torch.bfloat16).copy_(torch.randn(eng.arena.shape, generator=g))
        op.w = np.ascontiguousarray(torch.from_numpy(op.w).to(torch.bfloat16).float().numpy())
        A = plan_interp.Arena(P, n)
        A.flat.copy_(eng.arena.view(torch.bfloat16).float().cpu())
    else:
        eng.arena.copy_(torch.randn(eng.arena.shape, generator=g))
        A = plan_interp.Arena(P, n)
        A.flat.copy_(eng.arena.cpu())
    if force_tile is not None:
        eng.ops[0].tile_n = force_tile
    eng.run_raw(n)
    torch.cuda.synchronize()
    r = A.view(op.res).clone() if op.res is not None else None
    A.view(op.y).copy_(plan_interp.conv_ref(op, A.view(op.x).clone(), r))
    b = yb
    arena = eng.arena.view(torch.bfloat16).float().cpu() if dtype == "bf16" else eng.arena.cpu()
    got = arena[:, b.offset:b.offset + b.size].view(n, b.h, b.w, b.c)
    want = A.tensor(b)
    return got, want


def conv_bits_plan(*, n, x, xbuf, xview, ybuf, yview, wt, stride=1, pad=(0, 0), groups=1, bias=None, relu=0, pre=None, res=None, inplace_res=False,
                   post=None, x2=None, wt2=None, stride2=1):
    """The one-CONV plan of a case given as explicit arrays (tests/bf16_model.py's `spec`): weights with bn=None, bias=..., so the fold
    preserves every value.  -> (plan, op, views = dict(x, y, res | None, x2 | None)).  Host only."""
    P = MiniPlan()
    xv = PL.View(P.buf("x", *xbuf), *xview)
    yv = PL.View(P.buf("y", *ybuf), *yview)
    assert tuple(x.shape) == (n, xv.h, xv.w, xv.c)
    kw, views = {}, dict(x=xv, y=yv, res=None, x2=None)
    if res is not None:
        views["res"] = kw["res"] = yv if inplace_res else PL.View(P.buf("r", *ybuf), *yview)
    if x2 is not None:
        views["x2"] = PL.View(P.buf("x2", *x2.shape[1:]))
        kw.update(x2=views["x2"], wt2=np.asarray(wt2, np.float64), stride2=stride2)
    op = P.conv("case", xv, yv, np.asarray(wt, np.float64), stride=stride, pad=pad, groups=groups, bn=None, bias=bias, relu=relu, pre=pre,
                post=post, **kw)
    P.pack()
    return P, op, views


def run_conv_bits(force_tile, **spec):
    """One bf16 CONV launch on exactly the values given: x, res [n, h, w, c] (the views' contents) and x2 (its whole buffer; NaN where
    nothing may be read) float32 arrays of bf16-exact values, weights [cout, cin_g, k, k] bf16-exact, bias / pre / post fp32.  The
    rest of the arena -- the buffers around the views, the output, the alignment gaps -- holds the NaN pattern 0x7FC0.
    -> (the output view's raw bf16 bits, uint16 [n, ho, wo, cout]; the number of arena elements outside the output view whose bits
    changed -- a write outside the view, or an unwritten NaN that is no longer the fill pattern)."""
    from hover_net_amd.engine import Engine
    from net_ops_ref import bf16_bits

    P, op, views = conv_bits_plan(**spec)
    n = spec["n"]
    eng = Engine(P, max_batch=n, n_split=1, n_lanes=0, dtype="bf16")
    eng.ops[0].tile_n = force_tile
    eng.arena.fill_(0x7FC0)

    def put(view, a):
        bits = bf16_bits(a).view(np.int16).reshape(a.shape)
        eng.buffer(view, n).copy_(torch.from_numpy(bits).view(torch.bfloat16))

    put(views["x"], spec["x"])
    if views["res"] is not None:
        put(views["res"], spec["res"])
    if views["x2"] is not None:
        put(views["x2"], spec["x2"])
    before = eng.arena.cpu().numpy().view(np.uint16).copy()
    eng.run_raw(n)
    torch.cuda.synchronize()
    assert eng.ops[0].act_dtype == 1 and eng.ops[0].tile_n == force_tile
    after = eng.arena.cpu().numpy().view(np.uint16)

    def window(arena):
        v, b = views["y"], views["y"].buf
        return arena[:, b.offset:b.offset + b.size].reshape(n, b.h, b.w, b.c)[:, v.y0:v.y0 + v.h, v.x0:v.x0 + v.w, v.c0:v.c0 + v.c]

    got = window(after).copy()
    rest = after.copy()
    window(rest)[...] = window(before)
    return got, int((rest != before).sum())


def run_dot_conv(n, x, wt, *, stride=1, pad=(0, 0), x3=0, force_tile=None, x2=None, wt2=None, stride2=1, winograd=0):
    """One BARE convolution -- no bn, bias, relu, prologue or residual: every output element is a dot product -- on exactly the values
    given (tests/test_gpu_x3_budget.py).  x [n, h, w, cin] (and x2 [n, h2, w2, cin2], the fused shortcut's second K source) go into the
    arena as they are, everything else there is NaN; wt [cout, cin, k, k] (wt2 [cout, cin2, 1, 1]) float64 or float32.  x3 = 0 | 9 | 6: the
    fp32 pipe or the bf16x3 kernels; force_tile: the launch form.  winograd = m: the convolution as F(m x m, k x k), and the op under
    test is its batched transform-domain product alone.
    -> (got, a, w, A):
       got [B, M, cout] fp32 numpy: the op's whole output (B = 1, M = n * ho * wo pixels | B = the transform positions, M = n * tiles);
       a [B, M, K], w [B, cout, K] fp32 numpy: the operands of those dot products as the kernel got them -- a gathered (im2col) from
           the GPU arena after the run, w unpacked from the fp32 packing the engine uploaded (and split);
       A: the interpreter arena (plan_interp.Arena) holding what the GPU arena held before the run."""
    from hover_net_amd.engine import Engine
    import plan_interp

    x = torch.as_tensor(np.ascontiguousarray(x, np.float32))
    cout, cin, k, _ = wt.shape
    _, h, w_, _ = x.shape
    ho, wo = (h + pad[0] + pad[1] - k) // stride + 1, (w_ + pad[0] + pad[1] - k) // stride + 1
    P = MiniPlan()
    xv = PL.View(P.buf("x", h, w_, cin))
    ybuf = P.buf("y", ho, wo, cout)
    x2v = None
    if winograd:
        assert x2 is None and stride == 1
        P.conv_winograd("case", xv, PL.View(ybuf), np.asarray(wt, np.float64), pad=pad, m=winograd)
        ybuf.first = 0              # the output may not take the place of V: it is read back after the run
    else:
        kw = {}
        if x2 is not None:
            x2 = torch.as_tensor(np.ascontiguousarray(x2, np.float32))
            x2v = PL.View(P.buf("x2", x2.shape[1], x2.shape[2], x2.shape[3]))
            kw = dict(x2=x2v, wt2=np.asarray(wt2, np.float64), stride2=stride2)
        P.conv("case", xv, PL.View(ybuf), np.asarray(wt, np.float64), stride=stride, pad=pad, **kw)
    oi = [i for i, o in enumerate(P.ops) if o.kind == PL.OP_CONV]
    assert len(oi) == 1
    op = P.ops[oi[0]]
    assert op.bias is None and op.pre is None and op.post is None and op.res is None and not op.relu
    if x3:
        assert op.tile_n in (128, 64)
        op.extra["x3"] = x3
    P.pack()
    eng = Engine(P, max_batch=n, n_split=1, n_lanes=0)
    if force_tile is not None:
        eng.ops[oi[0]].tile_n = force_tile
    eng.arena.fill_(float("nan"))
    eng.buffer(xv, n).copy_(x)
    if x2v is not None:
        eng.buffer(x2v, n).copy_(x2)
    A = plan_interp.Arena(P, n)
    A.flat.copy_(eng.arena.cpu())
    eng.run_raw(n)
    torch.cuda.synchronize()
    assert eng.ops[oi[0]].act_dtype == {0: 0, 9: 2, 6: 3}[x3] and (force_tile is None or eng.ops[oi[0]].tile_n == force_tile)
    if winograd:
        n2, t1 = op.x.buf.h, op.x.buf.w
        v = eng.buffer(PL.View(op.x.buf), n).cpu()                                  # [n, n2, t1, cin]: what WINO_IN wrote and the product read
        a = v.permute(1, 0, 2, 3).reshape(n2, n * t1, cin).numpy()
        got = eng.buffer(PL.View(op.y.buf), n).cpu().permute(1, 0, 2, 3).reshape(n2, n * t1, cout).numpy()
        wk = op.w[:, :cout].reshape(n2, cout, cin)                                  # [n2, cout_pad, cin / 32, 1, 32]
        return got, np.ascontiguousarray(a), np.ascontiguousarray(wk), A
    xs = eng.buffer(xv, n).cpu()
    assert torch.equal(xs, x)
    cols = torch.nn.functional.unfold(torch.nn.functional.pad(xs.permute(0, 3, 1, 2), (pad[0], pad[1], pad[0], pad[1])), k, stride=stride)
    a = cols.permute(0, 2, 1).reshape(n * ho * wo, cin * k * k)                     # k index = (channel, tap), as unpack_conv orders it
    wk = PL.unpack_conv(op.w, cout)                                                 # [cout, cin (+ cin2), taps]
    if x2v is not None:
        assert k == 1
        a2 = eng.buffer(x2v, n).cpu()[:, ::stride2, ::stride2][:, :ho, :wo]
        a = torch.cat([a, a2.reshape(n * ho * wo, -1)], 1)
    got = eng.buffer(PL.View(ybuf), n).cpu().reshape(1, n * ho * wo, cout).numpy()
    return got, np.ascontiguousarray(a.numpy())[None], np.ascontiguousarray(wk.reshape(cout, -1))[None], A


def view_of(t, y0=0, x0=0, h=None, w=None, c0=0, c=None, step=1):
    """hvn_view over a contiguous [N, H, W, C] cuda tensor: the window that starts at pixel (y0, x0) and channel c0, h x w pixels (default:
    to the end) of c channels, every step-th pixel."""
    from hover_net_amd import lib as L
    n, H, W, C = t.shape
    v = L.hvn_view()
    h = (H - y0 + step - 1) // step if h is None else h
    w = (W - x0 + step - 1) // step if w is None else w
    c = C - c0 if c is None else c
    v.base = t.data_ptr() + t.element_size() * ((y0 * W + x0) * C + c0)
    v.sn, v.sy, v.sx = H * W * C, step * W * C, step * C
    v.h, v.w, v.c, v.sc = h, w, c, 1
    return v


def run_tops(tops, batch):
    """hvn_run_train_plan over `tops` (a list of hvn_top) on the current stream; asserts success and synchronises."""
    import ctypes

    from hover_net_amd import lib as L
    L.require_gpu()
    arr = (L.hvn_top * len(tops))()
    for i, t in enumerate(tops):
        ctypes.memmove(ctypes.addressof(arr[i]), ctypes.addressof(t), ctypes.sizeof(L.hvn_top))
    rc = L.lib().hvn_run_train_plan(arr, len(tops), batch, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.lib().hvn_train_last_error().decode()
    torch.cuda.synchronize()


def run_train_ops(tops, batch, stored_parts=False):
    """hvn_run_train_plan over `tops` (cross-workgroup sums by fp32 atomics), or -- stored_parts -- hvn_run_train_plan_ws with the
    workspace it asks for (per-split copies added in a fixed order).  -> the workspace's size in bytes (0: no split summed anything)."""
    import ctypes

    from hover_net_amd import lib as L
    L.require_gpu()
    lib = L.lib()
    arr = (L.hvn_top * len(tops))()
    for i, t in enumerate(tops):
        ctypes.memmove(ctypes.addressof(arr[i]), ctypes.addressof(t), ctypes.sizeof(L.hvn_top))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = 0
    if stored_parts:
        need = int(lib.hvn_train_workspace_bytes(arr, len(tops), batch))
        ws = torch.full((need // 4 + 64,), float("nan"), device="cuda")
        rc = lib.hvn_run_train_plan_ws(arr, len(tops), batch, stream, ctypes.c_void_p(ws.data_ptr()), need)
    else:
        rc = lib.hvn_run_train_plan(arr, len(tops), batch, stream)
    assert rc == 0, lib.hvn_train_last_error().decode()
    torch.cuda.synchronize()
    return need


# -- the pipeline tests of the point-pattern analyses (test_gpu_neighbours.py, test_gpu_clusters.py, test_gpu_density.py) --
def synth_net():
    """One synthetic five-type model on the GPU."""
    from hover_net_amd import net_desc
    from hover_net_amd.synth import synth_state_dict

    model = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    model.load_state_dict(synth_state_dict("original", 5, seed=51), strict=True)
    return model.to("cuda").eval()


def _tile_images():
    from hover_net_amd.synth import synth_tiles

    return [synth_tiles(1, 270, seed=52)[0], synth_tiles(1, 270, seed=53)[0][:170, :121]]


def _maps(h, w, seed):
    from hover_net_amd.synth import synth_pred_maps

    return synth_pred_maps(1, h, w, 5, seed=seed, k_lo=4, k_hi=12)[0][0]

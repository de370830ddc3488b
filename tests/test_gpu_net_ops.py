"""-m gpu: the plan's non-GEMM kernels (csrc/hvn_net_ops.hip: hvn_conv0_mfma, hvn_upadd, hvn_upadd_bf16, hvn_head, hvn_predmap,
hvn_wino_in / hvn_wino_out in five F(m, r) forms), one launch at a time through hvn_run_op, against tests/net_ops_ref.py.

Two kinds of statement only (net_ops_ref.py's docstring has the argument; tests/test_net_ops_ref.py proves on the CPU that they hold
for unfused fp32 arithmetic in any order and that they see twelve planted defects):

  bit equality   UPADD fp32 / bf16 (one add, one round-to-nearest-even store), conv0's bf16 store against the same launch's fp32
                 output, HEAD with bf16 input against the fp32-input launch on the widened values, WINO_IN's fused nearest2x(res) + x
                 against UPADD followed by WINO_IN, PREDMAP's type channel and crafted pixels, every byte outside an output view;
  |got - ref64| <= B = (2 L + 4) 2^-24 S on EVERY element: CONV0, HEAD, WINO_IN, WINO_OUT.

Every output view lies in a buffer of NaN whose other bits must survive; every windowed float input is NaN outside its view and
the windowed uint8 image of conv0's case 2 lies among 0xA5 bytes, so a read outside a view poisons an output.  Each test prints
`net-ops | kernel | case | max err / B`; the measured lines are in profiles/net_ops_budget.txt.  PREDMAP's np / hv channels follow test_gpu_tta._check_against_oracle for the single view (0,)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import net_ops_ref as R
import tta_ref as TR

pytestmark = pytest.mark.gpu
OP_CONV0, OP_UPADD, OP_HEAD, OP_PREDMAP, OP_WINO_IN, OP_WINO_OUT = 1, 3, 4, 5, 6, 7
NAN = float("nan")


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
def _run(op, n):
    from hover_net_amd import lib as L

    rc = L.lib().hvn_run_op(ctypes.addressof(op), n, L.stream_ptr("cuda"))
    torch.cuda.synchronize()
    return rc, L.lib().hvn_last_error()


def _new_op(kind):
    from hover_net_amd import lib as L

    op = L.hvn_op()
    op.kind = kind
    return op


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bf16_dev(bits):
    return _dev(bits.view(np.int16)).view(torch.bfloat16)


def _view(v, t):
    """Fill an hvn_view from a (possibly non-contiguous) channels-last [n][h][w][c] tensor view."""
    assert t.stride(3) == 1
    v.base, v.sn, v.sy, v.sx = t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)
    v.h, v.w, v.c = t.shape[1], t.shape[2], t.shape[3]


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _flat_guard(shape, dtype=torch.float32, lead=256):
    """A dense tensor of `shape` inside a flat NaN buffer with `lead` guard elements in front and 256 behind -> (buffer, tensor)."""
    numel = int(np.prod(shape))
    buf = _nan((lead + numel + 256,), dtype)
    return buf, buf[lead:lead + numel].view(*shape)


def _raw(t):
    """The tensor's bits as integers of its element size (NaN compares unequal to itself; its bits do not)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Guard:
    """Remembers a buffer's bits; `check(view)` asserts that everything outside `view` (a view of the buffer) still has them."""

    def __init__(self, buf):
        self.buf, self.before = buf, _raw(buf).clone()

    def check(self, view=None):
        now = _raw(self.buf).clone()
        if view is not None:
            inside = torch.zeros_like(self.buf, dtype=torch.bool)
            off = (view.data_ptr() - self.buf.data_ptr()) // self.buf.element_size()
            torch.as_strided(inside, view.shape, view.stride(), off).fill_(True)
            now[inside] = self.before[inside]
        assert torch.equal(now, self.before), "bits outside the output view changed"


def _line(kernel, case, q):
    print("net-ops | %s | %s | %s" % (kernel, case, q if isinstance(q, str) else "%.4f" % q))


def _bit_equal(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all())


@functools.lru_cache(None)
def _mats(m, r):
    from hover_net_amd import winograd

    at, _, bt = winograd.mats(m, r)
    return at.astype(np.float32), bt.astype(np.float32)


# ---- CONV0 -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _conv0_refs():
    w, bias = R.conv0_params()
    return {name: (c, R.conv0(c["img"], w, bias, c["pad"], c["relu"])) for name, c in R.conv0_cases().items()}


def _conv0_launch(c, out_bf16):
    """One CONV0 launch of a case -> the output view tensor (the bits around it are checked here)."""
    w, bias = R.conv0_params()
    wd, bd = _dev(w), _dev(bias)
    img = c["img"]
    n, H, W, _ = img.shape
    pad = c["pad"]
    ho, wo = H + 2 * pad - 6, W + 2 * pad - 6
    op = _new_op(OP_CONV0)
    op.kh = op.kw = 7
    op.pad_t = op.pad_l = pad
    op.relu, op.cout, op.act_dtype = c["relu"], 64, int(out_bf16)
    op.w, op.bias = wd.data_ptr(), bd.data_ptr()
    if c["layout"] == "u8" and c.get("window"):     # the bytes around the image are 0xA5 = 165: read as pixels they move every output
        xbuf = torch.full((n, H + 2, W + 3, 3), 0xA5, dtype=torch.uint8, device="cuda")
        x = xbuf[:, 1:1 + H, 2:2 + W]
        x.copy_(_dev(img))
        _view(op.x, x)
        op.x_dtype = 0
    elif c["layout"] == "u8":
        x = _dev(img)
        _view(op.x, x)
        op.x_dtype = 0
    elif c["layout"] == "nchw":
        xbuf, x = _flat_guard((n, 3, H, W))
        x.copy_(_dev(img.transpose(0, 3, 1, 2)))
        op.x.base, op.x.sn, op.x.sy, op.x.sx, op.x.sc = x.data_ptr(), 3 * H * W, W, 1, H * W
        op.x.h, op.x.w, op.x.c, op.x_dtype = H, W, 3, 1
    else:
        xbuf = _nan((n, H + 2, W + 5, 3))
        x = xbuf[:, 1:1 + H, 2:2 + W]
        x.copy_(_dev(img))
        _view(op.x, x)
        assert op.x.sy == 3 * (W + 5)
        op.x_dtype = 1
    dt = torch.bfloat16 if out_bf16 else torch.float32
    if c.get("window"):
        ybuf = _nan((n, 25, 41, 96), dt)
        y = ybuf[:, 1:1 + ho, 2:2 + wo, 32:96]
    else:
        ybuf = _nan((n, ho + 2, wo + 2, 64), dt)
        y = ybuf[:, 1:1 + ho, 1:1 + wo]
    _view(op.y, y)
    g = Guard(ybuf)
    rc, err = _run(op, n)
    assert rc == 0, err
    g.check(y)
    return y


@pytest.mark.parametrize("name", list(R.conv0_cases()))
def test_conv0_within_bound(name):
    c, (ref, S) = _conv0_refs()[name]
    y = _conv0_launch(c, False).cpu().numpy()
    q = R.ratio(y, ref, S, R.L_CONV0)
    _line("conv0", name, q)
    assert q <= 1.0
    if not c["relu"]:
        assert (y < 0).any()


@pytest.mark.parametrize("name", ["1 u8 23x38 valid", "2 u8 23x38 same window"])
def test_conv0_bf16_store_is_rne_of_the_fp32_output(name):
    """Same kernel, same accumulation order: the bf16 output is torch.bfloat16 (round to nearest even) of the fp32 output, bit for bit."""
    c, (ref, S) = _conv0_refs()[name]
    y32 = _conv0_launch(c, False).cpu()
    y16 = _conv0_launch(c, True).cpu()
    assert torch.equal(_raw(y16), _raw(y32.bfloat16()))
    assert _bit_equal(_raw(y16).numpy().view(np.uint16), R.bf16_bits(y32.numpy()))
    _line("conv0 bf16 store", name, "0 (bit-equal)")


# ---- UPADD -------------------------------------------------------------------------------------------------------------------
def _upadd_launch(lo, skip, bf16, windows):
    """lo / skip: numpy float32, or uint16 bf16 bits -> the output as numpy of the same kind."""
    n, h, w, C = lo.shape
    dt = torch.bfloat16 if bf16 else torch.float32
    put = _bf16_dev if bf16 else _dev
    if windows:
        lbuf = _nan((n, h + 1, w + 2, C + 8), dt)
        lv = lbuf[:, 1:, 1:1 + w, :C]
        sbuf = _nan((n, 2 * h + 4, 2 * w + 4, C), dt)
        sv = sbuf[:, 2:2 + 2 * h, 3:3 + 2 * w]
        ybuf = _nan((n, 2 * h + 2, 2 * w + 3, C + 32), dt)
        yv = ybuf[:, 1:1 + 2 * h, 2:2 + 2 * w, 32:]
        lv.copy_(put(lo))
        sv.copy_(put(skip))
    else:
        lv, sv = put(lo), put(skip)
        ybuf, yv = _flat_guard((n, 2 * h, 2 * w, C), dt)
    op = _new_op(OP_UPADD)
    op.act_dtype = int(bf16)
    _view(op.x, lv)
    _view(op.res, sv)
    _view(op.y, yv)
    g = Guard(ybuf)
    rc, err = _run(op, n)
    assert rc == 0, err
    g.check(yv)
    out = _raw(yv).cpu().numpy()
    return out.view(np.uint16) if bf16 else out.view(np.float32)


@pytest.mark.parametrize("C", [4, 72])
def test_upadd_fp32_is_the_one_add(C):
    lo, skip = R.upadd_case(C, False)
    assert _bit_equal(_upadd_launch(lo, skip, False, True), R.upadd(lo, skip))
    _line("upadd", "C=%d windows" % C, "0 (bit-equal)")


def test_upadd_fp32_grid_stride():
    """n = 4, 48 x 48 x 1024: 9216 workgroups' worth of float4s on the grid capped at 8192."""
    lo, skip = R.upadd_case(1024, False, n=4, h=24, w=24)
    assert 4 * 48 * 48 * (1024 // 4) // 256 == 9216
    assert _bit_equal(_upadd_launch(lo, skip, False, False), R.upadd(lo, skip))
    _line("upadd", "grid-stride 4x48x48x1024", "0 (bit-equal)")


@pytest.mark.parametrize("C", [8, 72])
def test_upadd_bf16_is_one_add_and_one_rne(C):
    """Exact ties (1 + 2^-8 -> 1, 1.0078125 + 2^-8 -> 1.015625), near-ties on both sides and their negatives are in the data."""
    lo, skip = R.upadd_case(C, True)
    got = _upadd_launch(lo, skip, True, True)
    tl, ts = (torch.from_numpy(a.view(np.int16)).view(torch.bfloat16) for a in (lo, skip))
    torch_want = (tl.float().repeat_interleave(2, 1).repeat_interleave(2, 2) + ts.float()).bfloat16()
    assert _bit_equal(got, _raw(torch_want).numpy().view(np.uint16))
    assert _bit_equal(got, R.upadd_bf16(lo, skip))
    w = R.bf16_widen(got)
    assert (w[:, 0, 0, 0] == 1.0).all() and (w[:, 1, 0, 1] == 1.015625).all()
    _line("upadd bf16", "C=%d windows" % C, "0 (bit-equal)")


def test_upadd_bf16_grid_stride():
    lo, skip = R.upadd_case(1024, True, n=8, h=24, w=24)
    assert 8 * 48 * 48 * (1024 // 8) // 256 == 9216
    assert _bit_equal(_upadd_launch(lo, skip, True, False), R.upadd_bf16(lo, skip))
    _line("upadd bf16", "grid-stride 8x48x48x1024", "0 (bit-equal)")


# ---- HEAD --------------------------------------------------------------------------------------------------------------------
def _head_launch(x, w, bias, bf16):
    """x: numpy float32 [n][h][w][64] (bf16: values that are exact in bf16) -> NCHW logits numpy."""
    n, h, wd_, _ = x.shape
    cout = w.shape[0]
    xbuf = _nan((n, h + 2, wd_ + 3, 96), torch.bfloat16 if bf16 else torch.float32)
    xv = xbuf[:, 1:1 + h, 2:2 + wd_, 32:]
    xv.copy_(_bf16_dev(R.bf16_bits(x)) if bf16 else _dev(x))
    wdev, bdev = _dev(w), _dev(bias)
    ybuf, y = _flat_guard((n, cout, h, wd_))
    op = _new_op(OP_HEAD)
    op.cout, op.act_dtype = cout, int(bf16)
    op.w, op.bias = wdev.data_ptr(), bdev.data_ptr()
    _view(op.x, xv)
    op.y.base, op.y.h, op.y.w, op.y.c = y.data_ptr(), h, wd_, cout
    g = Guard(ybuf)
    rc, err = _run(op, n)
    assert rc == 0, err
    g.check(y)
    return y.cpu().numpy()


@pytest.mark.parametrize("cout", [1, 2, 5])
def test_head(cout):
    """969 pixels per sample: the last workgroup is ragged.  The bf16-input launch equals the fp32-input launch on the widened values."""
    x, w, bias = R.head_case(cout)
    ref, S = R.head(x, w, bias)
    q = R.ratio(_head_launch(x, w, bias, False), ref, S, R.L_HEAD)
    _line("head", "fp32 cout=%d" % cout, q)
    assert q <= 1.0
    xb = R.bf16_widen(R.bf16_bits(x))
    ref_b, S_b = R.head(xb, w, bias)
    y16, y32 = _head_launch(xb, w, bias, True), _head_launch(xb, w, bias, False)
    qb = R.ratio(y16, ref_b, S_b, R.L_HEAD)
    _line("head", "bf16 in cout=%d" % cout, qb)
    assert qb <= 1.0
    assert _bit_equal(y16, y32)


# ---- PREDMAP -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 5])
def test_predmap(T):
    np_l, hv_l, tp_l, crafted = R.predmap_case(T)
    n, _, h, w = np_l.shape
    ch = 4 if T else 3
    ybuf, y = _flat_guard((n, h, w, ch), lead=256 if T else 257)
    assert y.data_ptr() % 16 == (0 if T else 4)              # without types the header allows any 4-byte alignment
    dn, dh = _dev(np_l), _dev(hv_l)
    dt = _dev(tp_l) if T else None
    op = _new_op(OP_PREDMAP)
    op.cout = T
    op.x.base, op.res.base, op.w = dn.data_ptr(), dh.data_ptr(), (dt.data_ptr() if T else None)
    op.y.base, op.y.h, op.y.w, op.y.c = y.data_ptr(), h, w, ch
    g = Guard(ybuf)
    rc, err = _run(op, n)
    assert rc == 0, err
    g.check(y)
    got = y.cpu().numpy()
    c0 = 1 if T else 0
    per = [{"np": np_l, "hv": hv_l}]
    r32, r64 = TR.reduce_f32(per, (0,)), TR.reduce_f64(per, (0,))
    assert _bit_equal(got[..., c0 + 1:], r32["hv"])
    own = np.abs(r32["np"] - r64["np"]).max()
    err_np = np.abs(got[..., c0].astype(np.float64) - r64["np"]).max()
    bound = min(4.0 * own, 1e-5)
    _line("predmap", "T=%d np: error %.3g / bound min(4 x fp32 oracle's own, 1e-5) = %.3g; hv, type, crafted pixels bit-equal" % (T, err_np, bound),
          err_np / bound)
    assert err_np <= bound
    assert np.abs(got[..., c0].astype(np.float64) - R.predmap(np_l, hv_l, tp_l)[..., c0]).max() <= bound
    if T:
        assert (got[..., 0] == R.first_max(tp_l)).all()      # the rule on the fp32 logits themselves: no tolerance
    for x, c, v in crafted:
        assert (got[:, 0, x, c] == v).all(), (x, c, v, got[:, 0, x, c])


# ---- WINO_IN -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _wino_in_refs(m, r):
    bt = _mats(m, r)[1]
    return {name: (c, R.wino_in(c["x"], bt, m, r, c["pad"], c["ty"], c["tx"])) for name, c in R.wino_in_cases(m, r).items()}


def _wino_in_op(m, r, xv, pad, ty, tx, v, bt_dev, res=None):
    op = _new_op(OP_WINO_IN)
    op.kh, op.kw, op.stride, op._rsv = ty, tx, m, r
    op.pad_t = op.pad_l = pad
    op.w = bt_dev.data_ptr()
    _view(op.x, xv)
    if res is not None:
        _view(op.res, res)
    op.y.base, op.y.sn, op.y.sy, op.y.sx = v.data_ptr(), v.stride(0), v.stride(1), v.stride(2)     # sy: between positions, sx: between tiles
    op.y.h, op.y.w, op.y.c = v.shape[1], v.shape[2], v.shape[3]
    return op


def _window(a, c0=32, tail=4):
    """The array as a window at (1, 2, c0) of a NaN buffer."""
    n, h, w, c = a.shape
    buf = _nan((n, h + 2, w + 3, c0 + c + tail))
    v = buf[:, 1:1 + h, 2:2 + w, c0:c0 + c]
    v.copy_(_dev(a))
    return v


@pytest.mark.parametrize("m,r", R.FORMS, ids=lambda v: str(v))
def test_wino_in(m, r):
    bt_dev = _dev(_mats(m, r)[1])
    nn = m + r - 1
    for name, (c, (ref, S)) in _wino_in_refs(m, r).items():
        x = c["x"]
        n, C, T = x.shape[0], x.shape[3], c["ty"] * c["tx"]
        xv = _window(x) if c.get("window") else _dev(x)
        if c.get("strided_v"):          # every V[a * nn + b][tile][c] where the header says: y.sy between positions, y.sx between tiles
            vbuf = _nan((n, nn * nn, T + 1, C + 4))
            v = vbuf[:, :, :T, 4:]
        else:
            vbuf, v = _flat_guard((n, nn * nn, T, C))
        g = Guard(vbuf)
        rc, err = _run(_wino_in_op(m, r, xv, c["pad"], c["ty"], c["tx"], v, bt_dev), n)
        assert rc == 0, err
        g.check(v)
        q = R.ratio(v.cpu().numpy(), ref, S, R.wino_L(m, r))
        _line("wino_in F(%d,%d)" % (m, r), name, q)
        assert q <= 1.0, name


@pytest.mark.parametrize("m,r", [(4, 5), (6, 5)], ids=lambda v: str(v))
def test_wino_in_fused_upadd_is_the_two_launches(m, r):
    """The header's claim, per kernel: WINO_IN with res = a half-resolution view equals UPADD followed by WINO_IN, bit for bit."""
    c = R.wino_fused_case(m, r)
    bt = _mats(m, r)[1]
    bt_dev = _dev(bt)
    nn, n, C, T = m + r - 1, 2, 8, c["ty"] * c["tx"]
    lo, xv = _window(c["lo"]), _window(c["x"])
    vbuf, v = _flat_guard((n, nn * nn, T, C))
    g = Guard(vbuf)
    rc, err = _run(_wino_in_op(m, r, xv, c["pad"], c["ty"], c["tx"], v, bt_dev, res=lo), n)
    assert rc == 0, err
    g.check(v)
    s = _nan((n, 16, 18, C))
    up = _new_op(OP_UPADD)
    _view(up.x, lo)
    _view(up.res, xv)
    _view(up.y, s)
    rc, err = _run(up, n)
    assert rc == 0, err
    summed = R.upadd(c["lo"], c["x"])
    assert _bit_equal(s.cpu().numpy(), summed)
    v2 = _nan((n, nn * nn, T, C))
    rc, err = _run(_wino_in_op(m, r, s, c["pad"], c["ty"], c["tx"], v2, bt_dev), n)
    assert rc == 0, err
    assert _bit_equal(v.cpu().numpy(), v2.cpu().numpy())
    ref, S = R.wino_in(summed, bt, m, r, c["pad"], c["ty"], c["tx"])
    q = R.ratio(v.cpu().numpy(), ref, S, R.wino_L(m, r))
    _line("wino_in F(%d,%d)" % (m, r), "fused nearest2x(res) + x", q)
    assert q <= 1.0


# ---- WINO_OUT ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,r", R.FORMS, ids=lambda v: str(v))
def test_wino_out(m, r):
    at = _mats(m, r)[0]
    at_dev = _dev(at)
    c = R.wino_out_case(m, r)
    n, _, T, C = c["M"].shape
    H, W = c["H"], c["W"]
    Md, bias_dev = _dev(c["M"]), _dev(c["bias"])
    for name, has_bias, relu, accum in R.WINO_OUT_VARIANTS:
        ref, S = R.wino_out(c["M"], at, m, r, c["ty"], c["tx"], H, W, bias=c["bias"] if has_bias else None, relu=relu,
                            old=c["old"] if accum else None)
        ybuf = _nan((n, H + 2, W + 3, 32 + C + 8))
        yv = ybuf[:, 1:1 + H, 2:2 + W, 32:32 + C]
        if accum:
            yv.copy_(_dev(c["old"]))
        op = _new_op(OP_WINO_OUT)
        op.kh, op.kw, op.stride, op._rsv, op.relu = c["ty"], c["tx"], m, r, int(relu)
        op.w, op.bias = at_dev.data_ptr(), (bias_dev.data_ptr() if has_bias else None)
        op.x.base, op.x.sn, op.x.sy, op.x.sx = Md.data_ptr(), Md.stride(0), Md.stride(1), Md.stride(2)
        op.x.h, op.x.w, op.x.c = Md.shape[1], T, C
        _view(op.y, yv)
        if accum:
            _view(op.res, yv)
        g = Guard(ybuf)
        rc, err = _run(op, n)
        assert rc == 0, err
        g.check(yv)
        q = R.ratio(yv.cpu().numpy(), ref, S, R.wino_L(m, r, out=True))
        _line("wino_out F(%d,%d)" % (m, r), name, q)
        assert q <= 1.0, name


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refused(op, n, name, guards):
    """rc -1, the kernel's name in the error text (a text of THIS refusal: the last error is first set to another kind's), and the
    outputs' bits unchanged."""
    stale = _new_op(99)
    rc, err = _run(stale, 1)
    assert rc == -1 and b"unknown op kind" in err
    rc, err = _run(op, n)
    assert rc == -1, (rc, err)
    assert name in err and b"unknown op kind" not in err, err
    for g in guards:
        g.check()


def test_upadd_refusals():
    n = 2

    def make(C, bf16):
        dt = torch.bfloat16 if bf16 else torch.float32
        lo, skip = torch.zeros((n, 4, 4, 16), dtype=dt, device="cuda"), torch.zeros((n, 8, 8, 16), dtype=dt, device="cuda")
        ybuf = _nan((n, 8, 8, 32), dt)
        op = _new_op(OP_UPADD)
        op.act_dtype = int(bf16)
        _view(op.x, lo[..., :C])
        _view(op.res, skip[..., :C])
        _view(op.y, ybuf[..., :C])
        return op, Guard(ybuf), (lo, skip)

    op, g, keep = make(8, False)
    assert _run(op, n)[0] == 0                                  # the descriptor the refusals below are one field away from
    op, g, keep = make(8, True)
    assert _run(op, n)[0] == 0
    for C, bf16 in ((6, False), (12, True)):                    # channel multiples: 4 (fp32), 8 (bf16)
        op, g, keep = make(C, bf16)
        _refused(op, n, b"upadd", [g])
    for bf16 in (False, True):
        op, g, keep = make(8, bf16)
        op.x.h = 3                                              # x.h * 2 != y.h
        _refused(op, n, b"upadd", [g])
        op, g, keep = make(8, bf16)
        op.y.base += 4                                          # base + 4 bytes
        _refused(op, n, b"upadd", [g])
        op, g, keep = make(8, bf16)
        op.res.base += 4
        _refused(op, n, b"upadd", [g])
    op, g, keep = make(8, True)
    op.x.sx = 12                                                # a bf16 stride of 12 elements: every other pixel 8 bytes off
    _refused(op, n, b"upadd", [g])


def test_conv0_refusals():
    n = 2
    w, bias = R.conv0_params()
    wd, bd = _dev(w), _dev(bias)
    img = torch.zeros((n, 9, 9, 4), dtype=torch.uint8, device="cuda")

    def make():
        ybuf = _nan((n, 3, 3, 96))
        op = _new_op(OP_CONV0)
        op.kh = op.kw = 7
        op.relu, op.cout = 1, 64
        op.w, op.bias = wd.data_ptr(), bd.data_ptr()
        _view(op.x, img[..., :3])
        _view(op.y, ybuf[..., :64])
        return op, Guard(ybuf)

    op, g = make()
    assert _run(op, n)[0] == 0
    for edit in ("kh", "xc", "yc", "bias", "ybase"):
        op, g = make()
        if edit == "kh":
            op.kh = 5
        elif edit == "xc":
            op.x.c = 4
        elif edit == "yc":
            op.y.c = 32
        elif edit == "bias":
            op.bias = None
        else:
            op.y.base += 4
        _refused(op, n, b"conv0", [g])


def test_head_refusals():
    n = 2
    wd, bd = torch.zeros((2, 64), device="cuda"), torch.zeros((2,), device="cuda")

    def make(bf16):
        x = torch.zeros((n, 4, 4, 136), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        ybuf = _nan((n, 2, 4, 4))
        op = _new_op(OP_HEAD)
        op.cout, op.act_dtype = 2, int(bf16)
        op.w, op.bias = wd.data_ptr(), bd.data_ptr()
        _view(op.x, x[..., :64])
        op.y.base, op.y.h, op.y.w, op.y.c = ybuf.data_ptr(), 4, 4, 2
        return op, Guard(ybuf), x

    for bf16 in (False, True):
        op, g, keep = make(bf16)
        assert _run(op, n)[0] == 0
        op, g, keep = make(bf16)
        op.x.c = 32
        _refused(op, n, b"head", [g])
        op, g, keep = make(bf16)
        op.w = None
        _refused(op, n, b"head", [g])
        op, g, keep = make(bf16)
        op.x.base += 4
        _refused(op, n, b"head", [g])
    op, g, keep = make(True)
    op.x.sx = 68                                                # a bf16 stride of 68 elements
    _refused(op, n, b"head", [g])


def test_predmap_refusals():
    n, h, w, T = 2, 4, 4, 5
    dn, dh, dt = (torch.zeros((n, k, h, w), device="cuda") for k in (2, 2, T))

    def make(types):
        ybuf = _nan((n * h * w * 4 + 8,))
        op = _new_op(OP_PREDMAP)
        op.cout = T if types else 0
        op.x.base, op.res.base, op.w = dn.data_ptr(), dh.data_ptr(), (dt.data_ptr() if types else None)
        op.y.base, op.y.h, op.y.w, op.y.c = ybuf.data_ptr(), h, w, 4 if types else 3
        return op, Guard(ybuf)

    for types in (False, True):
        op, g = make(types)
        assert _run(op, n)[0] == 0
        op, g = make(types)
        op.res.base = None                                      # no hv
        _refused(op, n, b"predmap", [g])
    op, g = make(True)
    op.w = None                                                 # types without type logits
    _refused(op, n, b"predmap", [g])
    op, g = make(True)
    op.y.base += 4                                              # the float4 store needs 16 bytes
    _refused(op, n, b"predmap", [g])


def test_wino_refusals():
    m, r, n = 4, 5, 2
    nn = m + r - 1
    at, bt = (_dev(a) for a in _mats(m, r))
    x = torch.zeros((n, 8, 8, 16), device="cuda")
    lo = torch.zeros((n, 4, 4, 16), device="cuda")
    ty = tx = 2
    M = torch.zeros((n, nn * nn, ty * tx, 8), device="cuda")

    def make_in(C=8, res=None):
        vbuf = _nan((n, nn * nn, ty * tx, 16))
        op = _wino_in_op(m, r, x[..., :C], 2, ty, tx, vbuf[..., :C], bt, res=res)
        return op, Guard(vbuf)

    def make_out(accum=False):
        ybuf = _nan((n, 8, 8, 8))
        op = _new_op(OP_WINO_OUT)
        op.kh, op.kw, op.stride, op._rsv = ty, tx, m, r
        op.w = at.data_ptr()
        op.x.base, op.x.sn, op.x.sy, op.x.sx = M.data_ptr(), M.stride(0), M.stride(1), M.stride(2)
        op.x.h, op.x.w, op.x.c = nn * nn, ty * tx, 8
        _view(op.y, ybuf)
        if accum:
            _view(op.res, ybuf)
        return op, Guard(ybuf), ybuf

    assert _run(make_in()[0], n)[0] == 0
    assert _run(make_in(res=lo[..., :8])[0], n)[0] == 0
    assert _run(make_out()[0], n)[0] == 0
    op, g = make_in()
    op.y.h, op.stride, op._rsv = 49, 0, 0                       # 49 transform positions: no F(m, r) of the library
    _refused(op, n, b"wino", [g])
    op, g = make_in(C=6)
    _refused(op, n, b"wino", [g])
    op, g, ybuf = make_out(accum=True)
    other = torch.zeros_like(ybuf)
    op.res.base = other.data_ptr()                              # res != y
    _refused(op, n, b"wino", [g, Guard(other)])
    op, g = make_in(res=lo[:, :3, :, :8])                       # a half-resolution view of the wrong extent
    _refused(op, n, b"wino", [g])
    op, g, ybuf = make_out()
    op.kh = 1                                                   # a tile grid that does not cover y
    _refused(op, n, b"wino", [g])
    op, g, ybuf = make_out()
    op.y.h = 9                                                  # ... nor one row more than the grid has
    _refused(op, n, b"wino", [g])

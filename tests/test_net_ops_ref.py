"""CPU proof of tests/net_ops_ref.py: the float64 references and the bound B = (2 L + 4) 2^-24 S that tests/test_gpu_net_ops.py holds
the non-GEMM kernels to (csrc/hvn_net_ops.hip) are right, and they see defects.

  1. every reference agrees with the other independent statement of the same op, tests/plan_interp.py's torch fp32 function, within
     B on the GPU file's shapes -- bit for bit where that file demands bit equality;
  2. a numpy fp32 emulation of each kernel with a SEPARATELY rounded multiply and add -- the worst arithmetic B allows -- stays
     within B on every element, in index order and in a seeded random order (the ratios are printed);
  3. each of twelve planted defects breaks the check it belongs to on at least one element.

The emulations follow the kernels' structure (two-stage transforms, bias and ReLU where the kernels have them), not their code.
`test_upadd_channel_multiple_is_refused_by_name` alone needs the built library (as tests/test_conv_launch_refusals.py does)."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import net_ops_ref as R
import plan_interp as PI
from hover_net_amd import winograd

F32 = np.float32


def mats(m, r):
    at, _, bt = winograd.mats(m, r)
    return at.astype(F32), bt.astype(F32)


# ---- fp32 emulations (every product and every sum rounded on its own) ---------------------------------------------------------
def emu_conv0(img, w, bias, pad, relu, order=None, skip=None, edge=False):
    xp = np.pad(img.astype(F32), ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="edge" if edge else "constant")
    ho, wo = xp.shape[1] - 6, xp.shape[2] - 6
    acc = np.zeros((img.shape[0], ho, wo, 64), F32)
    for k in (range(147) if order is None else order):          # k = (tap row, tap column, channel), the order of w's rows
        if k == skip:
            continue
        ky, kx, c = k // 21, (k % 21) // 3, k % 3
        acc = acc + xp[:, ky:ky + ho, kx:kx + wo, c, None] * w[ky, kx, c]
    acc = acc + bias
    assert acc.dtype == F32
    return np.maximum(acc, F32(0)) if relu else acc


def emu_head(x, w, bias, order=None, bias_first=False):
    acc = np.zeros(x.shape[:3] + (w.shape[0],), F32) + (bias if bias_first else F32(0))
    for c in (range(64) if order is None else order):
        acc = acc + x[..., c, None] * w[:, c]
    if not bias_first:
        acc = acc + bias
    assert acc.dtype == F32
    return np.ascontiguousarray(acc.transpose(0, 3, 1, 2))


def emu_wino_in(x, bt, m, r, pad, ty, tx, order=None, transposed=False, last_col_off=0):
    n, H, W, c = x.shape
    nn = m + r - 1
    order = range(nn) if order is None else order
    xp = np.zeros((n, pad + max(H, m * ty + nn) + nn, pad + max(W, m * tx + nn) + nn, c), F32)
    xp[:, pad:pad + H, pad:pad + W] = x
    d = np.empty((n, ty, tx, nn, nn, c), F32)
    for i in range(ty):
        for j in range(tx):
            x0 = m * j + (last_col_off if j == tx - 1 else 0)
            d[:, i, j] = xp[:, m * i:m * i + nn, x0:x0 + nn]
    b = bt.T if transposed else bt
    tmp = np.zeros((n, ty, tx, nn, nn, c), F32)                  # [a][j] = sum_i B^T[a][i] d[i][j]
    for i in order:
        tmp = tmp + b[:, i][None, None, None, :, None, None] * d[:, :, :, i][:, :, :, None]
    v = np.zeros((n, ty, tx, nn, nn, c), F32)                    # [a][b] = sum_j tmp[a][j] B^T[b][j]
    for j in order:
        v = v + tmp[:, :, :, :, j][:, :, :, :, None] * b[:, j][None, None, None, None, :, None]
    assert v.dtype == F32
    return v.transpose(0, 3, 4, 1, 2, 5).reshape(n, nn * nn, ty * tx, c)


def emu_wino_out(M, at, m, r, ty, tx, H, W, bias=None, relu=False, old=None, order=None, relu_after=False, surplus_rows=0):
    """-> [n][H + 2][W + 2][c]: the output view at the origin of a NaN buffer (its old values where accumulating)."""
    nn = m + r - 1
    n, _, _, c = M.shape
    order = range(nn) if order is None else order
    M6 = M.reshape(n, nn, nn, ty, tx, c)
    tmp = np.zeros((n, m, nn, ty, tx, c), F32)                   # [q][b] = sum_a A^T[q][a] M[a][b]
    for a in order:
        tmp = tmp + at[:, a][None, :, None, None, None, None] * M6[:, a][:, None]
    y = np.zeros((n, m, m, ty, tx, c), F32) + (F32(0) if bias is None else bias)
    for b in order:
        y = y + tmp[:, :, b][:, :, None] * at[:, b][None, None, :, None, None, None]
    full = y.transpose(0, 3, 1, 4, 2, 5).reshape(n, m * ty, m * tx, c)
    if relu and not relu_after:
        full = np.maximum(full, F32(0))
    buf = np.full((n, H + 2, W + 2, c), np.nan, F32)
    rows = min(H + surplus_rows, m * ty)
    if old is not None:
        buf[:, :H, :W] = old
        full = full.copy()
        full[:, :H, :W] = full[:, :H, :W] + old
    if relu and relu_after:
        full = np.maximum(full, F32(0))
    buf[:, :rows, :W] = full[:, :rows, :W]
    assert full.dtype == F32
    return buf


def emu_upadd(lo, skip, defect=False):
    h, w = lo.shape[1:3]
    yy = np.arange(2 * h)
    yy = np.minimum((yy + 1) >> 1, h - 1) if defect else yy >> 1
    return lo[:, yy][:, :, np.arange(2 * w) >> 1] + skip


def emu_bf16_store(x, mode="rne"):
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    if mode == "trunc":
        return (b >> 16).astype(np.uint16)
    if mode == "away":
        return ((b + 0x8000) >> 16).astype(np.uint16)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def emu_predmap_type(tp, last=False):
    best = np.zeros(tp[:, 0].shape, np.int64)
    bv = tp[:, 0].copy()
    for t in range(1, tp.shape[1]):
        up = tp[:, t] >= bv if last else tp[:, t] > bv
        bv = np.where(up, tp[:, t], bv)
        best = np.where(up, t, best)
    return best


def orders(k, seed):
    return (("index", None), ("random", [int(i) for i in np.random.default_rng(seed).permutation(k)]))


# ---- references, formed once -------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def conv0_refs():
    w, bias = R.conv0_params()
    return {name: (c, R.conv0(c["img"], w, bias, c["pad"], c["relu"])) for name, c in R.conv0_cases().items()}


@functools.lru_cache(None)
def wino_in_refs(m, r):
    bt = mats(m, r)[1]
    return {name: (c, R.wino_in(c["x"], bt, m, r, c["pad"], c["ty"], c["tx"])) for name, c in R.wino_in_cases(m, r).items()}


def wino_out_ref(m, r, variant):
    _, has_bias, relu, accum = variant
    c = R.wino_out_case(m, r)
    kw = dict(bias=c["bias"] if has_bias else None, relu=relu, old=c["old"] if accum else None)
    return c, kw, R.wino_out(c["M"], mats(m, r)[0], m, r, c["ty"], c["tx"], c["H"], c["W"], **kw)


# ---- 1. agreement with tests/plan_interp.py ----------------------------------------------------------------------------------
def test_conv0_agrees_with_plan_interp():
    w, bias = R.conv0_params()
    for name, (c, (ref, S)) in conv0_refs().items():
        op = NS(w=w, bias=bias, pad_t=c["pad"], pad_l=c["pad"])
        got = PI.conv0_ref(op, torch.from_numpy(c["img"])).numpy()          # always with ReLU, which moves no bound
        q = R.ratio(got, np.maximum(ref, 0.0), S, R.L_CONV0)
        print("net-ops-ref | conv0 vs plan_interp | %s | %.3f" % (name, q))
        assert q <= 1.0, name
        assert ref.shape[1:3] == {"1": (17, 32), "2": (23, 38), "5": (1, 1)}.get(name[0], ref.shape[1:3])
    assert (conv0_refs()["2 u8 23x38 same window"][1][0] < 0).any()          # relu 0: there are negative outputs to survive


@pytest.mark.parametrize("C", [4, 72])
def test_upadd_agrees_with_plan_interp(C):
    lo, skip = R.upadd_case(C, False)
    want = PI.upadd_ref(torch.from_numpy(lo), torch.from_numpy(skip)).numpy()
    assert (R.upadd(lo, skip).view(np.uint32) == want.view(np.uint32)).all()
    assert (emu_upadd(lo, skip).view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("C", [8, 72])
def test_upadd_bf16_agrees_with_torch(C):
    lo, skip = R.upadd_case(C, True)
    tl, ts = (torch.from_numpy(a.view(np.int16)).view(torch.bfloat16) for a in (lo, skip))
    want = PI.upadd_ref(tl.float(), ts.float()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = R.upadd_bf16(lo, skip)
    assert (got == want).all()
    assert (PI.upadd_ref(tl, ts).view(torch.int16).numpy().view(np.uint16) == want).all()      # torch's own bf16 add: the same rounding
    # the crafted sums: exact ties go to the even neighbour, near-ties to their side
    w = R.bf16_widen(got)
    for ch, v in enumerate([1.0, 1.015625, 1.0078125, 1.0, 1.015625, 1.0078125]):
        k = ch
        assert (w[:, k & 1, (k >> 1) * 2, k % C] == v).all(), (ch, v)
        k = ch + 6
        assert (w[:, k & 1, (k >> 1) * 2, k % C] == -v).all(), (ch, -v)


@pytest.mark.parametrize("cout", [1, 2, 5])
def test_head_agrees_with_plan_interp(cout):
    x, w, bias = R.head_case(cout)
    ref, S = R.head(x, w, bias)
    got = PI.head_ref(NS(w=w, bias=bias), torch.from_numpy(x)).numpy()
    q = R.ratio(got, ref, S, R.L_HEAD)
    print("net-ops-ref | head vs plan_interp | cout %d | %.3f" % (cout, q))
    assert q <= 1.0


@pytest.mark.parametrize("T", [0, 1, 5])
def test_predmap_agrees_with_plan_interp(T):
    """The type channel, the hv channels and the crafted pixels exactly; softmax(np)[1] within 8 x 2^-24: a difference, two
    exponentials, a sum and a quotient of values <= 1, each within an ulp or two of fp32."""
    np_l, hv_l, tp_l, crafted = R.predmap_case(T)
    ref = R.predmap(np_l, hv_l, tp_l)
    logits = {"np": torch.from_numpy(np_l), "hv": torch.from_numpy(hv_l)}
    if T:
        logits["tp"] = torch.from_numpy(tp_l)
    got = PI.predmap_ref(logits, ("tp", "np", "hv") if T else ("np", "hv")).numpy()
    c0 = 1 if T else 0
    assert (got[..., c0 + 1:] == ref[..., c0 + 1:]).all()
    assert np.abs(got[..., c0] - ref[..., c0]).max() <= 8 * R.U
    if T:
        assert (got[..., 0] == ref[..., 0]).all()
        assert (ref[..., 0] == np.argmax(tp_l, 1)).all()
    for x, ch, v in crafted:
        # exp(-400) is 1.9e-174 in float64 and underflows to 0 in fp32: the crafted value is the float64 one rounded to fp32
        assert (ref[:, 0, x, ch].astype(F32) == v).all() and (got[:, 0, x, ch] == v).all(), (x, ch, v)


@pytest.mark.parametrize("m,r", R.FORMS)
def test_wino_in_agrees_with_plan_interp(m, r):
    bt = mats(m, r)[1]
    for name, (c, (ref, S)) in wino_in_refs(m, r).items():
        op = NS(w=bt, pad_t=c["pad"], extra={"tiles": (c["ty"], c["tx"]), "m": m, "r": r})
        got = PI.wino_in_ref(op, torch.from_numpy(c["x"])).numpy()
        q = R.ratio(got, ref, S, R.wino_L(m, r))
        print("net-ops-ref | wino_in F(%d,%d) vs plan_interp | %s | %.3f" % (m, r, name, q))
        assert q <= 1.0, name


@pytest.mark.parametrize("m,r", R.FORMS)
def test_wino_out_agrees_with_plan_interp(m, r):
    at = mats(m, r)[0]
    for variant in R.WINO_OUT_VARIANTS:
        c, kw, (ref, S) = wino_out_ref(m, r, variant)
        op = NS(w=at, bias=kw["bias"], relu=kw["relu"], y=NS(h=c["H"], w=c["W"]), extra={"tiles": (c["ty"], c["tx"]), "m": m, "r": r})
        got = PI.wino_out_ref(op, torch.from_numpy(c["M"]))
        if kw["old"] is not None:
            got = got + torch.from_numpy(kw["old"])
        q = R.ratio(got.numpy(), ref, S, R.wino_L(m, r, out=True))
        print("net-ops-ref | wino_out F(%d,%d) vs plan_interp | %s | %.3f" % (m, r, variant[0], q))
        assert q <= 1.0, variant[0]


# ---- 2. the unfused fp32 emulation stays within B ------------------------------------------------------------------------------
def test_conv0_emulation_within_bound():
    w, bias = R.conv0_params()
    worst = 0.0
    for name, (c, (ref, S)) in conv0_refs().items():
        for oname, order in orders(147, 1):
            q = R.ratio(emu_conv0(c["img"], w, bias, c["pad"], c["relu"], order), ref, S, R.L_CONV0)
            worst = max(worst, q)
            assert q <= 1.0, (name, oname, q)
    print("net-ops-ref | conv0 emulation | max err / B = %.3f" % worst)


def test_head_emulation_within_bound():
    worst = 0.0
    for cout in (1, 2, 5):
        x, w, bias = R.head_case(cout)
        ref, S = R.head(x, w, bias)
        for oname, order in orders(64, 2):
            q = R.ratio(emu_head(x, w, bias, order), ref, S, R.L_HEAD)
            worst = max(worst, q)
            assert q <= 1.0, (cout, oname, q)
    print("net-ops-ref | head emulation | max err / B = %.3f" % worst)


@pytest.mark.parametrize("m,r", R.FORMS)
def test_wino_in_emulation_within_bound(m, r):
    bt = mats(m, r)[1]
    worst = 0.0
    for name, (c, (ref, S)) in wino_in_refs(m, r).items():
        for oname, order in orders(m + r - 1, 3):
            q = R.ratio(emu_wino_in(c["x"], bt, m, r, c["pad"], c["ty"], c["tx"], order), ref, S, R.wino_L(m, r))
            worst = max(worst, q)
            assert q <= 1.0, (name, oname, q)
    print("net-ops-ref | wino_in F(%d,%d) emulation | max err / B = %.3f" % (m, r, worst))


@pytest.mark.parametrize("m,r", R.FORMS)
def test_wino_out_emulation_within_bound(m, r):
    at = mats(m, r)[0]
    worst = 0.0
    for variant in R.WINO_OUT_VARIANTS:
        c, kw, (ref, S) = wino_out_ref(m, r, variant)
        for oname, order in orders(m + r - 1, 4):
            buf = emu_wino_out(c["M"], at, m, r, c["ty"], c["tx"], c["H"], c["W"], order=order, **kw)
            q = R.ratio(buf[:, :c["H"], :c["W"]], ref, S, R.wino_L(m, r, out=True))
            worst = max(worst, q)
            assert q <= 1.0, (variant[0], oname, q)
            buf[:, :c["H"], :c["W"]] = 0
            assert np.isnan(buf[:, c["H"]:]).all() and np.isnan(buf[:, :, c["W"]:]).all()
    print("net-ops-ref | wino_out F(%d,%d) emulation | max err / B = %.3f" % (m, r, worst))


# ---- 3. planted defects --------------------------------------------------------------------------------------------------------
def test_defect_conv0_loses_the_last_real_tap():
    w, bias = R.conv0_params()
    c, (ref, S) = conv0_refs()["1 u8 23x38 valid"]
    assert R.ratio(emu_conv0(c["img"], w, bias, c["pad"], c["relu"], skip=146), ref, S, R.L_CONV0) > 1.0


@pytest.mark.parametrize("name", ["2 u8 23x38 same window", "3 f32 nchw 19x21 same", "5b u8 1x1 same"])
def test_defect_conv0_padding_is_the_clamped_edge(name):
    w, bias = R.conv0_params()
    c, (ref, S) = conv0_refs()[name]
    assert R.ratio(emu_conv0(c["img"], w, bias, c["pad"], c["relu"], edge=True), ref, S, R.L_CONV0) > 1.0


@pytest.mark.parametrize("m,r", R.FORMS)
def test_defects_wino_in(m, r):
    bt = mats(m, r)[1]
    for name, (c, (ref, S)) in wino_in_refs(m, r).items():
        if name.startswith("a"):
            continue
        args = (c["x"], bt, m, r, c["pad"], c["ty"], c["tx"])
        assert R.ratio(emu_wino_in(*args, transposed=True), ref, S, R.wino_L(m, r)) > 1.0, name
        assert R.ratio(emu_wino_in(*args, last_col_off=1), ref, S, R.wino_L(m, r)) > 1.0, name


def dealt(v, vw, deal):
    """V as a launch of 256-thread workgroups leaves it when workgroup b works on list place deal(b, workgroups): thread i of the
    list owns (sample, tile, channel vector) = (i // cvn // T, i // cvn % T, i % cvn); places nobody works on stay NaN."""
    n, _, T, C = v.shape
    cvn = C // vw
    total = n * T * cvn
    grid = R.ceil_div(total, 256)
    written = np.zeros(grid * 256, bool)
    for b in range(grid):
        p = deal(b, grid)
        written[p * 256:(p + 1) * 256] = True
    w = written[:total].reshape(n, T, cvn)
    out = v.copy()
    out[~np.repeat(w, vw, axis=2)[:, None].repeat(v.shape[1], 1)] = np.nan
    return out


def xcd_deal(b, grid):
    per = grid >> 3
    return (b & 7) * per + (b >> 3) if b < per * 8 else b


def bad_deal(b, grid):          # right while per = 1, no bijection from per = 2 on
    per = grid >> 3
    return (b & 7) * per + (b >> 4) if b < per * 8 else b


@pytest.mark.parametrize("m,r", R.FORMS)
def test_defect_wino_in_deal_is_no_bijection(m, r):
    """Case a (per = 1) cannot see it; case a2 (per >= 2) must: unwritten elements are not finite, which `ratio` counts as a miss."""
    bt = mats(m, r)[1]
    refs = wino_in_refs(m, r)
    for name, sees in (("a grid", False), ("a2 re-dealt grid", True)):
        c, (ref, S) = refs[name]
        v = emu_wino_in(c["x"], bt, m, r, c["pad"], c["ty"], c["tx"])
        assert R.ratio(dealt(v, R.WINO_VW[(m, r)], xcd_deal), ref, S, R.wino_L(m, r)) <= 1.0, name
        assert (R.ratio(dealt(v, R.WINO_VW[(m, r)], bad_deal), ref, S, R.wino_L(m, r)) > 1.0) == sees, name


@pytest.mark.parametrize("m,r", R.FORMS)
def test_defects_wino_out(m, r):
    at = mats(m, r)[0]
    # surplus outputs of the partial last tile row written one row further: they land outside the view
    c, kw, (ref, S) = wino_out_ref(m, r, R.WINO_OUT_VARIANTS[0])
    buf = emu_wino_out(c["M"], at, m, r, c["ty"], c["tx"], c["H"], c["W"], surplus_rows=1, **kw)
    assert R.ratio(buf[:, :c["H"], :c["W"]], ref, S, R.wino_L(m, r, out=True)) <= 1.0       # the view itself is right
    assert not np.isnan(buf[:, c["H"]:]).all()                                                # the guard is not
    # ReLU after the accumulate
    c, kw, (ref, S) = wino_out_ref(m, r, R.WINO_OUT_VARIANTS[3])
    buf = emu_wino_out(c["M"], at, m, r, c["ty"], c["tx"], c["H"], c["W"], relu_after=True, **kw)
    assert R.ratio(buf[:, :c["H"], :c["W"]], ref, S, R.wino_L(m, r, out=True)) > 1.0


def test_defect_upadd_reads_the_next_row():
    lo, skip = R.upadd_case(4, False)
    assert (emu_upadd(lo, skip, defect=True).view(np.uint32) != R.upadd(lo, skip).view(np.uint32)).any()


@pytest.mark.parametrize("mode", ["trunc", "away"])
def test_defect_bf16_store(mode):
    """Truncation differs on half of all sums; ties away from zero only on the exact ties whose even neighbour lies towards zero
    (1 + 2^-8), which is why the case holds them."""
    lo, skip = R.upadd_case(8, True)
    s = emu_upadd(R.bf16_widen(lo), R.bf16_widen(skip))
    want = R.upadd_bf16(lo, skip)
    assert (emu_bf16_store(s) == want).all()
    bad = emu_bf16_store(s, mode) != want
    assert bad.any()
    if mode == "away":
        assert bad[:, 0, 0, 0].all() and not bad[:, 1, 0, 1].any()       # 1 + 2^-8 -> 1 (even is below); 1.0078125 + 2^-8 rounds up either way
    # the conv0 bf16 store: truncation of its fp32 output is seen as well
    w, bias = R.conv0_params()
    c = R.conv0_cases()["1 u8 23x38 valid"]
    y = emu_conv0(c["img"], w, bias, c["pad"], c["relu"])
    if mode == "trunc":
        assert (emu_bf16_store(y, mode) != R.bf16_bits(y)).any()


def test_defect_head_bf16_adds_the_bias_first():
    x, w, bias = R.head_case(5)
    xb = R.bf16_widen(R.bf16_bits(x))                            # what the bf16 kernel widens
    fp32_run = emu_head(xb, w, bias)
    assert (emu_head(xb, w, bias).view(np.uint32) == fp32_run.view(np.uint32)).all()
    assert (emu_head(xb, w, bias, bias_first=True).view(np.uint32) != fp32_run.view(np.uint32)).any()


def test_defect_predmap_takes_the_last_maximum():
    _, _, tp_l, crafted = R.predmap_case(5)
    want = R.first_max(tp_l)
    assert (emu_predmap_type(tp_l) == want).all()
    bad = emu_predmap_type(tp_l, last=True)
    for x, ch, v in crafted:
        if ch == 0:
            assert (want[:, 0, x] == v).all()
            assert (bad[:, 0, x] != v).all(), x


@pytest.mark.parametrize("C,bf16", [(6, False), (12, True)])
def test_upadd_channel_multiple_is_refused_by_name(C, bf16):
    """Needs the built libhvn_hip.so (no device): the one test of this file that calls the library.  Decided on the host before anything touches the device (on every version of the library: the launcher itself returns -1 for
    these), so made-up pointers are never dereferenced.  The refusal carries a text of its own, not an earlier failure's."""
    import ctypes

    from hover_net_amd import lib as L

    base = 0x10000000
    op = L.hvn_op()
    op.kind = 99
    assert L.lib().hvn_run_op(ctypes.byref(op), 1, None) == -1 and b"unknown op kind" in L.lib().hvn_last_error()
    op = L.hvn_op()
    op.kind, op.act_dtype = 3, int(bf16)
    op.x = L.hvn_view(base=base, sn=4 * 4 * 16, sy=4 * 16, sx=16, h=4, w=4, c=C)
    op.res = L.hvn_view(base=base + (1 << 20), sn=8 * 8 * 16, sy=8 * 16, sx=16, h=8, w=8, c=C)
    op.y = L.hvn_view(base=base + (2 << 20), sn=8 * 8 * 16, sy=8 * 16, sx=16, h=8, w=8, c=C)
    assert L.lib().hvn_run_op(ctypes.byref(op), 2, None) == -1
    err = L.lib().hvn_last_error()
    assert b"upadd" in err and b"unknown op kind" not in err, err


def test_bf16_helpers_are_torch_rne():
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.standard_normal(4096).astype(F32) * F32(10.0) ** rng.integers(-20, 20, 4096).astype(F32),
                        np.array([1 + 2.0 ** -8, 1.0078125 + 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, -0.0, 3.0e38], F32)])
    want = torch.from_numpy(x).bfloat16()
    assert (R.bf16_bits(x) == want.view(torch.int16).numpy().view(np.uint16)).all()
    assert (R.bf16_widen(R.bf16_bits(x)) == want.float().numpy()).all()

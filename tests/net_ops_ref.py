"""Float64 references of the plan's non-GEMM kernels (csrc/hvn_net_ops.hip) and their worst-case bound -- TEST INFRASTRUCTURE ONLY.

numpy only, written from include/hvn.h's comment block (CONV0, UPADD, HEAD, PREDMAP, WINO_IN, WINO_OUT), which this file thereby
pins; it imports nothing of the package.  tests/test_net_ops_ref.py proves the references and the bound on the CPU,
tests/test_gpu_net_ops.py holds the kernels to them.

Two kinds of statement:

  bit equality   where one rounding or pure data movement leaves nothing to tolerate (`upadd`, `upadd_bf16`, the bf16 store, the
                 type channel and the saturated / tied pixels of `predmap`);
  |got - ref64| <= B = (2 L + 4) 2^-24 S   per output element, `ref64` formed in float64 from the very fp32 / bf16 values the
                 kernel read and S = the float64 sum of the absolute values of all terms of that element (products, bias, the old
                 value when accumulating; |Mat| |d| |Mat|^T for the transforms, the matrices as the float32 values the kernel reads).

Why B holds for ANY summation order, fused or not.  A sum of k terms formed with one rounding per addition carries a relative error
of at most (k - 1) u (1 + O(k u)) of the sum of the terms' magnitudes, u = 2^-24, whatever the order or tree (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2); a product rounded on its own adds one more u per term.  With L the longest chain of
dependent additions of one output that is <= L u S fused and <= 2 L u S unfused.  A two-stage transform (tmp = Mat d, V = tmp Mat^T)
adds the stages' chains, which is how L counts them.  The + 4 covers the bias / accumulate / store roundings and the second-order
terms (L <= 148: L^2 u^2 < 2 u).  ReLU is 1-Lipschitz and moves no bound.  L: conv0 148 (147 taps and the zero of the odd K), head
65, WINO_IN 2 (m + r - 1), WINO_OUT 2 (m + r - 1) + 2."""
import numpy as np

U = 2.0 ** -24
L_CONV0 = 148
L_HEAD = 65


def wino_L(m, r, out=False):
    return 2 * (m + r - 1) + (2 if out else 0)


def bound(S, L):
    return (2 * L + 4) * U * np.asarray(S, np.float64)


def ratio(got, ref64, S, L):
    """max over ALL elements of |got - ref64| / B (inf where `got` is not finite or B is 0 with an error): <= 1 passes."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape == S.shape, (got.shape, ref64.shape, S.shape)
    assert np.isfinite(ref64).all() and np.isfinite(S).all()
    err = np.abs(got - ref64)
    b = bound(S, L)
    q = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1.0))
    q = np.where((b == 0) & (err > 0), np.inf, q)
    q = np.where(np.isfinite(got), q, np.inf)
    return float(q.max())


# ---- bf16 ---------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> uint16 bf16 bits, round to nearest, ties to even (finite inputs)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- CONV0 --------------------------------------------------------------------------------------
def conv0(img, w, bias, pad, relu):
    """img [n][H][W][3] uint8 or float32 (the logical NHWC image, whatever strides the device view has), w [7][7][3][64], bias [64]
    -> (ref64, S) [n][H + 2 pad - 6][W + 2 pad - 6][64]; zero padding."""
    n, H, W, _ = img.shape
    ho, wo = H + 2 * pad - 6, W + 2 * pad - 6
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, 3), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = img
    w64, b64 = np.asarray(w, np.float64), np.asarray(bias, np.float64)
    ref = np.zeros((n, ho, wo, 64), np.float64) + b64
    S = np.zeros((n, ho, wo, 64), np.float64) + np.abs(b64)
    for ky in range(7):
        for kx in range(7):
            a = xp[:, ky:ky + ho, kx:kx + wo]
            ref += a @ w64[ky, kx]
            S += np.abs(a) @ np.abs(w64[ky, kx])
    return (np.maximum(ref, 0.0) if relu else ref), S


# ---- UPADD --------------------------------------------------------------------------------------
def nearest2x(lo):
    """[n][h][w][c] -> [n][2h][2w][c]: out[y][x] = lo[y >> 1][x >> 1], by index arithmetic."""
    yy, xx = np.arange(2 * lo.shape[1]) >> 1, np.arange(2 * lo.shape[2]) >> 1
    return lo[:, yy][:, :, xx]


def upadd(lo, skip):
    """y = nearest2x(lo) + skip: ONE fp32 addition per element (IEEE round to nearest even, which numpy's float32 add is)."""
    assert lo.dtype == np.float32 and skip.dtype == np.float32
    y = nearest2x(lo) + skip
    exact = nearest2x(lo).astype(np.float64) + skip.astype(np.float64)       # the float64 statement of the same rounding
    assert (y == exact.astype(np.float32)).all()
    return y


def upadd_bf16(lo_bits, skip_bits):
    """bf16 bits in, bf16 bits out: the two values widened, one fp32 addition, rounded to bf16 to nearest even."""
    return bf16_bits(upadd(bf16_widen(lo_bits), bf16_widen(skip_bits)))


# ---- HEAD ---------------------------------------------------------------------------------------
def head(x, w, bias):
    """x [n][h][w][64] float32 (bf16 inputs widened by the caller), w [cout][64], bias [cout] -> (ref64, S) NCHW [n][cout][h][w]."""
    x64, w64, b64 = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    ref = x64 @ w64.T + b64
    S = np.abs(x64) @ np.abs(w64).T + np.abs(b64)
    return np.ascontiguousarray(ref.transpose(0, 3, 1, 2)), np.ascontiguousarray(S.transpose(0, 3, 1, 2))


# ---- PREDMAP ------------------------------------------------------------------------------------
def first_max(tp):
    """[n][T][h][w] -> index of the FIRST maximum along T, by the strict comparison the header's rule states (+0 == -0)."""
    best = np.zeros(tp[:, 0].shape, np.int64)
    bv = tp[:, 0].copy()
    for t in range(1, tp.shape[1]):
        up = tp[:, t] > bv
        bv = np.where(up, tp[:, t], bv)
        best = np.where(up, t, best)
    return best


def predmap(np_l, hv_l, tp_l=None):
    """NCHW logits -> float64 [n][h][w][3|4] = [first maximum of tp?, softmax(np)[1], hv0, hv1]."""
    l64 = np.asarray(np_l, np.float64)
    m = np.maximum(l64[:, 0], l64[:, 1])
    e0, e1 = np.exp(l64[:, 0] - m), np.exp(l64[:, 1] - m)
    ch = [] if tp_l is None else [first_max(np.asarray(tp_l)).astype(np.float64)]
    ch += [e1 / (e0 + e1), np.asarray(hv_l[:, 0], np.float64), np.asarray(hv_l[:, 1], np.float64)]
    return np.stack(ch, -1)


# ---- Winograd transforms ------------------------------------------------------------------------
def wino_tiles(x, m, r, pad, ty, tx):
    """x [n][H][W][c] -> d [n][ty][tx][nn][nn][c] float64: tile (i, j) starts at (m i - pad, m j - pad), zero outside the view."""
    n, H, W, c = x.shape
    nn = m + r - 1
    xp = np.zeros((n, pad + max(H, m * ty + nn) + nn, pad + max(W, m * tx + nn) + nn, c), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    d = np.empty((n, ty, tx, nn, nn, c), np.float64)
    for i in range(ty):
        for j in range(tx):
            d[:, i, j] = xp[:, m * i:m * i + nn, m * j:m * j + nn]
    return d


def wino_in(x, bt, m, r, pad, ty, tx):
    """V = B^T d B per tile: x [n][H][W][c] float32, bt [nn][nn] float32 -> (ref64, S) [n][nn * nn][ty * tx][c], position a * nn + b."""
    nn = m + r - 1
    b64 = np.asarray(bt, np.float32).astype(np.float64)
    d = wino_tiles(x, m, r, pad, ty, tx)
    n, c = x.shape[0], x.shape[3]
    v = np.einsum("ai,ntsijc,bj->nabtsc", b64, d, b64).reshape(n, nn * nn, ty * tx, c)
    S = np.einsum("ai,ntsijc,bj->nabtsc", np.abs(b64), np.abs(d), np.abs(b64)).reshape(n, nn * nn, ty * tx, c)
    return v, S


def wino_out(M, at, m, r, ty, tx, H, W, bias=None, relu=False, old=None):
    """y = relu?(A^T M A + bias) (+ old when accumulating: the ReLU comes BEFORE the accumulate): M [n][nn * nn][ty * tx][c] float32, at
    [m][nn] float32 -> (ref64, S) [n][H][W][c], the surplus outputs of partial last tiles dropped."""
    nn = m + r - 1
    n, _, _, c = M.shape
    a64 = np.asarray(at, np.float32).astype(np.float64)
    M6 = np.asarray(M, np.float64).reshape(n, nn, nn, ty, tx, c)
    y = np.einsum("pa,nabtsc,qb->ntpsqc", a64, M6, a64).reshape(n, m * ty, m * tx, c)[:, :H, :W]
    S = np.einsum("pa,nabtsc,qb->ntpsqc", np.abs(a64), np.abs(M6), np.abs(a64)).reshape(n, m * ty, m * tx, c)[:, :H, :W]
    assert y.shape == (n, H, W, c), "the tile grid does not cover y"
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
        S = S + np.abs(np.asarray(bias, np.float64))
    if relu:
        y = np.maximum(y, 0.0)
    if old is not None:
        y = y + np.asarray(old, np.float64)
        S = S + np.abs(np.asarray(old, np.float64))
    return y, S


# ---- the cases both test files run (made once per process, never changed) -----------------------------------------------------
FORMS = ((2, 5), (4, 5), (4, 3), (6, 3), (6, 5))
WINO_A_CHANNELS = {(2, 5): 64, (4, 5): 128, (4, 3): 192, (6, 3): 256, (6, 5): 128}    # > 8 workgroups and no multiple of 8
WINO_VW = {(2, 5): 4, (4, 5): 2, (4, 3): 4, (6, 3): 2, (6, 5): 1}                      # channels per thread of the kernels


def ceil_div(a, b):
    return -(-a // b)


def conv0_params():
    rng = np.random.default_rng(301)
    w = (rng.standard_normal((7, 7, 3, 64)) * 0.1 / 255).astype(np.float32)
    return w, (rng.standard_normal(64) * 0.2).astype(np.float32)


def conv0_cases():
    """name -> dict(img = logical NHWC image, pad, relu, layout).  Layouts: "u8" dense NHWC bytes; "nchw" float32 planes (sc = H W,
    sx = 1, sy = W); "nhwc_win" float32 NHWC window of an image 5 pixels wider (sy = 3 (W + 5))."""
    rng = np.random.default_rng(302)
    u8 = lambda h, w: rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)                      # noqa: E731
    f32 = lambda h, w: (rng.random((2, h, w, 3)) * 255).astype(np.float32)                     # noqa: E731
    big = u8(23, 38)
    return {
        "1 u8 23x38 valid": dict(img=big, pad=0, relu=1, layout="u8"),
        "2 u8 23x38 same window": dict(img=big, pad=3, relu=0, layout="u8", window=True),
        "3 f32 nchw 19x21 same": dict(img=f32(19, 21), pad=3, relu=1, layout="nchw"),
        "4 f32 nhwc window 13x24 valid": dict(img=f32(13, 24), pad=0, relu=1, layout="nhwc_win"),
        "5a u8 7x7 valid": dict(img=u8(7, 7), pad=0, relu=1, layout="u8"),
        "5b u8 1x1 same": dict(img=u8(1, 1), pad=3, relu=1, layout="u8"),
    }


def upadd_case(C, bf16, n=2, h=5, w=7, seed=310):
    """(lo, skip) [n][h][w][C] / [n][2h][2w][C]: float32, or uint16 bf16 bits of finite normal values whose first pixels hold exact
    ties (1 + 2^-8 -> 1, 1.0078125 + 2^-8 -> 1.015625), near-ties on both sides of them, and their negatives."""
    rng = np.random.default_rng(seed + C)
    lo = rng.standard_normal((n, h, w, C)).astype(np.float32)
    skip = rng.standard_normal((n, 2 * h, 2 * w, C)).astype(np.float32)
    if not bf16:
        return lo, skip
    lo, skip = bf16_widen(bf16_bits(lo)), bf16_widen(bf16_bits(skip))
    tie, above, below = 2.0 ** -8, 2.0 ** -8 * (1 + 2.0 ** -7), 2.0 ** -8 * (1 - 2.0 ** -8)
    crafted = [(1.0, tie), (1.0078125, tie), (1.0, above), (1.0, below), (1.0078125, above), (1.0078125, below)]
    crafted += [(-a, -b) for a, b in crafted]
    assert len(crafted) <= 2 * w
    for k, (a, b) in enumerate(crafted):              # output pixel (k & 1, 2 (k >> 1)), channel k % C, reads lo pixel (0, k >> 1)
        lo[:, 0, k >> 1, k % C] = a
        skip[:, k & 1, (k >> 1) * 2, k % C] = b
    for t in (lo, skip):
        assert (bf16_widen(bf16_bits(t)) == t).all() and (np.abs(t[t != 0]) > 1e-30).all()
    return bf16_bits(lo), bf16_bits(skip)


def head_case(cout, n=3, h=17, w=19):
    rng = np.random.default_rng(320 + cout)
    x = rng.standard_normal((n, h, w, 64)).astype(np.float32)
    return x, (rng.standard_normal((cout, 64)) * 0.1).astype(np.float32), (rng.standard_normal(cout) * 0.2).astype(np.float32)


def predmap_case(T, n=3, h=17, w=19):
    """NCHW logits with crafted pixels in row 0 of every sample -> (np, hv, tp | None, crafted) where crafted lists
    (x, channel, exact value) of output row 0.  Types: two and five exactly equal maxima, +0.0 against -0.0."""
    rng = np.random.default_rng(330 + T)
    np_l = (3 * rng.standard_normal((n, 2, h, w))).astype(np.float32)
    hv_l = (3 * rng.standard_normal((n, 2, h, w))).astype(np.float32)
    c0 = 1 if T else 0
    np_l[:, :, 0, 0] = 1.625
    np_l[:, :, 0, 1] = -37.5
    np_l[:, 0, 0, 2], np_l[:, 1, 0, 2] = 200.0, -200.0
    np_l[:, 0, 0, 3], np_l[:, 1, 0, 3] = -200.0, 200.0
    crafted = [(0, c0, 0.5), (1, c0, 0.5), (2, c0, 0.0), (3, c0, 1.0)]
    tp_l = None
    if T:
        tp_l = (3 * rng.standard_normal((n, T, h, w))).astype(np.float32)
        if T >= 5:
            tp_l[:, :, 0, 4] = -1.0
            tp_l[:, 1, 0, 4] = tp_l[:, 3, 0, 4] = 2.5          # two equal maxima -> 1
            tp_l[:, :, 0, 5] = 0.75                            # five equal maxima -> 0
            tp_l[:, :, 0, 6] = -3.0
            tp_l[:, 2, 0, 6], tp_l[:, 4, 0, 6] = 0.0, -0.0     # +0.0 then -0.0 -> 2
            tp_l[:, :, 0, 7] = -3.0
            tp_l[:, 1, 0, 7], tp_l[:, 2, 0, 7] = -0.0, 0.0     # -0.0 then +0.0 -> 1
            crafted += [(4, 0, 1.0), (5, 0, 0.0), (6, 0, 2.0), (7, 0, 1.0)]
        else:
            crafted += [(4, 0, 0.0)]
    return np_l, hv_l, tp_l, crafted


def wino_in_cases(m, r):
    """name -> dict(x [n][H][W][C] float32, pad, ty, tx).  hvn_wino_in deals workgroup b < 8 per (per = workgroups // 8) to list place
    (b % 8) per + b // 8 and leaves the tail b >= 8 per in place.  a: 12 .. 15 workgroups -- per = 1, where the deal is the identity,
    and a tail; a2: twice the channels, 23 .. 30 workgroups -- per = 2 | 3, where the deal moves workgroups (anything but a bijection
    leaves elements of V unwritten, i.e. NaN, or written from another tile's data), and a tail; b: one vector, tiles past the
    input, no padding; c: the placement case (a strided V)."""
    rng = np.random.default_rng(340 + 10 * m + r)
    C = WINO_A_CHANNELS[(m, r)]
    a = dict(x=rng.standard_normal((3, 15, 17, C)).astype(np.float32), pad=r // 2, ty=ceil_div(15, m), tx=ceil_div(17, m))
    wgs = ceil_div(3 * a["ty"] * a["tx"] * (C // WINO_VW[(m, r)]), 256)
    assert wgs > 8 and wgs % 8, wgs
    a2 = dict(a, x=np.random.default_rng(345 + 10 * m + r).standard_normal((3, 15, 17, 2 * C)).astype(np.float32))
    wgs2 = ceil_div(3 * a["ty"] * a["tx"] * (2 * C // WINO_VW[(m, r)]), 256)
    assert wgs2 >= 16 and wgs2 % 8, wgs2
    b = dict(x=rng.standard_normal((1, 9, 11, 4)).astype(np.float32), pad=0, ty=ceil_div(9 - r + 1, m), tx=ceil_div(11 - r + 1, m), window=True)
    nn = m + r - 1
    assert m * (b["ty"] - 1) + nn > 9 and m * (b["tx"] - 1) + nn > 11
    c = dict(x=rng.standard_normal((2, 6, 7, 8)).astype(np.float32), pad=r // 2, ty=ceil_div(6, m), tx=ceil_div(7, m), strided_v=True)
    return {"a grid": a, "a2 re-dealt grid": a2, "b small": b, "c placement": c}


def wino_fused_case(m, r):
    rng = np.random.default_rng(350 + 10 * m + r)
    return dict(lo=rng.standard_normal((2, 8, 9, 8)).astype(np.float32), x=rng.standard_normal((2, 16, 18, 8)).astype(np.float32),
                pad=r // 2, ty=ceil_div(16, m), tx=ceil_div(18, m))


def wino_out_case(m, r, n=2, H=15, W=17, C=8):
    rng = np.random.default_rng(360 + 10 * m + r)
    nn = m + r - 1
    ty, tx = ceil_div(H, m), ceil_div(W, m)
    return dict(M=rng.standard_normal((n, nn * nn, ty * tx, C)).astype(np.float32), bias=(rng.standard_normal(C) * 0.5).astype(np.float32),
                old=rng.standard_normal((n, H, W, C)).astype(np.float32), ty=ty, tx=tx, H=H, W=W)


# (name, bias, relu, accumulate); the last -- ReLU and accumulate together -- is the only combination at which "ReLU after the
# accumulate" differs from the kernel's order
WINO_OUT_VARIANTS = (("bias relu", True, True, False), ("plain", False, False, False), ("accumulate", False, False, True),
                     ("bias relu accumulate", True, True, True))

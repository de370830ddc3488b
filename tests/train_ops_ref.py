"""Float64 references, worst-case bounds and fp32 mirrors of the training step's non-GEMM kernels (csrc/hvn_train.hip: BN+ReLU forward
and backward, UPADD_BWD, HEAD_BWD, CONV0_WGRAD, the two loss stages, Adam) -- TEST INFRASTRUCTURE ONLY.

numpy only; it imports nothing of the package.  Written from the training section of include/hvn.h, which it thereby pins, and -- the
loss -- from the reference's formulae (utils.py:54-172 as composed by run_desc.py:40-82).  tests/test_train_ops_ref.py proves the
references and the bounds on the CPU, tests/test_gpu_train_ops.py holds the kernels to them.

Every `*_ref` function returns, per output, `(ref64, B)`: ref64 is the exact (float64) value of the operation on the very fp32 / uint8
/ int32 values the kernel read -- a later stage is given what the earlier stage of the SAME kernel left (save, coef, sums, sobel_ws,
the activation whose sign is the ReLU mask; Adam's m, v, w), so that no error compounds into a bound -- and B = K u S with u = 2^-24,
S the float64 sum of the magnitudes of the element's terms and K counted as in tests/net_ops_ref.py:

  * one u per fp32 rounding of a term, relative to that term;
  * a sum of k terms in ANY order or tree carries at most (k - 1) u (1 + O(k u)) of the sum of the terms' magnitudes (Higham, Accuracy
    and Stability of Numerical Algorithms, section 4.2), and no operand of a tree passes through more additions than the tree is high:
    L, the longest chain of dependent additions, is read off the kernel's structure (never off its results);  fused multiply-adds
    round once per step, separate products twice: L u S fused, 2 L u S where the hardware may do either (the MFMA);
  * sums the kernel keeps in double cost L_d 2^-53 S, which the constants below carry as one more u (L_d < 2^20);
  * expf, logf and sqrtf: 1 ulp = 2 u, the maximum the HIP math API documents for the device library; an error d of expf's
    argument is a relative error |d| of its value, an error of logf's argument a relative one of the argument;
  * "+ 1" in a constant covers the second-order terms (every K u < 2^-10);
  * TINY = 2^-126 absolute per probability: a softmax term that underflows (logits 200 apart) may be flushed.

K per output (the docstrings of the functions repeat them):
  BN forward   mean: 1, rstd: 1 + v, scale: 1 + v, shift: |beta - mean sc| + (v + 1)|mean sc| (v: the double sums' error amplified
               by (E z^2 + mean^2) / (var + eps)); running stats: 3 + 1 over |(1 - m) r| + |m x|; a: 2 + 1 over |z sc| + |sh|.
  BN backward  dbeta: 2 + 1, dgamma: 5 + 1, coef: 1 | 2 | 5 (+ 1), dz: 6 + 1 over |dz0| + |c1| (|g| + |c2| + |xhat c3|).
  UPADD_BWD    dskip: ONE addition, bit-exact; dlo: 4 + 1 over |dlo0| + sum |dy|.
  HEAD_BWD     da: cout + 1 (fused chain) + 1; dW, db: L + 1 (product) + 1, L = 6 (wave butterfly) + groups per workgroup + 2 (four wave rows)
               + workgroups (atomics in any order, or the fixed-order sum of the copies) + 1 (the old value).
  CONV0_WGRAD  2 L + 2 (pixel / 255 as a rounded product of a rounded constant) + 2, L = 64 per tile of the workgroup + 4 (waves) +
               workgroups + 1.
  loss, Adam   see loss_forward_ref, loss_backward_ref, adam_ref.

The `*_mirror` functions restate each kernel's arithmetic in numpy float32 (double accumulators where the kernel has them; numpy's own
summation order; expf / logf as the correctly rounded float32 of the float64 function).  They exist to prove on the CPU that the intact
arithmetic stays within B and that each named MUTANT of it does not."""
import numpy as np

U = 2.0 ** -24
UD = 2.0 ** -53
TINY = 2.0 ** -126
ULP_EXP = ULP_LOG = ULP_SQRT = 1          # documented maximum ulp error of the device library's expf / logf / sqrtf
F32, F64 = np.float32, np.float64


def f32(x):
    return np.asarray(x, F32)


def f64(x):
    return np.asarray(x, F64)


def ratio(got, ref64, B):
    """max over ALL elements of |got - ref64| / B (inf where `got` is not finite, or B is 0 with an error): <= 1 passes."""
    got, ref64, B = f64(got), f64(ref64), f64(B)
    assert got.shape == ref64.shape == B.shape, (got.shape, ref64.shape, B.shape)
    assert np.isfinite(ref64).all() and np.isfinite(B).all() and (B >= 0).all()
    err = np.abs(got - ref64)
    q = np.where(err == 0, 0.0, err / np.where(B > 0, B, 1.0))
    q = np.where((B == 0) & (err > 0), np.inf, q)
    q = np.where(np.isfinite(got), q, np.inf)
    return float(q.max()) if q.size else 0.0


def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even) as float32."""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def cdiv(a, b):
    return -(-a // b)


def colsum(a):
    """Sum over axis 0 of [rows][C] by numpy's pairwise scheme (it applies along the contiguous axis only): an error of O(log rows), where a
    plain a.sum(0) is a sequential chain over all rows -- longer than any chain of the kernels, which the bounds are counted for."""
    return np.ascontiguousarray(np.asarray(a).T).sum(1)


# ---- BatchNorm (train) + ReLU -------------------------------------------------------------------------------------------------------
BN_MAX_PARTS = 256


def bn_grid(C, rows):
    """csrc/hvn_train.hip:bn_grid -> dict(lq, rper, gx, gy, passes, capped): a thread owns one channel quad of every (gy * rper)-th row
    and takes them eight at a time (`passes` 8-row iterations, the last one ragged unless the rows divide)."""
    cq = C // 4
    lq = 64
    while lq > cq:
        lq >>= 1
    lq = max(lq, 1)
    rper = 256 // lq
    gx = cdiv(cq, lq)
    want = cdiv(rows, rper * 16)
    cap = max(1, min(1024 // gx, BN_MAX_PARTS))
    gy = max(1, min(want, cap))
    per_thread = cdiv(rows, gy * rper)
    return dict(lq=lq, rper=rper, gx=gx, gy=gy, passes=cdiv(per_thread, 8), per_thread=per_thread, capped=want > cap,
                ragged=rows % (8 * gy * rper) != 0)


def bn_chain(C, rows):
    """Longest chain of dependent double additions of one channel's sum: the thread's rows, the block's row lanes, the partials."""
    g = bn_grid(C, rows)
    return g["per_thread"] + g["rper"] + cdiv(g["gy"], 8) + 8


def bn_forward_ref(z, gamma, beta, rm, rv, eps, mom):
    """z [rows][C] fp32 (the logical view), gamma, beta, rm, rv [C] fp32, eps, mom fp32 scalars
    -> dict(save=(ref [4][C], B), rm=(ref, B), rv=(ref, B)).  save = scale, shift, mean, rstd.
    mean = sum z / n and var = sum z^2 / n - mean^2 are formed in double by the kernel; the reference takes the variance as the mean of
    (z - mean)^2.  With L_d = bn_chain: |d mean| <= em = L_d 2^-53 mean|z|; |d var| <= ev = (3 L_d + 8) 2^-53 (E z^2 + mean^2) (the two
    sums, and mean's error through mean^2: |mean| em <= L_d 2^-53 E z^2); rstd = (var + eps)^-1/2 moves by er = ev / (2 (var + eps)) + 4
    2^-53 relative.  Then one u for each float conversion."""
    z64, n = f64(z), z.shape[0]
    eps, mom = float(F32(eps)), float(F32(mom))
    Ld = bn_chain(z.shape[1], n)
    mean = colsum(z64) / n
    var = colsum((z64 - mean) ** 2) / n
    msq = colsum(z64 * z64) / n
    em = Ld * UD * colsum(np.abs(z64)) / n
    ev = (3 * Ld + 8) * UD * (msq + mean * mean)
    assert (ev <= 1e-3 * (var + eps)).all(), "the first-order amplification of the variance's error needs ev << var + eps"
    er = 0.5 * ev / (var + eps) + 4 * UD
    rstd = 1.0 / np.sqrt(var + eps)
    g64, b64 = f64(gamma), f64(beta)
    sc = g64 * rstd
    sh = b64 - mean * sc
    save = np.stack([sc, sh, mean, rstd])
    B = np.stack([(U + er + UD) * np.abs(sc), U * np.abs(sh) + (er + 4 * UD + U * U) * np.abs(mean * sc) + em * np.abs(sc) * (1 + U),
                  U * np.abs(mean) + em, (U + er) * rstd])
    t1, t2 = (1.0 - mom) * f64(rm), mom * mean
    rm_ref = t1 + t2
    B_rm = 4 * U * (np.abs(t1) + np.abs(t2)) + mom * em
    unb = var * n / (n - 1.0)
    v1, v2 = (1.0 - mom) * f64(rv), mom * unb
    B_rv = 4 * U * (np.abs(v1) + np.abs(v2)) + mom * ev * n / (n - 1.0) * (1 + U)
    return dict(save=(save, B), rm=(rm_ref, B_rm), rv=(v1 + v2, B_rv))


def bn_apply_ref(z, save):
    """a = relu(fl(fl(z sc) + sh)) from the scale / shift the kernel itself saved: two roundings, K = 2 + 1 over |z sc| + |sh|; the ReLU is
    1-Lipschitz."""
    z64, sc, sh = f64(z), f64(save[0]), f64(save[1])
    return np.maximum(z64 * sc + sh, 0.0), 3 * U * (np.abs(z64 * sc) + np.abs(sh))


def bn_backward_reduce_ref(z, da, mask, save, gamma, dgamma0, dbeta0):
    """mask [rows][C] bool: a > 0 of the activation the forward kernel STORED (the exact tests pin the recomputed predicate to it).
    g = da mask, xhat = fl(fl(z - mean) rstd) (2 u), g xhat rounded (3 u in all), both sums in double.
    -> dict(dgamma, dbeta, coef [3][C]): dbeta = fl(dbeta0 + fl(s1)): K = 2 + 1 over |dbeta0| + sum |g|; dgamma likewise with the
    products' 3 u: K = 5 + 1; coef = fl(gamma rstd): 1 (+ 1), fl(s1 / n): 1 + 1, fl(s2 / n): 1 + 3 + 1."""
    z64, n = f64(z), z.shape[0]
    mean, rstd = f64(save[2]), f64(save[3])
    g = f64(da) * mask
    xh = (z64 - mean) * rstd
    s1, s2 = colsum(g), colsum(g * xh)
    a1, a2 = colsum(np.abs(g)), colsum(np.abs(g * xh))
    c1 = f64(gamma) * rstd
    coef = np.stack([c1, s1 / n, s2 / n])
    Bc = np.stack([2 * U * np.abs(c1), 2 * U * a1 / n, 5 * U * a2 / n])
    return dict(dbeta=(f64(dbeta0) + s1, 3 * U * (np.abs(f64(dbeta0)) + a1)), dgamma=(f64(dgamma0) + s2, 6 * U * (np.abs(f64(dgamma0)) + a2)),
                coef=(coef, Bc))


def bn_backward_apply_ref(z, da, mask, save, coef, dz0):
    """dz = dz0 + c1 (g - c2 - xhat c3) from the save and coef the kernel itself left; xhat 2 u, xhat c3 3 u, two subtractions, the product
    with c1, the accumulation: every term within 6 u of S = |dz0| + |c1| (|g| + |c2| + |xhat c3|), K = 6 + 1."""
    z64 = f64(z)
    mean, rstd = f64(save[2]), f64(save[3])
    c1, c2, c3 = f64(coef[0]), f64(coef[1]), f64(coef[2])
    g = f64(da) * mask
    p = (z64 - mean) * rstd * c3
    ref = f64(dz0) + c1 * (g - c2 - p)
    S = np.abs(f64(dz0)) + np.abs(c1) * (np.abs(g) + np.abs(c2) + np.abs(p))
    return ref, 7 * U * S


BN_MUTANTS = ("sums_fp32", "biased_var", "shift_fp32", "mask_ge", "no_xhat")


def bn_mirror(z, gamma, beta, rm, rv, eps, mom, da, dgamma0, dbeta0, dz0, mutant=None):
    """The forward and backward kernels' arithmetic -> dict(save, rm, rv, a, dgamma, dbeta, coef, dz)."""
    assert mutant is None or mutant in BN_MUTANTS
    z, da = f32(z), f32(da)
    n = z.shape[0]
    eps, mom = F32(eps), F32(mom)
    if mutant == "sums_fp32":
        s1 = f64(np.cumsum(z, 0, dtype=F32)[-1])
        s2 = f64(np.cumsum(z * z, 0, dtype=F32)[-1])
    else:
        s1, s2 = colsum(f64(z)), colsum(f64(z) * f64(z))
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + f64(eps))
    sc = f64(gamma) * rstd
    sh = f64(beta) - mean * sc
    if mutant == "shift_fp32":
        sh = f32(beta) - f32(mean) * f32(sc)
    save = np.stack([f32(sc), f32(sh), f32(mean), f32(rstd)])
    unb = var if mutant == "biased_var" else var * n / (n - 1.0)
    one = F32(1.0)
    rm1 = (one - mom) * f32(rm) + mom * f32(mean)
    rv1 = (one - mom) * f32(rv) + mom * f32(unb)
    act = z * save[0] + save[1]                            # two roundings, as the library is built (no contraction)
    a = np.maximum(act, F32(0))
    mask = a >= 0 if mutant == "mask_ge" else act > 0
    g = np.where(mask, da, F32(0))
    xh = (z - save[2]) * save[3]
    t1, t2 = colsum(f64(g)), colsum(f64(g * xh))
    dgamma, dbeta = f32(dgamma0) + f32(t2), f32(dbeta0) + f32(t1)
    coef = np.stack([f32(gamma) * save[3], f32(t1 / n), f32(t2 / n)])
    inner = g - coef[1] if mutant == "no_xhat" else g - coef[1] - xh * coef[2]
    dz = f32(dz0) + coef[0] * inner
    return dict(save=save, rm=rm1, rv=rv1, a=a, dgamma=dgamma, dbeta=dbeta, coef=coef, dz=dz)


def bn_judge(inp, out):
    """inp: dict(z, gamma, beta, rm, rv, eps, mom, da, dgamma0, dbeta0, dz0) as the kernels read them, out: what a kernel (or mirror)
    left -> dict(output name -> max err / B), every stage judged from its own inputs."""
    z = inp["z"]
    f = bn_forward_ref(z, inp["gamma"], inp["beta"], inp["rm"], inp["rv"], inp["eps"], inp["mom"])
    r = {k: ratio(out[k], *f[k]) for k in ("save", "rm", "rv")}
    r["a"] = ratio(out["a"], *bn_apply_ref(z, out["save"]))
    mask = f32(out["a"]) > 0
    b = bn_backward_reduce_ref(z, inp["da"], mask, out["save"], inp["gamma"], inp["dgamma0"], inp["dbeta0"])
    r.update({k: ratio(out[k], *b[k]) for k in ("dgamma", "dbeta", "coef")})
    if out.get("dz") is not None:
        r["dz"] = ratio(out["dz"], *bn_backward_apply_ref(z, inp["da"], mask, out["save"], out["coef"], inp["dz0"]))
    return r


# ---- UPADD_BWD ----------------------------------------------------------------------------------------------------------------------
def upadd_bwd_ref(dy, dlo0, dskip0):
    """dy [n][h][w][c], dlo0 [n][h/2][w/2][c], dskip0 [n][h][w][c] fp32 -> dlo (ref, B), dskip as the ONE fp32 addition it is (bit-exact).
    dlo = dlo0 + the four taps: five terms in any order, K = 4 + 1."""
    n, h, w, c = dy.shape
    d = f64(dy).reshape(n, h // 2, 2, w // 2, 2, c)
    ref = f64(dlo0) + d.sum((2, 4))
    S = np.abs(f64(dlo0)) + np.abs(d).sum((2, 4))
    return (ref, 5 * U * S), f32(dskip0) + f32(dy)


def upadd_bwd_mirror(dy, dlo0, dskip0, mutant=None):
    assert mutant in (None, "three_taps")
    dy = f32(dy)
    t = [dy[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    s = (t[0] + t[1]) + t[2]
    if mutant is None:
        s = s + t[3]
    return f32(dlo0) + s, f32(dskip0) + dy


# ---- HEAD_BWD -----------------------------------------------------------------------------------------------------------------------
HEAD_MAX_WGS = 512


def head_bwd_chain(pixels):
    groups = cdiv(pixels, 256)
    wgs = min(groups, HEAD_MAX_WGS)
    return 6 + cdiv(groups, wgs) + 2 + wgs + 1


def head_bwd_ref(x, dl, w, da0, dW0, db0):
    """x, da0 [P][64] fp32 (P pixels in n, y, x order), dl [P][cout] (the NCHW logit gradient, pixel-major), w, dW0 [cout][64], db0 [cout]
    -> dict(da, dW, db).  da: a fused chain over cout, K = cout + 1 + 1 over |da0| + sum |dl w|; dW, db: K = L + 1 + 1, L = head_bwd_chain,
    over |dW0| + sum |dl x| (db: + sum |dl|; no product, the same K)."""
    x64, dl64, w64 = f64(x), f64(dl), f64(w)
    cout = w.shape[0]
    K = head_bwd_chain(x.shape[0]) + 2
    da = (f64(da0) + dl64 @ w64, (cout + 2) * U * (np.abs(f64(da0)) + np.abs(dl64) @ np.abs(w64)))
    dW = (f64(dW0) + dl64.T @ x64, K * U * (np.abs(f64(dW0)) + np.abs(dl64).T @ np.abs(x64)))
    db = (f64(db0) + dl64.sum(0), K * U * (np.abs(f64(db0)) + np.abs(dl64).sum(0)))
    return dict(da=da, dW=dW, db=db)


def head_bwd_mirror(x, dl, w, da0, dW0, db0, mutant=None):
    assert mutant in (None, "drop_last", "bf16_products")
    x, dl, w = f32(x), f32(dl), f32(w)
    da = f32(da0).copy()
    for co in range(w.shape[0]):                           # fmaf chain: one rounding per step
        da = f32(f64(dl[:, co:co + 1]) * f64(w[co]) + f64(da))
    P = x.shape[0] - (1 if mutant == "drop_last" else 0)
    dW = np.zeros(w.shape, F32)
    for co in range(w.shape[0]):
        prod = dl[:P, co:co + 1] * x[:P]                   # [P][64], each product rounded
        dW[co] = (bf16_round(prod) if mutant == "bf16_products" else prod).sum(0, dtype=F32)
    return dict(da=da, dW=f32(dW0) + dW, db=f32(db0) + dl[:P].sum(0, dtype=F32))


# ---- CONV0_WGRAD --------------------------------------------------------------------------------------------------------------------
CONV0_MAX_WGS = 512


def conv0_wgrad_chain(n, ho, wo):
    tiles = n * cdiv(ho, 16) * cdiv(wo, 16)
    wgs = min(tiles, CONV0_MAX_WGS)
    return 64 * cdiv(tiles, wgs) + 4 + wgs + 1


def _conv0_sums(img, dz, pad, scale):
    n, H, W, _ = img.shape
    ho, wo = dz.shape[1], dz.shape[2]
    assert (ho, wo) == (H + 2 * pad - 6, W + 2 * pad - 6)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, 3), dz.dtype)
    xp[:, pad:pad + H, pad:pad + W] = scale(img)
    win = np.lib.stride_tricks.sliding_window_view(xp, (7, 7), axis=(1, 2))              # [n][ho][wo][3][7][7]
    patches = np.ascontiguousarray(win.transpose(0, 1, 2, 4, 5, 3)).reshape(-1, 147)         # one GEMM over the pixels
    return (dz.reshape(-1, 64).T @ patches).reshape(64, 7, 7, 3)


def conv0_wgrad_ref(img, dz, pad, dW0):
    """img [n][H][W][3] uint8 (the logical image), dz [n][ho][wo][64] fp32, dW0 [64][7][7][3] -> (ref, B): dW += sum dz * img / 255 over
    the zero-padded image.  K = 2 L + 2 + 2, L = conv0_wgrad_chain."""
    ref = f64(dW0) + _conv0_sums(img, f64(dz), pad, lambda i: f64(i) / 255.0)
    S = np.abs(f64(dW0)) + _conv0_sums(img, np.abs(f64(dz)), pad, lambda i: f64(i) / 255.0)
    return ref, (2 * conv0_wgrad_chain(dz.shape[0], dz.shape[1], dz.shape[2]) + 4) * U * S


def conv0_wgrad_mirror(img, dz, pad, dW0, mutant=None):
    assert mutant in (None, "drop_last", "bf16_products")
    dz = f32(dz).copy()
    if mutant == "drop_last":
        dz[-1, -1, -1] = 0
    px = lambda i: f32(i) * (F32(1.0) / F32(255.0))
    if mutant == "bf16_products":        # every product rounded to bf16: the exact products in double, rounded, summed in fp32
        n, H, W, _ = img.shape
        ho, wo = dz.shape[1], dz.shape[2]
        xp = np.zeros((n, H + 2 * pad, W + 2 * pad, 3), F32)
        xp[:, pad:pad + H, pad:pad + W] = px(img)
        out = np.zeros((64, 7, 7, 3), F32)
        for r in range(7):
            for s in range(7):
                pr = bf16_round(dz[..., :, None] * xp[:, r:r + ho, s:s + wo][..., None, :])
                out[:, r, s, :] = pr.reshape(-1, 64, 3).sum(0, dtype=F32)
        return f32(dW0) + out
    return f32(dW0) + _conv0_sums(img, dz, pad, px)


# ---- losses -------------------------------------------------------------------------------------------------------------------------
EPS32 = F32(10e-8)                                  # utils.py:56 (the reference's literal)
LO, HI = float(EPS32), float(F32(1.0) - EPS32)      # clamp bounds as fp32 forms them
SMOOTH = float(F32(1e-3))


def sobel5(dtype):
    """kernel_h[r][s] = h / (h^2 + v^2 + 1e-15), h = r - 2, v = s - 2 (utils.py:135-137), formed in `dtype`; kernel_v is its transpose."""
    r = np.arange(-2, 3).astype(dtype)
    h, v = np.meshgrid(r, r, indexing="ij")
    return (h / (h * h + v * v + dtype(1.0e-15))).astype(dtype)


def _corr5(d, k, mode="zero"):
    """out[y][x] = sum_{r,s} k[r][s] d[y + r - 2][x + s - 2] over [n][h][w], zero (or, the mutant, edge) padding; fused chain in fp32."""
    n, h, w = d.shape
    p = np.pad(d, ((0, 0), (2, 2), (2, 2)), mode="edge" if mode == "edge" else "constant")
    acc = np.zeros(d.shape, F64)
    for r in range(5):
        for s in range(5):
            acc = f64(k[r, s]) * f64(p[:, r:r + h, s:s + w]) + acc
            if d.dtype == F32:
                acc = f64(f32(acc))
    return acc.astype(d.dtype)


def _softmax64(l):
    """l [..., T] fp32 -> (p, dp): float64 softmax and the absolute error bound of the kernel's fp32 one.  fl(l - mx): |a| u on the
    argument = relative on e; expf 2 ULP_EXP u; the sum of T positive terms (T - 1) u; the reciprocal, the product: relative
    ep_c = ee_c + max ee + (T + 1) u (+ 1)."""
    l64 = f64(l)
    a = l64 - l64.max(-1, keepdims=True)
    e = np.exp(a)
    p = e / e.sum(-1, keepdims=True)
    T = l.shape[-1]
    ee = (np.abs(a) + 2 * ULP_EXP) * U
    ep = ee + ee.max(-1, keepdims=True) + (T + 2) * U
    return p, ep * p + TINY, ep


def _exp32(x):
    return f32(np.exp(f64(x)))


def _log32(x):
    with np.errstate(divide="ignore"):
        return f32(np.log(f64(x)))


def _softmax32(l):
    l = f32(l)
    e = _exp32(l - l.max(-1, keepdims=True))
    s = e[..., 0].copy()
    for c in range(1, l.shape[-1]):
        s = s + e[..., c]
    return e * (F32(1.0) / s)[..., None]


def _psum32(p):
    s = p[..., 0].copy()
    for c in range(1, p.shape[-1]):
        s = s + p[..., c]
    return s


def loss_chain(pixels):
    return 8 + cdiv(pixels, 256)


def _branch_forward(l, t):
    """One softmax branch: l [P][T] fp32, t [P] class index -> per-class (inse, l, r) sums with bounds and the bce sum with its bound.
    q = p_t / sum p: relative eq = ep_t + max ep + T u; -logf(clamp(q)): the clamp is monotone and moves nothing apart in log q, so
    |d log| <= eq, + 2 ULP_LOG u |log q| for logf."""
    P, T = l.shape
    p, dp, ep = _softmax64(l)
    oh = np.arange(T)[None, :] == t[:, None]
    q = p[np.arange(P), t] / p.sum(-1)
    eq = ep[np.arange(P), t] + ep.max(-1) + T * U
    lq = -np.log(np.clip(q, LO, HI))
    Ld = loss_chain(P) * UD
    bce = (lq.sum(), (eq + (2 * ULP_LOG + 1) * U * lq).sum() + Ld * lq.sum())
    inse = ((p * oh).sum(0), (dp * oh).sum(0) + Ld * (p * oh).sum(0))
    ls = (p.sum(0), dp.sum(0) + Ld * p.sum(0))
    return bce, inse, ls, oh.sum(0).astype(F64)


def _hv_diff64(l_hv, t_hv):
    return f64(l_hv[:, 0]) - f64(t_hv[..., 0]), f64(l_hv[:, 1]) - f64(t_hv[..., 1])


def loss_forward_ref(l_np, l_hv, l_tp, t_np, t_hv, t_tp):
    """l_np, l_hv [n][2][h][w], l_tp [n][T][h][w] | None fp32; t_np, t_tp [n][h][w] int; t_hv [n][h][w][2] fp32
    -> (sums ref [64], B [64]), (sobel_ws ref [n][h][w][2], B).  The counts ([4], [12 + c], [48 + c]) are exact: B = 0.
    mse: fl(l - t) squared and the two added: 4 u (+ 1).  Sobel: coefficient fl(h / (h^2 + v^2)) (the 1e-15 vanishes in fp32, and
    against the float64 coefficient) 2 u, fl(l - t) 1 u, a fused chain of 25: K = 28 over S_g = sum |k| |l - t|; msge numerator
    f (g0^2 + g1^2): 2 |g| B_g + B_g^2 + 3 u g^2 per channel."""
    n, _, h, w = l_np.shape
    P = n * h * w
    sums, B = np.zeros(64), np.zeros(64)
    fg = (np.asarray(t_np) != 0)
    pm = lambda l: np.ascontiguousarray(np.moveaxis(l, 1, -1)).reshape(P, l.shape[1])
    bce, inse, ls, cnt = _branch_forward(pm(l_np), fg.reshape(P).astype(np.int64))
    sums[0], B[0] = bce
    sums[8:10], B[8:10] = inse
    sums[10:12], B[10:12] = ls
    sums[12:14] = cnt
    if l_tp is not None:
        T = l_tp.shape[1]
        bce, inse, ls, cnt = _branch_forward(pm(l_tp), np.asarray(t_tp).reshape(P).astype(np.int64))
        sums[1], B[1] = bce
        sums[16:16 + T], B[16:16 + T] = inse
        sums[32:32 + T], B[32:32 + T] = ls
        sums[48:48 + T] = cnt
    Ld = loss_chain(P) * UD
    d0, d1 = _hv_diff64(l_hv, t_hv)
    sq = d0 * d0 + d1 * d1
    sums[2], B[2] = sq.sum(), (5 * U + Ld) * sq.sum()
    k = sobel5(F64)
    g = np.stack([_corr5(d0, k), _corr5(d1, k.T)], -1)
    Sg = np.stack([_corr5(np.abs(d0), np.abs(k)), _corr5(np.abs(d1), np.abs(k.T))], -1)
    Bg = 28 * U * Sg
    f = fg.astype(F64)[..., None]
    sums[3] = (f * g * g).sum()
    B[3] = (f * (2 * np.abs(g) * Bg + Bg * Bg + 3 * U * g * g)).sum() + Ld * sums[3]
    sums[4] = 2.0 * fg.sum()
    return (sums, B), (f * g, f * Bg)


def _dice_D(sums, base_i, base_l, base_r, T):
    I, den = sums[base_i:base_i + T], sums[base_l:base_l + T] + sums[base_r:base_r + T] + SMOOTH
    return I, den


def _branch_backward(l, t, I, den, w_bce, w_dice, M, gate_on=True):
    """-> (ref [P][T], B): w_bce gate (p - onehot) / M + w_dice p_c (D_c - sum_j D_j p_j), D_c = -(2 [c == t] den_c - (2 I_c + smooth)) /
    den_c^2, in double from the fp32 softmax, stored as fp32.  Errors: dp through both parts (the dice part by its partial derivatives:
    d/dp_c = D_c - dot - p_c D_c, d/dp_j = -p_c D_j), 16 2^-53 of the double terms, u of the stored value; where q is within its own
    error of a clamp bound the gate may fall either way and the bce part's whole magnitude is allowed."""
    P, T = l.shape
    p, dp, ep = _softmax64(l)
    oh = (np.arange(T)[None, :] == t[:, None]).astype(F64)
    q = p[np.arange(P), t] / p.sum(-1)
    eq = (ep[np.arange(P), t] + ep.max(-1) + T * U) * q + TINY
    gate = ((q > LO) & (q < HI)).astype(F64)
    amb = (np.abs(q - LO) <= eq) | (np.abs(q - HI) <= eq)
    if not gate_on:
        gate, amb = np.ones(P), np.zeros(P, bool)
    D = -(2.0 * oh * den - (2.0 * I + SMOOTH)) / (den * den)
    dot = (D * p).sum(-1, keepdims=True)
    bce = w_bce * gate[:, None] * (p - oh) / M
    dice = w_dice * p * (D - dot)
    ref = bce + dice
    own = np.abs(D - dot - p * D) * dp
    cross = p * ((np.abs(D) * dp).sum(-1, keepdims=True) - np.abs(D) * dp)
    mag = w_bce * np.abs(p - oh) / M + w_dice * p * (np.abs(D) + (np.abs(D) * p).sum(-1, keepdims=True))
    B = w_bce * gate[:, None] * dp / M + w_dice * (own + cross) + 16 * UD * mag + U * np.abs(ref) + TINY
    B = B + amb[:, None] * w_bce * (np.abs(p - oh) + dp) / M
    return ref, B


def loss_backward_ref(l_np, l_hv, l_tp, t_np, t_hv, t_tp, sums, gws, wt, M):
    """The logit gradients from the sums and the sobel_ws the kernel itself left (sums: float64 [64], possibly all-reduced), wt [6] fp32,
    M = total_pixels -> dict(np, hv[, tp]) of (ref NCHW, B).
    hv: fl(fl(wt2 fl(d / fl(M))) + fl(wt3 fl(kf a))), kf = fl(2 / (sums[4] + 1e-8)): the mse term 4 u (+ 1), the msge term the Sobel
    chain's 28 u over S_a = sum |k| |gws| and 3 u more (+ 1), the sum 1 u of both."""
    n, _, h, w = l_np.shape
    P = n * h * w
    wt = [float(F32(x)) for x in wt]
    pm = lambda l: np.ascontiguousarray(np.moveaxis(l, 1, -1)).reshape(P, l.shape[1])
    back = lambda a: np.ascontiguousarray(np.moveaxis(a.reshape(n, h, w, -1), -1, 1))
    sums = f64(sums)
    out = {}
    I, den = _dice_D(sums, 8, 10, 12, 2)
    r, B = _branch_backward(pm(l_np), (np.asarray(t_np) != 0).reshape(P).astype(np.int64), I, den, wt[0], wt[1], float(M))
    out["np"] = (back(r), back(B))
    if l_tp is not None:
        T = l_tp.shape[1]
        I, den = _dice_D(sums, 16, 32, 48, T)
        r, B = _branch_backward(pm(l_tp), np.asarray(t_tp).reshape(P).astype(np.int64), I, den, wt[4], wt[5], float(M))
        out["tp"] = (back(r), back(B))
    d = np.stack(_hv_diff64(l_hv, t_hv), 1)                                   # [n][2][h][w]
    k = sobel5(F64)
    gw = f64(gws)
    flip = lambda kk: kk[::-1, ::-1]                                            # a[y][x] = sum k[r][s] gws[y - r + 2][x - s + 2]
    a = np.stack([_corr5(gw[..., 0], flip(k)), _corr5(gw[..., 1], flip(k.T))], 1)
    Sa = np.stack([_corr5(np.abs(gw[..., 0]), np.abs(flip(k))), _corr5(np.abs(gw[..., 1]), np.abs(flip(k.T)))], 1)
    kf = 2.0 / (sums[4] + 1.0e-8)
    t1, t2 = wt[2] * d / float(M), wt[3] * kf * a
    out["hv"] = (t1 + t2, U * (6 * np.abs(t1) + 2 * np.abs(t2) + wt[3] * kf * 32 * Sa) + TINY)
    return out


LOSS_MUTANTS = ("sobel_clamped", "no_transpose", "no_gate", "dice_fp32", "local_M")


def loss_mirror(l_np, l_hv, l_tp, t_np, t_hv, t_tp, wt, M, mutant=None, sums_in=None):
    """Both stages in fp32 / double as the kernels form them -> dict(sums, gws, np, hv[, tp]).  sums_in: the sums stage 2 reads (default:
    stage 1's own)."""
    assert mutant is None or mutant in LOSS_MUTANTS
    n, _, h, w = l_np.shape
    P = n * h * w
    if mutant == "local_M":
        M = float(P)
    pm = lambda l: np.ascontiguousarray(np.moveaxis(f32(l), 1, -1)).reshape(P, l.shape[1])
    back = lambda a: np.ascontiguousarray(np.moveaxis(a.reshape(n, h, w, -1), -1, 1))
    sums = np.zeros(64)
    fg = np.asarray(t_np) != 0
    branches = [("np", pm(l_np), fg.reshape(P).astype(np.int64), 0, (8, 10, 12), (0, 1))]
    if l_tp is not None:
        branches.append(("tp", pm(l_tp), np.asarray(t_tp).reshape(P).astype(np.int64), 1, (16, 32, 48), (4, 5)))
    soft = {}
    for name, l, t, slot, (bi, bl, br), _ in branches:
        T = l.shape[1]
        p = _softmax32(l)
        q = p[np.arange(P), t] / _psum32(p)
        soft[name] = (p, q, t)
        oh = np.arange(T)[None, :] == t[:, None]
        sums[slot] = f64(-_log32(np.minimum(np.maximum(q, EPS32), F32(1.0) - EPS32))).sum()
        sums[bi:bi + T] = (f64(p) * oh).sum(0)
        sums[bl:bl + T] = f64(p).sum(0)
        sums[br:br + T] = oh.sum(0)
    l_hv, t_hv = f32(l_hv), f32(t_hv)
    d0, d1 = l_hv[:, 0] - t_hv[..., 0], l_hv[:, 1] - t_hv[..., 1]
    sums[2] = f64(d0 * d0 + d1 * d1).sum()
    k = sobel5(F32)
    mode = "edge" if mutant == "sobel_clamped" else "zero"
    k1 = k if mutant == "no_transpose" else k.T
    g0, g1 = _corr5(d0, k, mode), _corr5(d1, k1, mode)
    f = fg.astype(F32)
    sums[3] = f64(f * (g0 * g0 + g1 * g1)).sum()
    sums[4] = f64(F32(2) * f).sum()
    gws = np.stack([f * g0, f * g1], -1)
    out = dict(sums=sums.copy(), gws=gws)
    s2 = sums if sums_in is None else f64(sums_in)
    wt = f32(wt)
    for name, l, t, slot, (bi, bl, br), (wb, wd) in branches:
        T = l.shape[1]
        p, q, t = soft[name]
        gate = ((q > EPS32) & (q < F32(1.0) - EPS32)).astype(F64)
        if mutant == "no_gate":
            gate = np.ones(P)
        oh = (np.arange(T)[None, :] == t[:, None]).astype(F64)
        I, den = s2[bi:bi + T], s2[bl:bl + T] + s2[br:br + T] + SMOOTH
        D = -(2.0 * oh * den - (2.0 * I + SMOOTH)) / (den * den)
        if mutant == "dice_fp32":
            D32 = f32(D)
            dot = np.zeros(P, F32)
            for c in range(T):
                dot = dot + D32[:, c] * p[:, c]
            comb = f64(D32 - dot[:, None])
        else:
            comb = D - (D * f64(p)).sum(-1, keepdims=True)
        out[name] = back(f32(f64(wt[wb]) * (gate[:, None] * (f64(p) - oh) / M) + f64(wt[wd]) * (f64(p) * comb)))
    flip = lambda kk: np.ascontiguousarray(kk[::-1, ::-1])
    a0, a1 = _corr5(np.ascontiguousarray(gws[..., 0]), flip(k)), _corr5(np.ascontiguousarray(gws[..., 1]), flip(k1))
    kf = F32(2.0 / (s2[4] + 1.0e-8))
    Mf = F32(M)
    out["hv"] = np.stack([wt[2] * (d0 / Mf) + wt[3] * (kf * a0), wt[2] * (d1 / Mf) + wt[3] * (kf * a1)], 1)
    return out


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, b1, b2, step):
    """hvn_adam_step's host part: the bias corrections in double from the float32 betas -> (step_size, 1 / sqrt(bc2)) as doubles."""
    lr, b1, b2 = float(F32(lr)), float(F32(b1)), float(F32(b2))
    return lr / (1.0 - b1 ** step), 1.0 / np.sqrt(1.0 - b2 ** step)


def adam_ref(w0, g, m0, v0, lr, b1, b2, eps, step):
    """ONE step from the m, v, w given (what the kernel itself left after the step before) -> dict(m, v, w) of (ref, B).
    m = fl(fl(b1 m0) + fl(fl(1 - b1) g)): K = 3 + 1 over |b1 m0| + |(1 - b1) g|;  v = fl(fl(b2 v0) + fl(fl(fl(1 - b2) g) g)): K = 4 + 1.
    w = fl(w0 - fl(fl(ss m) / fl(fl(sqrtf(v) inv) + eps))), ss and inv the rounded scalars: the denominator carries v's error halved
    (2.5 u: the terms of v are non-negative), sqrtf 2 u, inv, the product and the sum 3 u; the quotient ss's, the product's and the
    division's 3 u, and m's ABSOLUTE error B_m (m may cancel) times ss / den; the final subtraction u of |w0| + |update|:
    B_w = u (|w0| + |upd|) + 12 u |upd| + (ss / den) B_m, + TINY for the flush of a denormal."""
    b1f, b2f, epsf = float(F32(b1)), float(F32(b2)), float(F32(eps))
    ss, inv = adam_scalars(lr, b1, b2, step)
    w0, g, m0, v0 = f64(w0), f64(g), f64(m0), f64(v0)
    m = b1f * m0 + (1.0 - b1f) * g
    Bm = 4 * U * (np.abs(b1f * m0) + np.abs((1.0 - b1f) * g)) + TINY
    v = b2f * v0 + (1.0 - b2f) * g * g
    Bv = 5 * U * v + TINY
    den = np.sqrt(v) * inv + epsf
    upd = ss * m / den
    Bw = U * (np.abs(w0) + np.abs(upd)) + 12 * U * np.abs(upd) + ss / den * Bm + TINY
    return dict(m=(m, Bm), v=(v, Bv), w=(w0 - upd, Bw))


ADAM_MUTANTS = ("eps_in_sqrt", "no_bc1", "bc_fp32")
_POW32 = {}


def pow32_running(b, step):
    """beta^step as an fp32 running product (`beta_pow *= beta` once per step: one rounding per step), the state an optimizer that forms
    its bias corrections in fp32 carries."""
    key = (float(F32(b)), int(step))
    if key not in _POW32:
        p, bf = F32(1.0), F32(b)
        for _ in range(int(step)):
            p = F32(p * bf)
        _POW32[key] = p
    return _POW32[key]


def adam_mirror(w0, g, m0, v0, lr, b1, b2, eps, step, mutant=None):
    """Mutants: eps inside the square root; no first-moment bias correction; bc_fp32: the bias corrections formed in fp32 (beta^step an
    fp32 running product, 1 - beta^step, lr / bc1 and 1 / sqrt(bc2) in fp32)."""
    assert mutant is None or mutant in ADAM_MUTANTS
    w0, g, m0, v0 = f32(w0), f32(g), f32(m0), f32(v0)
    b1f, b2f, epsf, one = F32(b1), F32(b2), F32(eps), F32(1.0)
    ss, inv = adam_scalars(lr, b1, b2, step)
    if mutant == "bc_fp32":
        bc1, bc2 = one - pow32_running(b1f, step), one - pow32_running(b2f, step)
        ss, inv = F32(lr) / bc1, one / np.sqrt(bc2)
    if mutant == "no_bc1":
        ss = F32(lr)
    ss, inv = F32(ss), F32(inv)
    m = b1f * m0 + (one - b1f) * g
    v = b2f * v0 + (one - b2f) * g * g
    den = np.sqrt(v + epsf) * inv if mutant == "eps_in_sqrt" else np.sqrt(v) * inv + epsf
    return dict(m=m, v=v, w=w0 - ss * m / den)

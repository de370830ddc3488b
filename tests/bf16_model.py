"""The float64 reference, the numpy model and the two criteria the bf16 convolution kernels (csrc/hvn_conv_bf16.hip, hvn_conv_bf16g.hip)
are held to -- TEST INFRASTRUCTURE ONLY.  numpy only; this file imports nothing of the package (tests/x3_model.py, whose generators it
reuses, imports one helper of the engine for its own model).  tests/test_bf16_arithmetic.py proves on the CPU what the criteria see,
tests/test_gpu_bf16_rounding.py holds the kernels to them on the same cases.

THE CONTRACT (the kernel's header and code).  Operands are bf16, so every product is exact in fp32.  Accumulation in fp32; the epilogue
in fp32, in this order: v = max(acc + bias, relu_lo), v += residual (read as bf16), v = max(fma(v, post_s, post_b), post_lo); ONE
round-to-nearest-even conversion on the store.  The prologue is RNE_bf16(max(fma(x, pre_s, pre_b), 0)) on the A operand.

INPUTS of a case: activations, weights ([cout, cin_g, k, k], the checkpoint's layout) and residual are values exact in bf16; bias, pre
and post are fp32.  The weights go into the plan with bn=None, bias=...: the plan's fold and the engine's repack then preserve every
value, and the reference never touches a packing under test.  pre_s / pre_b lie on a coarse binary grid, so that x * s + b is exact in
float64 (asserted) and its fp32 rounding followed by the bf16 one gives what one rounding of the exact value gives (asserted).

ref64, S: the float64 result of the contract from those very values, and S = sum |a w| + |bias| + |res|, carried through the
block-closing BN as |post_s| S + |post_b| (as tests/net_ops_ref.py does); ReLU moves no bound.

CRITERION H (hard; per element, every element):  rne64(ref64 - B) <= got <= rne64(ref64 + B),  B = net_ops_ref.bound(S, L) =
(2 L + 4) 2^-24 S, L = the number of terms of the reduction (taps x channels of both K sources; of a grouped convolution run as a
block-diagonal dense GEMM the terms inside the block -- the others are exact zeros, and adding an exact zero rounds nothing).
net_ops_ref has the argument why B covers ANY summation order; rounding is monotone, so the rounded value of anything inside
[ref64 - B, ref64 + B] lies between the rounded ends.  Where the two ends coincide this is bit equality.

CRITERION R (rounding; per case):  #{got != rne64(ref64)} <= 2 m_model + 8,  m_model = the same count for `model()`: sequential fp32
accumulation in index order, the fp32 epilogue in the documented order, one RNE.  The factor 2 is the one tests/test_gpu_x3_budget.py
gives the same matrix pipe over the same kind of model (profiles/x3_error_budget.txt: the bf16 pipe sits at 0.34 - 0.41 of that doubled
bound); the 8 keeps a model count of 0 from demanding perfection.  Nothing in the bound depends on code under test.

CONDITIONS on the inputs (`conditions`; checked on the CPU for every case; x3_model.SEED meets them on all): >= 40 % of the outputs
are live -- no ReLU clips them and |ref64| > B -- and m_model <= 0.5 % of the outputs."""
import numpy as np

from net_ops_ref import bf16_bits, bf16_widen, bound
from x3_model import GENERATORS, SEED, exponent_sweep  # noqa: F401  (exponent_sweep: for the GPU test)

R_FACTOR, R_SLACK = 2, 8
MIN_LIVE, MAX_MODEL = 0.40, 0.005
MUTANT_FACTOR = 10                # a mutant of the model must miss R's allowance this many times over


def to_bf16(x):
    """float array -> float32 values exact in bf16 (RNE)."""
    return bf16_widen(bf16_bits(np.asarray(x, np.float32)))


def rne64(v):
    """float64 -> the nearest bf16 VALUE (as float64), ties to even, straight from float64 -- not through fp32.
    ulp = 2^(floor(log2 |v|) - 7), never below bf16's denormal spacing 2^-133; 0 -> 0."""
    v = np.asarray(v, np.float64)
    assert np.isfinite(v).all()
    _, e = np.frexp(v)                                   # |v| = m 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1
    ulp = np.ldexp(1.0, np.maximum(e - 8, -133))
    return np.rint(v / ulp) * ulp                        # v / ulp: exact (a power of two), |.| in [128, 256): rint's ties go to the even significand


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# n = 2, 13 x 13 unless noted: 338 rows, so the last 128-row tile is ragged.  `tiles`: the launch forms (tile_n codes) the GPU test
# runs; 896 / 640 = the LDS-DMA forms of hvn_conv_bf16g.hip, which exist for >= 128 output channels and no prologue.
CASES = {
    # K = one 64-channel chunk: the narrow loop (WIDE = false)
    "1x1_64_128_bare": dict(cin=64, cout=128, tiles=(128, 64, 32, 896, 640), gens=("random", "cancelling")),
    # the wide loop.  (Weights are padded to the plan's column tile, 64 rows here: a 128-wide tile would read past the packing -- a form
    # the engine never binds to a 64-channel output -- so this case has no tile 128; the 288 -> 128 and 2048 -> 256 cases run it.)
    "1x1_128_64_bare": dict(cin=128, cout=64, tiles=(64, 32), gens=("random", "cancelling")),
    # 288 channels = 4.5 k-steps (the zero half-step), a channel window of a 320-channel buffer whose other 32 channels are NaN, the
    # spatial window inset by 1 and 2 pixels; prologue + bias + ReLU; the output a 128-channel window of a 160-channel buffer
    "1x1_288_128_windows_pre": dict(cin=288, cout=128, xbuf=(16, 16, 320), xorg=(1, 2, 0), ybuf=(13, 13, 160), yc0=32, pre=True, bias=True,
                                    relu=1, tiles=(128, 64)),
    # the same windows without the prologue: the only way the LDS-DMA form (no prologue) meets the zero half-step
    "1x1_288_128_windows": dict(cin=288, cout=128, xbuf=(16, 16, 320), xorg=(1, 2, 0), ybuf=(13, 13, 160), yc0=32, bias=True, relu=1, tiles=(896,)),
    "1x1_2048_256": dict(cin=2048, cout=256, bias=True, relu=1, tiles=(128, 896)),                       # the deepest reduction
    "3x3_same_64_64": dict(cin=64, cout=64, k=3, pad=(1, 1), bias=True, relu=1, tiles=(64,)),
    "3x3_same_stride2_64_64": dict(cin=64, cout=64, k=3, stride=2, pad=(0, 1), hw=(14, 14), bias=True, relu=1, tiles=(64,)),
    "g5x5_128_32": dict(cin=128, cout=32, k=5, groups=4, hw=(12, 12), ybuf=(8, 8, 96), yc0=64, tiles=(32,)),
    "shortcut_64+64_128_post": dict(cin=64, cout=128, cin2=64, stride2=2, post=True, tiles=(128, 64)),   # the unread pixels of x2 are NaN
    # the three epilogue switches, each seen on and off (bare: all off; the shortcut: post alone)
    "res_post_64_256": dict(cin=64, cout=256, bias=True, relu=1, res=True, post=True, tiles=(128, 896)),
    "res_inplace_64_128": dict(cin=64, cout=128, bias=True, relu=1, res=True, inplace=True, tiles=(128, 640)),
    "res_only_64_128": dict(cin=64, cout=128, res=True, tiles=(128, 64)),
}


def case_ids():
    return [(name, gen) for name in CASES for gen in CASES[name].get("gens", ("random",))]


_BUILT = {}


def build(name, gen):
    """-> the case as explicit arrays (made once per process, never changed): what tests/gpu_util.run_conv_bits takes (`spec`), and the
    operands of its dot products."""
    if (name, gen) in _BUILT:
        return _BUILT[(name, gen)]
    c = CASES[name]
    n, (h, w) = 2, c.get("hw", (13, 13))
    cin, cout, k, stride, pad, groups = c["cin"], c["cout"], c.get("k", 1), c.get("stride", 1), c.get("pad", (0, 0)), c.get("groups", 1)
    cin2, cin_g = c.get("cin2", 0), c["cin"] // c.get("groups", 1)
    ho, wo = (h + pad[0] + pad[1] - k) // stride + 1, (w + pad[0] + pad[1] - k) // stride + 1
    a, wm = GENERATORS[gen](SEED, n * h * w if cin2 == 0 else n * ho * wo, cout, cin_g * k * k + cin2)
    rng = np.random.default_rng(1000 + SEED)
    x = to_bf16(a[:, :cin].reshape(n, h, w, cin))
    wt = to_bf16(wm[:, :cin_g * k * k].reshape(cout, cin_g, k, k))
    spec = dict(n=n, x=x, wt=wt, stride=stride, pad=pad, groups=groups, relu=c.get("relu", 0))
    xb = c.get("xbuf", (h, w, cin))
    y0, x0, c0 = c.get("xorg", (0, 0, 0))
    spec["xbuf"], spec["xview"] = xb, (y0, x0, h, w, c0, cin)
    yb = c.get("ybuf", (ho, wo, cout))
    spec["ybuf"], spec["yview"] = yb, (0, 0, ho, wo, c.get("yc0", 0), cout)
    if cin2:
        s2 = c["stride2"]
        x2 = np.full((n, s2 * ho, s2 * wo, cin2), np.nan, np.float32)
        x2[:, ::s2, ::s2] = to_bf16(a[:, cin:].reshape(n, ho, wo, cin2))
        spec.update(x2=x2, wt2=to_bf16(wm[:, cin:].reshape(cout, cin2, 1, 1)), stride2=s2)
    if c.get("bias"):
        spec["bias"] = rng.normal(0.5, 0.25, cout).astype(np.float32)
    if c.get("pre"):          # the coarse binary grid: s in {1/2 .. 3/2} by quarters, b in [-1/2, 1/2] by eighths
        spec["pre"] = ((rng.integers(2, 7, cin) / 4.0).astype(np.float32), (rng.integers(-4, 5, cin) / 8.0).astype(np.float32))
    if c.get("res"):
        spec["res"] = to_bf16(rng.normal(0, 1, (n, ho, wo, cout)))
        spec["inplace_res"] = bool(c.get("inplace"))
    if c.get("post"):
        spec["post"] = (rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0.2, 0.3, cout).astype(np.float32))
    out = dict(name=name, gen=gen, spec=spec, tiles=c["tiles"], L=k * k * cin_g + cin2, shape=(n, ho, wo, cout))
    out["A"], out["W"] = operands(spec)
    _BUILT[(name, gen)] = out
    return out


def _two_sum_exact(p, b):
    """True where the float64 sum p + b carries no rounding (Knuth's TwoSum: the error term is zero)."""
    t = p + b
    bb = t - p
    return ((p - (t - bb)) + (b - bb)) == 0


def prologue(x, pre):
    """The A operand of a launch with a prologue: RNE_bf16(max(x s + b, 0)), from the exact value; float32 out."""
    s, b = (np.asarray(v, np.float64) for v in pre)
    p = x.astype(np.float64) * s                                         # 8 x 3 significand bits: exact
    assert _two_sum_exact(p, np.broadcast_to(b, p.shape)).all(), "x s + b is not exact in float64: the grid of the prologue is too fine"
    t = np.maximum(p + b, 0.0)
    a = rne64(t).astype(np.float32)
    assert np.array_equal(a, to_bf16(t.astype(np.float32))), "fp32 rounding of x s + b, then bf16: not what one rounding of the exact value gives"
    return a


def operands(spec):
    """-> (A [M, K], W [cout, K]) float32, bf16-exact: the operands of the case's dot products as the contract states them -- the
    prologue applied and rounded, zeros for the padding, a grouped convolution block-diagonal; k = (tap, channel) of x, then x2's."""
    x, wt, stride, pad, groups = spec["x"], spec["wt"], spec["stride"], spec["pad"], spec["groups"]
    n, h, w, cin = x.shape
    cout, cin_g, k, _ = wt.shape
    assert cin == cin_g * groups and (to_bf16(x) == x).all() and (to_bf16(wt) == wt).all()
    if spec.get("pre") is not None:
        x = prologue(x, spec["pre"])
    ho, wo = (h + pad[0] + pad[1] - k) // stride + 1, (w + pad[0] + pad[1] - k) // stride + 1
    xp = np.zeros((n, h + pad[0] + pad[1], w + pad[0] + pad[1], cin), np.float32)
    xp[:, pad[0]:pad[0] + h, pad[0]:pad[0] + w] = x
    cols = [xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride].reshape(n * ho * wo, cin) for ky in range(k) for kx in range(k)]
    dense = np.zeros((cout, k * k, cin), np.float32)
    og = cout // groups
    for g in range(groups):
        dense[g * og:(g + 1) * og, :, g * cin_g:(g + 1) * cin_g] = wt[g * og:(g + 1) * og].transpose(0, 2, 3, 1).reshape(og, k * k, cin_g)
    A, W = np.concatenate(cols, 1), dense.reshape(cout, k * k * cin)
    if spec.get("x2") is not None:
        s2 = spec["stride2"]
        a2 = spec["x2"][:, ::s2, ::s2][:, :ho, :wo]
        assert k == 1 and np.isfinite(a2).all() and (to_bf16(a2) == a2).all() and (to_bf16(spec["wt2"]) == spec["wt2"]).all()
        A = np.concatenate([A, a2.reshape(n * ho * wo, -1)], 1)
        W = np.concatenate([W, spec["wt2"].reshape(cout, -1)], 1)
    return np.ascontiguousarray(A), np.ascontiguousarray(W)


def _epilogue(acc, spec, dt, order="contract"):
    """acc [M, cout] -> the value the store rounds, in float64 (the reference) or float32 (the model: one rounding per operation, the
    fma's single rounding taken from its exact float64 value).  order: "contract" | "res_before_relu" | "post_before_res" (mutants)."""
    v = acc.astype(dt)
    bias, res, post, relu = spec.get("bias"), spec.get("res"), spec.get("post"), spec.get("relu", 0)
    r = None if res is None else res.reshape(v.shape).astype(dt)
    clipped = np.zeros(v.shape, bool)

    def bias_relu(v, extra=None):
        if bias is not None:
            v = v + bias.astype(dt)
        if extra is not None:
            v = v + extra
        if relu:
            clipped[...] |= v <= 0
            v = np.maximum(v, dt(0))
        return v

    def block_bn(v):
        t = v.astype(np.float64) * post[0].astype(np.float64) + post[1].astype(np.float64)      # 24 x 24 bits: the product is exact
        clipped[...] |= t <= 0
        return np.maximum(t, 0.0).astype(dt)

    if order == "res_before_relu":
        assert r is not None and relu
        v = bias_relu(v, r)
        r = None
    else:
        v = bias_relu(v)
    if order == "post_before_res":
        assert r is not None and post is not None
        return block_bn(v) + r, clipped
    if r is not None:
        v = v + r
    if post is not None:
        v = block_bn(v)
    return v, clipped


_REFS = {}


def reference(case):
    """-> dict(ref [n, ho, wo, cout] float64, S, B, want = rne64(ref), lo, hi = the ends of criterion H, live), made once per case."""
    key = (case["name"], case["gen"])
    if key not in _REFS:
        spec, A, W = case["spec"], case["A"].astype(np.float64), case["W"].astype(np.float64)
        S = np.abs(A) @ np.abs(W).T
        if spec.get("bias") is not None:
            S = S + np.abs(spec["bias"].astype(np.float64))
        if spec.get("res") is not None:
            S = S + np.abs(spec["res"].reshape(S.shape).astype(np.float64))
        if spec.get("post") is not None:
            S = np.abs(spec["post"][0].astype(np.float64)) * S + np.abs(spec["post"][1].astype(np.float64))
        ref, clipped = _epilogue(A @ W.T, spec, np.float64)
        B = bound(S, case["L"])
        sh = case["shape"]
        _REFS[key] = dict(ref=ref.reshape(sh), S=S.reshape(sh), B=B.reshape(sh), want=rne64(ref).reshape(sh), lo=rne64(ref - B).reshape(sh),
                          hi=rne64(ref + B).reshape(sh), live=(~clipped & (np.abs(ref) > B)).reshape(sh))
    return _REFS[key]


# ---- the model and its mutants ----------------------------------------------------------------------------------------------------------
MUTANTS = ("truncating_store", "acc_bf16_before_epilogue", "acc_bf16_per_64_step", "res_before_relu", "post_before_res")


def applies(mutant, case):
    """Whether the mutant is a different function on this case at all (rounding the accumulator before an epilogue that does nothing,
    or once per 64-channel step of a reduction of one step, IS the contract's single rounding)."""
    s = case["spec"]
    return {"truncating_store": True,
            "acc_bf16_before_epilogue": any(s.get(f) is not None for f in ("bias", "res", "post")),
            "acc_bf16_per_64_step": case["A"].shape[1] > 64,
            "res_before_relu": s.get("res") is not None and bool(s.get("relu")),
            "post_before_res": s.get("res") is not None and s.get("post") is not None}[mutant]


def accumulate(A, W, step_round=0, kmax=None):
    """Sequential fp32 accumulation over k in index order (every product exact; one rounding per addition).  step_round = 64: the
    accumulator rounded to bf16 after every 64 terms (a mutant); kmax: the reduction cut short (a lost trailing slab)."""
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    K = A.shape[1] if kmax is None else kmax
    for k in range(K):
        acc = acc + A[:, k:k + 1] * W[None, :, k]
        if step_round and (k + 1) % step_round == 0:
            acc = to_bf16(acc)
    return acc


def model(case, mutant=None, kmax=None):
    """-> uint16 bits [n, ho, wo, cout] of the numpy model (mutant=None: the contract) of the case."""
    spec = case["spec"]
    acc = accumulate(case["A"], case["W"], step_round=64 if mutant == "acc_bf16_per_64_step" else 0, kmax=kmax)
    if mutant == "acc_bf16_before_epilogue":
        acc = to_bf16(acc)
    v, _ = _epilogue(acc, spec, np.float32, order=mutant if mutant in ("res_before_relu", "post_before_res") else "contract")
    v = np.ascontiguousarray(v, np.float32)
    bits = (v.view(np.uint32) >> 16).astype(np.uint16) if mutant == "truncating_store" else bf16_bits(v)
    return bits.reshape(case["shape"])


_M_MODEL = {}


def m_model(case):
    key = (case["name"], case["gen"])
    if key not in _M_MODEL:
        _M_MODEL[key] = mismatches(model(case), reference(case))
    return _M_MODEL[key]


def allowance(case):
    return R_FACTOR * m_model(case) + R_SLACK


# ---- the criteria -----------------------------------------------------------------------------------------------------------------------
def mismatches(bits, r):
    """Criterion R's count: elements that are not the correctly rounded float64 result (-0 counts as 0)."""
    return int((bf16_widen(bits).astype(np.float64) != r["want"]).sum())


def outside_H(bits, r):
    """Criterion H: the number of elements that are not finite or not within [rne64(ref - B), rne64(ref + B)]."""
    got = bf16_widen(bits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return int((~(np.isfinite(got) & (r["lo"] <= got) & (got <= r["hi"]))).sum())


def worst_ratio(bits, r):
    """max |got - ref64| / B over all elements (what the store's rounding adds included: it may exceed 1 where H holds)."""
    got = bf16_widen(bits).astype(np.float64)
    return float(np.max(np.where(np.isfinite(got), np.abs(got - r["ref"]) / r["B"], np.inf)))


def conditions(case):
    """-> (live fraction, m_model fraction); asserts the conditions on the inputs."""
    r = reference(case)
    live, frac = float(r["live"].mean()), m_model(case) / r["ref"].size
    assert live >= MIN_LIVE, (case["name"], case["gen"], "only %.1f %% of the outputs are live" % (100 * live))
    assert frac <= MAX_MODEL, (case["name"], case["gen"], "the model itself misses %.2f %% of the outputs" % (100 * frac))
    return live, frac

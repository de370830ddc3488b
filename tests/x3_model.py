"""The numpy restatement of the bf16x3 arithmetic (csrc/hvn_conv_x3.hip), the data classes and the error budget that
tests/test_x3_arithmetic.py (CPU: the model, and what a lost partial product does to it) and tests/test_gpu_x3_budget.py (GPU: the kernels)
share -- same generators, same seeds, same bound recipe, so that what the CPU test proves about the model is what the GPU test asks of
the kernels.

A case is an activation matrix a [M, K] and a weight matrix w [N, K], both fp32; its M x N outputs are the dot products over K.  The
error of a result is taken against float64 and relative to S = sum_k |a_k w_k| (the scale every rounding of the accumulation is
proportional to).  The BOUND comes from a plain sequential fp32 accumulation of the unsplit operands (`_dot_fp32`) on a fixed subset of
the same outputs, times the factor 2 test_x3_arithmetic.py states for the split forms: it depends on no code under test."""
import numpy as np

from hover_net_amd.engine import split_bf16x3

SECOND_ORDER = ((1, 1), (0, 2), (2, 0))       # the partial products of ~2^-16 of a product: m*m, h*l, l*h (plane of a, plane of b)
FACTOR = 2.0                                  # split forms vs plain fp32 accumulation (test_six_terms_sit_where_fp32_accumulation_sits)
MAX_REL = 64 * 2.0 ** -24                     # and never more than a few roundings' worth of the products' magnitude
DETECT = 4.0                                  # a lost second-order term must sit this far above the bound for a case to be pinned
SUBSET = 4096                                 # outputs the bound (and the numpy models) are formed on


def _f(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _planes(x):
    return [_f(p) for p in split_bf16x3(x)]


def _dot_terms(a, b, terms, drop=()):
    """fp32 accumulation (sequential over k, like an MFMA accumulator chain) of the partial products of a[k] * b[k].
    drop: (plane of a, plane of b) pairs left out -- the model of a kernel that loses a partial product."""
    pa, pb = _planes(a), _planes(b)
    pairs = [(i, j) for s in range(4, -1, -1) for i in range(2, -1, -1) for j in [s - i] if 0 <= j <= 2 and (terms == 9 or i + j <= 2)]
    assert all(d in pairs for d in drop), (terms, drop)
    pairs = [p for p in pairs if p not in drop]
    acc = np.zeros(a.shape[:-1], np.float32)
    for k0 in range(0, a.shape[-1], 16):                        # one 32x32x16 MFMA block after the other; inside: the kernel's pair order
        for i, j in pairs:
            acc = acc + np.sum((pa[i][..., k0:k0 + 16] * pb[j][..., k0:k0 + 16]).astype(np.float64), -1).astype(np.float32)
    return acc


def _dot_fp32(a, b):
    acc = np.zeros(a.shape[:-1], np.float32)
    for k in range(a.shape[-1]):
        acc = acc + a[..., k] * b[..., k]
    return acc


# ---- data classes: (a [m, k], w [n, k]) fp32 ------------------------------------------------------------------------------------------
def gen_random(seed, m, n, k):
    """N(0, 1) activations, He-scaled weights: O(1) outputs, what the GPU parity tests feed the kernels."""
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (m, k)).astype(np.float32), rng.normal(0, np.sqrt(2.0 / k), (n, k)).astype(np.float32)


def gen_cancelling(seed, m, n, k):
    """Positive activations against weights of alternating sign along k (test_x3_arithmetic.py's cancellation-heavy class): the partial
    sums swing far above the result."""
    rng = np.random.default_rng(seed)
    a = np.abs(rng.normal(0, 10, (m, k)))
    w = rng.normal(0, np.sqrt(2.0 / k), (n, k)) * np.where(np.arange(k) % 2, 1, -1)
    return a.astype(np.float32), w.astype(np.float32)


GENERATORS = {"random": gen_random, "cancelling": gen_cancelling}
SEED = 20
# (m, n, k) of the dot products the GPU cases of tests/test_gpu_x3_budget.py form (n = 2 samples of 13 x 13 pixels = 338 rows; the weight
# gradient: 128 x 128 channels over the pixels).  The CPU sensitivity test runs the same generators at the same shapes.  K = 576 (3x3,
# 64 -> 64) is NOT pinned: a lost h*l term sits only 3.7x above the bound there (2.8x at K = 1024), so the 3x3 case has 32 input channels.
DOT_SHAPES = {
    "1x1_64_128": (338, 128, 64),
    "1x1_256_64": (338, 64, 256),
    "3x3_32_64": (338, 64, 288),
    "shortcut_64+64_128": (338, 128, 128),
    "wgrad_64px": (128, 128, 64),
    "wgrad_242px": (128, 128, 242),
}


def exponent_sweep(seed, k, span=24):
    """2^e_k per reduction index, e_k uniform in [-span, span]: activations times it and weights over it leave every product -- and, the
    scaling being exact in every plane, every partial product -- unchanged."""
    e = np.random.default_rng(seed).integers(-span, span + 1, k)
    return np.ldexp(np.float32(1), e).astype(np.float32)


# ---- metric and bound -----------------------------------------------------------------------------------------------------------------
def subset(shape, seed=0, count=SUBSET):
    """A fixed choice of `count` of the outputs of an array of `shape` -> index arrays, one per axis."""
    total = int(np.prod(shape))
    flat = np.random.default_rng(seed).choice(total, size=min(count, total), replace=False)
    flat.sort()
    return np.unravel_index(flat, shape)


def pair_stats(got, ar, wc):
    """(median, p99, max) of the error of the results `got` of the dot products of the gathered operand pairs ar, wc [count, K]."""
    p = ar.astype(np.float64) * wc.astype(np.float64)
    return stats(rel_err(got, np.sum(p, -1), np.sum(np.abs(p), -1)))


def reference(a, w):
    """float64 dot products of the fp32 values a [..., m, k], w [..., n, k] and their scale: (a @ w^T, |a| @ |w|^T), each [..., m, n]."""
    a64, w64 = a.astype(np.float64), np.swapaxes(w.astype(np.float64), -1, -2)
    return a64 @ w64, np.abs(a64) @ np.abs(w64)


def rel_err(got, ref, scale):
    return np.abs(got.astype(np.float64) - ref) / scale


def stats(e):
    return float(np.median(e)), float(np.percentile(e, 99)), float(np.max(e))


def budget(ar, wc):
    """(B_med, B_99, (median, p99, max) of the plain fp32 accumulation) on the gathered operand pairs ar, wc [count, K] of a case."""
    e = pair_stats(_dot_fp32(ar, wc), ar, wc)
    return FACTOR * e[0], FACTOR * e[1], e

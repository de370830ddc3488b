"""-m gpu: the bf16 convolution kernels (csrc/hvn_conv_bf16.hip, hvn_conv_bf16g.hip) held to ONE correctly rounded bf16 store.

test_gpu_bf16.py accepts any output within 1.5 % of the largest output of the fp32 interpreter: a kernel whose store truncates, or that
rounds its accumulator to bf16 before the epilogue or once per k-step, passes it.  Here every case of tests/bf16_model.py runs on exactly
the values the float64 reference is formed from -- bf16-exact activations, weights and residual, fp32 bias / prologue / block-closing BN,
the rest of the arena NaN -- and the raw output bits are held to its two criteria:

  H  every element within [rne64(ref64 - B), rne64(ref64 + B)], B the worst-case bound of ANY fp32 summation order -- bit equality where
     the ends coincide -- finite, and nothing outside the output view changed;
  R  at most 2 m_model + 8 elements differ from rne64(ref64), m_model the count of a sequential fp32 numpy model of the contract.

tests/test_bf16_arithmetic.py proves on the CPU, for the same cases, that the intact arithmetic passes both and that a truncating store,
an early or per-step rounding of the accumulator and a reordered epilogue each miss R at least 10-fold (a lost 32-channel slab: H).

The two bare cases also get the tolerance-free checks of test_gpu_x3_budget.py: products of bf16 values are exact and RNE commutes with
powers of two, so scaling reduction index k of the activations by 2^e_k and of the weights by 2^-e_k (e_k in [-24, 24]) must leave every
output BIT unchanged, and all activations times 2^+-40 must give the outputs times 2^+-40, bit for bit.

The chained kernel (hvn_conv_chain_bf16.hip) has no bare form and stays tied to two unchained launches by test_gpu_bf16.py's
bit-equality test; the LDS-DMA forms (tile codes 896 / 640) appear where they exist: >= 128 output channels, no prologue.
Measured figures: profiles/bf16_rounding_budget.txt."""
import numpy as np
import pytest

import bf16_model as BM
from net_ops_ref import bf16_bits, bf16_widen

pytestmark = pytest.mark.gpu

_RUNS = {}        # (case, gen, tile) -> the output bits of the unscaled run: the criteria and the scaling test share them


def _run(name, gen, tile, **replace):
    from gpu_util import run_conv_bits

    got, changed = run_conv_bits(tile, **dict(BM.build(name, gen)["spec"], **replace))
    assert changed == 0, "%s %s tile %d: %d arena elements outside the output view changed" % (name, gen, tile, changed)
    return got


def _base(name, gen, tile):
    if (name, gen, tile) not in _RUNS:
        _RUNS[(name, gen, tile)] = _run(name, gen, tile)
    return _RUNS[(name, gen, tile)]


@pytest.mark.parametrize("name,gen", BM.case_ids())
def test_one_correctly_rounded_store(name, gen):
    case = BM.build(name, gen)
    r = BM.reference(case)
    BM.conditions(case)
    m, allow, bad = BM.m_model(case), BM.allowance(case), ""
    for tile in case["tiles"]:
        got = _base(name, gen, tile)
        assert got.shape == r["ref"].shape
        off, out = BM.mismatches(got, r), BM.outside_H(got, r)
        print("bf16-rounding | %-26s | %-10s | tile %3d | %6d outputs | %3d off, model %3d, allowance %3d | outside H %d, max |err| / B %.3f"
              % (name, gen, tile, got.size, off, m, allow, out, BM.worst_ratio(got, r)))
        if out or off > allow:
            bad += "%s %s tile %d: %d elements outside H, %d not correctly rounded (allowance %d)\n" % (name, gen, tile, out, off, allow)
    assert not bad, bad


BARE = [(name, tile) for name in ("1x1_64_128_bare", "1x1_128_64_bare") for tile in BM.CASES[name]["tiles"]]


@pytest.mark.parametrize("name,tile", BARE, ids=lambda v: str(v))
def test_power_of_two_scalings_keep_the_bits(name, tile):
    base = _base(name, "random", tile)
    spec = BM.build(name, "random")["spec"]
    sweep = BM.exponent_sweep(BM.SEED + 1, spec["x"].shape[-1])
    x, wt = spec["x"] * sweep, spec["wt"] / sweep[:, None, None]
    assert (BM.to_bf16(x) == x).all() and (BM.to_bf16(wt) == wt).all()
    swept = _run(name, "random", tile, x=x, wt=wt)
    assert np.array_equal(swept, base), "%d outputs change under 2^e_k / 2^-e_k" % int((swept != base).sum())
    for e in (40, -40):
        moved = _run(name, "random", tile, x=spec["x"] * np.float32(2.0 ** e))
        want = bf16_bits(bf16_widen(base) * np.float32(2.0 ** e))
        assert np.array_equal(moved, want), "%d outputs are not 2^%d times the unscaled ones" % (int((moved != want).sum()), e)

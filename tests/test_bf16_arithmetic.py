"""CPU: what the two criteria of tests/bf16_model.py see, proved on the numpy model (no GPU, no kernel) for every case and generator
tests/test_gpu_bf16_rounding.py runs on the kernels.

  1. `rne64` (float64 -> bf16 value, not through fp32) is the rounding of `net_ops_ref.bf16_bits` wherever both are defined, exact
     ties included.
  2. The conditions on the inputs hold: >= 40 % of the outputs live, the model's own mismatch count <= 0.5 % of the outputs.
  3. The intact model -- sequential fp32 accumulation, the fp32 epilogue in the documented order, one RNE -- passes H and R.
  4. Every mutant of the model that is a different function on a case at all (`bf16_model.applies`) misses R's allowance at least
     10-fold there: a truncating store, the accumulator rounded to bf16 before the epilogue, the accumulator rounded to bf16 once per
     64-channel step, the residual added before the ReLU, the block-closing BN applied before the residual.
  5. A lost trailing 32-channel slab fails H, at K = 64 and at K = 288.
  6. The packing the engine uploads -- `repack_conv_bf16` of the plan's fp32 packing -- un-permuted by an inverse written here holds the
     test's weight bits and zeros everywhere else: 288 channels (the zero half-step) and the grouped, block-diagonal convolution."""
import numpy as np
import pytest

import bf16_model as BM
from net_ops_ref import bf16_bits, bf16_widen

IDS = BM.case_ids()


def test_rne64_is_the_rounding_of_bf16_bits():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(0, 1, 200000), rng.normal(0, 1e-3, 50000), rng.uniform(-1, 1, 50000) * 2.0 ** rng.integers(-60, 60, 50000),
                        [0.0, -0.0, 1.0, -1.0, 255.0, 2.0 ** -100, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23]]).astype(np.float32)
    assert np.array_equal(BM.rne64(x.astype(np.float64)), bf16_widen(bf16_bits(x)).astype(np.float64))
    # exact ties: the even neighbour, upwards and downwards, positive and negative, and across a power of two
    m = np.arange(128, 256, dtype=np.float64)
    for e in (-20, -1, 0, 7, 30):
        tie = np.ldexp(m + 0.5, e - 7)
        want = np.ldexp(np.where(m % 2 == 0, m, m + 1), e - 7)
        for s in (1.0, -1.0):
            assert np.array_equal(BM.rne64(s * tie), s * want)
            assert np.array_equal(bf16_widen(bf16_bits((s * tie).astype(np.float32))).astype(np.float64), s * want)
        # a hair off the tie -- below fp32's resolution, which a rounding THROUGH fp32 would get wrong -- goes to the nearer neighbour
        assert np.array_equal(BM.rne64(tie * (1 + 2.0 ** -40)), np.ldexp(m + 1, e - 7))
        assert np.array_equal(BM.rne64(tie * (1 - 2.0 ** -40)), np.ldexp(m, e - 7))
    assert np.array_equal(BM.rne64(np.array([2.0 ** -133 * 1.5, 2.0 ** -133 * 2.5, 2.0 ** -134])), np.array([2.0 ** -132, 2.0 ** -132, 0.0]))


@pytest.mark.parametrize("name,gen", IDS)
def test_intact_model_passes_and_every_mutant_misses_the_rounding_count(name, gen):
    case = BM.build(name, gen)
    r = BM.reference(case)
    live, frac = BM.conditions(case)
    intact = BM.model(case)
    m, allow = BM.mismatches(intact, r), BM.allowance(case)
    print("bf16-model | %-26s | %-10s | %6d outputs, %4.1f %% live, %4.1f %% bit-exact under H | model: %d off (%.3f %%), allowance %d, max |err| / B %.3f"
          % (name, gen, r["ref"].size, 100 * live, 100 * float((r["lo"] == r["hi"]).mean()), m, 100 * frac, allow, BM.worst_ratio(intact, r)))
    assert BM.outside_H(intact, r) == 0 and m == BM.m_model(case) <= allow
    for mutant in BM.MUTANTS:
        if not BM.applies(mutant, case):
            assert mutant != "truncating_store"
            continue
        off = BM.mismatches(BM.model(case, mutant), r)
        print("bf16-model | %-26s | %-10s |     %-26s %6d off = %.0f x the allowance" % (name, gen, mutant, off, off / allow))
        assert off >= BM.MUTANT_FACTOR * allow, (name, gen, mutant, off, allow)


def test_every_mutant_meets_a_case():
    seen = {m: [n for n, g in IDS if BM.applies(m, BM.build(n, g))] for m in BM.MUTANTS}
    assert all(len(v) >= 2 for k, v in seen.items() if k != "post_before_res") and len(seen["post_before_res"]) >= 1, seen
    assert len(seen["truncating_store"]) == len(IDS)


@pytest.mark.parametrize("name", ["1x1_64_128_bare", "1x1_288_128_windows_pre"])
def test_a_lost_trailing_slab_fails_H(name):
    case = BM.build(name, "random")
    K = case["A"].shape[1]
    assert K in (64, 288)
    r = BM.reference(case)
    out = BM.outside_H(BM.model(case, kmax=K - 32), r)
    print("bf16-model | %-26s | without the last 32 channels: %d of %d outputs outside H" % (name, out, r["ref"].size))
    assert out >= 0.25 * r["ref"].size, (name, out)


def _unpermute(w16, cout, cin, taps):
    """Inverse of the device layout [cout_pad, ceil(cin / 64), taps, 64] -> ([cout, cin, taps] bits, everything else: padded rows, the
    zero half-step), written from the kernel's addressing: row = output channel, then k-step, tap, channel inside the step."""
    cout_pad, steps, t, lanes = w16.shape
    assert t == taps and lanes == 64 and steps == -(-cin // 64) and cout_pad >= cout
    full = w16.transpose(0, 1, 3, 2).reshape(cout_pad, steps * 64, taps)
    return full[:cout, :cin], np.concatenate([full[cout:].ravel(), full[:cout, cin:].ravel()])


@pytest.mark.parametrize("name", ["1x1_288_128_windows_pre", "g5x5_128_32"])
def test_the_uploaded_packing_holds_the_tests_weight_bits(name):
    from gpu_util import conv_bits_plan
    from hover_net_amd.engine import repack_conv_bf16

    spec = BM.build(name, "random")["spec"]
    _, op, _ = conv_bits_plan(**spec)
    wt = spec["wt"]
    cout, cin_g, k, _ = wt.shape
    groups = spec["groups"]
    cin = cin_g * groups
    got, rest = _unpermute(repack_conv_bf16(op.w), cout, cin, k * k)
    assert not rest.any()
    want = np.zeros((cout, cin, k * k), np.uint16)
    og = cout // groups
    for g in range(groups):
        want[g * og:(g + 1) * og, g * cin_g:(g + 1) * cin_g] = bf16_bits(wt[g * og:(g + 1) * og]).reshape(og, cin_g, k * k)
    assert np.array_equal(got, want)
    assert np.array_equal(op.bias, spec["bias"]) if spec.get("bias") is not None else op.bias is None

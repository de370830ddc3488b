"""CPU: tests/train_ops_ref.py is right, and its bounds can tell an intact kernel from a subtly wrong one.

1. The float64 references agree with independent float64 computations: torch autograd through tests/train_interp.py's bn_fwd_ref and
   upadd_bwd_ref, oracle.train_torch.loss_terms in float64, torch.optim.Adam in float64.
2. The shapes of tests/train_ops_cases.py reach the paths they are there for (the arithmetic of bn_grid and the launch functions).
3. The intact fp32 mirror of every kernel stays within B on every case and generator that tests/test_gpu_train_ops.py runs.
4. Every named mutant of a mirror exceeds B by at least 2x on the inputs named next to it (a dropped pixel or a bf16 product cannot be
   seen against the worst-case bound of a long sum: those are judged on the short sums, and the exact lattice statements of
   test_gpu_train_ops.py cover the long ones).

Run with -s: one `train-ops |` line per case with the mirror's ratio max |err| / B, one per mutant with its excess."""
import numpy as np
import pytest
import torch

import train_ops_cases as K
import train_ops_ref as R

MUTANT_MARGIN = 2.0


def say(kernel, case, what, value):
    print("train-ops | %-11s | %-34s | %-22s %9.3g" % (kernel, case, what, value))


def worst(r):
    return max(r.values())


# ---- 1. references against independent float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,rows", [(4, 30), (12, 126), (72, 961)])
def test_bn_references_agree_with_float64_autograd(C, rows):
    import train_interp
    inp = K.bn_inputs(C, rows, "randn", seed=C)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    z = t(inp["z"]).view(1, rows, 1, C).requires_grad_(True)
    gamma, beta = t(inp["gamma"]).requires_grad_(True), t(inp["beta"]).requires_grad_(True)
    rm, rv = t(inp["rm"]).clone(), t(inp["rv"]).clone()
    a, mean, rstd = train_interp.bn_fwd_ref(z, gamma, beta, rm, rv)
    da = t(inp["da"]).view(1, rows, 1, C)
    (a * da).sum().backward()
    f = R.bn_forward_ref(inp["z"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], inp["eps"], inp["mom"])
    save = f["save"][0]
    near = lambda got, want, tol: float(np.abs(got - want).max()) <= tol * (float(np.abs(want).max()) + 1e-300)
    assert near(save[2], mean.detach().numpy(), 1e-12) and near(save[3], rstd.detach().numpy(), 1e-7)        # eps, momentum: fp32 values here
    assert near(f["rm"][0], rm.detach().numpy(), 1e-7) and near(f["rv"][0], rv.detach().numpy(), 1e-7)
    a_ref, _ = R.bn_apply_ref(inp["z"], save)
    assert near(a_ref, a.detach().numpy().reshape(rows, C), 1e-7)
    mask = a.detach().numpy().reshape(rows, C) > 0
    zero = np.zeros(C)
    b = R.bn_backward_reduce_ref(inp["z"], inp["da"], mask, save, inp["gamma"], zero, zero)
    assert near(b["dgamma"][0], gamma.grad.numpy(), 1e-7) and near(b["dbeta"][0], beta.grad.numpy(), 1e-12)
    dz, _ = R.bn_backward_apply_ref(inp["z"], inp["da"], mask, save, b["coef"][0], np.zeros((rows, C)))
    assert near(dz, z.grad.numpy().reshape(rows, C), 1e-7)
    # the same backward formula as train_interp.bn_bwd_ref states it
    dz2, dg2, db2 = train_interp.bn_bwd_ref(z.detach(), a.detach(), da, t(inp["gamma"]), t(save[2]), t(save[3]))
    assert near(dz, dz2.numpy().reshape(rows, C), 1e-12) and near(b["dgamma"][0], dg2.numpy(), 1e-12) and near(b["dbeta"][0], db2.numpy(), 1e-12)


def test_upadd_reference_agrees_with_train_interp():
    import train_interp
    r = np.random.default_rng(1)
    dy, dlo0, dsk0 = (r.standard_normal(s).astype(np.float32) for s in ((2, 8, 6, 12), (2, 4, 3, 12), (2, 8, 6, 12)))
    (ref, B), dskip = R.upadd_bwd_ref(dy, dlo0, dsk0)
    want = train_interp.upadd_bwd_ref(torch.from_numpy(dy).double()).numpy() + dlo0
    assert float(np.abs(ref - want).max()) < 1e-14 and (dskip == dsk0 + dy).all() and (B > 0).all()


def test_head_and_conv0_references_agree_with_torch_float64():
    i = K.head_inputs(2, 5, 7, 5, False)
    h = R.head_bwd_ref(**i)
    dl, x, w = (torch.from_numpy(i[k]).double() for k in ("dl", "x", "w"))
    assert float(np.abs(h["dW"][0] - (i["dW0"] + (dl.T @ x).numpy())).max()) < 1e-12
    assert float(np.abs(h["da"][0] - (i["da0"] + (dl @ w).numpy())).max()) < 1e-12
    assert float(np.abs(h["db"][0] - (i["db0"] + dl.sum(0).numpy())).max()) < 1e-12
    for pad in (0, 3):
        c = K.conv0_inputs(2, 12, 11, pad, False)
        ref, B = R.conv0_wgrad_ref(c["img"], c["dz"], pad, c["dW0"])
        xp = torch.nn.functional.pad(torch.from_numpy(c["img"]).double().permute(0, 3, 1, 2) / 255.0, (pad,) * 4)
        want = torch.nn.grad.conv2d_weight(xp, (64, 3, 7, 7), torch.from_numpy(c["dz"]).double().permute(0, 3, 1, 2).contiguous())
        assert float(np.abs(ref - c["dW0"] - want.permute(0, 2, 3, 1).numpy()).max()) < 1e-11 and (B > 0).all()
    assert np.float32(255.0) * (np.float32(1.0) / np.float32(255.0)) == np.float32(1.0)         # the lattice images are exactly 0 and 1


@pytest.mark.parametrize("T", [0, 2, 5])
def test_loss_references_agree_with_the_training_oracle_in_float64(T, monkeypatch):
    from oracle import train_torch
    monkeypatch.setattr(R, "SMOOTH", 1e-3)          # the oracle's float64 run has the literals in double, the kernels (and R) in fp32
    monkeypatch.setattr(R, "LO", 10e-8)
    monkeypatch.setattr(R, "HI", 1.0 - 10e-8)
    n, h, w = 2, 9, 11
    i = K.loss_inputs(n, h, w, T, "randn", "mixed", seed=T)
    wt = (2.0, 0.5, 1.5, 0.25, 0.75, 3.0)
    lg = {k: torch.from_numpy(i["l_" + k]).double().requires_grad_(True) for k in (("tp",) if T else ()) + ("np", "hv")}
    batch = {"np_map": torch.from_numpy(i["t_np"]).long(), "hv_map": torch.from_numpy(i["t_hv"])}
    opts = {"np": {"bce": wt[0], "dice": wt[1]}, "hv": {"mse": wt[2], "msge": wt[3]}}
    if T:
        batch["tp_map"] = torch.from_numpy(i["t_tp"]).long()
        opts["tp"] = {"bce": wt[4], "dice": wt[5]}
    total, terms = train_torch.loss_terms(lg, batch, T or None, dtype=torch.float64, loss_opts=opts)
    total.backward()
    (sums, B), (gws, Bg) = R.loss_forward_ref(**i)
    m = n * h * w
    mine = {"loss_np_bce": sums[0] / m, "loss_hv_mse": sums[2] / (2 * m), "loss_hv_msge": sums[3] / (sums[4] + 1e-8),
            "loss_np_dice": sum(1 - (2 * sums[8 + c] + 1e-3) / (sums[10 + c] + sums[12 + c] + 1e-3) for c in range(2))}
    if T:
        mine["loss_tp_bce"] = sums[1] / m
        mine["loss_tp_dice"] = sum(1 - (2 * sums[16 + c] + 1e-3) / (sums[32 + c] + sums[48 + c] + 1e-3) for c in range(T))
    assert set(mine) == set(terms)
    for k, v in mine.items():
        assert abs(v - float(terms[k].detach())) <= 1e-12 * max(1.0, abs(float(terms[k].detach()))), k
    assert sums[4] == 2 * (i["t_np"] != 0).sum() and (sums[12:14] == [(i["t_np"] == 0).sum(), (i["t_np"] != 0).sum()]).all()
    g = R.loss_backward_ref(sums=sums, gws=gws, wt=wt, M=float(m), **i)
    for k, v in lg.items():
        ref, Bk = g[k]
        assert float(np.abs(ref - v.grad.numpy()).max()) <= 1e-11 * float(np.abs(ref).max()), k
        assert (Bk > 0).all() and float((Bk / (np.abs(ref) + 1e-30)).min()) < 1e-5


def test_adam_reference_agrees_with_torch_float64():
    H = K.ADAM_HYPER
    f = lambda x: float(np.float32(x))
    i = K.adam_inputs(257, "randn")
    p = torch.nn.Parameter(torch.from_numpy(i["w0"]).double())
    opt = torch.optim.Adam([p], lr=f(H["lr"]), betas=(f(H["b1"]), f(H["b2"])), eps=f(H["eps"]))
    w, m, v = i["w0"].astype(np.float64), np.zeros(257), np.zeros(257)
    r = np.random.default_rng(5)
    for step in range(1, 6):
        g = r.standard_normal(257)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        o = R.adam_ref(w, g, m, v, step=step, **H)
        w, m, v = o["w"][0], o["m"][0], o["v"][0]
        assert float(np.abs(w - p.detach().numpy()).max()) < 1e-13, step


# ---- 2. the shapes reach their paths ---------------------------------------------------------------------------------------------------
def test_the_cases_reach_the_paths_they_name():
    g = {c[0]: R.bn_grid(c[0], c[1] * (c[2] - 2 * c[4]) * (c[3] - 2 * c[4])) for c in K.BN_CASES}
    assert g[4]["lq"] == 1 and g[4]["rper"] == 256
    assert g[12]["lq"] == 2 and g[12]["gx"] == 2 and 12 // 4 % 2 == 1
    assert g[2048]["gx"] == 8 and g[2048]["lq"] == 64
    assert all(not g[c]["capped"] and g[c]["passes"] <= 2 for c in (4, 12, 72, 2048))
    big = g[64]
    assert big["capped"] and big["gy"] == 256 and big["passes"] == 3 and big["ragged"] and 2 * 182 * 182 > 65536
    C, n, h, w = K.UPADD_BIG
    assert n * (h // 2) * (w // 2) * (C // 4) > 16384 * 256 and n * h * w * C < 2 ** 31
    assert all(n * (h // 2) * (w // 2) * (C // 4) <= 16384 * 256 for C, n, h, w in K.UPADD_CASES)
    px = [n * h * w for n, h, w in K.HEAD_PIXELS]
    assert px[0] == 1 and px[1] < 64 and px[2] % 256 and R.cdiv(px[3], 256) == 517 > R.HEAD_MAX_WGS and px[3] % 256
    out = [(n, H + 2 * p - 6, W + 2 * p - 6) for n, H, W, p, _ in K.CONV0_CASES]
    assert out[0][1:] == (1, 1) and out[1][1:] == (16, 16) and out[2][1:] == (17, 33) and out[3][1:] == (8, 8) and out[4][1:] == (23, 39)
    assert out[5][0] * 4 * 4 == 528 > R.CONV0_MAX_WGS
    assert 3 * 37 * 53 % 256 != 0 and 3 * 37 * 53 > 256                   # inactive lanes in the last workgroup of hvn_loss_partial
    assert K.ADAM_LENGTHS[-1] > 8192 * 1024 and K.ADAM_LENGTHS[-1] % 4 == 3


# ---- 3 / 4. mirrors within B, mutants outside ------------------------------------------------------------------------------------------
BN_KILLS = {"sums_fp32": "offset", "biased_var": "randn", "shift_fp32": "offset", "mask_ge": "randn", "no_xhat": "randn"}


@pytest.mark.parametrize("case", K.BN_CASES, ids=lambda c: "C%d-%dx%dx%d" % c[:4])
def test_bn_mirror_and_mutants(case):
    C, n, h, w, crop = case
    rows = n * (h - 2 * crop) * (w - 2 * crop)
    for gen in K.BN_GENERATORS + ("zero_lattice",):
        inp = K.bn_zero_lattice(C, rows) if gen == "zero_lattice" else K.bn_inputs(C, rows, gen)
        r = R.bn_judge(inp, R.bn_mirror(mutant=None, **inp))
        say("bn", "C%d rows %d %s" % (C, rows, gen), "mirror", worst(r))
        assert worst(r) <= 1.0, r
        for mut, where in BN_KILLS.items():
            if where != gen:
                continue
            rm = R.bn_judge(inp, R.bn_mirror(mutant=mut, **inp))
            say("bn", "C%d rows %d %s" % (C, rows, gen), "mutant " + mut, worst(rm))
            assert worst(rm) >= MUTANT_MARGIN, (mut, rm)


@pytest.mark.parametrize("case", K.UPADD_CASES, ids=str)
def test_upadd_mirror_and_mutant(case):
    C, n, h, w = case
    r = np.random.default_rng(7)
    dy, dlo0, dsk0 = (r.standard_normal(s).astype(np.float32) for s in ((n, h, w, C), (n, h // 2, w // 2, C), (n, h, w, C)))
    (ref, B), dskip = R.upadd_bwd_ref(dy, dlo0, dsk0)
    dlo, dsk = R.upadd_bwd_mirror(dy, dlo0, dsk0)
    say("upadd_bwd", str(case), "mirror", R.ratio(dlo, ref, B))
    assert R.ratio(dlo, ref, B) <= 1.0 and (dsk.view(np.int32) == dskip.view(np.int32)).all()
    x = R.ratio(R.upadd_bwd_mirror(dy, dlo0, dsk0, "three_taps")[0], ref, B)
    say("upadd_bwd", str(case), "mutant three_taps", x)
    assert x >= MUTANT_MARGIN


def judge(out, ref):
    return {k: R.ratio(out[k], *ref[k]) for k in ref}


@pytest.mark.parametrize("cout", K.HEAD_COUTS)
@pytest.mark.parametrize("pix", K.HEAD_PIXELS, ids=str)
def test_head_mirror_and_mutants(pix, cout):
    n, h, w = pix
    i = K.head_inputs(n, h, w, cout, False)
    ref = R.head_bwd_ref(**i)
    r = judge(R.head_bwd_mirror(**i), ref)
    say("head_bwd", "%s cout %d" % (pix, cout), "mirror", worst(r))
    assert worst(r) <= 1.0, r
    lat = K.head_inputs(n, h, w, cout, True)
    lr, lm = R.head_bwd_ref(**lat), R.head_bwd_mirror(**lat)
    assert all((lm[k] == lr[k][0]).all() for k in lr), "the integer lattice is exact in fp32"
    if n * h * w <= 874:                                     # a dropped pixel / a bf16 product against the bound of a SHORT sum
        for mut in ("drop_last", "bf16_products"):
            x = judge(R.head_bwd_mirror(mutant=mut, **i), ref)
            say("head_bwd", "%s cout %d" % (pix, cout), "mutant " + mut, max(x["dW"], x["db"]))
            assert x["dW"] >= MUTANT_MARGIN, (mut, x)


@pytest.mark.parametrize("case", K.CONV0_CASES, ids=str)
def test_conv0_wgrad_mirror_and_mutants(case):
    n, H, W, pad, _ = case
    i = K.conv0_inputs(n, H, W, pad, False)
    ref, B = R.conv0_wgrad_ref(i["img"], i["dz"], pad, i["dW0"])
    x = R.ratio(R.conv0_wgrad_mirror(i["img"], i["dz"], pad, i["dW0"]), ref, B)
    say("conv0_wgrad", str(case[:4]), "mirror", x)
    assert x <= 1.0
    lat = K.conv0_inputs(n, H, W, pad, True)
    assert (R.conv0_wgrad_mirror(lat["img"], lat["dz"], pad, lat["dW0"]) == R.conv0_wgrad_ref(lat["img"], lat["dz"], pad, lat["dW0"])[0]).all()
    if n * (H + 2 * pad - 6) * (W + 2 * pad - 6) <= 2 * 16 * 16:
        for mut in ("drop_last", "bf16_products"):
            x = R.ratio(R.conv0_wgrad_mirror(i["img"], i["dz"], pad, i["dW0"], mut), ref, B)
            say("conv0_wgrad", str(case[:4]), "mutant " + mut, x)
            assert x >= MUTANT_MARGIN, mut


def loss_judge(i, out, wt, M):
    (sums, B), (gws, Bg) = R.loss_forward_ref(**i)
    r = {"sums": R.ratio(out["sums"], sums, B), "gws": R.ratio(out["gws"], gws, Bg)}
    g = R.loss_backward_ref(sums=out["sums"], gws=out["gws"], wt=wt, M=M, **i)
    r.update({k: R.ratio(out[k], *g[k]) for k in g})
    return r


# mutant -> (output judged, generator, map, weight table).  The fp32 dice combination shows where nothing else hides it: a dice-only branch
# (the table's tp bce weight is 0: no bce term in the stored value), 16 classes of which 15 never occur (|D| of the absent classes is
# orders above the present one's) and saturated logits, at the largest shape.
LOSS_KILLS = {"sobel_clamped": ("gws", "randn", "mixed", "ones"), "no_transpose": ("gws", "randn", "mixed", "ones"),
              "no_gate": ("np", "sat40", "mixed", "ones"), "local_M": ("hv", "randn", "mixed", "ones"),
              "dice_fp32": ("tp", "sat40", "background", "table")}
LOSS_EXTRA_WEIGHTED = (("randn", "mixed"), ("sat40", "background"))       # the combinations that also run with the other weight tables


@pytest.mark.parametrize("T", K.LOSS_TYPES)
@pytest.mark.parametrize("shape", K.LOSS_SHAPES, ids=str)
def test_loss_mirror_and_mutants(shape, T):
    n, h, w = shape
    M = 2.0 * n * h * w
    top = {}
    for gen in K.LOSS_GENERATORS:
        for kind in K.LOSS_MAPS:
            for wname, wt in K.LOSS_WEIGHTS.items():
                if wname != "ones" and (gen, kind) not in LOSS_EXTRA_WEIGHTED:
                    continue
                i = K.loss_inputs(n, h, w, T, gen, kind)
                r = loss_judge(i, R.loss_mirror(wt=wt, M=M, **i), wt, M)
                say("loss", "%s T%d %s %s %s" % (shape, T, gen, kind, wname), "mirror", worst(r))
                assert worst(r) <= 1.0, (gen, kind, wname, r)
                if n * h * w < 12:
                    continue
                for mut, (key, kgen, kkind, kw) in LOSS_KILLS.items():
                    if (kgen, kkind, kw) == (gen, kind, wname) and (mut != "dice_fp32" or (T == 16 and n * h * w > 5000)):
                        x = loss_judge(i, R.loss_mirror(wt=wt, M=M, mutant=mut, **i), wt, M)
                        top[mut] = max(top.get(mut, 0.0), x[key])
    for mut, x in top.items():
        say("loss", "%s T%d" % (shape, T), "mutant " + mut, x)
        assert x >= MUTANT_MARGIN, (mut, x)


ADAM_KILLS = {"eps_in_sqrt": ("wide", (1, 2, 1000, 100000)), "no_bc1": ("randn", (1, 2))}


@pytest.mark.parametrize("n", K.ADAM_LENGTHS)
def test_adam_mirror_and_mutants(n):
    H = K.ADAM_HYPER
    for gen in ("randn", "wide"):
        i = K.adam_inputs(n, gen)
        for step in K.ADAM_STEPS:
            ref = R.adam_ref(step=step, **i, **H)
            r = judge(R.adam_mirror(step=step, **i, **H), ref)
            say("adam", "n %d %s step %d" % (n, gen, step), "mirror", worst(r))
            assert worst(r) <= 1.0, r
            if n < 1023 or n > 10 ** 6:
                continue
            for mut, (where, steps) in ADAM_KILLS.items():
                if where == gen and step in steps:
                    x = judge(R.adam_mirror(step=step, mutant=mut, **i, **H), ref)["w"]
                    say("adam", "n %d %s step %d" % (n, gen, step), "mutant " + mut, x)
                    assert x >= MUTANT_MARGIN, (mut, step, x)


def test_adam_fp32_bias_corrections_mutant_exceeds_the_bound():
    """Bias corrections formed in fp32 (beta^step as an fp32 running product), at step 100000.  With the reference's betas the mutant is
    no mutant at that step -- 1 - beta^100000 is exactly 1 in fp32 and in double, the two forms give the same bits (asserted) -- so it is
    judged with train_ops_cases.ADAM_HYPER_SLOW, whose second-moment correction is still 0.091 there, on weights that are zero (B is then
    relative to the update).  The intact mirror stays within B on the same table at every step and generator."""
    i = K.adam_inputs(K.ADAM_SLOW_LENGTH, "randn")
    a, b = R.adam_mirror(step=100000, **i, **K.ADAM_HYPER), R.adam_mirror(step=100000, mutant="bc_fp32", **i, **K.ADAM_HYPER)
    assert all((a[k] == b[k]).all() for k in a)
    H = K.ADAM_HYPER_SLOW
    assert np.float32(H["b2"]) == H["b2"] and 0.9 < H["b2"] ** 100000 < 0.91
    for gen in ("randn", "wide", "zero_w"):
        i = K.adam_inputs(K.ADAM_SLOW_LENGTH, gen)
        for step in K.ADAM_STEPS:
            ref = R.adam_ref(step=step, **i, **H)
            r = judge(R.adam_mirror(step=step, **i, **H), ref)
            say("adam", "slow beta2 n %d %s step %d" % (K.ADAM_SLOW_LENGTH, gen, step), "mirror", worst(r))
            assert worst(r) <= 1.0, r
    i = K.adam_inputs(K.ADAM_SLOW_LENGTH, "zero_w")
    x = judge(R.adam_mirror(step=100000, mutant="bc_fp32", **i, **H), R.adam_ref(step=100000, **i, **H))["w"]
    say("adam", "slow beta2 n %d zero_w step 100000" % K.ADAM_SLOW_LENGTH, "mutant bc_fp32", x)
    assert x >= MUTANT_MARGIN, x

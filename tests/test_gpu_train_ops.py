"""-m gpu: the training step's non-GEMM kernels (csrc/hvn_train.hip), through the C ABI (hvn_run_train_plan, hvn_run_train_plan_ws,
hvn_loss_forward, hvn_loss_backward, hvn_adam_step), against tests/train_ops_ref.py.  Two kinds of statement:

  exact   no tolerance, on integer-lattice inputs (every sum an integer below 2^24, so any order of any fp32 summation gives the same
          bits): indexing, coverage, tails, duplication; every element outside a view is bit-unchanged; the recomputed ReLU mask equals
          the sign of the stored activation; the first-writer store equals += over zeros; the class counts of the loss;
  bound   |got - ref64| <= B for EVERY element on real-valued inputs, B the worst-case bound of train_ops_ref (proved on the CPU by
          tests/test_train_ops_ref.py, which also shows that the named mutants of each kernel fall outside it).

Cases and generators: tests/train_ops_cases.py (the smallest shapes that reach each path).  Every test prints one `train-ops |` line per
case: kernel, case, max |err| / B of the GPU result, and of the numpy fp32 mirror on the same inputs (profiles/train_ops_error.txt)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_ops_cases as K
import train_ops_ref as R
from gpu_util import run_tops, run_train_ops, view_of

pytestmark = pytest.mark.gpu


def L():
    from hover_net_amd import lib
    lib.require_gpu()
    return lib


def say(kernel, case, gpu, mirror):
    print("train-ops | %-11s | %-44s | gpu %8.3g | mirror %8.3g" % (kernel, case, gpu, mirror))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def dev_same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def noise(shape, seed):
    """What the buffers hold around the views: random values, drawn on the device (the large cases would spend their time drawing them)."""
    return torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def changed(t, t0):
    """Number of elements of the cuda tensor t whose bits differ from t0's."""
    return int((t.view(torch.int32) != t0.view(torch.int32)).sum())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def worst(r):
    return max(r.values())


# ---- BN -------------------------------------------------------------------------------------------------------------------------------
def bn_run(inp, n, h, w, C, crop, step, dz="accumulate"):
    """BN_FWD then BN_BWD on `inp` (train_ops_cases.bn_inputs: the logical [rows][C] tensors).  z and dz are windows (offset `crop`
    pixels, 32 channels in, every step-th pixel) of larger buffers.  dz: accumulate | store (mode & 1 over a NaN-filled dz) | none (base
    NULL) -> dict of what the kernels left (numpy, logical layout) + `outside`: elements outside the dz view that changed."""
    lib = L()
    Hb, Wb, Cb = (h + 2 * crop) * step, (w + 2 * crop) * step, C + 32
    sl = (slice(None), slice(crop * step, crop * step + (h - 1) * step + 1, step), slice(crop * step, crop * step + (w - 1) * step + 1, step),
          slice(32, None))
    zc = noise((n, Hb, Wb, Cb), 11)
    zc[sl] = dev(inp["z"]).view(n, h, w, C)
    dzc = noise((n, Hb, Wb, Cb), 12)
    dzc[sl] = float("nan") if dz == "store" else dev(inp["dz0"]).view(n, h, w, C)
    rest0 = dzc.clone()
    ab = torch.full((n, h, w, C), float("nan"), device="cuda")
    dab = dev(inp["da"]).view(n, h, w, C)
    ws = torch.full((256 * 2 * C,), 1e30, dtype=torch.float64, device="cuda")
    save, coef = torch.full((4 * C,), float("nan"), device="cuda"), torch.full((3 * C,), float("nan"), device="cuda")
    gm, bt, rm, rv = dev(inp["gamma"]), dev(inp["beta"]), dev(inp["rm"]), dev(inp["rv"])
    dgam, dbet = dev(inp["dgamma0"]), dev(inp["dbeta0"])
    zv = view_of(zc, crop * step, crop * step, h, w, 32, C, step=step)
    tf = lib.hvn_top()
    tf.kind, tf.x, tf.y = 3, zv, view_of(ab)
    for i, t in enumerate((ws, save, gm, bt, rm, rv)):
        tf.p[i] = t.data_ptr()
    tf.eps, tf.momentum = float(inp["eps"]), float(inp["mom"])
    run_tops([tf], n)
    a_out = host(ab).reshape(-1, C)
    save_out = host(save).reshape(4, C)
    tb = lib.hvn_top()
    tb.kind, tb.x, tb.y, tb.dy = 4, zv, view_of(ab), view_of(dab)
    if dz != "none":
        tb.dx = view_of(dzc, crop * step, crop * step, h, w, 32, C, step=step)
    tb.mode = 1 if dz == "store" else 0
    for i, t in enumerate((ws, save, gm, dgam, dbet, coef)):
        tb.p[i] = t.data_ptr()
    inputs = (zc, ab, dab, save, gm, rm, rv)
    before = [t.clone() for t in inputs]
    run_tops([tb], n)
    assert all(dev_same_bits(x, y) for x, y in zip(before, inputs)), "BN_BWD changed one of its inputs"
    got = host(dzc[sl]).reshape(-1, C)
    rest0[sl] = dzc[sl]                                   # everything outside the dz view, compared on the device
    outside = changed(dzc, rest0)
    return dict(save=save_out, rm=host(rm), rv=host(rv), a=a_out, dgamma=host(dgam), dbeta=host(dbet), coef=host(coef).reshape(3, C),
                dz=None if dz == "none" else got, dz_raw=got, outside=outside)


@pytest.mark.parametrize("gen", K.BN_GENERATORS)
@pytest.mark.parametrize("case", K.BN_CASES, ids=lambda c: "C%d-%dx%dx%d" % c[:4])
def test_bn_forward_backward_within_the_bound(case, gen):
    C, n, H, W, crop = case
    h, w = H - 2 * crop, W - 2 * crop
    inp = K.bn_inputs(C, n * h * w, gen)
    out = bn_run(inp, n, h, w, C, crop, step=2 if C == 12 else 1)
    r = R.bn_judge(inp, out)
    say("bn", "C%d %dx%dx%d crop %d %s" % (C, n, H, W, crop, gen), worst(r), bn_mirror_ratio(inp))
    assert worst(r) <= 1.0, r
    assert out["outside"] == 0


@pytest.mark.parametrize("case", K.BN_CASES, ids=lambda c: "C%d-%dx%dx%d" % c[:4])
def test_bn_backward_mask_store_and_frozen_forms_exactly(case):
    C, n, H, W, crop = case
    h, w = H - 2 * crop, W - 2 * crop
    inp = K.bn_zero_lattice(C, n * h * w)
    step = 2 if C == 12 else 1
    acc = bn_run(inp, n, h, w, C, crop, step)
    a = acc["a"]
    # the lattice did its work: many stored activations are exactly zero, many are positive and below one ulp-scale of the shift
    pre_zero_rows = inp["z"] == np.round(f64mean(inp["z"]))
    assert int((a[pre_zero_rows] == 0).sum()) > 0 and (C < 12 or int((a[pre_zero_rows] > 0).sum()) > 0)
    # dbeta (from 0) is the exact integer sum of da over the pixels whose STORED activation is positive
    want = (inp["da"].astype(np.float64) * (a > 0)).sum(0)
    assert np.abs(want).max() < 2 ** 24
    assert (acc["dbeta"].astype(np.float64) == want).all(), np.abs(acc["dbeta"] - want).max()
    r = R.bn_judge(inp, acc)
    say("bn", "C%d %dx%dx%d crop %d zero lattice" % (C, n, H, W, crop), worst(r), bn_mirror_ratio(inp))
    assert worst(r) <= 1.0 and acc["outside"] == 0, r
    # mode & 1 over a NaN-filled dz: the bits of += over a zeroed one
    zero = dict(inp, dz0=np.zeros_like(inp["dz0"]))
    added, stored = bn_run(zero, n, h, w, C, crop, step), bn_run(inp, n, h, w, C, crop, step, dz="store")
    assert same_bits(added["dz"], stored["dz"]) and stored["outside"] == 0
    assert all(same_bits(added[k], stored[k]) for k in ("dgamma", "dbeta", "coef", "save", "a"))
    # dz == NULL (the frozen encoder): dgamma, dbeta and coef as before, nothing else written
    frozen = bn_run(inp, n, h, w, C, crop, step, dz="none")
    assert frozen["outside"] == 0 and same_bits(frozen["dz_raw"], inp["dz0"])
    assert all(same_bits(frozen[k], acc[k]) for k in ("dgamma", "dbeta", "coef"))


def bn_mirror_ratio(inp):
    """The mirror's figure next to the GPU's; for the largest case it is in test_train_ops_ref.py's output (forming it here would
    dominate the test)."""
    return worst(R.bn_judge(inp, R.bn_mirror(**inp))) if inp["z"].size < 10 ** 6 else float("nan")


def f64mean(z):
    return R.colsum(z.astype(np.float64)) / z.shape[0]


# ---- UPADD_BWD --------------------------------------------------------------------------------------------------------------------------
def upadd_run(dy, dlo0, dsk0, form):
    """dy every second pixel of a larger buffer, dskip a window, dlo a channel window.  -> (dlo, dskip, changed elements outside the views)."""
    lib = L()
    n, h, w, C = dy.shape
    dyc = noise((n, 2 * h, 2 * w, C), 21)
    dyc[:, ::2, ::2] = dev(dy)
    skc = noise((n, h + 5, w + 3, C), 22)
    skc[:, 2:2 + h, 1:1 + w] = dev(dsk0)
    loc = noise((n, h // 2, w // 2, C + 8), 23)
    loc[..., 4:4 + C] = dev(dlo0)
    dy0, sk0, lo0 = dyc.clone(), skc.clone(), loc.clone()
    t = lib.hvn_top()
    t.kind, t.dy = 7, view_of(dyc, step=2)
    if form in ("both", "dlo"):
        t.dx = view_of(loc, c0=4, c=C)
    if form in ("both", "dskip"):
        t.y = view_of(skc, 2, 1, h, w)
    run_tops([t], n)
    assert changed(dyc, dy0) == 0
    got_sk, got_lo = host(skc[:, 2:2 + h, 1:1 + w]), host(loc[..., 4:4 + C])
    sk0[:, 2:2 + h, 1:1 + w] = skc[:, 2:2 + h, 1:1 + w]
    lo0[..., 4:4 + C] = loc[..., 4:4 + C]
    return got_lo, got_sk, changed(skc, sk0) + changed(loc, lo0)


@pytest.mark.parametrize("form", K.UPADD_FORMS)
@pytest.mark.parametrize("case", K.UPADD_CASES, ids=str)
def test_upadd_backward_exact_and_within_the_bound(case, form):
    C, n, h, w = case
    r = np.random.default_rng(31)
    for lattice in (True, False):
        gen = (lambda s: r.integers(-9, 10, s).astype(np.float32)) if lattice else (lambda s: r.standard_normal(s).astype(np.float32))
        dy, dlo0, dsk0 = gen((n, h, w, C)), gen((n, h // 2, w // 2, C)), gen((n, h, w, C))
        (ref, B), dskip = R.upadd_bwd_ref(dy, dlo0, dsk0)
        lo, sk, outside = upadd_run(dy, dlo0, dsk0, form)
        assert outside == 0
        assert same_bits(sk, dskip if form != "dlo" else dsk0)            # one addition: exact on any input; untouched when dskip is NULL
        if form == "dskip":
            assert same_bits(lo, dlo0)
        elif lattice:
            assert same_bits(lo, ref.astype(np.float32)) and (ref == ref.astype(np.float32)).all()
        else:
            m = R.ratio(R.upadd_bwd_mirror(dy, dlo0, dsk0)[0], ref, B)
            say("upadd_bwd", "C%d %dx%dx%d %s" % (C, n, h, w, form), R.ratio(lo, ref, B), m)
            assert R.ratio(lo, ref, B) <= 1.0


def test_upadd_backward_grid_stride_loop_exactly():
    """More channel quads than 16384 workgroups of 256 threads: every thread takes a second element.  Integer lattice, the reference formed
    with torch on the GPU (integer-valued fp32 sums are exact in any order)."""
    lib = L()
    C, n, h, w = K.UPADD_BIG
    g = torch.Generator(device="cuda").manual_seed(41)
    ri = lambda *s: torch.randint(-9, 10, s, device="cuda", generator=g, dtype=torch.int32)
    dy, dlo0, dsk0 = ri(n, h, w, C), ri(n, h // 2, w // 2, C), ri(n, h, w, C)
    want_lo = dlo0 + dy.view(n, h // 2, 2, w // 2, 2, C).sum((2, 4))
    want_sk = dsk0 + dy
    dyf, lo, sk = dy.float(), dlo0.float(), dsk0.float()
    del dlo0, dsk0
    t = lib.hvn_top()
    t.kind, t.dy, t.dx, t.y = 7, view_of(dyf), view_of(lo), view_of(sk)
    run_tops([t], n)
    assert torch.equal(lo, want_lo.float()) and torch.equal(sk, want_sk.float()) and torch.equal(dyf, dy.float())


# ---- HEAD_BWD ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def head_problem(n, h, w, cout, lattice):
    i = K.head_inputs(n, h, w, cout, lattice)
    ref = R.head_bwd_ref(**i)
    mirror = None
    if not lattice:         # the largest case's mirror figure is in test_train_ops_ref.py's output: forming it here would dominate the test
        mirror = {k: R.ratio(v, *ref[k]) for k, v in R.head_bwd_mirror(**i).items()} if n * h * w < 10 ** 5 else dict.fromkeys(ref, float("nan"))
    return i, ref, mirror


def head_run(i, n, h, w, cout, stored):
    """x and dx windows (2 pixels in, 64 of 96 / 80 channels) of larger buffers -> dict(da, dW, db), changed elements outside dx."""
    lib = L()
    xc, dc = noise((n, h + 3, w + 4, 96), 51), noise((n, h + 2, w + 2, 80), 52)
    xc[:, 1:1 + h, 2:2 + w, 32:] = dev(i["x"]).view(n, h, w, 64)
    dc[:, 2:2 + h, 1:1 + w, 16:] = dev(i["da0"]).view(n, h, w, 64)
    x0, d0 = xc.clone(), dc.clone()
    dl = dev(i["dl"].reshape(n, h, w, cout).transpose(0, 3, 1, 2))            # NCHW
    W_, dW, db = dev(i["w"]), dev(i["dW0"]), dev(i["db0"])
    t = lib.hvn_top()
    t.kind, t.cout, t.x, t.dx = 8, cout, view_of(xc, 1, 2, h, w, 32, 64), view_of(dc, 2, 1, h, w, 16, 64)
    for k, p in enumerate((dl, W_, dW, db)):
        t.p[k] = p.data_ptr()
    need = run_train_ops([t], n, stored_parts=stored)
    if stored:
        groups = R.cdiv(n * h * w, 256)
        assert need == 4 * min(groups, R.HEAD_MAX_WGS) * (cout * 64 + cout)
    assert changed(xc, x0) == 0 and same_bits(host(W_), i["w"])
    da = host(dc[:, 2:2 + h, 1:1 + w, 16:]).reshape(-1, 64)
    d0[:, 2:2 + h, 1:1 + w, 16:] = dc[:, 2:2 + h, 1:1 + w, 16:]
    return dict(da=da, dW=host(dW), db=host(db)), changed(dc, d0)


@pytest.mark.parametrize("stored", [False, True], ids=["atomic", "workspace"])
@pytest.mark.parametrize("cout", K.HEAD_COUTS)
@pytest.mark.parametrize("pix", K.HEAD_PIXELS, ids=lambda p: "%dx%dx%d" % p)
def test_head_backward_exact_and_within_the_bound(pix, cout, stored):
    n, h, w = pix
    i, ref, _ = head_problem(n, h, w, cout, True)
    got, outside = head_run(i, n, h, w, cout, stored)
    assert outside == 0
    for k in ref:
        assert (ref[k][0] == ref[k][0].astype(np.float32)).all() and same_bits(got[k], ref[k][0].astype(np.float32)), k
    i, ref, mirror = head_problem(n, h, w, cout, False)
    got, outside = head_run(i, n, h, w, cout, stored)
    r = {k: R.ratio(got[k], *ref[k]) for k in ref}
    for k in ("da", "dW", "db"):                  # per output: da's bound is a chain of cout, dW's and db's of the whole pixel sum
        say("head_bwd", "%dx%dx%d cout %d %s %s" % (n, h, w, cout, "workspace" if stored else "atomic", k), r[k], mirror[k])
    assert worst(r) <= 1.0 and outside == 0, r


# ---- CONV0_WGRAD ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def conv0_problem(n, H, W, pad, lattice):
    i = K.conv0_inputs(n, H, W, pad, lattice)
    ref, B = R.conv0_wgrad_ref(i["img"], i["dz"], pad, i["dW0"])
    return i, ref, B, (None if lattice else R.ratio(R.conv0_wgrad_mirror(i["img"], i["dz"], pad, i["dW0"]), ref, B))


def conv0_run(i, pad, window, stored):
    lib = L()
    n, H, W, _ = i["img"].shape
    oy, ox, Hb, Wb = (2, 3, H + 5, W + 7) if window else (0, 0, H, W)
    ib = torch.randint(0, 256, (n, Hb, Wb, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(61))
    ib[:, oy:oy + H, ox:ox + W] = torch.from_numpy(i["img"])
    ic, dz, dw = ib.cuda(), dev(i["dz"]), dev(i["dW0"].reshape(-1))
    t = lib.hvn_top()
    t.kind, t.pad_t = 6, pad
    t.x.base, t.x.sn, t.x.sy, t.x.sx, t.x.h, t.x.w, t.x.c, t.x.sc = ic.data_ptr() + (oy * Wb + ox) * 3, Hb * Wb * 3, Wb * 3, 3, H, W, 3, 1
    t.dy = view_of(dz)
    t.p[0] = dw.data_ptr()
    need = run_train_ops([t], n, stored_parts=stored)
    if stored:
        tiles = n * R.cdiv(dz.shape[1], 16) * R.cdiv(dz.shape[2], 16)
        assert need == 4 * min(tiles, R.CONV0_MAX_WGS) * 64 * 147
    assert same_bits(host(ic), ib.numpy()) and same_bits(host(dz), i["dz"])
    return host(dw).reshape(64, 7, 7, 3)


@pytest.mark.parametrize("stored", [False, True], ids=["atomic", "workspace"])
@pytest.mark.parametrize("case", K.CONV0_CASES, ids=lambda c: "%dx%dx%d-pad%d%s" % (c[:4] + ("-window" if c[4] else "",)))
def test_conv0_wgrad_exact_and_within_the_bound(case, stored):
    n, H, W, pad, window = case
    i, ref, _, _ = conv0_problem(n, H, W, pad, True)
    got = conv0_run(i, pad, window, stored)
    assert (ref == ref.astype(np.float32)).all() and same_bits(got, ref.astype(np.float32)), float(np.abs(got - ref).max())
    i, ref, B, mirror = conv0_problem(n, H, W, pad, False)
    x = R.ratio(conv0_run(i, pad, window, stored), ref, B)
    say("conv0_wgrad", "%dx%dx%d pad %d%s %s" % (n, H, W, pad, " window" if window else "", "workspace" if stored else "atomic"), x, mirror)
    assert x <= 1.0


# ---- loss -------------------------------------------------------------------------------------------------------------------------------
def loss_run(i, T, wt, M, partials):
    """Both stages -> dict(sums, gws, np, hv[, tp]).  Stage 2 reads the sums and the sobel_ws stage 1 left."""
    lib = L()
    n, _, h, w = i["l_np"].shape
    d = lib.hvn_loss()
    keep = {k: dev(v) for k, v in i.items() if v is not None}
    grads = {k: torch.full_like(keep["l_" + k], float("nan")) for k in ("np", "hv") + (("tp",) if T else ())}
    sums = torch.zeros(64, dtype=torch.float64, device="cuda")
    gws = torch.full((n, h, w, 2), float("nan"), device="cuda")
    d.logits_np, d.logits_hv, d.grad_np, d.grad_hv = keep["l_np"].data_ptr(), keep["l_hv"].data_ptr(), grads["np"].data_ptr(), grads["hv"].data_ptr()
    if T:
        d.logits_tp, d.grad_tp, d.true_tp = keep["l_tp"].data_ptr(), grads["tp"].data_ptr(), keep["t_tp"].data_ptr()
    d.true_np, d.true_hv, d.sums, d.sobel_ws = keep["t_np"].data_ptr(), keep["t_hv"].data_ptr(), sums.data_ptr(), gws.data_ptr()
    d.n, d.h, d.w, d.nr_types = n, h, w, T
    d.total_pixels = float(M)
    for k in range(6):
        d.weight[k] = float(wt[k])
    if partials:
        cnt = int(lib.lib().hvn_loss_partials_count(n, h, w))
        assert cnt == 64 * R.cdiv(n * h * w, 256)
        parts = torch.full((cnt + 64,), float("nan"), dtype=torch.float64, device="cuda")
        d.partials, d.partials_cap = parts.data_ptr(), cnt
    assert lib.lib().hvn_loss_forward(ctypes.byref(d), stream()) == 0, lib.lib().hvn_last_error()
    assert lib.lib().hvn_loss_backward(ctypes.byref(d), stream()) == 0, lib.lib().hvn_last_error()
    torch.cuda.synchronize()
    if partials:
        assert bool(torch.isnan(parts[cnt:]).all()) and not bool(torch.isnan(parts[:cnt]).any())
    out = dict(sums=host(sums), gws=host(gws))
    out.update({k: host(v) for k, v in grads.items()})
    return out


def loss_judge(i, out, wt, M):
    (sums, B), (gws, Bg) = R.loss_forward_ref(**i)
    r = {"sums": R.ratio(out["sums"], sums, B), "gws": R.ratio(out["gws"], gws, Bg)}
    g = R.loss_backward_ref(sums=out["sums"], gws=out["gws"], wt=wt, M=M, **i)
    r.update({k: R.ratio(out[k], *g[k]) for k in g})
    return r, sums


@pytest.mark.parametrize("T", K.LOSS_TYPES)
@pytest.mark.parametrize("shape", K.LOSS_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_loss_sums_exact_counts_and_gradients_within_the_bound(shape, T):
    n, h, w = shape
    M = 2.0 * n * h * w                                              # total_pixels != n h w: this rank is half of the batch
    for gen in K.LOSS_GENERATORS:
        for kind in K.LOSS_MAPS:
            for wname, wt in K.LOSS_WEIGHTS.items():
                if wname != "ones" and (gen, kind) not in (("randn", "mixed"), ("sat40", "background")):
                    continue
                i = K.loss_inputs(n, h, w, T, gen, kind)
                mi = loss_judge(i, R.loss_mirror(wt=wt, M=M, **i), wt, M)[0]
                forms = {}
                for partials in (False, True):
                    out = forms[partials] = loss_run(i, T, wt, M, partials)
                    r, sums = loss_judge(i, out, wt, M)
                    say("loss", "%dx%dx%d T%d %s %s %s %s" % (n, h, w, T, gen, kind, wname, "partials" if partials else "atomic"), worst(r), worst(mi))
                    assert worst(r) <= 1.0, (gen, kind, wname, partials, r)
                    # the class pixel counts and twice the foreground count are exact integers, in either form
                    fg = i["t_np"] != 0
                    assert out["sums"][4] == 2 * fg.sum() and (out["sums"][12:14] == [(~fg).sum(), fg.sum()]).all()
                    if T:
                        assert (out["sums"][48:48 + T] == np.bincount(i["t_tp"].reshape(-1), minlength=T)).all()
                    used = [0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13] + [b + c for b in (16, 32, 48) for c in range(T)]
                    assert (np.delete(out["sums"], used) == 0).all()
                # the atomic and the stored-partial form agree with each other: each is within B of the same reference, so within 2 B,
                # and the per-pixel values (sobel_ws) do not depend on the form at all
                B2 = 2 * R.loss_forward_ref(**i)[0][1]
                assert (np.abs(forms[False]["sums"] - forms[True]["sums"]) <= B2).all()
                assert same_bits(forms[False]["gws"], forms[True]["gws"])


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def adam_problem(n, gen):
    return K.adam_inputs(n, gen)


def adam_judge(state, got, step, H, mirror):
    """-> ({m, v, w: max err / B}, the mirror's worst ratio | nan).  Adam is elementwise, so the slab is judged in pieces of 2^20 elements
    on a few threads (numpy releases the interpreter lock): every element is still held to its own bound."""
    from concurrent.futures import ThreadPoolExecutor

    n = state["g"].shape[0]

    def piece(lo):
        sl = slice(lo, min(lo + 2 ** 20, n))
        part = {k: v[sl] for k, v in state.items()}
        ref = R.adam_ref(step=step, **part, **H)
        r = {k: R.ratio(got[k][sl], *ref[k]) for k in ref}
        m = worst({k: R.ratio(x, *ref[k]) for k, x in R.adam_mirror(step=step, **part, **H).items()}) if mirror else float("nan")
        return r, m

    with ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(piece, range(0, n, 2 ** 20)))
    return {k: max(p[0][k] for p in parts) for k in ("m", "v", "w")}, max(p[1] for p in parts)


@pytest.mark.parametrize("step", K.ADAM_STEPS)
@pytest.mark.parametrize("n", K.ADAM_LENGTHS)
def test_adam_one_step_at_a_time_within_the_bound(n, step):
    lib = L()
    tail = 61
    runs = [(K.ADAM_HYPER, "", gen) for gen in ("randn", "wide")]
    if n > 10 ** 6:                              # the large slab is about the loop over the grid, not the data: one generator per step, in turn
        runs = runs[K.ADAM_STEPS.index(step) % 2::2]
    if n == K.ADAM_SLOW_LENGTH:                  # the table whose second-moment correction is still alive at step 100000, and zero weights
        runs += [(K.ADAM_HYPER, "", "zero_w")] + [(K.ADAM_HYPER_SLOW, "slow beta2 ", gen) for gen in ("randn", "wide", "zero_w")]
    for H, hname, gen in runs:
        i = K.adam_inputs(n, gen) if n < 10 ** 6 else adam_problem(n, gen)
        pad = lambda a: torch.cat([torch.from_numpy(a), torch.full((tail,), -7.25, dtype=torch.float32)]).cuda()
        w, g, m, v = pad(i["w0"]), pad(i["g"]), pad(i["m0"]), pad(i["v0"])
        state = dict(i)
        for s in (step, step + 1) if n < 10 ** 6 else (step,):      # the second step starts from the m, v, w the kernel itself left
            rc = lib.lib().hvn_adam_step(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, H["lr"], H["b1"], H["b2"], H["eps"], s, stream())
            assert rc == 0, lib.lib().hvn_last_error()
            torch.cuda.synchronize()
            got = dict(w=host(w[:n]), m=host(m[:n]), v=host(v[:n]))
            r, mi = adam_judge(state, got, s, H, mirror=n < 10 ** 6)
            say("adam", "%sn %d %s step %d" % (hname, n, gen, s), worst(r), mi)
            assert worst(r) <= 1.0, r
            for t in (w, g, m, v):                # elements past n are untouched
                assert bool((t[n:] == -7.25).all())
            assert same_bits(host(g[:n]), state["g"])
            state = dict(w0=got["w"], m0=got["m"], v0=got["v"], g=state["g"])


# ---- refusals, over real buffers ----------------------------------------------------------------------------------------------------------
def test_mismatched_views_are_refused_and_nothing_is_written():
    lib = L()
    n, h, w, C = 2, 6, 4, 8
    bufs = [torch.full((n, h, w, C), float(k + 1), device="cuda") for k in range(4)]
    small = torch.full((n, h // 2, w // 2, C), 9.0, device="cuda")
    x64 = [torch.full((n, h, w, 64), float(k + 1), device="cuda") for k in range(2)]
    vec = [torch.full((64 * 16,), 0.5, device="cuda") for _ in range(6)]
    ws = torch.zeros(256 * 2 * C, dtype=torch.float64, device="cuda")
    everything = bufs + [small] + x64 + vec
    before = [host(t).copy() for t in everything]

    def refused(t, word, batch=n):
        rc = lib.lib().hvn_run_train_plan(ctypes.byref(t), 1, batch, stream())
        err = lib.lib().hvn_last_error()
        assert rc == -1 and word.encode() in err, (rc, err)

    def bn(kind):
        t = lib.hvn_top()
        t.kind, t.x, t.y, t.dy, t.dx, t.eps, t.momentum = kind, view_of(bufs[0]), view_of(bufs[1]), view_of(bufs[2]), view_of(bufs[3]), 1e-5, 0.1
        t.p[0] = ws.data_ptr()
        for k in range(1, 6):
            t.p[k] = vec[k].data_ptr()
        return t

    for kind, name, word in ((3, "y", "the a view"), (4, "y", "the a view"), (4, "dy", "the da view"), (4, "dx", "the dz view")):
        for field in ("h", "w", "c"):
            t = bn(kind)
            v = getattr(t, name)
            setattr(v, field, getattr(v, field) + (4 if field == "c" else 1))
            refused(t, word)
    t = bn(3)
    t.x.h = t.x.w = t.y.h = t.y.w = 1
    refused(t, "batch * h * w = 1 < 2", batch=1)
    t = lib.hvn_top()
    t.kind, t.dy = 7, view_of(bufs[0])
    refused(t, "both dlo and dskip are NULL")
    t.dx = view_of(bufs[1])                                           # a full-size dlo
    refused(t, "dlo must be (h / 2, w / 2, c) of dy")
    t.dx, t.y = view_of(small), view_of(small)
    refused(t, "dskip must be (h, w, c) of dy")
    t = lib.hvn_top()
    t.kind, t.cout, t.x, t.dx = 8, 5, view_of(x64[0]), view_of(x64[1])
    for k in range(4):
        t.p[k] = vec[k].data_ptr()
    t.dx.w += 1
    refused(t, "head backward: the dx view's extent")
    # a bad descriptor BEHIND a well-formed one: the whole list is checked first, so the well-formed op (which would add bufs[0] into
    # bufs[1]) does not run either
    good = lib.hvn_top()
    good.kind, good.dy, good.y = 7, view_of(bufs[0]), view_of(bufs[1])
    pair = (lib.hvn_top * 2)()
    for k, op in enumerate((good, t)):
        ctypes.memmove(ctypes.addressof(pair[k]), ctypes.addressof(op), ctypes.sizeof(lib.hvn_top))
    assert lib.lib().hvn_run_train_plan(pair, 2, n, stream()) == -1
    err = lib.lib().hvn_last_error()
    assert b"op 1" in err and b"head backward: the dx view's extent" in err, err
    torch.cuda.synchronize()
    assert all(same_bits(host(t), b) for t, b in zip(everything, before))

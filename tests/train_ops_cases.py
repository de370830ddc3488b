"""The cases and input generators shared by tests/test_train_ops_ref.py (CPU: mirrors and mutants against the bounds) and
tests/test_gpu_train_ops.py (the kernels against the same bounds) -- TEST INFRASTRUCTURE ONLY, numpy only.

Every shape is the smallest that reaches a path of csrc/hvn_train.hip; the comments say which, and test_train_ops_ref.py checks the
arithmetic against train_ops_ref.bn_grid and the launch functions' constants."""
import numpy as np

F32 = np.float32

# ---- BN: (C, n, h, w, crop) ----------------------------------------------------------------------------------------------------------
BN_CASES = [
    (4, 2, 3, 5, 0),          # lq = 1: 256 row lanes, one channel quad
    (12, 2, 9, 7, 0),         # lq = 2 over 3 quads: the second channel block is ragged
    (72, 1, 33, 33, 1),       # crop 1, 18 quads under lq = 16
    (2048, 2, 5, 5, 0),       # 8 channel blocks of 64 quads, 4 row lanes
    (64, 2, 182, 182, 0),     # 66248 rows > 65536: the partials cap at 256, 17 rows per thread = three 8-row passes, the last ragged
]
BN_GENERATORS = ("randn", "offset")


def bn_inputs(C, rows, gen, seed=0):
    """-> dict(z [rows][C], gamma, beta, rm, rv, eps, mom, da, dgamma0, dbeta0, dz0).  "offset": per-channel mean up to 10^3 std, and a
    beta that nearly cancels mean * scale in every second channel (the shift is then a small difference of large terms)."""
    r = np.random.default_rng(1000 + seed)
    gamma = r.uniform(0.5, 1.5, C).astype(F32)
    if gen == "randn":
        z = (r.standard_normal((rows, C)) * 2 + 0.5).astype(F32)
        beta = (r.standard_normal(C) * 0.3).astype(F32)
    else:
        std = r.uniform(0.5, 2.0, C)
        mean = std * 10.0 ** r.uniform(0, 3, C) * r.choice([-1.0, 1.0], C)
        z = (mean + std * r.standard_normal((rows, C))).astype(F32)
        beta = (r.standard_normal(C) * 0.3).astype(np.float64)
        beta[::2] += (mean * gamma / std)[::2]
        beta = beta.astype(F32)
    return dict(z=z, gamma=gamma, beta=beta, rm=r.standard_normal(C).astype(F32), rv=r.uniform(0.5, 1.5, C).astype(F32), eps=F32(1e-5), mom=F32(0.1),
                da=r.standard_normal((rows, C)).astype(F32), dgamma0=r.standard_normal(C).astype(F32), dbeta0=r.standard_normal(C).astype(F32),
                dz0=r.standard_normal((rows, C)).astype(F32))


def bn_zero_lattice(C, rows, seed=0):
    """Integer z = m_c + s d_c with sum s = 0 per channel: the double sums are exact, the mean is exactly m_c, and every row with s = 0 has
    the pre-activation fl(fl(m sc) + fl(beta - m sc)): zero, one ulp of the shift either side of it, or -- m = 0 -- beta itself, which is
    0, +-the smallest normal or +-2^-100 in those channels.  da: integers in [-8, 8]."""
    r = np.random.default_rng(2000 + seed)
    m = r.integers(-999, 1000, C).astype(np.float64)
    m[::5] = 0
    d = r.choice([1.0, 2.0, 5.0], C)
    s = np.zeros((rows, C))
    pat = np.array([0.0, 1.0, 0.0, -1.0])
    k = 4 * (rows // 4)
    s[:k] = np.tile(pat, rows // 4)[:, None]
    for c in range(C):
        s[:k, c] = s[r.permutation(k), c]
    z = (m + s * d).astype(F32)
    beta = np.zeros(C, F32)
    tiny = np.array([0.0, 2.0 ** -126, -2.0 ** -126, 2.0 ** -100, -2.0 ** -100], F32)
    beta[::5] = tiny[np.arange(len(beta[::5])) % 5]
    inp = bn_inputs(C, rows, "randn", seed)
    inp.update(z=z, beta=beta, da=r.integers(-8, 9, (rows, C)).astype(F32), dbeta0=np.zeros(C, F32))
    return inp


# ---- UPADD_BWD: (C, n, h, w) of dy; forms ----------------------------------------------------------------------------------------------
UPADD_CASES = [(4, 2, 2, 2), (72, 2, 8, 6)]
UPADD_FORMS = ("both", "dlo", "dskip")
UPADD_BIG = (256, 5, 256, 256)      # 5 * 128 * 128 * 64 = 5242880 channel quads > 16384 * 256: the grid-stride loop (lattice only)

# ---- HEAD_BWD: cout x (n, h, w) --------------------------------------------------------------------------------------------------------
HEAD_COUTS = (1, 5, 16)
HEAD_PIXELS = [(1, 1, 1), (1, 7, 9), (2, 19, 23), (2, 257, 257)]      # 1 | 63 < 64 | 874 = 3 groups + 106 | 132098 = 517 groups > 512 workgroups


def head_inputs(n, h, w, cout, lattice, seed=0):
    """-> dict(x, da0 [P][64], dl [P][cout], w, dW0 [cout][64], db0 [cout]), P = n h w pixels in n, y, x order.  lattice: small integers
    with every sum below 2^24 (x, dl in [-3, 3]: |sum| <= 9 P)."""
    r = np.random.default_rng(3000 + seed)
    P = n * h * w
    if lattice:
        gi = lambda lo, hi, *s: r.integers(lo, hi + 1, s).astype(F32)
        return dict(x=gi(-3, 3, P, 64), da0=gi(-9, 9, P, 64), dl=gi(-3, 3, P, cout), w=gi(-4, 4, cout, 64), dW0=gi(-9, 9, cout, 64), db0=gi(-9, 9, cout))
    gn = lambda *s: r.standard_normal(s).astype(F32)
    return dict(x=gn(P, 64), da0=gn(P, 64), dl=gn(P, cout), w=gn(cout, 64), dW0=gn(cout, 64), db0=gn(cout))


# ---- CONV0_WGRAD: (n, H, W, pad, window) -------------------------------------------------------------------------------------------------
CONV0_CASES = [
    (2, 7, 7, 0, False),       # a 1 x 1 output
    (2, 22, 22, 0, False),     # exactly one 16 x 16 tile
    (1, 23, 39, 0, False),     # 17 x 33 output: ragged tiles in both axes
    (2, 8, 8, 3, False),       # padding on every side of an 8 x 8 output
    (2, 23, 39, 3, True),      # ragged tiles with padding, the image a window of a larger one
    (33, 70, 70, 0, False),    # 64 x 64 output x 33: 528 tiles > 512 workgroups
]


def conv0_inputs(n, H, W, pad, lattice, seed=0):
    """-> dict(img [n][H][W][3] uint8, dz [n][ho][wo][64], dW0 [64][7][7][3]).  lattice: image bytes in {0, 255} (255 fl(1 / 255) == 1.0f) and
    integer dz in [-3, 3]: every sum an integer below 2^24."""
    r = np.random.default_rng(4000 + seed)
    ho, wo = H + 2 * pad - 6, W + 2 * pad - 6
    if lattice:
        return dict(img=(r.integers(0, 2, (n, H, W, 3)) * 255).astype(np.uint8), dz=r.integers(-3, 4, (n, ho, wo, 64)).astype(F32),
                    dW0=r.integers(-9, 10, (64, 7, 7, 3)).astype(F32))
    return dict(img=r.integers(0, 256, (n, H, W, 3)).astype(np.uint8), dz=r.standard_normal((n, ho, wo, 64)).astype(F32),
                dW0=r.standard_normal((64, 7, 7, 3)).astype(F32))


# ---- loss: (n, h, w) x nr_types x generator x map ----------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1, 1), (1, 3, 4), (2, 5, 7), (3, 37, 53)]          # below the 5 x 5 Sobel window; 5883 pixels = 22 groups + 251
LOSS_TYPES = (0, 1, 2, 16)
LOSS_GENERATORS = ("randn", "tied", "sat40", "sat100")
LOSS_MAPS = ("mixed", "background", "foreground", "absent")
LOSS_WEIGHTS = {"ones": (1, 1, 1, 1, 1, 1), "table": (2.0, 0.5, 1.5, 0.25, 0.0, 3.0), "np_msge": (0.3, 0.0, 0.0, 2.0, 0.0, 0.0)}


def loss_inputs(n, h, w, T, gen, kind, seed=0):
    """-> dict(l_np, l_hv [n][2][h][w], l_tp [n][T][h][w] | None, t_np, t_tp int32 [n][h][w], t_hv [n][h][w][2]).
    tied: every second pixel has equal logits in all classes; sat40 / sat100: every second pixel has one class at +x and the others at
    -x, whatever its label (so the true class is as often the saturated-away one).  Maps: mixed | all background | all foreground |
    absent (type class 1 -- the last one of two -- never occurs)."""
    r = np.random.default_rng(5000 + seed)
    gn = lambda *s: r.standard_normal(s).astype(F32)
    l_np, l_hv = gn(n, 2, h, w) * 2, gn(n, 2, h, w)
    l_tp = gn(n, T, h, w) * 2 if T else None
    alt = (np.arange(n * h * w).reshape(n, h, w) % 2 == 0)
    for l in [l_np] + ([l_tp] if T else []):
        c = l.shape[1]
        if gen == "tied":
            l[:] = np.where(alt[:, None], l[:, :1], l)
        elif gen in ("sat40", "sat100"):
            x = 40.0 if gen == "sat40" else 100.0
            hot = r.integers(0, c, (n, h, w))
            sat = np.where(np.arange(c)[None, :, None, None] == hot[:, None], x, -x).astype(F32)
            l[:] = np.where(alt[:, None], sat, l)
    t_np = r.integers(0, 2, (n, h, w)).astype(np.int32)
    t_tp = r.integers(0, max(T, 1), (n, h, w)).astype(np.int32)
    if kind == "background":
        t_np[:], t_tp[:] = 0, 0
    elif kind == "foreground":
        t_np[:] = 1
    elif kind == "absent" and T > 1:
        t_tp[t_tp == 1] = 0
    return dict(l_np=l_np, l_hv=l_hv, l_tp=l_tp, t_np=t_np, t_tp=t_tp if T else None, t_hv=gn(n, h, w, 2))


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
ADAM_LENGTHS = (1, 3, 4, 5, 1023, 1027, 8192 * 1024 + 1027)         # the scalar tail alone; vectors + tails; more than 8192 workgroups' worth
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_HYPER = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)
# A bias correction 1 - beta^step differs from 1 at step 100000 only where beta^100000 is not negligible: with the betas above it is 0
# (0.9) and 4e-44 (0.999), so HOW the corrections are formed cannot show at that step.  The second table keeps the correction of the
# second moment alive there: beta2 = 1 - 2^-20, an fp32 number (the float32 beta adds no error of its own), beta2^100000 = 0.909.
ADAM_HYPER_SLOW = dict(lr=1e-4, b1=0.9, b2=1.0 - 2.0 ** -20, eps=1e-8)
ADAM_SLOW_LENGTH = 1027                                              # the length the second table runs at


def adam_inputs(n, gen, seed=0):
    """-> dict(w0, g, m0, v0).  randn | "wide": gradient magnitudes log-uniform over 1e-14 .. 10, and a state of the same range | "zero_w":
    randn with every weight 0 (fresh biases): the update is then the whole of w, and B is relative to the update alone."""
    if gen == "zero_w":
        return dict(adam_inputs(n, "randn", seed), w0=np.zeros(n, F32))
    r = np.random.default_rng(6000 + seed)
    sn = lambda: r.standard_normal(n)
    if gen == "randn":
        return dict(w0=sn().astype(F32), g=sn().astype(F32), m0=(0.1 * sn()).astype(F32), v0=(0.01 * sn() ** 2).astype(F32))
    mag = lambda: 10.0 ** r.uniform(-14, 1, n)
    return dict(w0=sn().astype(F32), g=(mag() * r.choice([-1.0, 1.0], n)).astype(F32), m0=(mag() * r.choice([-1.0, 1.0], n)).astype(F32),
                v0=(mag() ** 2).astype(F32))

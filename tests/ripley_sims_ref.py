"""The oracle of the random-labelling test of hover_net_amd/ripley.py: the hash, the round keys, the Feistel bijection and the cycle
walk one value at a time in Python integers (reduced modulo 2^64 by hand), and per simulation the all-pairs oracle tests/ripley_ref.py
on the permuted types -- no arrays in the permutation, no shared geometry, no difference array."""
import functools

import numpy as np

import ripley_ref as R

M64 = (1 << 64) - 1


def mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def keys(seed, s):
    """The eight round keys of simulation s."""
    base = mix((seed + 0x9E3779B97F4A7C15 * (s + 1)) & M64)
    return [mix((base + p) & M64) for p in range(8)]


def feistel(x, key, hl, hh):
    lo, hi = x & ((1 << hl) - 1), x >> hl
    for p in range(8):
        if p % 2 == 0:
            hi ^= mix((lo + key[p]) & M64) & ((1 << hh) - 1)
        else:
            lo ^= mix((hi + key[p]) & M64) & ((1 << hl) - 1)
    return (hi << hl) | lo


def permutation(n, key):
    """-> (pi as a list of n ints, the longest walk)."""
    b = max(2, (n - 1).bit_length())
    hl = b // 2
    out, longest = [], 0
    for i in range(n):
        x, steps = feistel(i, key, hl, b - hl), 1
        while x >= n:
            x, steps = feistel(x, key, hl, b - hl), steps + 1
        out.append(x)
        longest = max(longest, steps)
    return out, longest


def sims(xy, types, radii, window, nr_types, nsim, seed):
    """-> (pairs_in [S, T, T, R], n_in [S, T, R]) int64: `ripley_ref.pairs` of the types permuted by pi_s, per simulation."""
    n = np.asarray(xy).shape[0]
    base = np.zeros(n, np.int64) if types is None else np.asarray(types, np.int64)
    seen, res = {}, []
    for s in range(nsim):
        lab = base[np.array(permutation(n, keys(seed, s))[0], np.int64)]
        if lab.tobytes() not in seen:                           # the same labels (untyped points: always) are counted once
            seen[lab.tobytes()] = R.pairs(xy, lab, radii, window, nr_types)
        res.append(seen[lab.tobytes()])
    return np.stack([r[1] for r in res]), np.stack([r[3] for r in res])


SIMS = 7                    # the relabellings of every case, seed 0; simulation s does not depend on S, so fewer are a prefix


@functools.lru_cache(maxsize=None)
def _case(name):
    args, _ = R.case(name)
    want = sims(*args, SIMS, 0)
    for a in want:
        a.setflags(write=False)
    return args, want


def case(name, nsim):
    """(args, oracle result) of a case of tests/ripley_ref.py under its first `nsim` <= SIMS relabellings with seed 0; built once per
    process and shared: treat both as read-only."""
    args, want = _case(name)
    assert 1 <= nsim <= SIMS
    return args, tuple(a[:nsim] for a in want)


def assert_same(got, want, what=""):
    """The simulated arrays of a LabelSims against the oracle's two, with ==."""
    for name, g, w in zip(("pairs_in", "n_in"), (got.pairs_in, got.n_in), want):
        assert isinstance(g, np.ndarray) and g.dtype == np.int64 and g.shape == w.shape, (what, name, getattr(g, "dtype", None), getattr(g, "shape", None))
        assert (g == w).all(), (what, name, np.argwhere(g != w)[:5].tolist())

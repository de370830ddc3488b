"""Test-time augmentation over the dihedral group of the square: the one definition of the views and of the rule for the HV field.

View k = r + 4 f (f in {0, 1}, r in 0..3) of an array `a` with two leading spatial axes is

    view_k(a) = np.rot90(a[:, ::-1] if f else a, r, axes=(0, 1))

-- the left-right flip first, then r counter-clockwise quarter turns.  A field u of (h, v) vectors transforms as view_k(u) with every
vector multiplied by M_k = R^r F^f, F = diag(-1, 1) (the flip negates the horizontal component), R = [[0, 1], [-1, 0]] (a quarter
turn sends "right" to "up", i.e. h to -v, and "down" to "right", i.e. v to h).  Every M_k is a signed permutation, so applying it or
its transpose is exact in fp32.  The network's answer on view k therefore comes back as

    p(i, j) = p_k(view_k's place of (i, j)),        (h, v)(i, j) = M_k^T (h_k, v_k)(that place),

which is what HVN_OP_TTA (csrc/hvn_tta.hip) accumulates; HVN_OP_VIEW makes the views of the uint8 patches.  numpy only: the host
side of `Engine.run_tta` and the reference point of the tests."""
import numpy as np

N_VIEWS = 8
SETS = {
    "flips": (0, 4, 6, 2),      # identity, left-right, up-down, half turn: no transposition
    "rot": (0, 1, 2, 3),        # the four quarter turns
    "d4": (0, 1, 2, 3, 4, 5, 6, 7),
}
_F = np.array([[-1, 0], [0, 1]], np.int64)
_R = np.array([[0, 1], [-1, 0]], np.int64)


def views(tta):
    """The tuple of view ids a `tta` argument names: a set name or a non-empty sequence of distinct ids in 0..7 (order kept: it is
    the summation order).  ValueError otherwise; None -> None (no augmentation)."""
    if tta is None:
        return None
    if isinstance(tta, str):
        if tta not in SETS:
            raise ValueError("tta=%r: unknown view set (known: %s)" % (tta, ", ".join(sorted(SETS))))
        return SETS[tta]
    try:
        ids = tuple(tta)
    except TypeError:
        raise ValueError("tta=%r: a set name (%s) or a tuple of view ids" % (tta, ", ".join(sorted(SETS)))) from None
    if not ids:
        raise ValueError("tta=(): at least one view")
    for k in ids:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < N_VIEWS:
            raise ValueError("tta=%r: view id %r outside 0..7" % (tta, k))
    ids = tuple(int(k) for k in ids)
    if len(set(ids)) != len(ids):
        raise ValueError("tta=%r: a view id is repeated" % (tta,))
    return ids


def view(a, k):
    """view_k of an array whose first two axes are the spatial ones."""
    a = np.asarray(a)
    return np.rot90(a[:, ::-1] if k & 4 else a, k & 3, axes=(0, 1))


def matrix(k):
    """M_k as a 2 x 2 integer matrix acting on (h, v) columns."""
    m = _F if k & 4 else np.eye(2, dtype=np.int64)
    for _ in range(k & 3):
        m = _R @ m
    return m


def view_field(u, k):
    """view_k of a field [h][w][2] of (h, v) vectors: the view of the map, every vector multiplied by M_k."""
    return view(u, k) @ matrix(k).T.astype(np.asarray(u).dtype)


def inverse(k):
    """The id g with view_g(view_k(a)) == a: a flipped view is its own inverse, a rotation's is the opposite rotation."""
    return k if k & 4 else (4 - k) & 3


def compose(k, g):
    """The id m with view_k(view_g(a)) == view_m(a).  With s the flip and t the quarter turn, s t = t^-1 s, so
    t^rk s^fk t^rg s^fg = t^(rk - rg) s^(fk + fg) if fk else t^(rk + rg) s^fg: the inner turns change sign when the outer view flips."""
    rk, fk, rg, fg = k & 3, k >> 2, g & 3, g >> 2
    r = (rk - rg) & 3 if fk else (rk + rg) & 3
    return r + 4 * (fk ^ fg)


COMPOSE = tuple(tuple(compose(k, g) for g in range(N_VIEWS)) for k in range(N_VIEWS))     # COMPOSE[k][g]: view_k o view_g

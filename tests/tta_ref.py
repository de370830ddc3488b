"""Oracle for the test-time augmentation (numpy only, written independently of hover_net_amd/tta.py and of the kernels) -- TEST
INFRASTRUCTURE ONLY.

View k = r + 4 f: the left-right flip if f, then r counter-clockwise quarter turns (`view`).  A field of (h, v) vectors
transforms as the view with every vector multiplied by `M(k)`.  `reduce_f32` is HVN_OP_TTA's contract in float32 numpy, one term
per view in the order given, summed in that order; `reduce_f64` the same in float64.  Their exponentials are numpy's, not the
device's: only the hv channels (no exponential) are bit-equal to the device."""
import numpy as np


def view(a, k):
    """The view of an array with two leading spatial axes, from index arithmetic (no rot90 / flip)."""
    a = np.asarray(a)
    f, r = divmod(k, 4)
    H, W = a.shape[:2]
    Ho, Wo = (W, H) if r & 1 else (H, W)
    i, j = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    # b = flipped a; out[i, j] = b[...] by quarter turn
    if r == 0:
        sy, sx = i, j
    elif r == 1:
        sy, sx = j, W - 1 - i
    elif r == 2:
        sy, sx = H - 1 - i, W - 1 - j
    else:
        sy, sx = H - 1 - j, i
    if f:
        sx = W - 1 - sx
    return a[sy, sx]


# written out, not multiplied: rows act on (h, v) columns
_M = {
    0: [[1, 0], [0, 1]],
    1: [[0, 1], [-1, 0]],
    2: [[-1, 0], [0, -1]],
    3: [[0, -1], [1, 0]],
    4: [[-1, 0], [0, 1]],
    5: [[0, 1], [1, 0]],
    6: [[1, 0], [0, -1]],
    7: [[0, -1], [-1, 0]],
}


def M(k):
    return np.array(_M[k], np.int64)


SIGNED_PERMUTATIONS = [np.array(m, np.int64) for m in
                       ([[1, 0], [0, 1]], [[1, 0], [0, -1]], [[-1, 0], [0, 1]], [[-1, 0], [0, -1]],
                        [[0, 1], [1, 0]], [[0, 1], [-1, 0]], [[0, -1], [1, 0]], [[0, -1], [-1, 0]])]


def _apply(m, h, v):
    """(m @ (h, v)) for a signed permutation, by selection and negation (exact, no 0 * x terms)."""
    out = []
    for row in m:
        c = 0 if row[0] else 1
        src = (h, v)[c]
        out.append(src if row[c] > 0 else -src)
    return out


def field_view(u, k, m=None):
    """view_k of a field [H][W][2] with every vector multiplied by m (default M(k))."""
    uv = view(u, k)
    h, v = _apply(M(k) if m is None else m, uv[..., 0], uv[..., 1])
    return np.stack([h, v], -1)


def _unview(a, k):
    """The map whose view k is `a`: out[i, j] = a[where view_k sends (i, j)]."""
    H, W = (a.shape[1], a.shape[0]) if k & 1 else a.shape[:2]
    idx = np.arange(H * W).reshape(H, W)
    where = np.empty(H * W, np.int64)
    where[view(idx, k).ravel()] = np.arange(H * W)          # view(idx)[p, q] = original flat index shown at (p, q)
    return a.reshape((-1,) + a.shape[2:])[where].reshape((H, W) + a.shape[2:])


def _terms(logits, k, dtype):
    """One view's term in the original orientation: (p_np [n,H,W], hv [n,H,W,2], p_t [n,H,W,T] or None)."""
    np_l = np.asarray(logits["np"], dtype)
    hv_l = np.asarray(logits["hv"], dtype)
    m = np.maximum(np_l[:, 0], np_l[:, 1])
    e0, e1 = np.exp(np_l[:, 0] - m), np.exp(np_l[:, 1] - m)
    p = e1 / (e0 + e1)
    h, v = _apply(M(k).T, hv_l[:, 0], hv_l[:, 1])
    pt = None
    if logits.get("tp") is not None:
        tp_l = np.asarray(logits["tp"], dtype)
        tm = tp_l.max(1)
        e = [np.exp(tp_l[:, t] - tm) for t in range(tp_l.shape[1])]
        s = np.zeros_like(e[0])
        for t in range(len(e)):                         # ascending, one add at a time (np.sum would add pairwise)
            s = s + e[t]
        pt = np.stack([e[t] / s for t in range(len(e))], -1)
    back = lambda a: np.stack([_unview(x, k) for x in a])      # noqa: E731
    return back(p), np.stack([back(h), back(v)], -1), (None if pt is None else back(pt))


def _reduce(per_view, views, dtype):
    assert len(per_view) == len(views)
    acc = None
    terms = []
    for logits, k in zip(per_view, views):
        t = _terms(logits, k, dtype)
        terms.append(t)
        acc = list(t) if acc is None else [None if a is None else a + b for a, b in zip(acc, t)]
    K = dtype(len(views))
    out = {"np": acc[0] / K, "hv": acc[1] / K, "acc_np": acc[0], "acc_hv": acc[1], "terms": terms}
    if acc[2] is not None:
        out["acc_tp"] = acc[2]
        out["tp"] = acc[2] / K
        out["type"] = np.argmax(out["tp"], -1)          # first maximum
    return out


def reduce_f32(per_view, views):
    """per_view: one dict {"np": [n,2,h,w], "hv": [n,2,h,w], "tp": [n,T,h,w] or absent} per view, in the VIEW's orientation ->
    {"np", "hv", "tp", "type", "acc_*", "terms"} in the original orientation, every operation in float32, views summed in order."""
    return _reduce(per_view, views, np.float32)


def reduce_f64(per_view, views):
    return _reduce(per_view, views, np.float64)


def top2_gap(p):
    """The difference of the two largest entries along the last axis."""
    s = np.sort(p, -1)
    return s[..., -1] - s[..., -2]

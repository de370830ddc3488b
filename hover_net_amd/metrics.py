"""Instance-segmentation metrics of the reference's metrics/stats_utils.py, scored from one exact integer object per image.

Every score that `compute_stats.py run_nuclei_inst_stat` records -- Dice 1, AJI, DQ / SQ / PQ, AJI+ -- and Dice 2 is a function of
the PAIR TABLE of an image: the pixel count of every distinct (true id, pred id) pair, background pairs with one side 0 included
(they give the areas and the Dice-1 counts).  The table is built on the device (`hvn_pair_table`, csrc/hvn_metrics.hip: one pass
over the two int32 maps, integer atomics only) or on the host (`host_triples`: `np.unique` of an int64 key, the yardstick of the
GPU tests); only the K triples (a few times the instance count) leave the device.  All floating-point arithmetic then happens here,
in numpy, from the exact integers and in the reference's expression order -- PQ IoU = inter / (total - inter), AJI IoU =
inter / (union + 1e-6), SQ = the paired IoUs summed in row-major (t, p) order / (tp + 1e-6), the same dense float64 matrices
for `linear_sum_assignment` -- so the results EQUAL the reference's, container kinds included.

Where the reference's result is undefined this module raises ValueError instead: `get_fast_*` on ids that are not 1..n
(the reference indexes its masks by id and scores the wrong ones or raises IndexError) or on a map without a background pixel
(it drops the smallest id as if it were 0); negative labels; values outside the int32 range (every function).

Float label maps (MATLAB ground truth is often double) are accepted when every value is a whole number: remap_label, get_dice_1
and get_dice_2 score them as the reference does.  The get_fast_* functions raise TypeError on a float map that holds an instance:
the reference indexes Python lists of masks by the float ids and fails the same way (in a few degenerate cases, e.g. a float
true map without instances, it still returns a value; here it is TypeError throughout).  Call remap_label first, as
compute_stats.py does.  A map of any shape is scored as ONE map, as in the reference (a [N, H, W] stack passed to a reference-named
function is one map of N * H * W pixels; `instance_stats` and `pair_tables` are the per-image batched forms).

Every function takes numpy arrays or torch tensors and a keyword-only `device`: None = the CUDA device of a CUDA input, else
CUDA when available, else the host; "cpu" forces the host path.
"""
import sys

import numpy as np

INT32_MAX = 2 ** 31 - 1
WORKSPACE_BUDGET = 1 << 30      # device bytes one group of maps may use (workspace + outputs); a single map may exceed it


# ------------------------------------------------------------------------------------------------------------- inputs / device
def _is_tensor(x):
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


def _resolve_device(device, *xs):
    import torch

    if device is not None:
        d = torch.device(device)
        return None if d.type == "cpu" else d
    for x in xs:
        if _is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None


def _np_dtype(x):
    if _is_tensor(x):
        import torch

        return torch.empty(0, dtype=x.dtype).numpy().dtype
    return np.asarray(x).dtype


def _host_map(x):
    """numpy view of a label map, checked: whole-number labels (integer, bool or float dtype), none negative, none above the
    int32 range."""
    a = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    if a.dtype.kind not in "iubf":
        raise ValueError("label maps must hold whole numbers (got %s)" % a.dtype)
    if a.size:
        if a.dtype.kind == "f" and not np.all(np.isfinite(a) & (a == np.floor(a))):
            raise ValueError("float label maps must hold whole numbers")
        if a.dtype.kind in "if" and a.min() < 0:
            raise ValueError("negative labels are not instance ids")
        if a.max() > INT32_MAX:
            raise ValueError("labels above the int32 range")
    return a


def _device_maps(x, dev):
    """int32 CUDA tensor of `x` on `dev`, contiguous, with leading image axis (labels beyond int32 raise)."""
    import torch

    t = x if _is_tensor(x) else torch.from_numpy(np.ascontiguousarray(_host_map(x)))
    if t.dtype != torch.int32:
        if t.dtype.is_complex:
            raise ValueError("label maps must hold whole numbers (got %s)" % t.dtype)
        if t.dtype.is_floating_point and t.numel() and not bool((torch.isfinite(t) & (t == t.floor())).all()):
            raise ValueError("float label maps must hold whole numbers")
        if t.numel() and (float(t.min()) < 0 or float(t.max()) > INT32_MAX):
            raise ValueError("labels outside [0, int32 max]")
        t = t.to(torch.int32)
    return t.to(dev).contiguous()


# ------------------------------------------------------------------------------------------------------------------ the tables
class PairTable:
    """The pair table of one image: `t`, `p`, `count` (int64 [K]) = every distinct (true id, pred id) pair other than (0, 0)
    with its pixel count, sorted by (t, p); `pixels` = h * w; `dtype` / `pdtype` = the numpy dtypes of the true / pred map (the
    reference's id lists hold numpy scalars of them)."""

    __slots__ = ("t", "p", "count", "pixels", "dtype", "pdtype")

    def __init__(self, triples, pixels, dtype=np.dtype(np.int32), pdtype=None):
        tr = np.asarray(triples, np.int64).reshape(-1, 3)
        if len(tr) and (tr[:, :2] < 0).any():
            raise ValueError("negative labels are not instance ids")
        order = np.lexsort((tr[:, 1], tr[:, 0]))
        self.t, self.p, self.count = (np.ascontiguousarray(tr[order, k]) for k in range(3))
        self.pixels = int(pixels)
        self.dtype = np.dtype(dtype)
        self.pdtype = self.dtype if pdtype is None else np.dtype(pdtype)

    @property
    def triples(self):
        return np.stack([self.t, self.p, self.count], 1)

    @property
    def background_pixels(self):
        """pixels whose pair is (0, 0)"""
        return self.pixels - int(self.count.sum())

    def _areas(self, ids):
        u, inv = np.unique(ids, return_inverse=True)
        a = np.zeros(len(u), np.int64)
        np.add.at(a, inv, self.count)
        n00 = self.background_pixels
        if n00 and (len(u) == 0 or u[0] != 0):
            u, a = np.concatenate([[0], u]), np.concatenate([[0], a])
        if n00:
            a[0] += n00
        return u.astype(np.int64), a

    def true_areas(self):
        """(ids, areas) of the true map, ascending ids, background included when present"""
        return self._areas(self.t)

    def pred_areas(self):
        return self._areas(self.p)

    def ranked(self):
        """The table of remap_label(true), remap_label(pred) (by_size=False): ids replaced by their rank among the nonzero ids.
        Raises ValueError where remap_label does (a map with labels but no background)."""
        out = PairTable.__new__(PairTable)
        out.pixels, out.dtype, out.pdtype, out.count = self.pixels, np.dtype(np.int32), np.dtype(np.int32), self.count
        for side in ("t", "p"):
            ids, _ = (self.true_areas if side == "t" else self.pred_areas)()
            v = getattr(self, side)
            if len(ids) and ids[-1] > 0 and ids[0] != 0:
                raise ValueError("remap_label: the map has no background (id 0)")
            nz = ids[ids > 0]
            setattr(out, side, np.where(v > 0, np.searchsorted(nz, v) + 1, 0).astype(np.int64))
        return out


def host_triples(true, pred):
    """The pair table of one image in numpy: (t, p, count) int64 [K, 3] sorted by (t, p), from `np.unique` of t << 32 | p."""
    t, p = _host_map(true), _host_map(pred)
    if t.shape != p.shape:
        raise ValueError("true and pred differ in shape: %s vs %s" % (t.shape, p.shape))
    key = (t.astype(np.int64).ravel() << 32) | p.astype(np.int64).ravel()
    u, c = np.unique(key[key != 0], return_counts=True)
    return np.stack([u >> 32, u & 0xFFFFFFFF, c.astype(np.int64)], 1)


def device_triples(true, pred, dev=None):
    """The pair tables of [n, h, w] map pairs built on the GPU (hvn_pair_table), in groups that fit WORKSPACE_BUDGET: a list of
    n int64 [K_i, 3] arrays in the kernel's (non-canonical) order.  Only the triples are copied to the host."""
    import torch

    from . import lib as L

    dev = dev if dev is not None else _resolve_device(None, true, pred)
    tt, pt = _device_maps(true, dev), _device_maps(pred, dev)
    if tt.dim() == 2:
        tt, pt = tt[None], pt[None]
    if tt.shape != pt.shape or tt.dim() != 3:
        raise ValueError("true and pred must both be [n, h, w] (or [h, w]) of one shape: %s vs %s" % (tuple(tt.shape), tuple(pt.shape)))
    n, h, w = tt.shape
    if n == 0:
        return []
    per = L.lib().hvn_pair_table_workspace_bytes(1, h, w) + 12 * h * w
    g = max(1, min(n, 65535, WORKSPACE_BUDGET // max(per, 1)))
    out = []
    with torch.cuda.device(dev):
        for i0 in range(0, n, g):
            m = min(g, n - i0)
            need = L.lib().hvn_pair_table_workspace_bytes(m, h, w)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            tri = torch.empty((m, h * w, 3), dtype=torch.int32, device=dev)
            cnt = torch.empty(m, dtype=torch.int32, device=dev)
            L.call("hvn_pair_table", tt[i0:i0 + m].data_ptr(), pt[i0:i0 + m].data_ptr(), m, h, w, tri.data_ptr(), cnt.data_ptr(),
                   ws.data_ptr(), need, L.stream_ptr(dev))
            k = cnt.cpu().numpy().astype(np.int64)
            flat = torch.cat([tri[j, :int(k[j])] for j in range(m)]).cpu().numpy().astype(np.int64)
            del ws, tri
            out += np.split(flat, np.cumsum(k)[:-1])
    return out


def pair_tables(true, pred, *, device=None):
    """Public: the PairTable of every image pair.  `true` / `pred`: [h, w] or [n, h, w] arrays / tensors, or equal-length lists
    of [h, w] maps (shapes may differ between images; one device pass per group of equal shape)."""
    dev = _resolve_device(device, true, pred)
    tl, pl = _as_list(true), _as_list(pred)
    if len(tl) != len(pl):
        raise ValueError("%d true maps, %d pred maps" % (len(tl), len(pl)))
    dtypes = [(_np_dtype(t), _np_dtype(p)) for t, p in zip(tl, pl)]
    shapes = [tuple(t.shape) for t in tl]
    for t, p in zip(tl, pl):
        if tuple(t.shape) != tuple(p.shape):
            raise ValueError("true and pred differ in shape: %s vs %s" % (tuple(t.shape), tuple(p.shape)))
    if dev is not None and not isinstance(true, (list, tuple)) and getattr(true, "ndim", 0) == 3:
        n, h, w = true.shape                              # one [N, H, W] batch: straight to the device, no restacking
        return [PairTable(tr, h * w, *dtypes[0]) for tr in device_triples(true, pred, dev)]
    out = [None] * len(tl)
    if dev is None:
        for i, (t, p) in enumerate(zip(tl, pl)):
            out[i] = PairTable(host_triples(t, p), int(np.prod(shapes[i])), *dtypes[i])
        return out
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    for s, idx in groups.items():
        if len(s) != 2:
            raise ValueError("maps must be 2-D, got shape %s" % (s,))
        tb, pb = _stack([tl[i] for i in idx], dev), _stack([pl[i] for i in idx], dev)
        for i, tr in zip(idx, device_triples(tb, pb, dev)):
            out[i] = PairTable(tr, s[0] * s[1], *dtypes[i])
    return out


def _as_list(x):
    if isinstance(x, (list, tuple)):
        return list(x)
    if _is_tensor(x) or isinstance(x, np.ndarray):
        return [x] if x.ndim == 2 else [x[i] for i in range(x.shape[0])]
    return [np.asarray(x)]


def _stack(maps, dev):
    import torch

    if all(_is_tensor(m) for m in maps):
        return torch.stack([_device_maps(m, dev) for m in maps])
    return _device_maps(np.stack([_host_map(m) for m in maps]), dev)


def _table(true, pred, device):
    """The table of ONE map pair, whatever the arrays' shape (the reference's functions treat any array as one map)."""
    true, pred = (x if _is_tensor(x) else np.asarray(x) for x in (true, pred))
    if true.ndim != 2 or pred.ndim != 2:
        if tuple(true.shape) != tuple(pred.shape):
            raise ValueError("true and pred differ in shape: %s vs %s" % (tuple(true.shape), tuple(pred.shape)))
        true, pred = true.reshape(1, -1), pred.reshape(1, -1)
    if true.shape[1] == 0:
        device = "cpu"                                    # no pixel: nothing to launch
    return pair_tables(true, pred, device=device)[0]


# ------------------------------------------------------------------------------------------------------------------ scoring
class _Scored:
    """Dense per-pair quantities of a table whose ids are 1..T and 1..P (validated)."""

    def __init__(self, tab, what):
        tid, tarea = tab.true_areas()
        pid, parea = tab.pred_areas()
        for ids, dt in ((tid, tab.dtype), (pid, tab.pdtype)):
            if dt.kind == "f" and len(ids) and ids[-1] > 0:
                raise TypeError("%s: float ids cannot index the reference's mask lists (call remap_label first)" % what)
        for ids in (tid, pid):
            if len(ids) and ids[0] != 0:
                raise ValueError("%s: a map without background (id 0) is undefined in the reference" % what)
            nz = ids[1:] if len(ids) else ids
            if len(nz) and (nz[0] != 1 or nz[-1] != len(nz)):
                raise ValueError("%s needs contiguous ids 1..n (call remap_label first)" % what)
        self.T, self.P = max(len(tid) - 1, 0), max(len(pid) - 1, 0)
        self.tarea, self.parea = tarea, parea             # index = id (0 = background)
        m = (tab.t > 0) & (tab.p > 0)
        self.ti, self.pi, self.inter = tab.t[m], tab.p[m], tab.count[m]
        self.total = self.tarea[self.ti] + self.parea[self.pi]
        self.ids_t = [tab.dtype.type(i) for i in range(1, self.T + 1)]
        self.ids_p = [tab.pdtype.type(i) for i in range(1, self.P + 1)]

    def dense(self, values):
        d = np.zeros([self.T, self.P], dtype=np.float64)
        d[self.ti - 1, self.pi - 1] = values
        return d

    def unpaired_area(self, paired_t, paired_p):
        st, sp = set(int(i) for i in paired_t), set(int(i) for i in paired_p)
        ut = [i for i in range(1, self.T + 1) if i not in st]
        up = [i for i in range(1, self.P + 1) if i not in sp]
        return int(self.tarea[ut].sum()) + int(self.parea[up].sum())


def _lsa():
    from scipy.optimize import linear_sum_assignment

    return linear_sum_assignment


def pq_from_table(tab, match_iou=0.5):
    assert match_iou >= 0.0, "Cant' be negative"
    s = _Scored(tab, "get_fast_pq")
    iou = s.inter / (s.total - s.inter)
    if match_iou >= 0.5:
        keep = iou > match_iou                            # the table is in row-major (t, p) order, as np.nonzero is
        paired_true, paired_pred, paired_iou = s.ti[keep].astype(np.intp), s.pi[keep].astype(np.intp), iou[keep]
    else:
        dense = s.dense(iou)
        rows, cols = _lsa()(-dense)
        piou = dense[rows, cols]
        keep = piou > match_iou
        paired_true, paired_pred, paired_iou = list(rows[keep] + 1), list(cols[keep] + 1), piou[keep]
    st, sp = set(int(i) for i in paired_true), set(int(i) for i in paired_pred)
    unpaired_true = [i for i in s.ids_t if int(i) not in st]
    unpaired_pred = [i for i in s.ids_p if int(i) not in sp]
    tp, fp, fn = len(paired_true), len(unpaired_pred), len(unpaired_true)
    dq = tp / (tp + 0.5 * fp + 0.5 * fn)
    sq = paired_iou.sum() / (tp + 1.0e-6)
    return [dq, sq, dq * sq], [paired_true, paired_pred, unpaired_true, unpaired_pred]


def aji_from_table(tab):
    s = _Scored(tab, "get_fast_aji")
    inter, union = s.dense(s.inter), s.dense(s.total - s.inter)
    iou = inter / (union + 1.0e-6)
    best = np.argmax(iou, axis=1)                         # ties: smallest pred id; one pred may serve several true instances
    paired_true = np.nonzero(np.max(iou, axis=1) > 0.0)[0]
    paired_pred = best[paired_true]
    overall_inter = inter[paired_true, paired_pred].sum()
    overall_union = union[paired_true, paired_pred].sum() + s.unpaired_area(paired_true + 1, paired_pred + 1)
    return overall_inter / overall_union


def aji_plus_from_table(tab):
    s = _Scored(tab, "get_fast_aji_plus")
    inter, union = s.dense(s.inter), s.dense(s.total - s.inter)
    iou = inter / (union + 1.0e-6)
    rows, cols = _lsa()(-iou)
    keep = iou[rows, cols] > 0.0
    rows, cols = rows[keep], cols[keep]
    overall_inter = inter[rows, cols].sum()
    overall_union = union[rows, cols].sum() + s.unpaired_area(rows + 1, cols + 1)
    return overall_inter / overall_union


def _dice2(inter, total):
    if len(inter) == 0:
        raise ZeroDivisionError("division by zero")       # no overlapping pair: 2 * 0 / 0 in the reference
    return 2 * np.uint64(inter.sum()) / np.uint64(total.sum())


def fast_dice_2_from_table(tab):
    s = _Scored(tab, "get_fast_dice_2")
    return _dice2(s.inter, s.total)


def dice_2_from_table(tab):
    tid, tarea = tab.true_areas()
    pid, parea = tab.pred_areas()
    if len(tid) and tid[0] != 0 or len(pid) and pid[0] != 0:
        raise ValueError("get_dice_2: a map without background (id 0)")
    m = (tab.t > 0) & (tab.p > 0)
    total = tarea[np.searchsorted(tid, tab.t[m])] + parea[np.searchsorted(pid, tab.p[m])]
    return _dice2(tab.count[m], total)


def dice_1_from_table(tab):
    inter = np.int64(tab.count[(tab.t > 0) & (tab.p > 0)].sum())
    denom = np.int64(tab.count[tab.t > 0].sum() + tab.count[tab.p > 0].sum())
    return 2.0 * inter / denom


# ---------------------------------------------------------------------------------------------------- the reference's names
def get_fast_pq(true, pred, match_iou=0.5, *, device=None):
    """[dq, sq, pq], [paired_true, paired_pred, unpaired_true, unpaired_pred] (paired ids as ndarrays for match_iou >= 0.5, lists
    below; dq a Python float, sq / pq numpy float64), equal to metrics/stats_utils.py get_fast_pq."""
    assert match_iou >= 0.0, "Cant' be negative"
    return pq_from_table(_table(true, pred, device), match_iou)


def get_fast_aji(true, pred, *, device=None):
    return aji_from_table(_table(true, pred, device))


def get_fast_aji_plus(true, pred, *, device=None):
    return aji_plus_from_table(_table(true, pred, device))


def get_fast_dice_2(true, pred, *, device=None):
    return fast_dice_2_from_table(_table(true, pred, device))


def get_dice_1(true, pred, *, device=None):
    return dice_1_from_table(_table(true, pred, device))


def get_dice_2(true, pred, *, device=None):
    return dice_2_from_table(_table(true, pred, device))


def remap_label(pred, by_size=False, *, device=None):
    """Ids renumbered 1..n in ascending order of the old id, or by descending area with `by_size` (equal areas keep ascending
    id).  Returns `pred` itself when it holds no label and raises ValueError when it has labels but no background, as the
    reference does.  numpy in -> numpy int32 out; a tensor in -> an int32 tensor on the input's device."""
    dev = _resolve_device(device, pred)
    if dev is None or (pred.numel() if _is_tensor(pred) else np.size(pred)) == 0:
        a = _host_map(pred)
        u, inv, cnt = np.unique(a, return_inverse=True, return_counts=True)
        if len(u) == 0 or u[0] != 0:
            raise ValueError("remap_label: the map has no background (id 0)")
        if len(u) == 1:
            return pred                                   # no label
        lut = np.arange(len(u), dtype=np.int32)
        if by_size:
            lut[1:][np.argsort(-cnt[1:], kind="stable")] = np.arange(1, len(u), dtype=np.int32)
        out = lut[inv.reshape(a.shape)]
        return _like(out, pred)
    x = _device_maps(pred, dev)
    flat = x.reshape(1, 1, -1) if x.dim() != 2 else x[None]
    res = remap_device(flat, by_size)
    if res is None:
        return pred
    return _like(res.reshape(x.shape), pred)


def _like(out, ref):
    """numpy result for numpy input; an int32 tensor on the input's device for tensor input."""
    if _is_tensor(ref):
        import torch

        return (out if _is_tensor(out) else torch.from_numpy(out)).to(ref.device)
    return out.cpu().numpy() if _is_tensor(out) else out


def remap_device(maps, by_size=False):
    """remap_label of every map of an int32 CUDA tensor [n, h, w] (a new tensor), or None when no map holds a label.  Raises
    ValueError when a map holds a negative label, or labels but no background.  Maps run in groups whose bitmap fits
    WORKSPACE_BUDGET."""
    import torch

    from . import lib as L

    n, h, w = maps.shape
    dev = maps.device
    rng = torch.empty((n, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("hvn_label_range", maps.data_ptr(), n, h, w, rng.data_ptr(), L.stream_ptr(dev))
        r = rng.cpu().numpy()
        if (r[:, 0] < 0).any():
            raise ValueError("negative labels are not instance ids")
        if (r[:, 1] <= 0).all():
            return None
        if ((r[:, 0] > 0) & (r[:, 1] > 0)).any():
            raise ValueError("remap_label: the map has no background (id 0)")
        out = torch.empty_like(maps)
        n_ids = torch.empty(n, dtype=torch.int32, device=dev)
        i0 = 0
        while i0 < n:                                    # groups: the largest id of the group decides the bitmap size
            m, mx = 1, max(0, int(r[i0, 1]))
            while i0 + m < n:
                grown = max(mx, int(r[i0 + m, 1]))
                if L.lib().hvn_remap_label_workspace_bytes(m + 1, h, w, grown) > WORKSPACE_BUDGET:
                    break
                m, mx = m + 1, grown
            need = L.lib().hvn_remap_label_workspace_bytes(m, h, w, mx)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            L.call("hvn_remap_label", maps[i0:i0 + m].data_ptr(), m, h, w, mx, out[i0:i0 + m].data_ptr(), n_ids[i0:i0 + m].data_ptr(),
                   ws.data_ptr(), need, L.stream_ptr(dev))
            del ws
            i0 += m
        if by_size:
            k = n_ids.cpu().numpy().astype(np.int64)
            kmax = int(k.max())
            areas = torch.empty((n, kmax + 1), dtype=torch.int32, device=dev)
            L.call("hvn_label_areas", out.data_ptr(), n, h, w, kmax, areas.data_ptr(), L.stream_ptr(dev))
            a = areas.cpu().numpy().astype(np.int64)
            perm = np.tile(np.arange(kmax + 1, dtype=np.int32), (n, 1))
            for i in range(n):
                perm[i, 1:k[i] + 1][np.argsort(-a[i, 1:k[i] + 1], kind="stable")] = np.arange(1, k[i] + 1, dtype=np.int32)
            dperm = torch.from_numpy(perm).to(dev)
            L.call("hvn_label_permute", out.data_ptr(), n, h, w, kmax, dperm.data_ptr(), L.stream_ptr(dev))
            torch.cuda.current_stream(dev).synchronize()
    return out


def pair_coordinates(setA, setB, radius):
    """Optimal unique pairing of two point sets by Euclidean distance (scipy cdist + linear_sum_assignment), pairs farther than
    `radius` dropped: (pairing int [k, 2], unpairedA, unpairedB), equal to the reference's.  Host only."""
    from scipy.spatial.distance import cdist

    a, b = (x.detach().cpu().numpy() if _is_tensor(x) else x for x in (setA, setB))
    dist = cdist(a, b, metric="euclidean")
    ia, ib = _lsa()(dist)
    near = dist[ia, ib] <= radius
    pa, pb = ia[near], ib[near]
    pairing = np.concatenate([pa[:, None], pb[:, None]], axis=-1)
    return pairing, np.delete(np.arange(a.shape[0]), pa), np.delete(np.arange(b.shape[0]), pb)


# -------------------------------------------------------------------------------------------------------------- batched scores
def instance_stats(true, pred, remap=True, *, device=None):
    """float64 [N, 6] = (dice1, aji, dq, sq, pq, aji_plus) per image: the row `compute_stats.py run_nuclei_inst_stat` records
    (remap_label of both maps first when `remap`).  `true` / `pred`: [N, H, W] arrays or tensors (CUDA tensors such as the
    instance maps of post_proc.process_batch_device stay on the device; only the triples leave it), or lists of 2-D maps of
    different shapes (one device pass per group of equal shape).  Raises what the reference's calls raise, in its call order."""
    tabs = pair_tables(true, pred, device=device)
    out = np.zeros((len(tabs), 6), np.float64)
    for i, tab in enumerate(tabs):
        if remap:
            tab = tab.ranked()
        (dq, sq, pq), _ = pq_from_table(tab, 0.5)
        out[i] = (dice_1_from_table(tab), aji_from_table(tab), dq, sq, pq, aji_plus_from_table(tab))
    return out

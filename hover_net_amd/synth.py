"""Synthetic workloads of the shapes BASELINE.json names (pure numpy, no torch).

* `synth_tiles`     -- uint8 RGB network input patches (seeded noise).
* `synth_pred_maps` -- structured `[type?, p, h, v]` prediction maps the way a trained
  HoVer-Net emits them: random, partly overlapping elliptical nuclei, `p` high inside,
  `h`/`v` the per-instance horizontal/vertical distance maps in [-1, 1] (semantics of
  /root/reference/models/hovernet/targets.py:63-93), plus noise.  These give the
  post-processing a realistic instance load independent of any weights.
* `synth_inst_pair` -- a ground-truth / prediction pair of int32 instance maps (disks; the prediction shifted, with merged,
  split, missed and spurious instances) for the metrics (hover_net_amd/metrics.py).
"""
import numpy as np


def synth_tiles(n, size=270, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, size=(n, size, size, 3), dtype=np.uint8)


def _one_map(rng, H, W, nr_types, k_lo, k_hi, noise):
    inst = np.zeros((H, W), np.int32)
    k = int(rng.integers(k_lo, k_hi + 1))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for i in range(1, k + 1):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ra, rb = rng.uniform(4, 12), rng.uniform(4, 12)
        th = rng.uniform(0, np.pi)
        c, s = np.cos(th), np.sin(th)
        u = (xx - cx) * c + (yy - cy) * s
        v = -(xx - cx) * s + (yy - cy) * c
        m = (u / ra) ** 2 + (v / rb) ** 2 <= 1.0
        inst[m] = i  # later nuclei overwrite earlier ones -> touching instances
    hmap = np.zeros((H, W), np.float64)
    vmap = np.zeros((H, W), np.float64)
    tmap = np.zeros((H, W), np.float64)
    for i in range(1, k + 1):
        m = inst == i
        if not m.any():
            continue
        ys, xs = np.nonzero(m)
        dx = xs - np.round(xs.mean())
        dy = ys - np.round(ys.mean())
        if dx.min() < 0:
            dx[dx < 0] /= -dx.min()
        if dx.max() > 0:
            dx[dx > 0] /= dx.max()
        if dy.min() < 0:
            dy[dy < 0] /= -dy.min()
        if dy.max() > 0:
            dy[dy > 0] /= dy.max()
        hmap[ys, xs] = dx
        vmap[ys, xs] = dy
        if nr_types:
            tmap[ys, xs] = 1 + (i % (nr_types - 1))
    mask = inst > 0
    p = 0.9 * mask + 0.05 + rng.normal(0, noise, (H, W))
    hmap = hmap + rng.normal(0, noise, (H, W))
    vmap = vmap + rng.normal(0, noise, (H, W))
    chans = [p, hmap, vmap]
    if nr_types:
        flip = rng.uniform(size=(H, W)) < 0.05  # some mis-typed pixels
        tmap = np.where(flip, rng.integers(0, nr_types, (H, W)), tmap)
        chans = [tmap] + chans
    return np.stack(chans, -1).astype(np.float32), inst


def synth_pred_maps(n, H=80, W=80, nr_types=None, seed=0, k_lo=5, k_hi=40, noise=0.02):
    """-> (pred [n,H,W,3|4] float32, painted instance maps [n,H,W] int32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    scale = (H * W) / 6400.0
    lo, hi = max(1, int(k_lo * scale)), max(1, int(k_hi * scale))
    maps, insts = zip(*[_one_map(rng, H, W, nr_types, lo, hi, noise) for _ in range(n)])
    return np.stack(maps), np.stack(insts)


_GAINS = (("conv3.weight", 0.35), ("shortcut.weight", 0.6), ("conv_bot.weight", 0.6), ("conva.weight", 0.6),
          ("convf.weight", 0.6), ("u0.conv.weight", 1.5))


def _conv_gain(key):
    for suffix, g in _GAINS:
        if key.endswith(suffix):
            return g
    return 1.0


_SD_CACHE = {}


def synth_state_dict(mode="original", nr_types=None, seed=0, as_torch=True):
    """Seeded, platform-independent (numpy PCG64) checkpoint in the reference's key
    format: Kaiming fan_out convs like `Net.weights_init`
    (/root/reference/models/hovernet/net_utils.py:18-32) but with NON-trivial BatchNorm
    affine + running statistics so that BN folding / prologues are really exercised."""
    from .arch import param_table

    key_ = (mode, nr_types, int(seed))
    if key_ in _SD_CACHE:                       # (the last few checkpoints drawn in this process: 37 - 55 M normals take ~2 s; fresh copies are handed out)
        sd = {k: v.copy() for k, v in _SD_CACHE[key_].items()}
        if as_torch:
            import torch

            sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
        return sd
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, (kind, shape) in param_table(mode, nr_types).items():
        if kind == "conv":
            # He-normal over fan_in, with the residual / skip-summing convs damped so that
            # activations (and the logits) stay O(1..10) through the ~50 layers; absolute
            # tolerances on logits are only meaningful at that scale.
            fan_in = shape[1] * shape[2] * shape[3]
            a = rng.normal(0.0, np.sqrt(2.0 / fan_in) * _conv_gain(key), shape)
        elif kind == "bias":
            a = rng.normal(0.0, 0.1, shape)
        elif kind == "bn_w":
            a = rng.uniform(0.6, 1.4, shape)
        elif kind == "bn_b":
            a = rng.normal(0.0, 0.2, shape)
        elif kind == "bn_rm":
            a = rng.normal(0.0, 0.2, shape)
        elif kind == "bn_rv":
            a = rng.uniform(0.5, 1.5, shape)
        elif kind == "bn_nbt":
            a = np.array(0, np.int64)
        elif kind == "ones":
            a = np.ones(shape)
        else:
            raise KeyError(kind)
        sd[key] = a.astype(np.int64 if kind == "bn_nbt" else np.float32)
    _SD_CACHE[key_] = {k: v.copy() for k, v in sd.items()}
    while len(_SD_CACHE) > 6:
        _SD_CACHE.pop(next(iter(_SD_CACHE)))
    if as_torch:
        import torch

        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    return sd


def synth_train_batch(n, mode="original", nr_types=None, seed=0):
    """Synthetic training batch in the reference's loader format (dataloader/train_loader.py:109-137 feeds
    run_desc.train_step): img uint8 [n,S,S,3], np_map int64 [n,h,w] in {0,1}, hv_map float32 [n,h,w,2] in [-1,1],
    tp_map int64 [n,h,w] in [0,nr_types) (only with nr_types).  Nuclei are painted ellipses (synth_pred_maps)."""
    size, out = (270, 80) if mode == "original" else (256, 164)
    pm, inst = synth_pred_maps(n, out, out, nr_types, seed=seed + 17, noise=0.0)
    c0 = 0 if nr_types is None else 1
    batch = {"img": synth_tiles(n, size, seed=seed),
             "np_map": (inst > 0).astype(np.int64),
             "hv_map": np.ascontiguousarray(np.clip(pm[..., c0 + 1:c0 + 3], -1.0, 1.0), np.float32)}
    if nr_types is not None:
        batch["tp_map"] = np.clip(pm[..., 0].round().astype(np.int64), 0, nr_types - 1) * (inst > 0)
    return batch


def synth_inst_pair(h, w, n_inst, seed=0, r_lo=3, r_hi=9, shift=(2, 1), n_merge=None, n_split=None, n_miss=None, n_spurious=None,
                    id_stride=1, id_base=0):
    """(true, pred) int32 [h, w]: `n_inst` disks of radius r_lo..r_hi (later ones drawn over earlier ones, ids 1..n_inst);
    pred = true rolled by `shift`, then n_merge neighbouring pairs merged, n_split instances cut in two along their centre
    column, n_miss removed and n_spurious new disks added (each defaults to ~3 % of n_inst).  Non-zero ids of both maps become
    id_base + id_stride * id (non-contiguous ids; the largest must stay within int32)."""
    rng = np.random.default_rng(seed)
    d = lambda v: max(1, n_inst // 33) if v is None else v  # noqa: E731
    true = np.zeros((h, w), np.int64)
    yy, xx = np.ogrid[:h, :w]
    cen = []
    for i in range(1, n_inst + 1):
        r = int(rng.integers(r_lo, r_hi + 1))
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        y0, y1, x0, x1 = max(0, cy - r), min(h, cy + r + 1), max(0, cx - r), min(w, cx + r + 1)
        m = (yy[y0:y1] - cy) ** 2 + (xx[:, x0:x1] - cx) ** 2 <= r * r
        true[y0:y1, x0:x1][m] = i
        cen.append((cy, cx))
    pred = np.roll(true, shift, (0, 1)).copy()
    nxt = n_inst + 1
    ids = np.unique(pred)[1:]
    for _ in range(d(n_merge)):
        if len(ids) < 2:
            break
        a, b = rng.choice(ids, 2, replace=False)
        pred[pred == b] = a
    for _ in range(d(n_split) if len(ids) else 0):
        a = int(rng.choice(ids))
        ys, xs = np.nonzero(pred == a)
        if len(xs) > 1:
            half = xs > int(np.median(xs))
            pred[ys[half], xs[half]] = nxt
            nxt += 1
    for _ in range(d(n_miss) if len(ids) else 0):
        pred[pred == int(rng.choice(ids))] = 0
    for _ in range(d(n_spurious)):
        r = int(rng.integers(r_lo, r_hi + 1))
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        y0, y1, x0, x1 = max(0, cy - r), min(h, cy + r + 1), max(0, cx - r), min(w, cx + r + 1)
        m = ((yy[y0:y1] - cy) ** 2 + (xx[:, x0:x1] - cx) ** 2 <= r * r) & (pred[y0:y1, x0:x1] == 0)
        pred[y0:y1, x0:x1][m] = nxt
        nxt += 1
    out = []
    for a in (true, pred):
        a = np.where(a > 0, id_base + id_stride * a, 0)
        assert a.max() <= 2 ** 31 - 1
        out.append(a.astype(np.int32))
    return out[0], out[1]


def synth_thumbnail(h, w, seed=0, tissue=0.42):
    """A seeded 1.25x slide thumbnail for the tissue-mask path: uint8 [h, w, 3], bright noisy background, blobby stained tissue
    over about `tissue` of the area (a smoothed random field cut at that quantile) with small tears inside it, and dark dust
    specks of 1 - 9 px on the background.  Returns (thumb, fraction of pixels drawn as tissue)."""
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    field = ndimage.gaussian_filter(rng.standard_normal((h, w)), sigma=max(2.0, min(32.0, min(h, w) / 40.0)))
    blob = field > np.quantile(field, 1.0 - tissue)
    tears = ndimage.gaussian_filter(rng.standard_normal((h, w)), sigma=3.0) > 0.12
    blob &= ~tears
    dust = ndimage.binary_dilation(rng.random((h, w)) < 2e-4, iterations=1) & (rng.random((h, w)) < 0.7)
    dark = blob | dust
    thumb = np.clip(rng.normal(232, 5, (h, w, 3)), 0, 255)
    stain = np.clip(rng.normal((150, 90, 160), 18, (h, w, 3)), 0, 255)
    thumb[dark] = stain[dark]
    return thumb.astype(np.uint8), float(dark.mean())

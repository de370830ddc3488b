"""Reference side of the stain-normalisation tests, written without hover_net_amd.stain: a seeded H&E-like image generator and
the textbook per-pixel Macenko in float64 (np.cov and np.percentile on pixels, the direct exp apply)."""
import numpy as np

IO, BETA, ALPHA = 240.0, 0.15, 1.0
HE_REF = np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]])
MAXC_REF = np.array([1.9705, 1.0308])
OD = -np.log((np.arange(256) + 1.0) / IO)


def he_image(h, w, seed, he=((0.65, 0.70, 0.29), (0.07, 0.99, 0.11)), strength=(1.0, 1.0)):
    """uint8 [h, w, 3]: Gaussian nuclei in haematoxylin, blocky eosin, 25 % background blocks, OD noise."""
    rng = np.random.default_rng(seed)
    he = np.array(he, np.float64)
    he /= np.linalg.norm(he, axis=1, keepdims=True)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = np.zeros((h, w))
    ce = 0.3 + 0.5 * rng.random((h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w]
    for _ in range(max(4, h * w // 400)):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(3, 7)
        ch = np.maximum(ch, (1.2 + rng.random()) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * r * r)))
    bg = rng.random((h // 16 + 1, w // 16 + 1)).repeat(16, 0).repeat(16, 1)[:h, :w] < 0.25
    ce[bg] = 0
    ch[bg] *= 0.05
    od = strength[0] * ch[..., None] * he[0] + strength[1] * ce[..., None] * he[1] + rng.normal(0, 0.02, (h, w, 3))
    return np.clip(IO * np.exp(-od) - 1, 0, 255).astype(np.uint8)


def fit_pixels(img, mask=None):
    """(HE [3, 2], maxC [2]) of the textbook per-pixel fit."""
    px = img.reshape(-1, 3) if mask is None else img[np.asarray(mask) != 0]
    od = OD[px]
    od_hat = od[~np.any(od < BETA, axis=1)]
    _, evec = np.linalg.eigh(np.cov(od_hat.T))
    e = evec[:, 1:3].copy()
    for j in range(2):
        if e[:, j].sum() < 0:
            e[:, j] = -e[:, j]
    that = od_hat @ e
    phi = np.arctan2(that[:, 1], that[:, 0])
    mn, mx = np.percentile(phi, ALPHA), np.percentile(phi, 100 - ALPHA)
    v_min = e @ np.array([np.cos(mn), np.sin(mn)])
    v_max = e @ np.array([np.cos(mx), np.sin(mx)])
    he = np.array([v_min, v_max]).T if v_min[0] > v_max[0] else np.array([v_max, v_min]).T
    conc = np.linalg.pinv(he) @ od.T
    return he, np.array([np.percentile(conc[0], 99), np.percentile(conc[1], 99)])


def matrix(he, max_c):
    return HE_REF @ np.diag(MAXC_REF / max_c) @ np.linalg.pinv(he)


def apply_direct(img, m):
    """min(255, Io exp(-M od)) per pixel, truncated to uint8."""
    x = IO * np.exp(-(m @ OD[img.reshape(-1, 3)].T))
    return np.minimum(x, 255).astype(np.uint8).T.reshape(img.shape)

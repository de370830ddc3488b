"""Inputs and window lists shared by tests/test_resample_host.py and tests/test_gpu_resample.py (no tests in here)."""
import numpy as np


def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def checkerboard(h, w, cell=1):
    """0 / 255 in cells of `cell` pixels: the cubic kernel overshoots at every edge (cells of 3: past both ends, where it saturates)."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy // cell + xx // cell) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def windows(H, W):
    """(y0, x0, h, w) of an [H, W] output: each corner, the interior from an odd origin, one row, one column, everything."""
    h, w = max(1, H // 3), max(1, W // 3)
    return [(0, 0, h, w), (0, W - w, h, w), (H - h, 0, h, w), (H - h, W - w, h, w), (3, 5, H // 2, W // 2), (H // 2 + 1, 0, 1, W),
            (0, W // 2 + 1, H, 1), (H - 1, W - 1, 1, 1), (0, 0, H, W)]

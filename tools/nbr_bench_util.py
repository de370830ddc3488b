"""What tools/neighbours_bench.py, clusters_bench.py and density_bench.py share: the synthetic slide, the count of candidate tests, the
timing of one op between two HIP events and the write-out of the table and the JSON line."""
import json
import os
import statistics

import numpy as np

TYPES = 5


def points(n, seed):
    """Tissue-like density, about one nucleus per 20 x 20 px: 70 % of the points uniform over a square of side 20 sqrt(N), 30 % in
    Gaussian clusters (sigma 40 px, 200 points each), TYPES types -> (xy, types, side)."""
    rng = np.random.default_rng(seed)
    side = 20.0 * np.sqrt(n)
    n_cl = int(0.3 * n)
    centres = rng.random((max(1, n_cl // 200), 2)) * side
    cl = centres[rng.integers(0, centres.shape[0], n_cl)] + rng.normal(0.0, 40.0, (n_cl, 2))
    xy = np.concatenate([rng.random((n - n_cl, 2)) * side, np.clip(cl, 0.0, side)])
    return np.ascontiguousarray(xy[rng.permutation(n)]), rng.integers(0, TYPES, n).astype(np.int32), side


def candidates(xy, g):
    """Distance tests a 3 x 3 search needs: per point, the points in the nine cells around it (itself included)."""
    from hover_net_amd import neighbours as NB

    cx, cy = NB.cells(xy, g)
    per = np.zeros((g.ncy + 2, g.ncx + 2), np.int64)
    np.add.at(per, (cy + 1, cx + 1), 1)
    box = sum(per[1 + dy:g.ncy + 1 + dy, 1 + dx:g.ncx + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return int((box * per[1:-1, 1:-1]).sum())


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(fn):
    """Milliseconds between two HIP events around fn() on the current stream."""
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def write_out(name, lines, out, path):
    """Prints the table, writes it to `path` if given, and prints the ONE JSON line {name: out}."""
    text = "\n".join(lines)
    print(text)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
    print(json.dumps({name: out}))

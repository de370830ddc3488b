"""-m gpu: the five point-pattern analyses through the one table of hover_net_amd/points.py (`annotate` + `summaries`) on the device
against the same calls on the host, with ==.  Every analysis has its own device tests (tests/test_gpu_neighbours.py and the four
beside it); this one holds the table to them.  Integers and numpy's own floats only: no tolerance anywhere."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZE = (400, 400)


def _info():
    """600 nuclei of 3 types on a 400 x 400 image: more than two workgroups of 256 slots, several grid cells at every radius below."""
    rng = np.random.default_rng(5)
    xy = np.round(rng.uniform(0.0, 399.0, (600, 2)) * 4.0) / 4.0
    types = rng.integers(0, 3, 600)
    return {2 * i + 1: {"centroid": xy[i].copy(), "type": int(types[i])} for i in range(600)}


def _same(a, b, where):
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (tuple, list)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), where
    else:
        assert type(a) is type(b) and a == b, where


def test_all_five_on_device_equal_host():
    from hover_net_amd import points as P

    rects = [[[[(20, 30), (260, 30), (260, 300), (20, 300)]]], [[[(180, 150), (390, 150), (390, 380), (180, 380)]]]]
    specs = P.resolve_specs({"radius": 25.0, "k": 5}, {"radius": 15.0, "min_pts": 4, "types": [0, 2]}, {"radius": 30.0, "step": 16},
                            {"radii": [4.0 * (k + 1) for k in range(16)]}, {"regions": rects})
    got, want = {}, {}
    for out, device in ((want, None), (got, torch.device("cuda"))):
        out["info"] = P.annotate(copy.deepcopy(_info()), specs, 3, device)
        out["results"] = P.summaries(out["info"], SIZE, specs, 3, device)
    assert all(list(e) == ["centroid", "type", "neighbours", "cluster", "region"] for e in got["info"].values())
    _same(got["info"], want["info"], "info")
    for name in P.PointResults._fields:
        _same(tuple(getattr(got["results"], name)), tuple(getattr(want["results"], name)), name)
    res = want["results"]                                            # and the host's side is not an empty case
    assert res.density.count.shape == (3, 25, 25) and res.ripley.pairs.shape == (3, 3, 16) and (res.ripley.pairs[..., 0] > 0).any()
    assert set(res.regions.first.tolist()) == {-1, 0, 1} and res.regions.hits.max() == 2
    assert any(e["cluster"]["id"] is not None for e in want["info"].values()) and any(len(e["neighbours"]["knn"]) == 5 for e in want["info"].values())

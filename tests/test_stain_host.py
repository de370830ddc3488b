"""CPU: the host definition of Macenko stain normalisation (hover_net_amd/stain.py) against the textbook per-pixel
form of tests/stain_ref.py, and what the three STAIN op kinds refuse before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

import stain_ref as R
from hover_net_amd import stain

EXTENTS = [(96, 96, 1), (270, 270, 2), (512, 512, 3)]


@pytest.fixture(scope="module")
def images():
    return {(h, w): R.he_image(h, w, seed) for h, w, seed in EXTENTS}


@pytest.mark.parametrize("h,w,seed", EXTENTS)
def test_fit_agrees_with_the_textbook_fit(images, h, w, seed):
    """The two differ only in float64 summation order over <= 3e5 terms of size O(1): about 1e-11 at the most; the bound is 1e-9."""
    img = images[(h, w)]
    keys, counts = np.unique((img[..., 0].astype(np.int64) << 16 | img[..., 1].astype(np.int64) << 8 | img[..., 2]).reshape(-1), return_counts=True)
    f = stain.fit_from_counts(keys, counts)
    he, max_c = R.fit_pixels(img)
    d_he, d_mc = np.abs(f.he - he).max(), np.abs(f.max_c - max_c).max()
    print("%dx%d: %d colours, kept %d of %d, |dHE| %.3g, |dmaxC| %.3g" % (h, w, len(keys), f.kept, f.pixels, d_he, d_mc))
    assert f.pixels == h * w and 64 <= f.kept <= h * w
    assert d_he <= 1e-9 and d_mc <= 1e-9
    # a non-degenerate fit: haematoxylin first, both stains present
    assert f.he[0, 0] > f.he[0, 1] and (f.max_c > 0.1).all()
    # colour_counts_host is np.unique
    k2, c2 = stain.colour_counts_host(img)
    assert np.array_equal(k2, keys) and np.array_equal(c2, counts)
    f2 = stain.fit(img)
    assert np.array_equal(f2.he, f.he) and np.array_equal(f2.max_c, f.max_c)


def test_weighted_percentile_is_np_percentile():
    rng = np.random.default_rng(5)
    for trial in range(40):
        m = int(rng.integers(1, 60))
        v = rng.standard_normal(m)
        if trial % 3 == 0:
            v = np.round(v, 1)                  # ties between rows
        c = rng.integers(1, 9, m)
        full = np.repeat(v, c)
        for q in (0.0, 1.0, 25.0, 50.0, 99.0, 100.0, float(rng.random() * 100)):
            want = np.percentile(full, q)
            got = stain.weighted_percentile(v, c, q)
            assert got == want, (trial, q, got, want)
    # q lands exactly on an element: 101 values, q = 37 -> index 37
    v = rng.standard_normal(101)
    assert stain.weighted_percentile(v, np.ones(101, np.int64), 37.0) == np.sort(v)[37] == np.percentile(v, 37.0)
    # counts: 5 values of 21 copies each but the last -> n = 101
    v5, c5 = np.array([0.3, -1.0, 2.5, 0.7, 9.0]), np.array([21, 20, 20, 20, 20])
    for q in (20.0, 37.0, 99.0):
        assert stain.weighted_percentile(v5, c5, q) == np.percentile(np.repeat(v5, c5), q)
    # a single row
    for q in (1.0, 50.0, 99.0):
        assert stain.weighted_percentile(np.array([0.25]), np.array([7]), q) == 0.25 == np.percentile(np.full(7, 0.25), q)
        assert stain.weighted_percentile(np.array([0.25]), np.array([1]), q) == 0.25


def test_apply_host_against_the_textbook_apply(images):
    total = differ = 0
    for img in images.values():
        f = stain.fit(img)
        m = stain.matrix(f)
        assert np.abs(m - R.matrix(*R.fit_pixels(img))).max() < 1e-6
        got, want = stain.apply_host(img, stain.tables(f)), R.apply_direct(img, m)
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1
        total += d.size
        differ += int((d > 0).sum())
        assert not np.array_equal(got, img)
    print("apply: %d of %d channel values differ from the textbook" % (differ, total))
    assert differ * 10000 <= total
    assert differ == 0          # on these inputs


def test_tables_of_a_target_fit(images):
    """A StainFit of a target image is a valid target; an image normalised to its own fit keeps its stain matrix: M = HE diag(1) pinv(HE)
    projects onto the stain plane."""
    a, b = images[(96, 96)], images[(270, 270)]
    fa, fb = stain.fit(a), stain.fit(b)
    m = stain.matrix(fa, fa)
    assert np.allclose(m @ fa.he, fa.he, atol=1e-12)
    assert stain.tables(fa, fb).shape == (3, 3, 256)
    assert np.array_equal(stain.matrix(fa, None), stain.matrix(fa, stain.resolve("macenko")))
    assert stain.resolve(fb) is fb and stain.resolve(None) is None


def test_fit_is_invariant_under_pixel_permutations(images):
    img = images[(270, 270)]
    f = stain.fit(img)
    rng = np.random.default_rng(3)
    for _ in range(2):
        p = img.reshape(-1, 3)[rng.permutation(270 * 270)].reshape(img.shape)
        g = stain.fit(p)
        assert np.array_equal(g.he, f.he) and np.array_equal(g.max_c, f.max_c) and g.kept == f.kept
    # and under a mask that selects everything
    g = stain.fit(img, np.ones((270, 270), np.uint8))
    assert np.array_equal(g.he, f.he) and np.array_equal(g.max_c, f.max_c)


def test_masked_fit_is_the_fit_of_the_selected_pixels(images):
    img = images[(270, 270)]
    mask = (np.random.default_rng(4).random((270, 270)) < 0.6).astype(np.uint8)
    f = stain.fit(img, mask)
    he, max_c = R.fit_pixels(img, mask)
    assert f.pixels == int(mask.sum())
    assert np.abs(f.he - he).max() <= 1e-9 and np.abs(f.max_c - max_c).max() <= 1e-9


def test_degenerate_images_raise():
    with pytest.raises(stain.StainFitError):
        stain.fit(np.full((40, 40, 3), 255, np.uint8))
    with pytest.raises(stain.StainFitError):
        stain.fit(np.full((40, 40, 3), (120, 60, 140), np.uint8))            # one colour
    img = np.full((40, 40, 3), 255, np.uint8)
    img.reshape(-1, 3)[:63] = R.he_image(96, 96, 1).reshape(-1, 3)[(R.OD[R.he_image(96, 96, 1).reshape(-1, 3)] >= R.BETA).all(1)][:63]
    with pytest.raises(stain.StainFitError, match="fewer than 64"):
        stain.fit(img)                                                       # 63 kept pixels
    assert issubclass(stain.StainFitError, ValueError)
    for bad in ("reinhard", "Macenko", 3, ("macenko",)):
        with pytest.raises(ValueError):
            stain.resolve(bad)


def test_thumbnail_mask_rule():
    m = np.array([[1, 0, 0], [0, 0, 2]], np.uint8)
    t = stain.thumbnail_mask((5, 7), m)
    want = np.array([[m[(y * 2) // 5, (x * 3) // 7] != 0 for x in range(7)] for y in range(5)], np.uint8)
    assert t.dtype == np.uint8 and np.array_equal(t, want)


@pytest.mark.parametrize("kind,name", [(11, b"stain_hist"), (12, b"stain_compact"), (13, b"stain_apply")])
def test_an_all_zero_op_is_refused_by_name(kind, name):
    """Decided on the host before anything touches a device; skipped where a GPU is present, as tests/test_error_channel.py is."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    op = L.hvn_op()
    op.kind = 99
    assert l.hvn_run_op(ctypes.byref(op), 1, None) == -1 and b"unknown op kind" in l.hvn_last_error()
    op = L.hvn_op()
    op.kind = kind
    assert l.hvn_run_op(ctypes.byref(op), 1, None) < 0
    err = l.hvn_last_error()
    assert err.startswith(name + b":") and b"unknown op kind" not in err, err


def test_refusals_with_made_up_pointers():
    """Each refusal of DESIGN 4.17's list that the host decides; the pointers are never dereferenced (nothing is launched)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    from hover_net_amd import lib as L

    l = L.lib()
    P = lambda i: 0x10000000 + (i << 24)  # noqa: E731

    def image(v, base, h=20, w=30, c=3, sy=0, sn=0):
        v.base, v.h, v.w, v.c, v.sy, v.sn = base, h, w, c, sy, sn

    def hist(**kw):
        op = L.hvn_op()
        op.kind = 11
        image(op.x, P(1), **kw)
        op.y.base = P(2)
        return op

    def apply(ykw=None, **kw):
        op = L.hvn_op()
        op.kind = 13
        image(op.x, P(1), **kw)
        image(op.y, P(3), **(kw if ykw is None else ykw))
        op.w = P(4)
        return op

    def refused(op, batch, code, name):
        rc = l.hvn_run_op(ctypes.byref(op), batch, None)
        err = l.hvn_last_error()
        assert rc == code and err.startswith(name + b":"), (rc, err)

    for make, name in ((hist, b"stain_hist"), (apply, b"stain_apply")):
        refused(make(c=4), 1, -1, name)
        refused(make(sy=89), 1, -1, name)                       # shorter than a row of 90 bytes
        refused(make(sy=96, sn=96 * 19), 2, -1, name)           # shorter than a sample
        refused(make(), 65536, -1, name)
        refused(make(h=1 << 15, w=(1 << 15) + 1), 1, -4, name)  # h * w > 2^30
        op = make()
        op.x_dtype = 1
        refused(op, 1, -1, name)
        op = make()
        op.x.base = None
        refused(op, 1, -1, name)
    op = hist()
    op.y.base = P(2) + 2
    refused(op, 1, -1, b"stain_hist")                           # misaligned bins
    op = apply()
    op.w = P(4) + 4
    refused(op, 1, -1, b"stain_apply")                          # misaligned tables
    refused(apply(ykw=dict(h=20, w=29)), 1, -1, b"stain_apply")  # different extents
    op = apply()
    op.y.base = P(1) + 90                                       # y starts one row into x
    refused(op, 1, -1, b"stain_apply")
    op = apply(sy=96)
    op.y.base, op.y.sy = P(1), 100                              # same base, other strides
    refused(op, 1, -1, b"stain_apply")

    def compact():
        op = L.hvn_op()
        op.kind = 12
        op.x.base, op.y.base, op.y.h, op.y2.base, op.x2.base = P(1), P(5), 100, P(6), P(7)
        return op

    refused(compact(), 2, -1, b"stain_compact")                 # batch must be 1
    for field, off in (("x", 4), ("y", 4), ("y2", 4), ("x2", 4)):
        op = compact()
        getattr(op, field).base = getattr(op, field).base + off
        refused(op, 1, -1, b"stain_compact")
    for cap in (0, -1, (1 << 24) + 1):
        op = compact()
        op.y.h = cap
        refused(op, 1, -4, b"stain_compact")
    op = compact()
    op.y2.base = None
    refused(op, 1, -1, b"stain_compact")

"""csrc/hvn_tissue.hip against the host functions of hover_net_amd/tissue_mask.py and the scikit-image goldens: every comparison
is bit equality.  The grey kernel takes four pixels per lane where its planes are dword-aligned and one otherwise; the row
kernels take 64 pixels per step; the dilation's tile is 32 rows x 64 columns."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from hover_net_amd import lib as L, tissue_mask as TM
from hover_net_amd.synth import synth_thumbnail

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "tissue_mask.npz")
GUARD, FILL = 3, 0xA5                                                   # sentinel rows on either side of every output, and their byte


def host_chain(gray, t, min_obj=256, max_hole=16384, radius=16):
    """(a, b, c) of the host functions after the threshold, as uint8."""
    a = TM.remove_small_objects(~(gray > t), min_obj, 2)
    b = TM.remove_small_holes(a, max_hole)
    c = ndimage.binary_dilation(b, structure=TM.disk(radius))
    return tuple(x.astype(np.uint8) for x in (a, b, c))


def guarded(h, w):
    """A uint8 plane [h, w] inside a buffer with GUARD sentinel rows before and after it."""
    buf = torch.full(((h + 2 * GUARD) * w,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD * w:(GUARD + h) * w].view(h, w)


def intact(buf, h, w):
    b = buf.cpu().numpy()
    return bool((b[:GUARD * w] == FILL).all() and (b[(GUARD + h) * w:] == FILL).all())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_mask(gray, t, min_obj=256, max_hole=16384, radius=16, h=None, w=None, short=0, taps=True):
    """hvn_tissue_mask itself on guarded outputs: ((mask, a, b) as numpy, return code, sentinels intact, buffers)."""
    H, W = gray.shape
    h, w = (H if h is None else h), (W if w is None else w)
    g = torch.from_numpy(np.ascontiguousarray(gray)).to("cuda")
    need = int(L.lib().hvn_tissue_mask_workspace_bytes(H, W))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    bufs, views = zip(*[guarded(H, W) for _ in range(3)])
    rc = L.lib().hvn_tissue_mask(g.data_ptr(), h, w, int(t), min_obj, max_hole, radius, views[0].data_ptr(),
                                 views[1].data_ptr() if taps else None, views[2].data_ptr() if taps else None, ws.data_ptr(), need - short, stream())
    torch.cuda.synchronize()
    return tuple(v.cpu().numpy() for v in views), rc, all(intact(b, H, W) for b in bufs), bufs


def check_chain(gray, t=127, **kw):
    (c, a, b), rc, ok, _ = raw_mask(gray, t, **kw)
    assert rc == 0 and ok
    wa, wb, wc = host_chain(gray, t, **kw)
    assert np.array_equal(a, wa), "objects"
    assert np.array_equal(b, wb), "holes"
    assert np.array_equal(c, wc), "dilation"
    return a, b, c


def gray_of(m0):
    return np.where(m0, 0, 255).astype(np.uint8)


# -- goldens ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_goldens(k):
    g = np.load(GOLD)
    (c, a, b), rc, ok, _ = raw_mask(gray_of(g["in%d" % k]), 127)
    assert rc == 0 and ok
    assert np.array_equal(a, g["a%d" % k]) and np.array_equal(b, g["b%d" % k]) and np.array_equal(c, g["c%d" % k])
    one = TM.mask_from_gray_device(torch.from_numpy(gray_of(g["in%d" % k])).to("cuda"), 127)          # the wrapper, without taps
    assert one.dtype == torch.uint8 and np.array_equal(one.cpu().numpy(), g["c%d" % k])


# -- grey + histogram ---------------------------------------------------------------------------
def _rgb_cases():
    rng = np.random.default_rng(21)
    two = np.where(rng.random((40, 45, 1)) < 0.3, np.uint8(40), np.uint8(200)).repeat(3, -1)
    return {"1x1": rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), "37x53": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
            "50x60": rng.integers(0, 256, (50, 60, 3), dtype=np.uint8), "1030x1027": rng.integers(0, 256, (1030, 1027, 3), dtype=np.uint8),
            "constant": np.full((33, 47, 3), 181, np.uint8), "two-valued": two}


@pytest.mark.parametrize("name", ["1x1", "37x53", "50x60", "1030x1027", "constant", "two-valued"])
@pytest.mark.parametrize("offset", [0, 1])
def test_gray_and_histogram(name, offset):
    """offset 1 puts both planes off a dword: the byte form of the kernel; offset 0 is the four-pixel form with its tail."""
    rgb = _rgb_cases()[name]
    h, w = rgb.shape[:2]
    src = torch.empty(rgb.size + 4, dtype=torch.uint8, device="cuda")
    src[offset:offset + rgb.size] = torch.from_numpy(rgb.reshape(-1)).to("cuda")
    buf = torch.full((h * w + 2 * 64,), FILL, dtype=torch.uint8, device="cuda")
    gray = buf[64 + offset:64 + offset + h * w]
    hist = torch.full((258,), -7, dtype=torch.int32, device="cuda")
    L.check(L.lib().hvn_tissue_gray_hist(src.data_ptr() + offset, h, w, gray.data_ptr(), hist[1:].data_ptr(), stream()), "hvn_tissue_gray_hist")
    want = TM.rgb_to_gray(rgb)
    assert np.array_equal(gray.cpu().numpy().reshape(h, w), want)
    b = buf.cpu().numpy()
    assert (b[:64 + offset] == FILL).all() and (b[64 + offset + h * w:] == FILL).all()
    counts = hist.cpu().numpy()
    assert counts[0] == -7 and counts[257] == -7
    assert np.array_equal(counts[1:257], np.bincount(want.reshape(-1), minlength=256))
    assert TM.otsu_from_hist(counts[1:257]) == TM.otsu_threshold(want)
    g2, h2 = TM.gray_hist_device(torch.from_numpy(rgb).to("cuda"))                                      # the wrapper
    assert np.array_equal(g2.cpu().numpy(), want) and np.array_equal(h2.cpu().numpy(), counts[1:257])


# -- size thresholds and connectivity -----------------------------------------------------------
def test_size_thresholds_and_connectivity():
    m = np.zeros((300, 333), bool)
    m[5:300, 10:170] = True                 # a tissue block that reaches the bottom border
    m[10:137, 20:149] = False               # hole of 127 x 129 = 16 383 px: filled
    m[150:278, 20:148] = False              # hole of 128 x 128 = 16 384 px: kept
    m[295:300, 50:60] = False               # small hole on the image border: filled
    m[5, 10] = False                        # the block's corner is background ...
    m[6, 11] = False                        # ... and this hole touches it only diagonally: filled (4-connectivity)
    m[10:25, 200:217] = True                # object of 15 x 17 = 255 px: dropped
    m[40:56, 200:216] = True                # object of 256 px: kept
    m[80:88, 200:216] = True                # two blobs of 128 px that touch only diagonally: kept (8-connectivity)
    m[88:96, 216:232] = True
    assert (~m[10:137, 20:149]).sum() == 16383 and m[10:25, 200:217].sum() == 255
    a, b, _ = check_chain(gray_of(m))
    assert a[15, 205] == 0 and a[45, 205] == 1 and a[84, 205] == 1 and a[90, 220] == 1
    assert b[70, 80] == 1 and b[200, 80] == 0 and b[297, 55] == 1 and b[6, 11] == 1 and b[5, 10] == 0


# -- long chains and giant components ------------------------------------------------------------
def _serpentine(h=257, w=255):
    m = np.zeros((h, w), bool)
    m[::2] = True
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


@pytest.mark.parametrize("name", ["serpentine", "serpentine-complement", "checkerboard", "background", "tissue"])
def test_long_chains_and_giant_components(name):
    sp = _serpentine()
    m = {"serpentine": sp, "serpentine-complement": ~sp, "checkerboard": np.indices((130, 131)).sum(0) % 2 == 0,
         "background": np.zeros((130, 200), bool), "tissue": np.ones((130, 200), bool)}[name]
    a, b, c = check_chain(gray_of(m))
    if name == "serpentine":                # one path of 129 * 255 + 128 pixels
        assert np.array_equal(a, sp) and int(sp.sum()) == 129 * 255 + 128
        a2, _, _ = check_chain(gray_of(m), min_obj=int(sp.sum()), max_hole=1, radius=0)
        a3, _, _ = check_chain(gray_of(m), min_obj=int(sp.sum()) + 1, max_hole=1, radius=0)
        assert np.array_equal(a2, sp) and not a3.any()
    if name == "checkerboard":              # one 8-connected object whose complement is 4-connected singletons
        assert b.all() and c.all()
    if name == "background":                # 26 000 px: one component of the complement, too large to be a hole
        assert not c.any()
    if name == "tissue":
        assert c.all()


# -- dilation -----------------------------------------------------------------------------------
def test_single_pixel_reproduces_the_disk():
    m = np.zeros((80, 90), bool)
    m[40, 45] = True
    _, _, c = check_chain(gray_of(m), min_obj=1, max_hole=1)
    want = np.zeros((80, 90), np.uint8)
    want[24:57, 29:62] = TM.disk(16)
    assert np.array_equal(c, want)


@pytest.mark.parametrize("shape", [(70, 150), (1, 50), (50, 1), (40, 20)])
@pytest.mark.parametrize("radius", [16, 0, 32])
def test_corners_small_images_and_radii(shape, radius):
    m = np.zeros(shape, bool)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    check_chain(gray_of(m), min_obj=1, max_hole=1, radius=radius)


def test_random_rows_cross_the_64_pixel_steps():
    """Sparse random pixels in an image of 2 1/3 steps: nearest set pixels lie in the step before, the lane's own and the next."""
    rng = np.random.default_rng(5)
    for radius in (16, 32):
        check_chain(gray_of(rng.random((45, 150)) < 0.01), min_obj=1, max_hole=1, radius=radius)


# -- end to end ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _thumb(name):
    if name == "blocks":                    # the thumbnail of tests/test_tissue_mask.py
        thumb = np.full((600, 700, 3), 235, np.uint8)
        thumb[100:400, 150:500] = (150, 90, 160)
        thumb[200:230, 250:280] = 235
        thumb[500:505, 600:605] = (150, 90, 160)
    else:
        thumb = synth_thumbnail(1250, 1300, seed=3)[0]
    want = TM.simple_get_mask(thumb)
    want.setflags(write=False)
    return thumb, want


@pytest.mark.parametrize("name", ["blocks", "blobs"])
def test_end_to_end_equals_the_host_mask(name):
    thumb, want = _thumb(name)
    got = TM.simple_get_mask(thumb, device="cuda")
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert 0 < int(want.sum()) < want.size
    again = TM.simple_get_mask(thumb, device="cuda")
    assert again.tobytes() == got.tobytes()
    if name == "blobs":                     # the taps of the device form, against the host chain spelt out
        gray = TM.rgb_to_gray(thumb)
        mask, a, b = TM.simple_get_mask_device(torch.from_numpy(thumb).to("cuda"), taps=True)
        wa, wb, wc = host_chain(gray, TM.otsu_threshold(gray))
        assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(b.cpu().numpy(), wb) and np.array_equal(mask.cpu().numpy(), wc)
        assert (wa != ~(gray > TM.otsu_threshold(gray))).any() and (wa != wb).any()                     # both filters act on it


# -- containment --------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["short workspace", "radius 33", "h 0", "h * w > 2^30"])
def test_refusals_leave_the_outputs_untouched(bad):
    gray = gray_of(np.random.default_rng(9).random((40, 50)) < 0.5)
    kw = {"short workspace": dict(short=1), "radius 33": dict(radius=33), "h 0": dict(h=0), "h * w > 2^30": dict(h=1 << 15, w=(1 << 15) + 1)}[bad]
    _, rc, _, bufs = raw_mask(gray, 127, **kw)
    assert rc != 0
    assert L.lib().hvn_last_error().decode().startswith("tissue_mask")
    for b in bufs:
        assert bool((b == FILL).all())
    with pytest.raises(L.HvnError):
        L.check(rc, "hvn_tissue_mask")
    if bad == "radius 33":
        with pytest.raises(L.HvnError):
            TM.mask_from_gray_device(torch.from_numpy(gray).to("cuda"), 127, radius=33)


def test_null_pointers_are_refused():
    g = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    hist = torch.full((256,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.lib().hvn_tissue_mask_workspace_bytes(4, 4)), dtype=torch.uint8, device="cuda")
    assert L.lib().hvn_tissue_gray_hist(None, 4, 4, g.data_ptr(), hist.data_ptr(), stream()) != 0
    assert L.lib().hvn_tissue_gray_hist(g.data_ptr(), 0, 4, g.data_ptr(), hist.data_ptr(), stream()) != 0
    assert L.lib().hvn_tissue_mask(g.data_ptr(), 4, 4, 127, 1, 1, 1, None, None, None, ws.data_ptr(), ws.numel(), stream()) != 0
    assert L.lib().hvn_tissue_mask(g.data_ptr(), 4, 4, 127, 1, 1, 1, g.data_ptr(), None, None, None, ws.numel(), stream()) != 0
    assert L.lib().hvn_tissue_mask_workspace_bytes(0, 4) == 0
    torch.cuda.synchronize()
    assert bool((hist == -7).all())


# -- wiring -------------------------------------------------------------------------------------
def test_wsi_inference_with_the_device_mask():
    """`run(slide, "auto")` on the synthetic slide of tests/test_gpu_net.py's whole-slide test, mask from the device against mask
    from the host: the same instance map and records."""
    from hover_net_amd import infer_wsi, net_desc
    from hover_net_amd.synth import synth_state_dict

    net = net_desc.create_model(mode="original", nr_types=5, input_ch=3)
    net.load_state_dict(synth_state_dict("original", 5, seed=81), strict=True)
    net = net.to("cuda").eval()
    slide = infer_wsi.ArraySlide(np.random.default_rng(82).integers(0, 256, (900, 1010, 3), dtype=np.uint8))
    thumb = slide.thumbnail(32)
    assert np.array_equal(TM.simple_get_mask(thumb, device="cuda"), TM.simple_get_mask(thumb))
    kw = dict(nr_types=5, batch_size=16, chunk_shape=700, tile_shape=512, ambiguous_size=64)
    inst_h, info_h = infer_wsi.WsiInference(net, **kw).run(slide, "auto")
    inst_d, info_d = infer_wsi.WsiInference(net, device_mask=True, **kw).run(slide, "auto")
    assert np.array_equal(inst_d, inst_h) and sorted(info_d) == sorted(info_h)
    for k in info_h:
        for f in info_h[k]:
            assert np.array_equal(np.asarray(info_d[k][f]), np.asarray(info_h[k][f])), (k, f)

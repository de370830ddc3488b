"""CPU: the geometry and the host definition of training-from-whole-images (`hover_net_amd/patching.py`) against the live reference's
misc/patch_extractor.py `PatchExtractor` where the reference tree exists, and against tests/golden/patching_ref.npz (made by
tools/make_golden_patching.py with the reference's own extractor) everywhere; the dataset parsers of `hover_net_amd/dataset.py` on
files written into tmp_path; the table validation of `ImageStore`; the ABI of `hvn_augment_shape_images`.  `==` everywhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from hover_net_amd import lib as L
from hover_net_amd import patching as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
FIXTURE = os.path.join(REPO, "tests", "golden", "patching_ref.npz")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "misc")), reason="needs the reference tree (build container only)")

WIN, STEP = (25, 22), (8, 6)          # odd difference in h: the pad before (8) differs from the pad after (9); w: 8 and 8
# (h, w).  Heights 8 and widths 6 are narrower than the pad (numpy's reflect wraps more than once), width 9 is the pad exactly.  The last three complete the
# edge-flag combinations: (16, 10) is the mirror kind's (no bottom edge, right edge), (30, 28) and (33, 30) the valid kind's mixed ones.
SIZES = [(61, 47), (41, 40), (8, 90), (33, 6), (25, 22), (49, 46), (57, 52), (8, 6), (100, 9), (16, 10), (30, 28), (33, 30)]


def _flags(h, w, kind):
    (pt, pb), (pl, pr) = P.pads(WIN, STEP, kind)
    return (h + pt + pb - WIN[0]) % STEP[0] != 0, (w + pl + pr - WIN[1]) % STEP[1] != 0


def _image(h, w, c=5):
    return np.random.default_rng([h, w, c]).integers(0, 1 << 20, (h, w, c)).astype(np.int32)


@pytest.fixture
def reference_extractor(monkeypatch):
    """The reference's PatchExtractor class, imported through oracle/refimport.py with oracle/cv2_shim ahead of it."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import refimport

    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    refimport.use_reference(first=[os.path.join(REPO, "oracle", "cv2_shim")])
    import matplotlib

    matplotlib.use("Agg")
    monkeypatch.setattr(np.lib, "pad", np.pad, raising=False)         # the alias patch_extractor.py:131 pads with; gone from numpy >= 2
    try:
        yield refimport.ref_import("misc.patch_extractor").PatchExtractor
    finally:
        sys.path[:] = saved_path
        for name in list(sys.modules):
            if name.split(".")[0] in ("models", "dataloader", "misc", "metrics", "infer", "run_utils", "cv2"):
                if name in saved_mods:
                    sys.modules[name] = saved_mods[name]
                else:
                    del sys.modules[name]


@needs_reference
def test_extract_host_equals_the_live_reference(reference_extractor):
    X = reference_extractor(WIN, STEP)
    total, seen, wraps = 0, {"mirror": set(), "valid": set()}, 0
    for kind in ("mirror", "valid"):
        (pt, pb), (pl, pr) = P.pads(WIN, STEP, kind)
        for h, w in SIZES:
            x = _image(h, w)
            if h + pt + pb < WIN[0] or w + pl + pr < WIN[1]:              # a padded size below the window: the reference dies on its
                try:                                                      # patch-size assert, or finds no window to cut at all ((16, 10))
                    assert X.extract(x.copy(), kind) == [] and (h, w) == (16, 10)
                except AssertionError as e:
                    assert "Incorrect Patch Size" in str(e), (kind, h, w)
                with pytest.raises(ValueError, match="%d x %d" % (h, w)):
                    P.extract_host(x, WIN, STEP, kind)
                with pytest.raises(ValueError, match="%d x %d" % (h, w)):
                    P.patch_origins(h, w, WIN, STEP, kind)
                continue
            want, got = X.extract(x.copy(), kind), P.extract_host(x, WIN, STEP, kind)
            assert len(got) == len(want) == len(P.patch_origins(h, w, WIN, STEP, kind)), (kind, h, w)
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.dtype == b.dtype and a.shape == b.shape == WIN + (5,) and np.array_equal(a, b), (kind, h, w, k)
            seen[kind].add(_flags(h, w, kind))
            wraps += kind == "mirror" and (max(pt, pb) > h - 1 or max(pl, pr) > w - 1)
            if (h, w) in SIZES[:9]:
                total += len(want)
    assert total == 396                                                   # the nine first sizes, both kinds
    for kind in seen:
        assert seen[kind] == {(False, False), (False, True), (True, False), (True, True)}, (kind, seen[kind])
    assert wraps == 3                                                     # (8, 90), (33, 6), (8, 6): a pad wider than n - 1, more than one wrap


def test_refusals_and_order_without_the_reference():
    with pytest.raises(ValueError, match="8 x 90"):
        P.patch_origins(8, 90, WIN, STEP, "valid")
    with pytest.raises(ValueError, match="7 x 90"):
        P.patch_origins(7, 90, WIN, STEP, "mirror")
    with pytest.raises(ValueError, match="Unknown Patch Type"):
        P.patch_origins(30, 30, WIN, STEP, "same")
    with pytest.raises(ValueError):
        P.patch_origins(30, 30, (4, 4), (8, 8), "mirror")
    org = P.patch_origins(61, 47, WIN, STEP, "Mirror")
    assert org.dtype == np.int32 and org.shape == (64, 2) and org[0].tolist() == [-8, -8]
    # valid block 7 x 7 row-major, bottom-edge row (7), right-edge column (7), corner
    assert org[1].tolist() == [-8, -2] and org[7].tolist() == [0, -8]
    assert org[49:56, 0].tolist() == [61 + 9 - 25] * 7 and org[56:63, 1].tolist() == [47 + 8 - 22] * 7 and org[63].tolist() == [45, 33]
    assert P.refl([-3, -1, 0, 4, 5, 8, 9], 5).tolist() == [3, 1, 0, 4, 3, 0, 1] and P.refl([-7, 0, 3], 1).tolist() == [0, 0, 0]
    assert P.refl(np.arange(-6, 7), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]


def test_origins_and_patches_equal_the_committed_fixture():
    d = np.load(FIXTURE)
    win, step = tuple(d["win"]), tuple(d["step"])
    assert win == (9, 8) and step == (4, 3) and os.path.getsize(FIXTURE) < 100 * 1024
    n = 0
    for name, (h, w) in {"21x17": (21, 17), "4x12": (4, 12), "13x3": (13, 3)}.items():
        x = np.concatenate([d[name + "_img"], d[name + "_ann"]], axis=-1)
        assert x.shape == (h, w, 5) and x.dtype == np.int32
        for kind in ("mirror", "valid"):
            key = "%s_%s_" % (name, kind)
            if key + "refused" in d.files:
                with pytest.raises(ValueError, match="%d x %d" % (h, w)):
                    P.extract_host(x, win, step, kind)
                continue
            org, got = P.patch_origins(h, w, win, step, kind), P.extract_host(x, win, step, kind)
            assert org.dtype == d[key + "origins"].dtype and np.array_equal(org, d[key + "origins"]), key
            want = d[key + "patches"]
            assert len(got) == len(want) and all(g.dtype == want.dtype and np.array_equal(g, p) for g, p in zip(got, want)), key
            n += len(got)
    assert n == 36 + 16 + 4 + 4 and sum(k.endswith("refused") for k in d.files) == 2


@needs_reference
def test_recipe_regenerates_the_fixture(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", HVN_GOLDEN_OUT=str(tmp_path), MPLBACKEND="Agg")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-W", "ignore", os.path.join(REPO, "tools", "make_golden_patching.py")], capture_output=True, text=True,
                       env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.listdir(tmp_path) == ["patching_ref.npz"]
    new, old = np.load(tmp_path / "patching_ref.npz"), np.load(FIXTURE)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = new[k], old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.dtype != object and a.tobytes() == b.tobytes(), k


def _store_inputs(sizes, c=2, seed=0):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    anns = [rng.integers(0, 50, (h, w, c)).astype(np.int32) for h, w in sizes]
    return images, anns


def test_image_store_tables_on_the_host():
    sizes = [(61, 47), (8, 90), (8, 6)]
    images, anns = _store_inputs(sizes)
    st = P.ImageStore(images, anns, WIN, STEP, "mirror", device="cpu")
    assert st.n_patches == 64 + 15 + 1 and st.n_images == 3 and st.win == WIN and st.c == 2
    assert st.image_table["offset"].tolist() == [0, 61 * 47, 61 * 47 + 8 * 90] and st.total_pixels == 61 * 47 + 8 * 90 + 48
    assert st.first_patch.tolist() == [0, 64, 79, 80]
    assert st.nbytes == st.total_pixels * (3 + 2 * 4) + 3 * 16 + 80 * 12
    for i, (h, w) in enumerate(sizes):
        rows = st.patch_table[st.first_patch[i]:st.first_patch[i + 1]]
        assert (rows["image"] == i).all() and np.array_equal(np.stack([rows["row"], rows["col"]], 1), P.patch_origins(h, w, WIN, STEP, "mirror"))
    a = int(st.image_table["offset"][1])
    assert np.array_equal(st.pixels[a:a + 720].numpy().reshape(8, 90, 3), images[1]) and np.array_equal(st.ann[a:a + 720].numpy().reshape(8, 90, 2), anns[1])
    # what the constructor refuses
    with pytest.raises(ValueError, match="8 x 90"):
        P.ImageStore(images, anns, WIN, STEP, "valid", device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        P.ImageStore([images[0].astype(np.int32)], anns[:1], WIN, STEP, device="cpu")
    with pytest.raises(ValueError, match="annotation 0"):
        P.ImageStore(images[:1], [anns[0][:-1]], WIN, STEP, device="cpu")
    with pytest.raises(ValueError, match="planes"):
        P.ImageStore(images[:2], [anns[0], anns[1][..., :1]], WIN, STEP, device="cpu")
    with pytest.raises(ValueError):
        P.ImageStore(images, anns[:2], WIN, STEP, device="cpu")
    # what validate_tables refuses: every way a table could send the kernel outside the buffers
    ok_i, ok_p, total = st.image_table, st.patch_table, st.total_pixels
    P.validate_tables(ok_i, ok_p, total, WIN, STEP, "mirror")

    def bad(field, row, value, tab="patch", total_pixels=total, match=None):
        it, pt = ok_i.copy(), ok_p.copy()
        (pt if tab == "patch" else it)[field][row] = value
        with pytest.raises(ValueError, match=match):
            P.validate_tables(it, pt, total_pixels, WIN, STEP, "mirror")

    bad("image", 5, 3, match="image index")
    bad("image", 5, -1, match="image index")
    bad("image", 5, 1, match="patch_origins")
    bad("row", 70, 1, match="patch_origins")
    bad("col", 0, -9, match="patch_origins")
    bad("offset", 1, 61 * 47 + 1, tab="image", match="offset")
    bad("offset", 0, -1, tab="image", match="offset")
    bad("h", 2, 9, tab="image", match="does not fit|covers")
    bad("w", 1, 0, tab="image", match="positive")
    bad("h", 0, 61, tab="image", total_pixels=total - 1, match="does not fit")
    it = ok_i.copy()
    it["h"][2], it["w"][2] = 1 << 16, 1 << 15
    with pytest.raises(ValueError, match="2\\^31"):
        P.validate_tables(it, ok_p, total, WIN, STEP, "mirror")
    with pytest.raises(ValueError, match="rows"):
        P.validate_tables(ok_i, ok_p[:-1], total, WIN, STEP, "mirror")
    with pytest.raises(ValueError, match="src|source index"):
        from hover_net_amd.augment import identity_params

        P.augment_shape_images(st, identity_params(2, [0, 80]), WIN)        # refused before the device is asked for


def test_loader_bookkeeping_is_that_of_the_materialised_form():
    from hover_net_amd.augment import DevicePatchLoader

    images, anns = _store_inputs([(41, 40), (33, 6)])                         # 42 + 5 patches
    data = np.concatenate([np.stack(P.extract_host(np.concatenate([i, a], -1), WIN, STEP, "mirror")) for i, a in zip(images, anns)])
    assert data.shape == (47, 25, 22, 5)
    for mode in ("train", "valid"):
        for rank, world in ((0, 1), (1, 2)):
            a = DevicePatchLoader.from_images(images, anns, (16, 14), (8, 8), 4, win=WIN, step=STEP, kind="mirror", mode=mode, with_type=True,
                                              seed=3, device="cpu", rank=rank, world=world)
            b = DevicePatchLoader(data, (16, 14), (8, 8), 4, mode=mode, with_type=True, seed=3, device="cpu", rank=rank, world=world)
            assert (len(a), a.n_samples, a._source()) == (len(b), b.n_samples, b._source()) and a.store.n_patches == 47 and b.store is None
    with pytest.raises(AssertionError, match="type plane"):
        DevicePatchLoader.from_images(images, [a[..., :1] for a in anns], (16, 14), (8, 8), 4, win=WIN, step=STEP, with_type=True, device="cpu")


def _write_png(path, rgb):
    from PIL import Image

    Image.fromarray(rgb).save(path)


def test_dataset_parsers_round_trip(tmp_path):
    sio = pytest.importorskip("scipy.io")
    pytest.importorskip("PIL")
    from hover_net_amd.dataset import get_dataset

    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (13, 17, 3)).astype(np.uint8)
    inst = rng.integers(0, 9, (13, 17)).astype(np.float64)                 # the CoNSeP .mat files hold doubles
    types = np.arange(13 * 17).reshape(13, 17) % 8
    _write_png(str(tmp_path / "a.png"), rgb)
    sio.savemat(str(tmp_path / "a.mat"), {"inst_map": inst, "type_map": types.astype(np.float64)})
    merged = np.array([0, 1, 2, 3, 3, 4, 4, 4])[types]
    for name in ("kumar", "cpm17", "consep", "CoNSeP"):
        ds = get_dataset(name)
        img = ds.load_img(str(tmp_path / "a.png"))
        assert img.dtype == np.uint8 and np.array_equal(img, rgb)
        ann = ds.load_ann(str(tmp_path / "a.mat"))
        assert ann.dtype == np.int32 and ann.shape == (13, 17, 1) and np.array_equal(ann[..., 0], inst.astype(np.int32))
        if name.lower() == "consep":
            ann = ds.load_ann(str(tmp_path / "a.mat"), with_type=True)
            assert ann.dtype == np.int32 and ann.shape == (13, 17, 2)
            assert np.array_equal(ann[..., 0], inst.astype(np.int32)) and np.array_equal(ann[..., 1], merged)
            assert set(np.unique(ann[..., 1])) == {0, 1, 2, 3, 4}
        else:
            with pytest.raises(AssertionError, match="Not support"):
                ds.load_ann(str(tmp_path / "a.mat"), with_type=True)
    with pytest.raises(AssertionError, match="Unknown dataset `pannuke`"):
        get_dataset("pannuke")
    # the store takes what the parsers give
    st = P.ImageStore([img], [ann], (9, 8), (4, 3), "mirror", device="cpu")
    assert st.c == 2 and st.n_patches == len(P.patch_origins(13, 17, (9, 8), (4, 3), "mirror"))


def test_refusals_are_host_arithmetic():
    lib = L.lib()
    # refusals are host arithmetic: no device is touched.  Dummy non-null, aligned "pointers" are never dereferenced.
    p = ctypes.c_void_p(4096)

    def call(n_images=1, n_patches=1, total=100, wh=9, ww=8, c=2, n=1, oh=9, ow=8, images=p, status=p):
        return lib.hvn_augment_shape_images(p, p, images, p, n_images, n_patches, total, wh, ww, c, p, n, oh, ow, p, p, status, None)

    assert call(n_images=0) == -1 and call(n_patches=0) == -1 and call(total=0) == -1 and call(total=1 << 40) == -1
    assert call(wh=0) == -1 and call(ww=-1) == -1 and call(c=0) == -1 and call(c=5) == -1 and call(n=0) == -1
    assert call(oh=10) == -1 and call(ow=9) == -1 and call(oh=0) == -1
    assert call(images=None) == -1 and call(images=ctypes.c_void_p(4100)) == -1 and call(status=ctypes.c_void_p(4098)) == -1
    assert b"augment_shape_images" in lib.hvn_train_last_error()

"""-m gpu: training from whole images (`hover_net_amd/patching.py`, hvn_aug_shape_images_k in csrc/hvn_augment.hip): the extractor
through the training kernel against the host definition `patching.extract_host` and the reference's own patches
(tests/golden/patching_ref.npz); the gather, the loader and one training step against the same code fed from the materialised patch
set; the refusals and the kernel's index guards.  `==` everywhere."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIN, STEP = (25, 22), (8, 6)
# mirror: (8, 90) and (33, 6) are narrower than the pad, (8, 6) pads to exactly one window (no edge patch); valid: (25, 22) is one window
SIZES = {"mirror": [(61, 47), (8, 90), (33, 6), (8, 6), (41, 40)], "valid": [(61, 47), (41, 40), (25, 22), (30, 28), (33, 30)]}
_CACHE = {}


def _inputs(sizes, c, seed=0):
    rng = np.random.default_rng(seed)
    images = [rng.integers(1, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    anns = [rng.integers(1, 50, (h, w, c)).astype(np.int32) for h, w in sizes]
    return images, anns


def _case(kind, c):
    """(images, anns, store, materialised uint8 [P,25,22,3], int32 [P,25,22,c]): made once, shared, never written to."""
    from hover_net_amd import patching as P

    if (kind, c) not in _CACHE:
        images, anns = _inputs(SIZES[kind], c)
        both = np.concatenate([np.stack(P.extract_host(np.concatenate([i, a], -1), WIN, STEP, kind)) for i, a in zip(images, anns)])
        _CACHE[kind, c] = (images, anns, P.ImageStore(images, anns, WIN, STEP, kind), both[..., :3].astype(np.uint8), np.ascontiguousarray(both[..., 3:]))
    return _CACHE[kind, c]


@pytest.mark.parametrize("kind,c", [("mirror", 2), ("mirror", 1), ("valid", 2), ("valid", 1)])
def test_extract_device_equals_the_host_definition(kind, c):
    from hover_net_amd import patching as P

    _, _, store, want_img, want_ann = _case(kind, c)
    assert store.n_patches == len(want_img) == {"mirror": 64 + 15 + 5 + 1 + 42, "valid": 36 + 12 + 1 + 4 + 6}[kind] and store.c == c
    img, ann = P.extract_device(store)
    assert img.dtype == torch.uint8 and ann.dtype == torch.int32 and tuple(ann.shape) == (store.n_patches, 25, 22, c)
    np.testing.assert_array_equal(img.cpu().numpy(), want_img)
    np.testing.assert_array_equal(ann.cpu().numpy(), want_ann)
    idx = [store.n_patches - 1, 0, 40, 0]
    img, ann = P.extract_device(store, idx)
    np.testing.assert_array_equal(img.cpu().numpy(), want_img[idx])
    np.testing.assert_array_equal(ann.cpu().numpy(), want_ann[idx])
    assert int(store.status.item()) == 0


def test_extract_device_equals_the_references_patches(golden_dir):
    from hover_net_amd import patching as P

    d = np.load(os.path.join(golden_dir, "patching_ref.npz"))
    win, step = tuple(d["win"]), tuple(d["step"])
    names = ["21x17", "4x12", "13x3"]
    store = P.ImageStore([d[n + "_img"] for n in names], [d[n + "_ann"] for n in names], win, step, "mirror")
    img, ann = P.extract_device(store)
    got = np.concatenate([img.cpu().numpy().astype(np.int32), ann.cpu().numpy()], -1)
    np.testing.assert_array_equal(got, np.concatenate([d[n + "_mirror_patches"] for n in names]))
    store = P.ImageStore([d["21x17_img"]], [d["21x17_ann"]], win, step, "valid")
    img, ann = P.extract_device(store)
    np.testing.assert_array_equal(np.concatenate([img.cpu().numpy().astype(np.int32), ann.cpu().numpy()], -1), d["21x17_valid_patches"])


def _ten_records(n_patches):
    """The records of test_gpu_augment.test_shape_kernel_matches_oracle in the 25 x 22 patch frame."""
    from hover_net_amd import augment as G

    rng = np.random.default_rng(5)
    src = rng.integers(0, n_patches, 10)
    prm = G.draw_params(rng, src, WIN[0], WIN[1])
    prm[0] = G.identity_params(1, [n_patches - 1])[0]                                              # one plain centre crop
    prm["inv"][1] = np.linalg.inv(G.affine_matrix(WIN[0], WIN[1], (1, 1), (10, -12), 0, 0))[:2].reshape(-1)     # mostly outside -> zeros
    return prm


@pytest.mark.parametrize("kind,c", [("mirror", 2), ("valid", 1)])
def test_gather_equals_the_gather_over_the_materialised_set(kind, c):
    from hover_net_amd import augment as G
    from hover_net_amd import patching as P

    _, _, store, mat_img, mat_ann = _case(kind, c)
    prm = _ten_records(store.n_patches)
    oi, oa = P.augment_shape_images(store, prm, (16, 14))
    wi, wa = G.augment_shape(torch.from_numpy(mat_img).cuda(), torch.from_numpy(mat_ann).cuda(), prm, (16, 14))
    assert oi.shape == (10, 16, 14, 3) and oa.shape == (10, 16, 14, c) and oa.dtype == torch.int32
    assert torch.equal(oi, wi) and torch.equal(oa, wa)
    np.testing.assert_array_equal(oi[0].cpu().numpy(), mat_img[-1, 4:20, 4:18])
    assert float((oi[1] == 0).float().mean()) > 0.3 and float((oi[2:] != 0).float().mean()) > 0.5        # pixels are >= 1: zeros are "outside"
    assert int(store.status.item()) == 0


def test_source_index_out_of_range_is_refused_before_any_launch(monkeypatch):
    from hover_net_amd import patching as P

    store = _case("mirror", 2)[2]

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(P, "_launch", no_launch)
    for bad_src in (store.n_patches, -1):
        prm = _ten_records(store.n_patches)
        prm["src"][3] = bad_src
        with pytest.raises(ValueError, match="augment: source index outside the resident set of %d patches" % store.n_patches):
            P.augment_shape_images(store, prm, (16, 14))
        with pytest.raises(ValueError, match="outside the resident set"):
            P.extract_device(store, [0, bad_src])


def test_kernel_guards_every_index_it_reads():
    """The tables hold valid rows throughout (nothing is read outside an allocation); the counts DECLARED to the kernel are smaller, so
    a missing guard shows as a patch that comes back with its pixels instead of zeros."""
    from hover_net_amd import augment as G
    from hover_net_amd import patching as P

    _, _, store, mat_img, mat_ann = _case("mirror", 2)
    n = store.n_patches
    last_image = int(store.first_patch[-2])                                  # first patch of the last image, (41, 40)
    assert mat_img[n - 1].min() > 0 and mat_ann[n - 1].min() > 0

    def run(src, **declared):
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        img, ann = P._launch(store, G.identity_params(len(src), src), WIN, status=status, **declared)
        return img.cpu().numpy(), ann.cpu().numpy(), int(status.item())

    src = [3, n - 1, 0, n - 2]
    img, ann, status = run(src, n_patches=n - 1)                             # src = P - 1 is outside the declared table
    assert status == 1 and not img[1].any() and not ann[1].any()
    for k in (0, 2, 3):
        np.testing.assert_array_equal(img[k], mat_img[src[k]])
        np.testing.assert_array_equal(ann[k], mat_ann[src[k]])
    img, ann, status = run([n - 1, -1, n, 5], n_patches=n)                   # what Python refuses, handed to the kernel all the same
    assert status == 2 and not img[1:3].any() and not ann[1:3].any()
    np.testing.assert_array_equal(img[[0, 3]], mat_img[[n - 1, 5]])
    src = [last_image, 3, last_image - 1, n - 1]
    img, ann, status = run(src, n_images=store.n_images - 1)                 # the last image is outside the declared image table
    assert status == 2 and not img[[0, 3]].any() and not ann[[0, 3]].any()
    np.testing.assert_array_equal(img[[1, 2]], mat_img[[3, last_image - 1]])
    img, ann, status = run(src, total_pixels=store.total_pixels - 1)         # ... or ends one pixel past the declared buffer
    assert status == 2 and not img[[0, 3]].any() and not ann[[0, 3]].any()
    np.testing.assert_array_equal(ann[[1, 2]], mat_ann[[3, last_image - 1]])
    assert int(store.status.item()) == 0


@pytest.mark.parametrize("mode,rank,world", [("train", 0, 1), ("valid", 0, 1), ("train", 1, 2), ("valid", 1, 2)])
def test_loader_yields_the_batches_of_the_materialised_loader(mode, rank, world):
    from hover_net_amd import patching as P
    from hover_net_amd.augment import DevicePatchLoader

    images, anns = _inputs([(41, 40), (33, 6)], 2, seed=3)                   # 42 + 5 patches
    for a in anns:
        a[..., 0] = 0
        for i in range(1, 7):                                                # a few rectangular "nuclei": the targets have something to do
            y, x = (5 * i) % max(a.shape[0] - 8, 1), (7 * i) % max(a.shape[1] - 5, 1)
            a[y:y + 8, x:x + 5, 0] = i
    data = np.concatenate([np.stack(P.extract_host(np.concatenate([i, a], -1), WIN, STEP, "mirror")) for i, a in zip(images, anns)])
    kw = dict(mode=mode, with_type=True, seed=7, rank=rank, world=world)
    a = DevicePatchLoader.from_images(images, anns, (16, 14), (8, 8), 4, win=WIN, step=STEP, kind="mirror", **kw)
    b = DevicePatchLoader(data, (16, 14), (8, 8), 4, **kw)
    seen, batch = [], a.batch

    def recording(prm, **k):
        seen.append(prm.copy())
        return batch(prm, **k)

    a.batch = recording
    assert len(a) == len(b) and a.n_samples == b.n_samples
    for epoch in range(2):
        fa, fb = list(a), list(b)
        assert len(fa) == len(fb) == len(a) > 0
        for x, y in zip(fa, fb):
            assert set(x) == set(y) == {"img", "np_map", "hv_map", "tp_map"}
            for k in x:
                assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), (epoch, k)
        assert fa[0]["img"].shape[1:] == (16, 14, 3) and fa[0]["hv_map"].shape[1:] == (8, 8, 2)
    prm = np.concatenate(seen)
    if mode == "train":
        assert (prm["kind"] == 2).any() and (prm["kind"] != 2).any()          # noise records included
        assert len(prm) == 2 * (47 // world // 4) * 4
    else:
        assert sorted(prm["src"][:len(prm) // 2].tolist()) == list(range(rank, 47, world))
    assert float(sum(f["np_map"].sum() for f in fa)) > 0


def test_one_training_step_gives_the_bits_of_the_materialised_loader():
    """The training engine is deterministic by default: the same feed gives the same loss, bit for bit."""
    from hover_net_amd import net_desc, optim, run_desc
    from hover_net_amd import patching as P
    from hover_net_amd.augment import DevicePatchLoader
    from hover_net_amd.synth import synth_state_dict

    win, step = (280, 280), (90, 90)                                         # pad 95 on a 100-pixel image: 2 x 2 patches
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (100, 100, 3)).astype(np.uint8)
    ann = np.zeros((100, 100, 2), np.int32)
    for i in range(1, 9):
        y, x = rng.integers(0, 86), rng.integers(0, 86)
        ann[y:y + rng.integers(6, 14), x:x + rng.integers(6, 14)] = (i, rng.integers(1, 5))
    data = np.stack(P.extract_host(np.concatenate([img, ann], -1), win, step, "mirror"))
    assert data.shape == (4, 280, 280, 5)
    kw = dict(mode="train", with_type=True, seed=1)
    loaders = [DevicePatchLoader.from_images([img], [ann], (270, 270), (80, 80), 2, win=win, step=step, kind="mirror", **kw),
               DevicePatchLoader(data, (270, 270), (80, 80), 2, **kw)]
    sd = synth_state_dict("original", 5, seed=0)
    net = net_desc.create_model(mode="original", nr_types=5, input_ch=3, freeze=True)
    net.load_state_dict(sd, strict=True)
    net = net.to("cuda").train()
    loss_tab = {"np": {"bce": 1, "dice": 1}, "hv": {"mse": 1, "msge": 1}, "tp": {"bce": 1, "dice": 1}}
    ema = []
    for ld in loaders:
        net.load_state_dict(sd, strict=True)                                 # same weights and running statistics at the start of each step
        opt = optim.FusedAdam(filter(lambda p: p.requires_grad, net.parameters()), lr=1e-4)
        feed = next(iter(ld))
        ema.append(run_desc.train_step(feed, [{"net": {"desc": net, "optimizer": opt, "extra_info": {"loss": loss_tab}}}, {}])["EMA"])
    assert np.isfinite(ema[0]["overall_loss"]) and ema[0]["overall_loss"] > 0
    assert ema[0] == ema[1], (ema[0], ema[1])


def test_extract_patches_module_writes_the_host_definition(tmp_path):
    sio = pytest.importorskip("scipy.io")
    Image = pytest.importorskip("PIL.Image")
    from hover_net_amd import extract_patches as X
    from hover_net_amd import patching as P

    images, anns = _inputs([(41, 40), (33, 30)], 2, seed=8)
    for sub in ("Images", "Labels"):
        os.makedirs(tmp_path / sub)
    for name, img, ann in zip(("b_2", "a_1"), images, anns):
        Image.fromarray(img).save(str(tmp_path / "Images" / (name + ".png")))
        sio.savemat(str(tmp_path / "Labels" / (name + ".mat")), {"inst_map": ann[..., 0].astype(np.float64), "type_map": ann[..., 1] % 3})
    X.main(["--dataset", "consep", "--split", "train", str(tmp_path / "Images"), str(tmp_path / "Labels"), "--save-root", str(tmp_path / "out"),
            "--win", "25", "22", "--step", "8", "6", "--kind", "mirror"])
    out = tmp_path / "out" / "consep" / "train" / "25x22_8x6"
    want = {}
    for name, img, ann in zip(("b_2", "a_1"), images, anns):
        x = np.concatenate([img, np.stack([ann[..., 0], ann[..., 1] % 3], -1)], -1)
        for k, p in enumerate(P.extract_host(x, WIN, STEP, "mirror")):
            want["%s_%03d.npy" % (name, k)] = p
    assert sorted(os.listdir(out)) == sorted(want) and len(want) == 42 + 25
    for f, p in want.items():
        got = np.load(out / f)
        assert got.dtype == np.int32 and got.shape == (25, 22, 5) and got.tobytes() == np.ascontiguousarray(p).tobytes(), f

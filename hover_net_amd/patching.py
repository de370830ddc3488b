"""Training from whole images: `extract_patches.py` + `misc/patch_extractor.py` folded into the augmentation gather.

The reference prepares training data offline: `PatchExtractor.extract` (misc/patch_extractor.py:58-144) slides a `win` window with
stride `step` over every image (kind "valid"), or over the image reflect-padded by `win - step` (kind "mirror"), and
extract_patches.py:72-96 writes each window as an int32 `.npy` file.  With win 540 / step 164 every source pixel is then stored
about 14 times.  A patch is nothing but (image, row, col): `hvn_augment_shape_images` (csrc/hvn_augment.hip) takes that triple from
a device table and reads the whole image through the periodic mirror, so the patch set never exists -- not on disk, not in HBM.

    patch_origins   the extractor's geometry: which windows, in which order (host, numpy)
    extract_host    the extractor's result, restated as an index map -- THE DEFINITION the device path is held to, `==`
    ImageStore      images + annotations resident in HBM, ragged, with the image and patch tables
    augment_shape_images / extract_device   the gather (any parameter records / identity records = the extractor itself)

Parity: tests/test_patching_host.py (live reference and tests/golden/patching_ref.npz), tests/test_gpu_patching.py.  No CPU fallback."""
import numpy as np
import torch

from . import lib as L
from .augment import _upload, identity_params

IMAGE_DTYPE, PATCH_DTYPE = np.dtype(L.hvn_image_rec), np.dtype(L.hvn_patch_rec)


def _pair(v):
    a, b = v
    return int(a), int(b)


def pads(win, step, kind):
    """((top, bottom), (left, right)) of `__extract_mirror` (patch_extractor.py:122-128); zeros for "valid"."""
    kind = str(kind).lower()
    if kind == "valid":
        return (0, 0), (0, 0)
    if kind != "mirror":
        raise ValueError("Unknown Patch Type [%s]" % kind)
    (wh, ww), (sh, sw) = _pair(win), _pair(step)
    if wh < sh or ww < sw:
        raise ValueError("mirror patches need win >= step, got win %s step %s" % ((wh, ww), (sh, sw)))
    return ((wh - sh) // 2, (wh - sh) - (wh - sh) // 2), ((ww - sw) // 2, (ww - sw) - (ww - sw) // 2)


def patch_origins(h, w, win, step, kind):
    """int32 [P, 2] = (row, col) of every patch of an h x w image in UNPADDED coordinates (negative under "mirror"), in the order
    of `__extract_valid` (patch_extractor.py:83-107): the valid block row-major, the bottom-edge row, the right-edge column, the corner."""
    (wh, ww), (sh, sw) = _pair(win), _pair(step)
    if min(wh, ww, sh, sw) <= 0:
        raise ValueError("win and step must be positive, got win %s step %s" % ((wh, ww), (sh, sw)))
    (pt, pb), (pl, pr) = pads(win, step, kind)
    ph, pw = int(h) + pt + pb, int(w) + pl + pr
    if ph < wh or pw < ww:
        raise ValueError("image of %d x %d pixels (%d x %d with the %s pad) is smaller than the %d x %d window"
                         % (h, w, ph, pw, str(kind).lower(), wh, ww))

    def infos(length, win_size, step_size):
        return (length - win_size) % step_size != 0, ((length - win_size) // step_size + 1) * step_size

    h_flag, h_last = infos(ph, wh, sh)
    w_flag, w_last = infos(pw, ww, sw)
    rows, cols = range(0, h_last, sh), range(0, w_last, sw)
    out = [(r, c) for r in rows for c in cols]
    if h_flag:
        out += [(ph - wh, c) for c in cols]
    if w_flag:
        out += [(r, pw - ww) for r in rows]
    if h_flag and w_flag:
        out.append((ph - wh, pw - ww))
    return np.asarray(out, np.int32).reshape(-1, 2) - np.asarray([pt, pl], np.int32)


def refl(i, n):
    """numpy "reflect" as an index map: the periodic mirror without edge repeat, period 2(n - 1); n == 1 -> 0 (`hvn_reflect`)."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    j = np.mod(i, p)
    return np.where(j < n, j, p - j)


def extract_host(x, win, step, kind):
    """`PatchExtractor(win, step).extract(x, kind)` for x [H, W, ...]: the list of patches, without materialising a pad."""
    x = np.asarray(x)
    wh, ww = _pair(win)
    out = []
    for r, c in patch_origins(x.shape[0], x.shape[1], win, step, kind):
        rows, cols = refl(np.arange(r, r + wh), x.shape[0]), refl(np.arange(c, c + ww), x.shape[1])
        out.append(x[rows[:, None], cols[None, :]])
    return out


def validate_tables(image_tab, patch_tab, total_pixels, win, step, kind):
    """What the kernel is entitled to assume of the two tables, checked on the host before they are uploaded."""
    if image_tab.dtype != IMAGE_DTYPE or patch_tab.dtype != PATCH_DTYPE or image_tab.ndim != 1 or patch_tab.ndim != 1:
        raise ValueError("image / patch tables: IMAGE_DTYPE / PATCH_DTYPE records, one axis")
    if len(image_tab) == 0 or len(patch_tab) == 0:
        raise ValueError("image store: no images or no patches")
    end = 0
    for i, rec in enumerate(image_tab):
        h, w, off = int(rec["h"]), int(rec["w"]), int(rec["offset"])
        if h <= 0 or w <= 0 or h * w >= 2 ** 31:
            raise ValueError("image %d: %d x %d pixels (each side positive, H * W < 2^31)" % (i, h, w))
        if off != end or off + h * w > int(total_pixels):
            raise ValueError("image %d: offset %d + %d pixels does not fit the buffer of %d (previous image ends at %d)"
                             % (i, off, h * w, int(total_pixels), end))
        end = off + h * w
    if end != int(total_pixels):
        raise ValueError("image table covers %d pixels, the buffer holds %d" % (end, int(total_pixels)))
    if patch_tab["image"].min() < 0 or patch_tab["image"].max() >= len(image_tab):
        raise ValueError("patch table: image index outside the %d images" % len(image_tab))
    at = 0
    for i, rec in enumerate(image_tab):
        want = patch_origins(int(rec["h"]), int(rec["w"]), win, step, kind)
        got = patch_tab[at:at + len(want)]
        if len(got) != len(want) or (got["image"] != i).any() or (got["row"] != want[:, 0]).any() or (got["col"] != want[:, 1]).any():
            raise ValueError("patch table: rows %d.. are not image %d's patch_origins" % (at, i))
        at += len(want)
    if at != len(patch_tab):
        raise ValueError("patch table has %d rows, the images yield %d patches" % (len(patch_tab), at))


class ImageStore:
    """Whole images and their annotations resident on the device, back to back (ragged), plus the tables the gather reads:
    `images`: list of uint8 [H_i, W_i, 3]; `anns`: list of int32 [H_i, W_i, c], c = 1 (instance ids) or 2 (+ types), the same for all.
    Patch k of the store is patch k of the files extract_patches.py would write: images in list order, `patch_origins` order within."""

    def __init__(self, images, anns, win, step, kind="mirror", device="cuda"):
        if len(images) == 0 or len(images) != len(anns):
            raise ValueError("image store: %d images, %d annotations" % (len(images), len(anns)))
        self.win, self.step, self.kind = _pair(win), _pair(step), str(kind).lower()
        self.device = torch.device(device)
        self.c = None
        image_tab = np.zeros(len(images), IMAGE_DTYPE)
        tabs, first, total = [], [], 0
        for i, (img, ann) in enumerate(zip(images, anns)):
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise ValueError("image %d: uint8 [H, W, 3] expected, got %s %s" % (i, img.dtype, img.shape))
            if ann.dtype != np.int32 or ann.ndim != 3 or ann.shape[:2] != img.shape[:2] or ann.shape[2] not in (1, 2):
                raise ValueError("annotation %d: int32 %s + (1 | 2,) expected, got %s %s" % (i, img.shape[:2], ann.dtype, ann.shape))
            if self.c is None:
                self.c = int(ann.shape[2])
            if ann.shape[2] != self.c:
                raise ValueError("annotation %d has %d planes, the set's have %d" % (i, ann.shape[2], self.c))
            h, w = img.shape[:2]
            image_tab[i] = (total, h, w)
            org = patch_origins(h, w, self.win, self.step, self.kind)
            tab = np.zeros(len(org), PATCH_DTYPE)
            tab["image"], tab["row"], tab["col"] = i, org[:, 0], org[:, 1]
            first.append(sum(len(t) for t in tabs))
            tabs.append(tab)
            total += h * w
        patch_tab = np.concatenate(tabs)
        validate_tables(image_tab, patch_tab, total, self.win, self.step, self.kind)
        self.image_table, self.patch_table, self.total_pixels = image_tab, patch_tab, int(total)
        self.first_patch = np.asarray(first + [len(patch_tab)], np.int64)          # patches of image i: first_patch[i] .. first_patch[i + 1]
        self.pixels = torch.empty((total, 3), dtype=torch.uint8, device=self.device)
        self.ann = torch.empty((total, self.c), dtype=torch.int32, device=self.device)
        for rec, img, ann in zip(image_tab, images, anns):                           # one image at a time: no second host copy of the set
            a, b = int(rec["offset"]), int(rec["offset"]) + int(rec["h"]) * int(rec["w"])
            self.pixels[a:b] = torch.from_numpy(np.require(img, requirements=["C", "W"]).reshape(-1, 3)).to(self.device)
            self.ann[a:b] = torch.from_numpy(np.require(ann, requirements=["C", "W"]).reshape(-1, self.c)).to(self.device)
        self.image_dev, self.patch_dev = _upload(image_tab, self.device), _upload(patch_tab, self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)          # samples the kernel's guards zeroed, ever

    @property
    def n_images(self):
        return len(self.image_table)

    @property
    def n_patches(self):
        return len(self.patch_table)

    @property
    def nbytes(self):
        """Device bytes of the store: pixels, annotations and both tables."""
        return sum(int(t.numel()) * t.element_size() for t in (self.pixels, self.ann, self.image_dev, self.patch_dev))

    def check(self):
        """Raises if the kernel ever refused a sample of this store (reads one int32 back: call it per epoch, not per batch)."""
        bad = int(self.status.item())
        if bad:
            raise L.HvnError("hvn_augment_shape_images zeroed %d sample(s): an index left the store's tables" % bad)


def _launch(store, prm, out_hw, status=None, **declared):
    """One `hvn_augment_shape_images` launch.  `declared`: n_images / n_patches / total_pixels as DECLARED to the kernel (the store's by
    default; tests/test_gpu_patching.py declares fewer than the tables hold to see the kernel's guards work)."""
    L.require_gpu()
    assert store.pixels.is_cuda
    n = len(prm)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    dev = store.device
    prm_dev = _upload(prm, dev)
    oimg = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    oann = torch.empty((n, oh, ow, store.c), dtype=torch.int32, device=dev)
    status = store.status if status is None else status
    L.call("hvn_augment_shape_images", store.pixels.data_ptr(), store.ann.data_ptr(), store.image_dev.data_ptr(), store.patch_dev.data_ptr(),
           int(declared.get("n_images", store.n_images)), int(declared.get("n_patches", store.n_patches)),
           int(declared.get("total_pixels", store.total_pixels)),
           store.win[0], store.win[1], store.c, prm_dev.data_ptr(), n, oh, ow, oimg.data_ptr(), oann.data_ptr(),
           status.data_ptr(), L.stream_ptr(dev))
    return oimg, oann


def augment_shape_images(store, prm, out_hw):
    """`augment.augment_shape` over the patches of `store` without the patches: prm AUG_DTYPE records (src = patch index of the
    store) -> (uint8 [n,oh,ow,3], int32 [n,oh,ow,c]), equal to the gather over the materialised set bit for bit."""
    if len(prm) and (prm["src"].min() < 0 or prm["src"].max() >= store.n_patches):
        raise ValueError("augment: source index outside the resident set of %d patches" % store.n_patches)
    return _launch(store, prm, out_hw)


def extract_device(store, indices=None):
    """The materialised patches `indices` (all by default) of the store: identity records at out_hw = win, i.e. the extractor itself
    through the training kernel -> (uint8 [n,win_h,win_w,3], int32 [n,win_h,win_w,c])."""
    src = np.arange(store.n_patches) if indices is None else np.asarray(indices, np.int64).reshape(-1)
    img, ann = augment_shape_images(store, identity_params(len(src), src), store.win)
    store.check()
    return img, ann

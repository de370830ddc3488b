"""Generate tests/golden/patching_ref.npz with the REFERENCE's own misc/patch_extractor.py `PatchExtractor.extract` (imported through
oracle/refimport.py: reference first on sys.path, `__file__` asserted; oracle/cv2_shim ahead of it, since misc/ imports cv2 and the
extractor never calls it; matplotlib on the Agg backend).

Per case (CASES: image height, width) the fixture holds the seeded inputs `<case>_img` uint8 [h,w,3] and `<case>_ann` int32 [h,w,2] and,
per kind, what the reference makes of `np.concatenate([img, ann], -1)` with WIN / STEP -- extract_patches.py:81-82 --:
`<case>_<kind>_patches` int32 [P,9,8,5] in the reference's order and `<case>_<kind>_origins` int32 [P,2], or `<case>_<kind>_refused`
where the reference dies on its patch-size assert.  The origins are the reference's too: an image whose pixels are their own
coordinates, as large as the padded case, goes through the "valid" extractor (which is what `__extract_mirror` calls after padding),
and the pad before each axis is read off the first mirror patch of a coordinate image larger than the pad.  Arrays only.

    python tools/make_golden_patching.py       (HVN_GOLDEN_OUT=DIR writes elsewhere: tests/test_patching_host.py)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
from refimport import out_dir, ref_import, use_reference  # noqa: E402

WIN, STEP = (9, 8), (4, 3)
CASES = {"21x17": (21, 17), "4x12": (4, 12), "13x3": (13, 3)}      # an ordinary image; narrower than the pad in h; in w (numpy wraps twice)
KINDS = ("mirror", "valid")


def case_inputs(name):
    h, w = CASES[name]
    rng = np.random.default_rng([h, w])
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    ann = np.stack([rng.integers(0, 40, (h, w)), rng.integers(0, 5, (h, w))], -1).astype(np.int32)
    return img, ann


def coords(h, w):
    return np.stack(np.meshgrid(np.arange(h), np.arange(w), indexing="ij"), -1).astype(np.int32)


def main():
    use_reference(first=[os.path.join(REPO, "oracle", "cv2_shim")])
    import matplotlib

    matplotlib.use("Agg")
    if not hasattr(np.lib, "pad"):          # numpy >= 2 dropped the alias the reference pads with (patch_extractor.py:131)
        np.lib.pad = np.pad
    X = ref_import("misc.patch_extractor").PatchExtractor(WIN, STEP)
    pad_before = X.extract(coords(64, 64), "mirror")[0][0, 0]            # refl(-pad) == pad on an image larger than the pad
    diff = np.asarray(WIN) - np.asarray(STEP)
    out = {"win": np.asarray(WIN, np.int32), "step": np.asarray(STEP, np.int32)}
    for name, (h, w) in CASES.items():
        img, ann = case_inputs(name)
        out[name + "_img"], out[name + "_ann"] = img, ann
        for kind in KINDS:
            key = "%s_%s_" % (name, kind)
            try:
                patches = X.extract(np.concatenate([img, ann], axis=-1), kind)
            except AssertionError:
                out[key + "refused"] = np.ones(1, np.uint8)
                continue
            ph, pw = (h + diff[0], w + diff[1]) if kind == "mirror" else (h, w)
            org = np.asarray([p[0, 0] for p in X.extract(coords(ph, pw), "valid")], np.int32)
            out[key + "origins"] = org - (pad_before if kind == "mirror" else 0)
            out[key + "patches"] = np.asarray(patches)
            assert out[key + "patches"].dtype == np.int32 and len(org) == len(patches)
    np.savez_compressed(os.path.join(out_dir(), "patching_ref.npz"), **out)


if __name__ == "__main__":
    main()

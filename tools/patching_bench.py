"""Times one training batch read from WHOLE images (`DevicePatchLoader.from_images`, hvn_aug_shape_images_k) against the same batch
read from the materialised patch set (`DevicePatchLoader`, hvn_aug_shape_k: the form extract_patches.py feeds), on one GPU, and
reports what either form keeps resident.  Prints a small table plus ONE JSON line.  Records only: no threshold.

    python tools/patching_bench.py [--reps 20] [--images 27] [--size 1000] [--out FILE]

set         --images synthetic images of --size x --size pixels with instance and type planes; win 540, step 164, "mirror" (the
            reference's extract_patches.py settings: 49 patches per 1000 x 1000 image); 'original' mode shapes 540 -> 270 -> 80, batch 16
batch       DevicePatchLoader.batch on --reps different batches of "train" records (affine + flips + blur / noise + colour + targets),
            the SAME records and noise generator seed for both forms, HIP events around the call:
            patches_ms    the materialised set (built on the device with patching.extract_device; this code path is the parent's)
            images_ms     the image store
            the feed dicts are compared with == first; the legs alternate inside one loop; median [min .. max] after 3 warm-ups
gather      the two shape kernels alone on those records (augment.augment_shape / patching.augment_shape_images), HIP events
bytes       device bytes of the two resident forms
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WIN, STEP, KIND = (540, 540), (164, 164), "mirror"
ACT, OUT, BATCH = (270, 270), (80, 80), 16


def stat(xs, nd=4):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def synthetic_images(n, size, nt=5, seed=0):
    """Random pixels; ~one disk-shaped "nucleus" of radius 5..11 per 1800 pixels, with an id and a type."""
    rng = np.random.default_rng(seed)
    images, anns = [], []
    for _ in range(n):
        ann = np.zeros((size, size, 2), np.int32)
        for i in range(1, max(8, size * size // 1800) + 1):
            r = int(rng.integers(5, 12))
            cy, cx = (int(v) for v in rng.integers(r, size - r, 2))
            yy, xx = np.ogrid[-r:r + 1, -r:r + 1]
            box = ann[cy - r:cy + r + 1, cx - r:cx + r + 1]
            box[yy * yy + xx * xx <= r * r] = (i, i % nt + 1)
        images.append(rng.integers(0, 256, (size, size, 3)).astype(np.uint8))
        anns.append(ann)
    return images, anns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=27)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    import torch

    from hover_net_amd import augment as G
    from hover_net_amd import lib as L
    from hover_net_amd import patching as P

    L.require_gpu()
    images, anns = synthetic_images(args.images, args.size)
    kw = dict(mode="train", with_type=True, seed=0)
    a = G.DevicePatchLoader.from_images(images, anns, ACT, OUT, BATCH, win=WIN, step=STEP, kind=KIND, **kw)
    store = a.store
    # the materialised set, cut on the device one image at a time (on the host it is 3 + c int32 planes per patch pixel)
    b = G.DevicePatchLoader(np.zeros((1,) + WIN + (5,), np.int32), ACT, OUT, BATCH, **kw)
    b.img = torch.empty((store.n_patches,) + WIN + (3,), dtype=torch.uint8, device="cuda")
    b.ann = torch.empty((store.n_patches,) + WIN + (2,), dtype=torch.int32, device="cuda")
    for i in range(store.n_images):
        lo, hi = int(store.first_patch[i]), int(store.first_patch[i + 1])
        b.img[lo:hi], b.ann[lo:hi] = P.extract_device(store, np.arange(lo, hi))
    rng = np.random.default_rng(1)
    records = [G.draw_params(rng, rng.integers(0, store.n_patches, BATCH), WIN[0], WIN[1]) for _ in range(args.reps + 3)]

    def gen():
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        return g

    fa, fb = a.batch(records[0], generator=gen()), b.batch(records[0], generator=gen())
    assert set(fa) == set(fb) and all(torch.equal(fa[k], fb[k]) for k in fa), "the two forms yield different batches"

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {"patches_ms": [], "images_ms": [], "gather_patches_ms": [], "gather_images_ms": []}
    for it, prm in enumerate(records):
        t = {"patches_ms": events(lambda: b.batch(prm, generator=gen())),
             "images_ms": events(lambda: a.batch(prm, generator=gen())),
             "gather_patches_ms": events(lambda: G.augment_shape(b.img, b.ann, prm, ACT)),
             "gather_images_ms": events(lambda: P.augment_shape_images(store, prm, ACT))}
        if it >= 3:
            for k, v in t.items():
                legs[k].append(v)
    store.check()
    res = {k: stat(v) for k, v in legs.items()}
    patch_bytes = int(b.img.numel()) + 4 * int(b.ann.numel())
    res.update({"tool": "patching_bench", "reps": args.reps, "images": args.images, "size": args.size, "patches": store.n_patches, "batch": BATCH,
                "win": list(WIN), "step": list(STEP), "kind": KIND, "patch_set_bytes": patch_bytes, "image_store_bytes": store.nbytes,
                "images_over_patches": round(res["images_ms"]["median"] / res["patches_ms"]["median"], 4)})
    lines = ["training batch from whole images against the materialised patch set, %s (%s); median [min .. max] of %d warm runs"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, args.reps),
             "set       %d images of %d x %d -> %d patches (win %d, step %d, %s); batch %d, %d -> %d -> %d, with types"
             % (args.images, args.size, args.size, store.n_patches, WIN[0], STEP[0], KIND, BATCH, WIN[0], ACT[0], OUT[0])]
    for k, what in (("patches_ms", "batch     DevicePatchLoader.batch, materialised set"), ("images_ms", "batch     DevicePatchLoader.batch, image store"),
                    ("gather_patches_ms", "gather    hvn_augment_shape alone"), ("gather_images_ms", "gather    hvn_augment_shape_images alone")):
        lines.append("%-52s %9.4f  [%9.4f .. %9.4f] ms" % (what, res[k]["median"], res[k]["min"], res[k]["max"]))
    lines.append("batch     image store / materialised set (medians): %.4f" % res["images_over_patches"])
    lines.append("bytes     materialised set %.3f GB, image store %.3f GB (%.1f x)" % (patch_bytes / 1e9, store.nbytes / 1e9, patch_bytes / store.nbytes))
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

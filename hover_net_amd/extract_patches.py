"""extract_patches.py of the reference, for those who want the files: every image of a split is cut into `win` windows with stride
`step` ("mirror": over the reflect-padded image; "valid": inside it) and each window is written as int32 [win_h, win_w, 3 + c]
(RGB, instance id, type) to

    <save_root>/<dataset>/<split>/<win_h>x<win_w>_<step_h>x<step_w>/<base>_<idx:03d>.npy            (extract_patches.py:53-94)

The windows come from `patching.extract_device`, i.e. from the kernel the training loader gathers with, and equal
`patching.extract_host` on the concatenated [img | ann] array byte for byte.  Training itself does not need the files:
`train.image_loaders` reads the whole images.

    python -m hover_net_amd.extract_patches --dataset consep --split train Train/Images Train/Labels \\
        --split valid Test/Images Test/Labels --save-root dataset/training_data
"""
import argparse
import glob
import os
import pathlib
import re
import shutil

import numpy as np

from . import patching
from .dataset import get_dataset


def extract_split(parser, img_dir, ann_dir, out_dir, win=(540, 540), step=(164, 164), kind="mirror", with_type=True, img_ext=".png",
                  ann_ext=".mat", device="cuda"):
    """One split: the annotation files of `ann_dir` in sorted order, the image of the same stem from `img_dir`.  `out_dir` is
    emptied first (rm_n_mkdir).  Returns the number of files written."""
    pattern = re.sub(r"([\[\]])", "[\\1]", "%s/*%s" % (ann_dir, ann_ext))
    files = sorted(glob.glob(pattern))
    if os.path.isdir(out_dir):
        shutil.rmtree(out_dir)
    os.makedirs(out_dir)
    written = 0
    for path in files:
        base = pathlib.Path(path).stem
        img = parser.load_img("%s/%s%s" % (img_dir, base, img_ext))
        ann = parser.load_ann(path, with_type)
        store = patching.ImageStore([img], [ann], win, step, kind, device=device)          # one image resident at a time
        pimg, pann = patching.extract_device(store)
        both = np.concatenate([pimg.cpu().numpy().astype(np.int32), pann.cpu().numpy()], axis=-1)
        for idx, patch in enumerate(both):
            np.save("%s/%s_%03d.npy" % (out_dir, base, idx), patch)
        written += len(both)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", default="consep", help="kumar | cpm17 | consep")
    ap.add_argument("--split", nargs=3, action="append", metavar=("NAME", "IMG_DIR", "ANN_DIR"), required=True)
    ap.add_argument("--save-root", required=True)
    ap.add_argument("--win", type=int, nargs=2, default=(540, 540))
    ap.add_argument("--step", type=int, nargs=2, default=(164, 164))
    ap.add_argument("--kind", choices=("mirror", "valid"), default="mirror")
    ap.add_argument("--no-type", action="store_true", help="instance ids only (Kumar and CPM17 have no type labels)")
    ap.add_argument("--img-ext", default=".png")
    ap.add_argument("--ann-ext", default=".mat")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    parser = get_dataset(a.dataset)
    for name, img_dir, ann_dir in a.split:
        out_dir = "%s/%s/%s/%dx%d_%dx%d" % (a.save_root, a.dataset, name, a.win[0], a.win[1], a.step[0], a.step[1])
        n = extract_split(parser, img_dir, ann_dir, out_dir, tuple(a.win), tuple(a.step), a.kind, not a.no_type, a.img_ext, a.ann_ext, a.device)
        print("%s: %d patches -> %s" % (name, n, out_dir))


if __name__ == "__main__":
    main()

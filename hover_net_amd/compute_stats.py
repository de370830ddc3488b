"""The reference's compute_stats.py scoring entry points, batched through hover_net_amd.metrics.

    python -m hover_net_amd.compute_stats --mode instance|type --pred_dir DIR --true_dir DIR

run_nuclei_inst_stat   every image's (dice1, aji, dq, sq, pq, aji_plus) row from ONE pair-table pass per group of maps of
                       equal shape (`metrics.instance_stats`; on the GPU when one is available): the [6, N] array and the printed
                       lines of the reference's function.
run_nuclei_type_stat   detection / type F1 from centroid pairing (`metrics.pair_coordinates`, host): the reference's printed line
                       and return value (None).

Reads the `.mat` files InferManager writes (`inst_map`, `inst_centroid`, `inst_type`); needs scipy.io, not cv2 or pandas.
"""
import argparse
import glob
import os

import numpy as np

from .metrics import instance_stats, pair_coordinates

_PRINT = {"formatter": {"float": "{: 0.5f}".format}}


def _loadmat(path):
    import scipy.io as sio

    return sio.loadmat(path)


def _centroids_and_types(info):
    """(centroids float32 [k, 2], types [k]); an image without instances counts as one point (0, 0) of type 0, as in the reference."""
    cen = info["inst_centroid"].astype("float32")
    typ = info["inst_type"].astype("int32")
    if cen.shape[0] == 0:
        return np.array([[0, 0]]), np.array([0])
    return cen, typ[:, 0]


def run_nuclei_type_stat(pred_dir, true_dir, type_uid_list=None, exhaustive=True):
    files = sorted(glob.glob(pred_dir + "*.mat"))
    paired_all, unpaired_true_all, unpaired_pred_all, true_type_all, pred_type_all = [], [], [], [], []
    true_off = pred_off = 0
    for k, f in enumerate(files):
        base = os.path.basename(f).split(".")[0]
        true_cen, true_type = _centroids_and_types(_loadmat(os.path.join(true_dir, base + ".mat")))
        pred_cen, pred_type = _centroids_and_types(_loadmat(os.path.join(pred_dir, base + ".mat")))
        paired, unpaired_true, unpaired_pred = pair_coordinates(true_cen, pred_cen, 12)
        if k:                                             # indices run over the instances of all images
            true_off += true_type_all[-1].shape[0]
            pred_off += pred_type_all[-1].shape[0]
        true_type_all.append(true_type)
        pred_type_all.append(pred_type)
        if paired.shape[0] != 0:
            paired[:, 0] += true_off
            paired[:, 1] += pred_off
            paired_all.append(paired)
        unpaired_true_all.append(unpaired_true + true_off)
        unpaired_pred_all.append(unpaired_pred + pred_off)

    paired_all = np.concatenate(paired_all, axis=0)
    true_type_all = np.concatenate(true_type_all, axis=0)
    pred_type_all = np.concatenate(pred_type_all, axis=0)
    paired_true_type = true_type_all[paired_all[:, 0]]
    paired_pred_type = pred_type_all[paired_all[:, 1]]
    unpaired_true_type = true_type_all[np.concatenate(unpaired_true_all, axis=0)]
    unpaired_pred_type = pred_type_all[np.concatenate(unpaired_pred_all, axis=0)]

    def f1_type(type_id, w):
        sel = (paired_true_type == type_id) | (paired_pred_type == type_id)
        pt, pp = paired_true_type[sel], paired_pred_type[sel]
        tp_dt = ((pt == type_id) & (pp == type_id)).sum()
        tn_dt = ((pt != type_id) & (pp != type_id)).sum()
        fp_dt = ((pt != type_id) & (pp == type_id)).sum()
        fn_dt = ((pt == type_id) & (pp != type_id)).sum()
        if not exhaustive:
            fp_dt -= (pt == -1).sum()
        fp_d = (unpaired_pred_type == type_id).sum()
        fn_d = (unpaired_true_type == type_id).sum()
        return (2 * (tp_dt + tn_dt)) / (2 * (tp_dt + tn_dt) + w[0] * fp_dt + w[1] * fn_dt + w[2] * fp_d + w[3] * fn_d)

    tp_d, fp_d, fn_d = paired_pred_type.shape[0], unpaired_pred_type.shape[0], unpaired_true_type.shape[0]
    tp_tn_dt = (paired_pred_type == paired_true_type).sum()
    fp_fn_dt = (paired_pred_type != paired_true_type).sum()
    if not exhaustive:
        fp_fn_dt -= (paired_true_type == -1).sum()
    acc_type = tp_tn_dt / (tp_tn_dt + fp_fn_dt)
    f1_d = 2 * tp_d / (2 * tp_d + 1 * fp_d + 1 * fn_d)
    if type_uid_list is None:
        type_uid_list = np.unique(true_type_all).tolist()
    results = [f1_d, acc_type] + [f1_type(u, [2, 2, 1, 1]) for u in type_uid_list]
    with np.printoptions(**_PRINT):
        print(np.array(results))
    return None


def run_nuclei_inst_stat(pred_dir, true_dir, print_img_stats=False, ext=".mat", *, device=None):
    print(pred_dir)
    names, true, pred = [], [], []
    for f in sorted(glob.glob("%s/*%s" % (pred_dir, ext))):
        base = os.path.basename(f).split(".")[0]
        names.append(base)
        true.append(_loadmat(os.path.join(true_dir, base + ".mat"))["inst_map"].astype("int32"))
        pred.append(_loadmat(os.path.join(pred_dir, base + ".mat"))["inst_map"].astype("int32"))
    rows = instance_stats(true, pred, remap=True, device=device)
    if print_img_stats:
        for base, row in zip(names, rows):
            print(base, end="\t")
            for v in row:
                print("%f " % v, end="  ")
            print()
    metrics = np.ascontiguousarray(rows.T)
    with np.printoptions(**_PRINT):
        print(np.mean(metrics, axis=-1))
    return metrics


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", help="`instance` (segmentation) or `type` (classification)", nargs="?", default="instance", const="instance")
    ap.add_argument("--pred_dir", help="directory of predicted .mat files", nargs="?", default="", const="")
    ap.add_argument("--true_dir", help="directory of ground-truth .mat files", nargs="?", default="", const="")
    args = ap.parse_args(argv)
    if args.mode == "instance":
        run_nuclei_inst_stat(args.pred_dir, args.true_dir, print_img_stats=False)
    if args.mode == "type":
        run_nuclei_type_stat(args.pred_dir, args.true_dir)


if __name__ == "__main__":
    main()

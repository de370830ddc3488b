"""How each public dataset stores its images and annotations: the reference's dataset.py (`get_dataset` for Kumar, CPM17 and
CoNSeP), which extract_patches.py and now `DevicePatchLoader.from_images` / `train.image_loaders` read whole images through.

    load_img(path)                  uint8 RGB [H, W, 3]                      (dataset.py:31-32: cv2.imread + BGR2RGB)
    load_ann(path, with_type)       int32 [H, W, 1] instance ids, or [H, W, 2] with the type map (CoNSeP only)

Host code only (PIL for the image, scipy.io for the `.mat` annotation)."""
import numpy as np

from .infer_manager import read_image


class _AbstractDataset(object):
    def load_img(self, path):
        return read_image(path)

    def load_ann(self, path, with_type=False):
        raise NotImplementedError


def _inst_only(path, with_type):
    """dataset.py:34-40 / :56-62: `inst_map` of the `.mat` file, HxW -> int32 [H, W, 1]; these sets carry no type labels."""
    import scipy.io as sio

    assert not with_type, "Not support"
    return np.expand_dims(sio.loadmat(path)["inst_map"].astype("int32"), -1)


class _Kumar(_AbstractDataset):
    """Kumar et al., IEEE TMI 36(7), 2017."""

    def load_ann(self, path, with_type=False):
        return _inst_only(path, with_type)


class _CPM17(_AbstractDataset):
    """Vu et al., Front. Bioeng. Biotechnol. 7, 2019."""

    def load_ann(self, path, with_type=False):
        return _inst_only(path, with_type)


class _CoNSeP(_AbstractDataset):
    """Graham et al., Medical Image Analysis 58, 2019."""

    def load_ann(self, path, with_type=False):
        import scipy.io as sio

        mat = sio.loadmat(path)
        ann_inst = mat["inst_map"]
        if not with_type:
            return np.expand_dims(ann_inst, -1).astype("int32")
        ann_type = mat["type_map"].copy()
        # dataset.py:84-87: the paper uses 3 nuclear classes + "other": 3|4 -> 3 first, then 5|6|7 -> 4
        ann_type[(ann_type == 3) | (ann_type == 4)] = 3
        ann_type[(ann_type == 5) | (ann_type == 6) | (ann_type == 7)] = 4
        return np.dstack([ann_inst, ann_type]).astype("int32")


def get_dataset(name):
    """The parser of a pre-defined dataset (dataset.py:99-109; any letter case -- the reference lower-cases the name for the test and
    then reads its table with the name as given, a KeyError for "CoNSeP")."""
    name_dict = {"kumar": _Kumar, "cpm17": _CPM17, "consep": _CoNSeP}
    if name.lower() in name_dict:
        return name_dict[name.lower()]()
    assert False, "Unknown dataset `%s`" % name

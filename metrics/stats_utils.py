"""Drop-in for the reference's metrics/stats_utils.py: the same names and signatures, scored by hover_net_amd.metrics (pair table on the GPU)."""
from hover_net_amd.metrics import get_dice_1, get_dice_2, get_fast_aji, get_fast_aji_plus, get_fast_dice_2, get_fast_pq, pair_coordinates, remap_label  # noqa: F401

"""Drop-in for /root/reference/models/hovernet/run_desc.py: `train_step` (:12-109), `valid_step` (:113-167),
`infer_step` (:171-197), `viz_step_output` (:201-256, numpy only: no matplotlib, no cv2), `proc_valid_step_output` (:262-344; the
picture half with `image=True`) -> hover_net_amd.run_desc.  `valid_step_stats` and `viz_step_output_device` have no counterpart
there: `valid_step` with the statistics accumulated on the device (hover_net_amd.valid_stats), and the picture drawn on the device."""
from hover_net_amd.run_desc import (infer_step, proc_valid_step_output, train_step, valid_step, valid_step_stats,  # noqa: F401
                                    viz_step_output, viz_step_output_device)

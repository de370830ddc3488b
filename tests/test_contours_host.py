"""CPU: host-side contract of the device contour tracer -- like every GPU stage it refuses to run off a gfx950 device."""
import numpy as np
import pytest
import torch

from hover_net_amd import lib as L
from hover_net_amd import post_proc as PP


def test_trace_contours_device_has_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(L.lib(), "hvn_device_ok", lambda: 0)          # the answer of a machine without the device
    inst = torch.zeros((1, 8, 9), dtype=torch.int32)
    rec = torch.zeros((1, 6, PP._REC_DTYPE.itemsize), dtype=torch.uint8)
    with pytest.raises(L.HvnError, match="no CPU fallback"):
        PP.trace_contours_device(inst, rec)


def test_split_contours_is_the_flat_form_per_map():
    pts = np.arange(14, dtype=np.int32).reshape(7, 2)
    offs = np.array([0, 2, 2, 3, 3, 7, 7], np.int64)                 # two maps of three slots
    (p0, o0), (p1, o1) = PP.split_contours(pts, offs, 2, 3)
    assert o0.tolist() == [0, 2, 2, 3] and p0.tolist() == pts[:3].tolist()
    assert o1.tolist() == [0, 0, 4, 4] and p1.tolist() == pts[3:].tolist()
    assert PP.check_contour_status(np.array([0, 1, -1, 0], np.int32), 3) is True
    with pytest.raises(L.HvnError, match="map 1, label 3"):
        PP.check_contour_status(np.array([2, 0, 5, 0], np.int32), 3)

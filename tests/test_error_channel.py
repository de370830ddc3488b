"""CPU: the library has one error channel.  Every entry point that returns a nonzero status leaves its own text in hvn_last_error(),
leading with its name, and hvn_train_last_error() is the same buffer: L.call can quote it for any export.

Every refusal exercised here is decided on the host before anything touches a device, with pointers that are never dereferenced; like
tests/test_conv_launch_refusals.py the module skips where a GPU is present, so that made-up arguments are never near one."""
import ctypes

import pytest
import torch

from hover_net_amd import lib as L
from test_conv_launch_refusals import conv_op

E_ARG, E_SIZE = -1, -4
POISON = b"unknown op kind"
# exports that return an int / long which is no hvn_status
NOT_STATUS = ("hvn_version", "hvn_device_ok", "hvn_profile_enable", "hvn_profile_conv_launches", "hvn_profile_conv_ms_list", "hvn_loss_partials_count")
STATUS_EXPORTS = [n for n, (restype, _) in L.PROTOS.items() if restype in (ctypes.c_int, ctypes.c_long) and n not in NOT_STATUS]
PLAN_RUNNERS = ("hvn_run_train_plan", "hvn_run_train_plan_ws")     # the first is the second without a workspace: the text names that one


def lib():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: calls with made-up arguments must not be launched")
    return L.lib()


def poison(l):
    """An earlier failure on this thread, whose text no later refusal may repeat."""
    op = L.hvn_op()
    op.kind = 99
    assert l.hvn_run_op(ctypes.byref(op), 1, None) == E_ARG and POISON in l.hvn_last_error()


def own_text(l, name):
    err = l.hvn_last_error()
    assert POISON not in err, (name, err)
    assert l.hvn_train_last_error() == err, (name, err, l.hvn_train_last_error())
    return err


def test_the_exports_under_test_are_the_status_returning_ones():
    assert len(STATUS_EXPORTS) == 32 and "hvn_postproc" in STATUS_EXPORTS and "hvn_trace_contours" in STATUS_EXPORTS
    assert not set(NOT_STATUS) - set(L.PROTOS)


@pytest.mark.parametrize("name", STATUS_EXPORTS)
def test_a_refusal_of_all_zero_arguments_has_its_own_text(name):
    l = lib()
    poison(l)
    args = [None if t is ctypes.c_void_p else t(0).value for t in L.PROTOS[name][1]]
    assert getattr(l, name)(*args) < 0
    err, short = own_text(l, name), name[len("hvn_"):].encode()
    assert short in err if name in PLAN_RUNNERS else err.startswith(short + b":"), (name, err)


def P(i):
    return 0x10000000 + (i << 20)        # 16-byte aligned, never dereferenced


N, H, W, WS = 1, 16, 16, 16              # one 16 x 16 map and a 16-byte workspace
OUT10, DOT = (ctypes.c_longlong * 10)(), (ctypes.c_uint8 * 3)()
SHORT_WORKSPACE = {
    "hvn_postproc": (P(0), N, H, W, 4, 1, P(1), P(2), WS, None),
    "hvn_postproc_taps": (P(0), N, H, W, 4, 1, P(1), None, None, None, P(2), WS, None),
    "hvn_postproc_stats": (P(2), WS, N, H, W, ctypes.addressof(OUT10), None),
    "hvn_instance_table": (P(1), P(0), N, H, W, 4, 5, P(3), P(4), 8, P(2), WS, None),
    "hvn_pair_table": (P(0), P(1), N, H, W, P(3), P(4), P(2), WS, None),
    "hvn_remap_label": (P(0), N, H, W, 100, P(1), P(3), P(2), WS, None),
    "hvn_trace_contours_device": (P(1), N, H, W, P(3), 8, P(4), 64, P(5), P(6), P(2), WS, None),
    "hvn_draw_overlay": (P(0), P(1), N, H, W, P(3), 0, P(4), 8, P(5), None, 1, 0, ctypes.addressof(DOT), P(6), P(2), WS, None),
    "hvn_tissue_mask": (P(0), H, W, 127, 10, 10, 2, P(1), None, None, P(2), WS, None),
    "hvn_valid_stats": (P(0), P(1), P(3), P(4), N, H, W, 4, 5, P(5), P(6), P(2), WS, None),
    "hvn_gen_targets": (P(0), N, H, W, 8, 8, P(1), P(3), P(2), WS, None),
}


@pytest.mark.parametrize("name", SHORT_WORKSPACE)
def test_a_short_workspace_is_refused_by_name(name):
    l = lib()
    poison(l)
    assert getattr(l, name)(*SHORT_WORKSPACE[name]) == E_SIZE
    err = own_text(l, name)
    assert name[len("hvn_"):].encode() in err and b"workspace" in err, (name, err)


def test_a_launcher_refusal_keeps_its_status_and_gets_a_text():
    l = lib()
    poison(l)
    # the API layer has no check of cout's multiple: hvn_launch_conv_bf16 refuses 100 output channels (not a multiple of the 8 of a 16-byte store)
    assert l.hvn_run_op(ctypes.byref(conv_op(1, 128, cout=100)), 2, None) == E_ARG
    assert b"conv" in own_text(l, "hvn_run_op")

"""CPU: what the implicit-GEMM launchers refuse, through the public hvn_run_op.

Every refusal of hvn_launch_conv / _x3 / _x3g / _bf16 / _bf16g is decided on the host before anything touches the device, and comes back
as HVN_E_ARG (-1).  A descriptor that passes them goes on to set the kernel's LDS attribute, which without a device fails as
HVN_E_LAUNCH (-2).  So on a machine without a GPU the two codes tell "refused" from "would have launched", with pointers that are never
dereferenced.  The kernels rely on these checks (16-byte stores of 8 bf16 / 4 fp32 channels, 32-bit byte offsets into x, x2, y and res)."""
import ctypes

import pytest
import torch

from hover_net_amd import lib as L

E_ARG, E_LAUNCH = -1, -2
BASE = 0x10000000          # 16-byte aligned, never dereferenced
# (name, act_dtype, tile_n, element bytes, channels per 16-byte store, 32-bit offsets into y / res)
LAUNCHERS = [("f32", 0, 128, 4, 4, False), ("x3", 2, 128, 4, 4, True), ("x3g128", 2, 640, 4, 4, True), ("x3g256", 3, 896, 4, 4, True),
             ("bf16", 1, 128, 2, 8, True), ("bf16g128", 1, 640, 2, 8, True), ("bf16g256", 1, 896, 2, 8, True)]
IDS = [l[0] for l in LAUNCHERS]


def view(base, h, w, c):
    return L.hvn_view(base=base, sn=h * w * c, sy=w * c, sx=c, h=h, w=w, c=c, sc=1)


def conv_op(act_dtype, tile_n, cin=128, cout=128, hw=32, res=False):
    op = L.hvn_op()
    op.kind, op.kh, op.kw, op.stride, op.cout, op.tile_n, op.act_dtype, op.groups = 2, 1, 1, 1, cout, tile_n, act_dtype, 1
    op.x = view(BASE, hw, hw, cin)
    op.y = view(BASE + (1 << 26), hw, hw, cout)
    if res:
        op.res = view(BASE + (2 << 26), hw, hw, cout)
    op.w = BASE + (3 << 26)
    return op


def run(op, batch=2):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: a descriptor with made-up pointers must not be launched")
    return L.lib().hvn_run_op(ctypes.byref(op), batch, None)


@pytest.mark.parametrize("name,dt,tn,es,piece,out32", LAUNCHERS, ids=IDS)
def test_a_well_formed_conv_passes_every_host_check(name, dt, tn, es, piece, out32):
    assert run(conv_op(dt, tn)) == E_LAUNCH
    assert run(conv_op(dt, tn, res=True)) == E_LAUNCH


@pytest.mark.parametrize("name,dt,tn,es,piece,out32", LAUNCHERS, ids=IDS)
def test_cout_must_be_a_multiple_of_the_16_byte_store(name, dt, tn, es, piece, out32):
    assert run(conv_op(dt, tn, cout=128 + piece // 2)) == E_ARG       # 130 for fp32, 132 for bf16
    if piece == 8 and "g" not in name:
        assert run(conv_op(dt, tn, cout=136)) == E_LAUNCH


@pytest.mark.parametrize("name,dt,tn,es,piece,out32", [l for l in LAUNCHERS if l[4] == 8], ids=[l[0] for l in LAUNCHERS if l[4] == 8])
def test_bf16_output_and_residual_views_must_be_16_byte_aligned(name, dt, tn, es, piece, out32):
    op = conv_op(dt, tn)
    op.y.base += 8
    assert run(op) == E_ARG
    op = conv_op(dt, tn)
    op.y.sx = 132                          # 264 bytes per pixel
    assert run(op) == E_ARG
    op = conv_op(dt, tn, res=True)
    op.res.base += 8
    assert run(op) == E_ARG
    op = conv_op(dt, tn, res=True)
    op.res.sy += 4
    assert run(op) == E_ARG


@pytest.mark.parametrize("name,dt,tn,es,piece,out32", LAUNCHERS, ids=IDS)
def test_views_beyond_the_32_bit_reach_are_refused(name, dt, tn, es, piece, out32):
    far = (1 << 31) // es                  # elements: the sample stride alone reaches 2^31 bytes
    op = conv_op(dt, tn)
    op.x.sn = far
    assert run(op) == E_ARG
    op = conv_op(dt, tn)
    op.x.sn = far // 2                     # half of it is fine
    assert run(op) == E_LAUNCH
    op = conv_op(dt, tn, res=True)
    op.y.sn = far
    assert run(op) == (E_ARG if out32 else E_LAUNCH)     # the fp32-pipe kernel addresses y / res with 64 bits
    op = conv_op(dt, tn, res=True)
    op.res.sn = far
    assert run(op) == (E_ARG if out32 else E_LAUNCH)
    assert run(conv_op(dt, tn), batch=(1 << 31) // (32 * 32)) == E_ARG          # 2^31 pixels


@pytest.mark.parametrize("name,dt,tn,es,piece,out32", [l for l in LAUNCHERS if "g" in l[0]], ids=[l[0] for l in LAUNCHERS if "g" in l[0]])
def test_lds_dma_forms_need_128_output_channels(name, dt, tn, es, piece, out32):
    assert run(conv_op(dt, tn, cout=64)) == E_ARG
    assert run(conv_op(dt, tn, cout=256)) == E_LAUNCH


@pytest.mark.parametrize("name,dt,tn,es,piece,out32", [l for l in LAUNCHERS if "bf16g" in l[0]], ids=[l[0] for l in LAUNCHERS if "bf16g" in l[0]])
def test_bf16_lds_dma_form_has_no_prologue(name, dt, tn, es, piece, out32):
    op = conv_op(dt, tn)
    op.pre_scale, op.pre_shift = BASE + (4 << 26), BASE + (5 << 26)
    assert run(op) == E_ARG
    op.tile_n = 128                        # the staged bf16 kernel takes it
    assert run(op) == E_LAUNCH


@pytest.mark.parametrize("name,dt,tn,es,piece,out32", [l for l in LAUNCHERS if "g" not in l[0]], ids=[l[0] for l in LAUNCHERS if "g" not in l[0]])
def test_unknown_column_tile_and_padding_with_prologue_are_refused(name, dt, tn, es, piece, out32):
    assert run(conv_op(dt, 48)) == E_ARG
    op = conv_op(dt, tn)
    op.kh = op.kw = 3
    op.pad_t = op.pad_l = 1
    assert run(op) == E_LAUNCH
    op.pre_scale, op.pre_shift = BASE + (4 << 26), BASE + (5 << 26)
    assert run(op) == E_ARG

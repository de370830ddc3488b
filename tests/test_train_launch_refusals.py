"""CPU: the extent rules of the training ops (include/hvn.h, "Extent rules"), through the public hvn_run_train_plan.

The kernels of BN, UPADD_BWD and HEAD_BWD take N, H, W, C from one view and walk the other views with them, so a descriptor whose views
disagree would read and write outside a buffer.  Every such descriptor is refused on the host (HVN_E_ARG, -1, with its own text) before
anything touches the device; one that passes goes on to launch, which without a device fails as HVN_E_LAUNCH (-2).  As in
tests/test_conv_launch_refusals.py the two codes tell "refused" from "would have launched" with pointers that are never dereferenced,
and the module skips where a GPU is present.  tests/test_gpu_train_ops.py repeats the refusals on the GPU over real buffers, which
must come back unchanged."""
import ctypes

import pytest
import torch

from hover_net_amd import lib as L

E_ARG, E_LAUNCH = -1, -2
BASE = 0x10000000          # 16-byte aligned, never dereferenced


def view(i, h, w, c):
    return L.hvn_view(base=BASE + (i << 24), sn=h * w * c, sy=w * c, sx=c, h=h, w=w, c=c, sc=1)


def ptrs(t, n):
    for i in range(n):
        t.p[i] = BASE + ((8 + i) << 24)
    return t


def bn_fwd(h=6, w=5, c=8):
    t = L.hvn_top()
    t.kind, t.x, t.y, t.eps, t.momentum = 3, view(0, h, w, c), view(1, h, w, c), 1e-5, 0.1
    return ptrs(t, 6)


def bn_bwd(h=6, w=5, c=8, dz=True):
    t = L.hvn_top()
    t.kind, t.x, t.y, t.dy = 4, view(0, h, w, c), view(1, h, w, c), view(2, h, w, c)
    if dz:
        t.dx = view(3, h, w, c)
    return ptrs(t, 6)


def upadd_bwd(h=6, w=4, c=8, dlo=True, dskip=True):
    t = L.hvn_top()
    t.kind, t.dy = 7, view(0, h, w, c)
    if dlo:
        t.dx = view(1, h // 2, w // 2, c)
    if dskip:
        t.y = view(2, h, w, c)
    return t


def head_bwd(h=6, w=5, cout=5):
    t = L.hvn_top()
    t.kind, t.cout, t.x, t.dx = 8, cout, view(0, h, w, 64), view(1, h, w, 64)
    return ptrs(t, 4)


def run(t, batch=2):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: a descriptor with made-up pointers must not be launched")
    l = L.lib()
    rc = l.hvn_run_train_plan(ctypes.byref(t), 1, batch, None)
    return rc, l.hvn_last_error()


def refused(t, *words, batch=2):
    rc, err = run(t, batch)
    assert rc == E_ARG, (rc, err)
    for w in words:
        assert w.encode() in err, (w, err)
    return err


@pytest.mark.parametrize("make", [bn_fwd, bn_bwd, lambda: bn_bwd(dz=False), upadd_bwd, lambda: upadd_bwd(dlo=False), lambda: upadd_bwd(dskip=False),
                                  head_bwd, lambda: bn_fwd(1, 1, 4)],
                         ids=["bn_fwd", "bn_bwd", "bn_bwd_frozen", "upadd_both", "upadd_dskip_only", "upadd_dlo_only", "head_bwd", "bn_fwd_two_values"])
def test_a_well_formed_descriptor_passes_every_host_check(make):
    rc, err = run(make())
    assert rc == E_LAUNCH, (rc, err)


@pytest.mark.parametrize("field", ["h", "w", "c"])
@pytest.mark.parametrize("delta", [-4, 4])
def test_bn_views_must_have_the_extent_of_z(field, delta):
    seen = set()
    for make, name, word in ((bn_fwd, "y", "the a view"), (bn_bwd, "y", "the a view"), (bn_bwd, "dy", "the da view"), (bn_bwd, "dx", "the dz view")):
        t = make(8, 8, 8)
        v = getattr(t, name)
        setattr(v, field, getattr(v, field) + delta)
        seen.add(refused(t, "bn", word, "differs from z's (8, 8, 8)"))
    assert len(seen) == 3          # the a view's text is shared by forward and backward; da and dz have their own


def test_bn_forward_over_one_value_per_channel_is_refused():
    err = refused(bn_fwd(1, 1, 4), "bn forward", "batch * h * w = 1 < 2", batch=1)
    assert b"unbiased variance" in err
    assert run(bn_fwd(1, 1, 4), batch=2)[0] == E_LAUNCH
    assert run(bn_fwd(1, 2, 4), batch=1)[0] == E_LAUNCH
    assert run(bn_bwd(1, 1, 4), batch=1)[0] == E_LAUNCH            # the backward pass divides by n only


def test_upadd_backward_extents():
    for field in ("h", "w", "c"):
        for delta in (-4, 4) if field == "c" else (-1, 1, 2):
            t = upadd_bwd(8, 8, 8)
            setattr(t.dx, field, getattr(t.dx, field) + delta)
            refused(t, "upadd backward: dlo must be (h / 2, w / 2, c) of dy")
            t = upadd_bwd(8, 8, 8)
            setattr(t.y, field, getattr(t.y, field) + delta)
            refused(t, "upadd backward: dskip must be (h, w, c) of dy")
    t = upadd_bwd(8, 8, 8)
    t.dx = t.y                                                      # a full-size dlo: the commonest mix-up
    refused(t, "dlo must be")
    refused(upadd_bwd(dlo=False, dskip=False), "upadd backward: both dlo and dskip are NULL")
    refused(upadd_bwd(7, 8, 8, dlo=False), "upadd backward: extent must be even")
    refused(upadd_bwd(8, 5, 8, dlo=False), "upadd backward: extent must be even")


def test_head_backward_dx_must_match_x():
    for field, delta in (("h", 1), ("h", -1), ("w", 1), ("w", -1)):
        t = head_bwd()
        setattr(t.dx, field, getattr(t.dx, field) + delta)
        refused(t, "head backward: the dx view's extent", "differs from x's (6, 5, 64)")
    t = head_bwd()
    t.dx.c = 32
    refused(t, "head backward")
    for field in ("h", "w"):                                       # an empty x has its own text
        t = head_bwd()
        setattr(t.x, field, 0)
        setattr(t.dx, field, 0)
        assert b"differs" not in refused(t, "head backward: x has an empty extent")


@pytest.mark.parametrize("bad_at", [0, 1, 2])
def test_a_bad_descriptor_anywhere_in_a_list_is_refused_before_the_first_launch(bad_at):
    """The extent rules run over the whole list first: with well-formed ops in front of the bad one the answer is still HVN_E_ARG, where
    launching op 0 would have answered HVN_E_LAUNCH on a machine without a device."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: a descriptor with made-up pointers must not be launched")
    ops = [bn_fwd(), upadd_bwd(), head_bwd()]
    ops[bad_at] = upadd_bwd(dlo=False, dskip=False)
    tops = (L.hvn_top * 3)()
    for i, t in enumerate(ops):
        ctypes.memmove(ctypes.addressof(tops[i]), ctypes.addressof(t), ctypes.sizeof(L.hvn_top))
    l = L.lib()
    assert l.hvn_run_train_plan(tops, 3, 2, None) == E_ARG
    err = l.hvn_last_error()
    assert b"both dlo and dskip are NULL" in err and b"op %d" % bad_at in err and l.hvn_train_last_error() == err, err
    assert l.hvn_run_train_plan_ws(tops, 3, 2, None, None, 0) == E_ARG


@pytest.mark.parametrize("mode,nt,freeze", [("original", 5, False), ("original", 5, True), ("original", None, True), ("fast", None, False)])
def test_the_ops_the_training_plan_lowers_obey_the_extent_rules(mode, nt, freeze):
    """What TrainEngine hands to the library: the views of every BN, upadd-backward and head-backward op of every plan it builds."""
    from hover_net_amd.train_plan import TrainPlan
    P = TrainPlan(mode, nt, freeze)
    ext = lambda v: (v.h, v.w, v.c)
    seen = set()
    for op in list(P.fwd) + list(P.bwd):
        if op.kind == "bnrelu":
            assert ext(op.a) == ext(op.z), op.name
        elif op.kind == "bnrelu_bwd":
            assert ext(op.a) == ext(op.z) == ext(op.da), op.name
            assert op.dz is None or ext(op.dz) == ext(op.z), op.name
        elif op.kind == "upadd_bwd":
            h, w, c = ext(op.dy)
            assert h % 2 == 0 and w % 2 == 0 and (op.dlo is not None or op.dskip is not None), op.name
            assert op.dlo is None or ext(op.dlo) == (h // 2, w // 2, c), op.name
            assert op.dskip is None or ext(op.dskip) == (h, w, c), op.name
        elif op.kind == "head_bwd":
            assert ext(op.dx) == ext(op.x) and op.x.c == 64, op.name
        else:
            continue
        seen.add(op.kind)
    assert seen == {"bnrelu", "bnrelu_bwd", "upadd_bwd", "head_bwd"}

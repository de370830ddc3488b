"""-m gpu: nuclei by distance to an annotation's boundary on the device (csrc/hvn_margins.hip: HVN_OP_NBR_GRID + HVN_OP_NBR_MARGINS)
against the all-segments oracle tests/margins_ref.py and the host path with ==, on all of near, near_d2, near_inside, count (and widths,
names), then `regions.of_info` with a "margin" on the device against the host.  No tolerance anywhere: near_d2 is compared as float64
values."""
import numpy as np
import pytest

import margins_ref as M

pytestmark = pytest.mark.gpu


def _mg():
    from hover_net_amd import margins as MG

    return MG


def _assert_all(got, want, args, name):
    M.assert_same(got, want, name)
    assert got.widths == tuple(float(w) for w in args[3]) and got.names == args[2].names


# -- 1: device == host == oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_device_equals_host_and_oracle(name):
    """Every case of tests/margins_ref.py.  `single_point` and `n257` are the workgroup's edges; `many_rows` has the points of one
    workgroup in more than 256 grid rows; `long_ring` walks one list of three staging tiles with a region's run across a tile's end;
    `overlap` has a point near three regions; `sixteen_by_sixteen` and `one_band_untyped` are the caps and the floor of B and T;
    `coincident` has 3000 lanes adding into one word; `far` has empty lists; `outside` has segments in the clamped end rows and a far
    edge that decides a parity; the `random_*` cases take the division branch; `strip` has five workgroups in one row, each leaving
    the segments to its left out of the tiles it stages."""
    args, want = M.case(name)
    MG = _mg()
    got = MG.margins_device(*args[:4], nr_types=args[4], cell=args[5])
    _assert_all(got, want, args, name)
    M.assert_case_facts(name, got)
    _assert_all(MG.margins_host(*args[:4], nr_types=args[4], cell=args[5]), want, args, name)
    _assert_all(MG.margins(*args[:4], nr_types=args[4], device="cuda", cell=args[5]), want, args, name)


@pytest.mark.parametrize("name,cell", [("long_ring", 2.0), ("hole", 1.0e5), ("sixteen_by_sixteen", 1.5), ("random_1", 0.5), ("overlap", 1.0e5)])
def test_the_cell_side_changes_nothing(name, cell):
    """Many rows per workgroup, and one row for all (the brute-force form): the same numbers."""
    (xy, types, rs, widths, t, _), want = M.case(name)
    M.assert_same(_mg().margins_device(xy, types, rs, widths, t, cell=cell), want, name)


@pytest.mark.parametrize("name", ["n257", "outside", "long_ring", "many_rows", "random_3", "coincident", "far", "strip"])
def test_the_form_without_the_x_cull_gives_the_same_numbers(name):
    """The default form leaves out of a staged tile the segments left of all the lanes it serves; `cull=False` stages them all.
    `strip` is the case in which the default form's tiles lose most of their entries, whole region runs among them."""
    args, want = M.case(name)
    q = _mg().DeviceMargins(*args[:4], nr_types=args[4], cell=args[5], cull=False)
    _assert_all(q.run().result(), want, args, name)


@pytest.mark.parametrize("name", ["single_point", "n257", "hole", "far", "outside", "sixteen_by_sixteen", "coincident"])
def test_the_op_writes_every_element_and_runs_twice_on_one_workspace(name):
    """The output holds a poison pattern before the op (as doubles a NaN, as integers -7-ish garbage): the result is still the
    oracle's -- points near nothing and words that no point reaches included -- and so is that of the op run again on the same workspace
    and its own output."""
    args, want = M.case(name)
    q = _mg().DeviceMargins(*args[:4], nr_types=args[4], cell=args[5])
    q.run_grid()
    q.out.fill_(-7)
    q.run_op()
    first = q.result()
    _assert_all(first, want, args, name)
    q.run_op()
    _assert_all(q.result(), first[:4], args, name)


@pytest.mark.parametrize("name", ["n257", "overlap", "long_ring", "coincident", "random_2", "strip"])
def test_same_bits_twice_and_in_reversed_order(name):
    """The order of the points inside a cell depends on atomic arrival, and so does the order of the adds; the results may not, and
    with the points reversed the per-point fields are the reversed arrays."""
    (xy, types, rs, widths, t, cell), want = M.case(name)
    MG = _mg()
    M.assert_same(MG.margins_device(xy, types, rs, widths, t, cell=cell), want, name)
    rxy = np.ascontiguousarray(xy[::-1])
    rtypes = None if types is None else np.ascontiguousarray(types[::-1])
    M.assert_same(MG.margins_device(rxy, rtypes, rs, widths, t, cell=cell), (want[0][::-1], want[1][::-1], want[2][::-1], want[3]), name)


def test_a_device_that_is_no_gpu_is_refused():
    args, _ = M.case("n257")
    with pytest.raises(ValueError, match="GPU"):
        _mg().margins_device(*args[:4], nr_types=args[4], device="cpu")


# -- 2: the pipeline ----------------------------------------------------------------------------------------------
def _info40():
    rng = np.random.default_rng(40)
    return {int(lab): {"centroid": rng.random(2) * np.array([40.0, 30.0]), "type": int(rng.integers(0, 3)), "bbox": None, "contour": None, "type_prob": 0.5}
            for lab in rng.permutation(np.arange(1, 400))[:40]}


def test_of_info_on_the_device_equals_the_host():
    import torch

    from hover_net_amd import regions as RG

    rs = RG.RegionSet.from_polygons([[[M.R._square(5.0, 5.0, 25.0, 20.0), M.R._square(10.0, 9.0, 16.0, 14.0)]], [[M.R._circle(28.0, 15.0, 9.0, 30)]]], names=["tumour", "node"])
    spec = RG.resolve({"regions": rs, "margin": [1.0, 2.5, 6.0]})
    for nr_types in (3, None):
        host, dev = RG.of_info(_info40(), spec, nr_types), RG.of_info(_info40(), spec, nr_types, device=torch.device("cuda"))
        M.assert_same(dev.margins, host.margins[:4], "of_info")
        M.R.assert_same(dev.counts, host.counts[:3], "of_info")
        assert dev.margins.widths == host.margins.widths == (1.0, 2.5, 6.0) and dev.margins.names == ["tumour", "node"]
        assert 10 < int((host.margins.near >= 0).sum()) < 40 and set(host.margins.near_inside.tolist()) == {-1, 0, 1}
        a, b = RG.annotate(_info40(), host), RG.annotate(_info40(), dev)
        assert [e["margin"] for e in a.values()] == [e["margin"] for e in b.values()] and [e["region"] for e in a.values()] == [e["region"] for e in b.values()]

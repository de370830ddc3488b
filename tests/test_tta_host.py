"""Test-time augmentation, host side: the rule for the HV field against the reference's own target definition, hover_net_amd.tta's
tables against the independent oracle (tests/tta_ref.py) and against numpy, and the validation of the `tta` argument."""
import numpy as np
import pytest

import tta_ref as R


def _ellipse_map():
    """96 x 96 label map of nine ellipses: centres on a 3 x 3 grid at 20 / 48 / 76, radii 8..12."""
    rng = np.random.default_rng(3)
    ann = np.zeros((96, 96), np.int32)
    yy, xx = np.mgrid[:96, :96]
    lab = 0
    for cy in (20, 48, 76):
        for cx in (20, 48, 76):
            ry, rx = rng.integers(8, 13, size=2)
            lab += 1
            ann[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = lab
    return ann


def test_hv_rule_matches_the_reference_target_definition():
    """hv(view_k(ann)) against m . view_k(hv(ann)) for the eight signed permutations m: the oracle's M_k must beat each of the
    seven others by a factor of three (it is not exactly zero: the reference rounds the centre of mass, one pixel of asymmetry)."""
    from oracle.targets_np import gen_instance_hv_map

    ann = _ellipse_map()
    hv = gen_instance_hv_map(ann, (96, 96))
    for k in range(8):
        want = gen_instance_hv_map(np.ascontiguousarray(R.view(ann, k)), (96, 96))
        right = np.abs(R.field_view(hv, k) - want).mean()
        wrong = [np.abs(R.field_view(hv, k, m) - want).mean() for m in R.SIGNED_PERMUTATIONS if not np.array_equal(m, R.M(k))]
        assert len(wrong) == 7
        print("view %d: right rule %.4f, best wrong rule %.4f" % (k, right, min(wrong)))
        assert right < min(wrong) / 3.0, (k, right, min(wrong))


def test_oracle_view_is_numpy_rot90_of_the_flip():
    a = np.random.default_rng(0).integers(0, 1000, (5, 7, 2))
    for k in range(8):
        want = np.rot90(a[:, ::-1] if k >= 4 else a, k % 4, axes=(0, 1))
        np.testing.assert_array_equal(R.view(a, k), want)


def test_package_tables_match_oracle_and_numpy():
    from hover_net_amd import tta

    assert tta.SETS == {"flips": (0, 4, 6, 2), "rot": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
    a = np.random.default_rng(1).integers(0, 1000, (6, 6, 3))      # random, hence without any symmetry
    u = np.random.default_rng(2).standard_normal((6, 6, 2)).astype(np.float32)
    for k in range(8):
        np.testing.assert_array_equal(tta.matrix(k), R.M(k))
        np.testing.assert_array_equal(tta.view(a, k), R.view(a, k))
        np.testing.assert_array_equal(tta.view_field(u, k), R.field_view(u, k))
        np.testing.assert_array_equal(tta.view(tta.view(a, k), tta.inverse(k)), a)
        np.testing.assert_array_equal(tta.matrix(tta.inverse(k)) @ tta.matrix(k), np.eye(2, dtype=np.int64))
        for g in range(8):
            m = tta.COMPOSE[k][g]
            assert m == tta.compose(k, g)
            np.testing.assert_array_equal(tta.view(tta.view(a, g), k), tta.view(a, m))
            np.testing.assert_array_equal(tta.matrix(k) @ tta.matrix(g), tta.matrix(m))
    # a non-square array: the views that do not transpose keep its shape
    b = np.random.default_rng(3).integers(0, 1000, (4, 9))
    for k in range(8):
        np.testing.assert_array_equal(tta.view(b, k), R.view(b, k))


def test_views_argument_validation():
    from hover_net_amd import tta

    assert tta.views(None) is None
    assert tta.views("flips") == (0, 4, 6, 2) and tta.views("rot") == (0, 1, 2, 3) and tta.views("d4") == tuple(range(8))
    assert tta.views((3, 6, 1)) == (3, 6, 1) and tta.views([5]) == (5,)
    for bad in ("d8", "", (), [], (0, 0), (1, 2, 1), (8,), (-1,), (0, 1.5), 3):
        with pytest.raises(ValueError):
            tta.views(bad)


def test_entry_points_refuse_a_bad_view_set_before_touching_the_model():
    """`infer_step_device`, `TilePipeline`, `process_images` and `WsiInference` check `tta` first: no model is needed to be refused."""
    from hover_net_amd import infer_tile, run_desc

    with pytest.raises(ValueError):
        run_desc.infer_step_device(None, None, tta="d8")
    with pytest.raises(ValueError):
        run_desc.infer_step(None, None, tta=(0, 0))
    with pytest.raises(ValueError):
        infer_tile.process_images([], None, tta=())


def test_run_args_tta_is_checked_before_any_file_is_touched(tmp_path):
    from hover_net_amd import infer_manager as im

    method = {"model_args": {"nr_types": None, "mode": "original"}, "model_path": None}
    out = tmp_path / "out"
    args = {"input_dir": str(tmp_path), "output_dir": str(out), "tta": "d8"}
    with pytest.raises(ValueError):
        im.InferManager(method, process_fn=lambda images: []).process_file_list(dict(args))
    with pytest.raises(ValueError):
        im.WsiManager(method, wsi_fn=lambda slide, mask: (None, {})).process_wsi_list(dict(args, tta=(1, 1)))
    assert not out.exists()

"""Two corners of the BA handle that the other suites leave open (csrc/ba_build.hip, the host routes of csrc/ba.hip).

1. The host routes stage their results in buffers of the handle.  pcd_ba_observation_errors stages in the filter's
   f_sq / f_depth, pcd_ba_evaluate's jac_q / jac_t in o_jq / o_jt: the routes called one after the other, with
   pcd_ba_filter_tracks (which rewrites f_sq / f_depth) in between, must each give the same bits again.
2. A handle without observations (O = 0, LiDAR terms only) through the routes test_ba_load_order_gpu.py does not take:
   the compact Ceres route, the observation errors and the track filter.

Scenes: tests/test_ba_load_order_gpu.track_scene, P = 65 (two 64-track slices).  Bounds: those of
tests/test_ba_edge_gpu.py::test_filters and tests/ba_edge_ref.check_raw (the project's 1e-9 relative per column)."""
import numpy as np
import pytest

from tests import ba_edge_ref as er
from tests.test_ba_load_order_gpu import track_scene

pytestmark = pytest.mark.gpu
DBL_MAX = np.finfo(np.float64).max
FILTER_ARRAYS = ("obs_erase", "obs_negative_depth", "point_delete")
FILTER_COUNTS = ("num_filtered", "num_points_with_error", "num_negative_depth")


def _check_filter(got, exp):
    for k in FILTER_ARRAYS:
        assert got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), k
    for k in FILTER_COUNTS:
        assert got[k] == exp[k], (k, got[k], exp[k])
    np.testing.assert_allclose(got["point_error"], exp["point_error"], rtol=1e-12, atol=1e-12)
    assert abs(got["mean_reproj_error"] - exp["mean_reproj_error"]) <= 1e-12 * max(1.0, exp["mean_reproj_error"])


def test_host_route_staging_does_not_alias(gpu, oracle):
    kw = track_scene(oracle, 65, "shared")
    P, O = 65, len(kw["obs_image"])
    assert O > 64 and len(kw["lidar_point"]) > 0 and len(kw["cam_model"]) == 1
    ob = oracle.BA(**kw)
    esq, edepth = ob.observation_errors()
    _, Jq, Jt, _, _, _ = ob.evaluate_raw()
    ba = gpu.BA(**kw)
    sq1, depth1 = ba.observation_errors()
    jac1 = ba.evaluate(("jac_q", "jac_t"))
    filt = ba.filter_tracks(4.0)
    sq2, depth2 = ba.observation_errors()
    jac2 = ba.evaluate(("jac_q", "jac_t"))
    ba.close()
    assert np.array_equal(sq2, sq1) and np.array_equal(depth2, depth1)
    assert np.array_equal(jac2["jac_q"], jac1["jac_q"]) and np.array_equal(jac2["jac_t"], jac1["jac_t"])
    behind = edepth < np.finfo(np.float64).eps
    assert np.array_equal(sq1 == DBL_MAX, behind)
    np.testing.assert_allclose(depth1, edepth, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sq1[~behind], esq[~behind], rtol=1e-9, atol=1e-9)
    er.col_close(jac1["jac_q"], Jq, "jac_q")
    er.col_close(jac1["jac_t"], Jt, "jac_t")
    assert np.abs(Jq).max() > 0 and np.abs(Jt).max() > 0
    _check_filter(filt, oracle.filter_tracks(esq, edepth, kw["obs_point"], P, 4.0))


@pytest.mark.parametrize("cams", ["shared", "two_cameras"])
def test_no_observations_through_the_remaining_routes(gpu, oracle, cams):
    kw = track_scene(oracle, 65, "shared", lidar=True, obs=False)
    if cams == "two_cameras":
        kw["cam_model"] = np.array([4, 4], np.int32)
        kw["cam_params_list"] = [kw["cam_params_list"][0], kw["cam_params_list"][0] * 1.002]
        kw["image_camera"] = (np.arange(10) % 2).astype(np.int32)
    P, L = 65, len(kw["lidar_point"])
    assert len(kw["obs_image"]) == 0 and L > P
    res, _, _, _, _, JL = oracle.BA(**kw).evaluate_raw()
    ba = gpu.BA(**kw)
    c = ba.evaluate_blocks_compact(True, True)
    assert c["residuals"] is None and c["records"].shape == (0, 8) and c["cam_stride"] == 8
    assert c["jac_cam"].shape == (0, 2, 8) and c["jac_lidar"].shape == (L, 3) and c["lidar_residuals"].shape == (L,)
    er.col_close(c["lidar_residuals"], res, "lidar residuals")
    er.col_close(c["jac_lidar"], JL, "jac_lidar")
    assert np.abs(res).max() > 0 and np.abs(JL).max() > 0 and c["bytes_d2h"] == 8 * 4 * L
    r = ba.evaluate_blocks_compact(False, True)
    assert r["records"] is None and r["jac_lidar"] is None and r["jac_cam"] is None
    assert r["residuals"].shape == (0,) and r["bytes_d2h"] == 8 * L
    assert np.array_equal(r["lidar_residuals"], c["lidar_residuals"])
    sq, depth = ba.observation_errors()
    assert sq.shape == (0,) and depth.shape == (0,)
    got = ba.filter_tracks(4.0)
    ba.close()
    exp = oracle.filter_tracks(np.zeros(0), np.zeros(0), kw["obs_point"], P, 4.0)
    _check_filter(got, exp)
    # every track is shorter than two observations: all points deleted, nothing filtered, no point has an error
    assert got["point_delete"].all() and (got["point_error"] == -1.0).all()
    assert got["num_filtered"] == 0 and got["num_points_with_error"] == 0 and got["mean_reproj_error"] == 0.0

"""tests/ba_filter_ref.py pinned on cases computed by hand (no GPU): the reference the device tests of
pcd_ba_filter_points and pcd_ba_remove_observations_device compare against."""
import math

import numpy as np

from tests import ba_filter_ref as fr

IDENT = [1.0, 0.0, 0.0, 0.0]


def pose_at(center):
    """identity rotation: the projection centre is -tvec"""
    return IDENT + [-float(c) for c in center]


def run(poses, points, obs_image, obs_point, sq_err, max_err=8.0, min_angle=1.5, **kw):
    return fr.filter_points(np.asarray(sq_err, np.float64), np.ones(len(obs_image)), np.asarray(obs_image),
                            np.asarray(obs_point), np.asarray(poses, np.float64), np.asarray(points, np.float64), max_err,
                            min_angle, **kw)


def test_projection_centre():
    assert np.array_equal(fr.proj_center(pose_at([1.0, -2.0, 3.0])), [1.0, -2.0, 3.0])
    # 90 degrees about z (x -> y): R^T applied to -t; the quaternion is given at twice its unit length
    h = math.sqrt(0.5)
    c = fr.proj_center([2 * h, 0.0, 0.0, 2 * h, -1.0, 0.0, 0.0])
    np.testing.assert_allclose(c, [0.0, -1.0, 0.0], atol=1e-15)
    assert np.array_equal(fr.proj_center([0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0]), [-1.0, -2.0, -3.0])   # zero norm: identity


def test_a_known_angle_on_both_sides_of_the_threshold():
    hgt = 10.0
    for deg, kept in ((1.5 + 1e-6, True), (1.5 - 1e-6, False)):
        b = hgt * math.tan(math.radians(deg) / 2)       # centres at (+-b, 0, 0), the point at (0, 0, h): 2 atan(b / h)
        poses = [pose_at([b, 0, 0]), pose_at([-b, 0, 0])]
        assert abs(fr.tri_angle(fr.proj_center(poses[0]), fr.proj_center(poses[1]), np.array([0, 0, hgt])) -
                   math.radians(deg)) < 1e-12
        r = run(poses, [[0, 0, hgt]], [0, 1], [0, 0], [1.0, 1.0])
        assert r["point_delete"][0] == (0 if kept else 1)
        assert list(r["obs_erase"]) == ([0, 0] if kept else [1, 1])
        assert r["point_error"][0] == (1.0 if kept else -1.0)
        assert r["num_filtered"] == (0 if kept else 1) and r["num_points_with_error"] == (1 if kept else 0)
    # the obtuse side: min(angle, pi - angle)
    poses = [pose_at([1000.0, 0, 0]), pose_at([-1000.0, 0, 0])]
    a = fr.tri_angle(fr.proj_center(poses[0]), fr.proj_center(poses[1]), np.array([0, 0, 1.0]))
    assert abs(a - 2 * math.atan(1 / 1000.0)) < 1e-12


def test_a_point_on_a_centre_is_deleted():
    poses = [pose_at([0, 0, 5.0]), pose_at([3.0, 0, 0])]
    assert fr.tri_angle(fr.proj_center(poses[0]), fr.proj_center(poses[1]), np.array([0, 0, 5.0])) == 0.0
    r = run(poses, [[0, 0, 5.0]], [0, 1], [0, 0], [0.0, 0.0])
    assert r["point_delete"][0] == 1 and r["num_filtered"] == 1


def test_the_same_image_twice_is_deleted_also_when_acos_gives_nan():
    poses = [pose_at([0.3, 0.1, 0.0])]
    r = run(poses, [[0.7, 0.2, 9.0]], [0, 0], [0, 0], [1.0, 4.0])
    assert r["point_delete"][0] == 1 and list(r["obs_erase"]) == [1, 1] and r["num_filtered"] == 1
    # the argument 1 + eps: NaN through abs and min, and NaN >= threshold is false -- also for a threshold of 0+
    c = np.array([0.0, 0.0, 0.0])
    nan = fr.tri_angle(c, c, np.array([1.0, 1.0, 1.0]), acos=lambda x: math.nan)
    assert nan != nan
    r = run(poses, [[0.7, 0.2, 9.0]], [0, 0], [0, 0], [1.0, 4.0], min_angle=1e-300, acos=lambda x: math.nan)
    assert r["point_delete"][0] == 1
    # a wide pair next to a NaN pair keeps the point
    poses2 = [pose_at([5.0, 0, 0]), pose_at([-5.0, 0, 0])]
    assert run(poses2, [[0, 0, 9.0]], [0, 1], [0, 0], [1.0, 1.0])["point_delete"][0] == 0


def test_stage_two_sees_only_the_survivors():
    # images 0 and 1 are close together, image 2 is far away: (2, .) gives the angle, and stage 1 erases element 2
    poses = [pose_at([0.0, 0, 0]), pose_at([0.01, 0, 0]), pose_at([5.0, 0, 0])]
    kept = run(poses, [[0, 0, 10.0]], [0, 1, 2], [0, 0, 0], [1.0, 1.0, 1.0])
    assert kept["point_delete"][0] == 0 and kept["num_filtered"] == 0
    r = run(poses, [[0, 0, 10.0]], [0, 1, 2], [0, 0, 0], [1.0, 1.0, 100.0])      # 100 > 8^2
    assert r["point_delete"][0] == 1 and list(r["obs_erase"]) == [1, 1, 1] and r["point_error"][0] == -1.0
    assert r["num_filtered"] == 2                       # one element in stage 1, one POINT in stage 2
    # without stage 2 the point lives on with two elements
    r = run(poses, [[0, 0, 10.0]], [0, 1, 2], [0, 0, 0], [1.0, 1.0, 100.0], min_angle=0.0)
    assert r["point_delete"][0] == 0 and list(r["obs_erase"]) == [0, 0, 1] and r["num_filtered"] == 1
    assert r["point_error"][0] == 1.0


def test_summary_counts_elements_in_stage_one_and_points_in_stage_two():
    poses = [pose_at([0.0, 0, 0]), pose_at([0.01, 0, 0]), pose_at([5.0, 0, 0]), pose_at([-5.0, 0, 0])]
    points = [[0, 0, 10.0]] * 4
    # point 0: wide pair, one bad element -> 1; point 1: all three bad -> 3 (stage 1 deletes it); point 2: narrow pair
    # -> 1 point; point 3: wide pair, clean -> 0
    obs_point = [0, 0, 0, 1, 1, 1, 2, 2, 3, 3]
    obs_image = [2, 3, 0, 0, 1, 2, 0, 1, 2, 3]
    sq = [4.0, 16.0, 100.0, 100.0, 100.0, 100.0, 1.0, 1.0, 9.0, 9.0]
    r = run(poses, points, obs_image, obs_point, sq)
    assert list(r["point_delete"]) == [0, 1, 1, 0]
    assert list(r["obs_erase"]) == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0]
    assert r["num_filtered"] == 1 + 3 + 1
    assert list(r["point_error"]) == [3.0, -1.0, -1.0, 3.0]
    assert r["num_points_with_error"] == 2 and r["mean_reproj_error"] == 3.0
    assert r["max_angle"][1] == -1.0 and 0 < r["max_angle"][2] < math.radians(1.5) < r["max_angle"][0]


def test_fixed_order_sum_is_a_sum():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 257, 70000):
        v = rng.integers(0, 5, n).astype(np.float64)
        assert fr._reduce(v) == v.sum()


def test_the_gpu_scenes_keep_every_angle_away_from_the_threshold(oracle):
    """The seeds of tests/test_ba_filter_gpu.py, checked without a GPU: with the ORACLE's reprojection errors every
    point's largest pair angle lies at least 1e-9 rad from both thresholds the device test uses, no point left out, and
    both stages fire.  No error lies within 1e-6 (relative) of the 8 px bound, so the device's stage 1 -- whose errors
    agree with the oracle's to 1e-9 -- erases the same elements and stage 2 sees the same survivors."""
    from tests import test_ba_filter_gpu as fg
    for cams in ("shared", "two"):
        s = fg.filter_scene(oracle, cams)
        O = len(s["obs_point"])
        res = oracle.BA(**s).evaluate_raw()[0][:2 * O].reshape(O, 2)
        sq = (res * res).sum(axis=1)
        assert np.isfinite(sq).all() and (np.abs(sq - 64.0) > 64e-6).all()
        for min_angle in (1.5, 2.5):
            ref = fr.filter_points(sq, np.ones(O), s["obs_image"], s["obs_point"], s["poses"], s["points"], 8.0, min_angle)
            one = fr.filter_points(sq, np.ones(O), s["obs_image"], s["obs_point"], s["poses"], s["points"], 8.0, 0.0)
            ran = ref["max_angle"] >= 0
            assert ran.sum() > 20 and np.array_equal(ran, one["point_delete"] == 0)
            assert (np.abs(ref["max_angle"][ran] - min_angle * fr.DEG) >= fg.MARGIN).all()
            assert ref["point_delete"].sum() > one["point_delete"].sum() >= 1 and one["obs_erase"].sum() > 0


def test_shim_refusals_without_a_gpu():
    """shim/test_ba_filter without --gpu: NULL handles, the option defaults, FilterPoints without a live handle, and the
    point2D index SetUp records per observation"""
    import os
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_filter"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_filter")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


def test_compaction_rule():
    scene = dict(points=np.zeros((4, 3)), obs_image=np.array([0, 1, 0, 1, 2, 2], np.int32),
                 obs_point=np.array([0, 0, 1, 1, 2, 3], np.int32), obs_xy=np.arange(12.0).reshape(6, 2),
                 lidar_point=np.array([3, 1, 1, 0], np.int32), lidar_abcd=np.arange(16.0).reshape(4, 4),
                 lidar_weight=np.arange(4.0))
    kw, obs_map, info, lkeep = fr.fresh_args_after_remove(scene, [0, 1, 0, 0, 1, 0], [0, 1, 0, 0])
    assert list(kw["obs_point"]) == [0, 3] and list(kw["obs_image"]) == [0, 2]
    assert np.array_equal(kw["obs_xy"], [[0.0, 1.0], [10.0, 11.0]])
    assert list(obs_map) == [0, fr.DROPPED, fr.DROPPED, fr.DROPPED, fr.DROPPED, 1]
    assert list(kw["lidar_point"]) == [3, 0] and list(kw["lidar_weight"]) == [0.0, 3.0] and list(lkeep) == [1, 0, 0, 1]
    assert info == dict(num_obs=2, num_obs_removed=4, num_lidar=2, num_lidar_removed=2, num_points_emptied=2)
    same, ident, info0, _ = fr.fresh_args_after_remove(scene)
    assert list(ident) == list(range(6)) and info0["num_obs_removed"] == 0 and np.array_equal(same["obs_xy"], scene["obs_xy"])
    none, _, _, _ = fr.fresh_args_after_remove(scene, None, [1, 1, 1, 1])
    assert len(none["obs_point"]) == 0 and "lidar_point" not in none

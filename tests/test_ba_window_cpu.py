"""The sphere window of a global round (pcd_ba_window_create_device / pcd_ba_window_commit_device) without a
GPU: the exported symbols and their guards, the defaults of the options, tests/ba_window_ref.py on hand cases whose
results are exact (integer inputs), and the refusal leg of the shim's test."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import ba_window_ref as wr


def test_symbols_defaults_and_guards(pcdhip):
    L = pcdhip.lib()
    for name in ("pcd_ba_window_opts_default", "pcd_ba_window_create_device", "pcd_ba_window_commit_device"):
        assert hasattr(L, name) and name in pcdhip.ABI_SYMBOLS
    assert callable(pcdhip.BA.sphere_window) and callable(pcdhip.BA.commit_window) and callable(pcdhip.global_round)
    assert C.sizeof(pcdhip.BAWindowOpts) == 64 and C.sizeof(pcdhip.BAWindowInfo) == 48
    o = pcdhip.BAWindowOpts(7, 1.0, 1, 2)
    o.reserved[3] = 5
    L.pcd_ba_window_opts_default(C.byref(o))
    assert (o.center_image, o.radius, o.d_image_set, o.d_extra_const_pose) == (-1, 40.0, None, None)
    assert list(o.reserved) == [0] * 8
    L.pcd_ba_window_opts_default(None)                  # a null pointer is ignored
    # NULL src, opts or window: INVALID, the info cleared and *window NULL on every return
    h, info = C.c_void_p(123), pcdhip.BAWindowInfo(1, 2, 3, 4, 5, 6.0)
    assert L.pcd_ba_window_create_device(None, C.byref(o), None, None, None, None, C.byref(h),
                                         C.byref(info)) == pcdhip.PCD_ERR_INVALID
    assert h.value is None and (info.num_images_in, info.num_obs, info.build_ms) == (0, 0, 0.0)
    assert L.pcd_ba_window_create_device(None, None, None, None, None, None, C.byref(h), None) == pcdhip.PCD_ERR_INVALID
    assert L.pcd_ba_window_create_device(None, C.byref(o), None, None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
    assert L.pcd_ba_window_commit_device(None, None, None) == pcdhip.PCD_ERR_INVALID
    assert b"null" in L.pcd_last_error()
    # PCD_ERR_NO_DEVICE of the two new entry points cannot be reached without a device: their NULL guard comes first, as
    # the header orders the guards, and the only way to a non-NULL handle is pcd_ba_create, which itself refuses here.
    # So this is NOT that check; it only shows that no handle can exist on this box.
    if pcdhip.device_count() == 0:
        s = dict(cam_model=[0], cam_params_list=[[100.0, 50.0, 50.0]], poses=np.array([[1.0, 0, 0, 0, 0, 0, 0]]),
                 image_camera=[0], points=np.array([[0.0, 0, 5]]), obs_image=[0], obs_point=[0], obs_xy=[[50.0, 50.0]])
        try:
            pcdhip.BA(**s)
            raise AssertionError("pcd_ba_create succeeded without a device")
        except pcdhip.PcdError as e:
            assert e.status == pcdhip.PCD_ERR_NO_DEVICE


def ident(c):
    """identity rotation with projection centre c"""
    return [1.0, 0.0, 0.0, 0.0, -c[0], -c[1], -c[2]]


def test_identity_quaternions_give_minus_t_and_equality_is_in():
    poses = np.array([ident([1, 2, 3]), ident([4, 6, 3]), ident([1, 7, 15]), ident([4, 6, 4]), ident([1, 7, 16])])
    assert np.array_equal(wr.centers(poses), -poses[:, 4:])
    assert list(wr.distances(poses, 0)) == [0.0, 5.0, 13.0, np.sqrt(26.0), np.sqrt(25.0 + 169.0)]
    assert list(wr.image_in(poses, 0, 5.0)) == [1, 1, 0, 0, 0]             # 3-4-5: dist == radius is in
    assert list(wr.image_in(poses, 0, 13.0)) == [1, 1, 1, 1, 0]            # 5-12-13
    assert list(wr.image_in(poses, 0, np.nextafter(5.0, 0))) == [1, 0, 0, 0, 0]
    assert list(wr.image_in(poses, 0, 0.0)) == [1, 0, 0, 0, 0]
    assert list(wr.image_in(poses, 0, np.inf)) == [1] * 5
    assert list(wr.image_in(poses, 2, 1.0)) == [0, 0, 1, 0, 1]             # another centre


def test_the_stored_quaternion_is_not_normalised():
    # q = 2 * (0, 0, 0, 1), a half turn about z scaled by 2: tz = 4, tzz = 8, so R = diag(1 - 8, 1 - 8, 1) where the
    # unit quaternion gives diag(-1, -1, 1).  (Scaling the identity shows nothing: with x = y = z = 0, R = I for any w.)
    poses = np.array([ident([0, 0, 0]), [0.0, 0.0, 0.0, 2.0, 3.0, 4.0, 0.0]])
    assert np.array_equal(wr.centers(poses)[1], [21.0, 28.0, 0.0]) and wr.distances(poses, 0)[1] == 35.0
    assert np.array_equal(wr.centers_normalised(poses)[1], [3.0, 4.0, 0.0])
    assert list(wr.image_in(poses, 0, 5.0)) == [1, 0]                       # the selection: 35 > 5
    assert list(wr.image_in(poses, 0, 35.0)) == [1, 1]
    n = wr.centers_normalised(poses)
    assert np.sqrt(((n[1] - n[0]) ** 2).sum()) == 5.0                       # the normalised centre would be in at 5


def test_fresh_args_on_a_hand_case():
    poses = np.array([ident([0, 0, 0]), ident([3, 4, 0]), ident([30, 0, 0])])
    d = dict(poses=poses, points=np.arange(12.0).reshape(4, 3), image_const_pose=np.array([1, 0, 0], np.uint8),
             obs_image=np.array([0, 2, 1, 2, 2, 1], np.int32), obs_point=np.array([0, 0, 1, 2, 1, 3], np.int32),
             obs_xy=np.arange(12.0).reshape(6, 2), lidar_point=np.array([2, 1, 0], np.int32),
             lidar_abcd=np.arange(12.0).reshape(3, 4), lidar_weight=np.array([1.0, 2.0, 3.0]))
    moved = d["points"] + 100.0
    kw, obs_map, info, lkeep, inn, act = wr.fresh_args_window(d, poses, moved, dict(center_image=0, radius=5.0))
    assert list(inn) == [1, 1, 0] and list(act) == [1, 1, 0, 1]            # point 2 is seen from image 2 alone
    assert list(kw["obs_image"]) == [0, 2, 1, 2, 1] and list(kw["obs_point"]) == [0, 0, 1, 1, 3]   # outside rows stay
    assert list(obs_map) == [0, 1, 2, wr.NOT_IN, 3, 4] and list(lkeep) == [False, True, True]
    assert list(kw["image_const_pose"]) == [1, 0, 1] and list(kw["lidar_point"]) == [1, 0]
    assert np.array_equal(kw["points"], moved)
    assert info == dict(num_images_in=2, num_points_active=3, num_obs=5, num_lidar=2, num_pose_rows=2)
    kw, _, info, _, inn, act = wr.fresh_args_window(d, poses, moved, dict(image_set=[0, 0, 1], extra_const_pose=[0, 0, 1]))
    assert list(act) == [1, 1, 1, 0] and list(kw["image_const_pose"]) == [1, 1, 1] and info["num_pose_rows"] == 0
    kw, obs_map, info, _, _, act = wr.fresh_args_window(d, poses, moved, dict(image_set=[0, 0, 0]))
    assert not act.any() and len(kw["obs_image"]) == 0 and "lidar_point" not in kw and (obs_map == wr.NOT_IN).all()
    assert len(d["obs_image"]) == 6                                         # the input is left alone


def test_shim_refusals_without_a_gpu():
    """shim/test_ba_window without --gpu: GlobalRound without a live handle and the host selection of the mock scene"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_window"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_window")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

"""The local round's start (pcd_ba_local_bundle_device, pcd_ba_local_window_create_device) without a GPU:
the exported symbols, the defaults of the options and the NULL guards, tests/ba_local_ref.py on cases worked out by
hand, and the refusal leg of the shim's test."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from tests import ba_filter_ref as fr
from tests import ba_local_ref as lb

M = 6.0 * fr.DEG                                        # the first pass's angle: 0.10472 rad


def test_symbols_defaults_and_guards(pcdhip):
    L = pcdhip.lib()
    for name in ("pcd_ba_local_bundle_opts_default", "pcd_ba_local_bundle_device", "pcd_ba_local_bundle",
                 "pcd_ba_local_window_opts_default", "pcd_ba_local_window_create_device"):
        assert hasattr(L, name) and name in pcdhip.ABI_SYMBOLS
    assert callable(pcdhip.BA.local_bundle) and callable(pcdhip.BA.local_window) and callable(pcdhip.local_round)
    assert C.sizeof(pcdhip.BALocalBundleOpts) == 48 and C.sizeof(pcdhip.BALocalWindowOpts) == 64
    assert C.sizeof(pcdhip.BALocalWindowInfo) == 56
    o = pcdhip.BALocalBundleOpts(3, 9, 1.0)
    o.reserved[2] = 5
    L.pcd_ba_local_bundle_opts_default(C.byref(o))
    assert (o.image, o.num_images, o.min_tri_angle_deg) == (-1, 6, 6.0) and list(o.reserved) == [0] * 8
    L.pcd_ba_local_bundle_opts_default(None)            # a null pointer is ignored
    w = pcdhip.BALocalWindowOpts(1, 2, 3, 4, 5)
    w.reserved[7] = 1
    L.pcd_ba_local_window_opts_default(C.byref(w))
    assert (w.d_image_set, w.d_point_variable, w.image, w.max_track_length, w.d_extra_const_pose) == (None, None, -1, 1000, None)
    assert list(w.reserved) == [0] * 8
    L.pcd_ba_local_window_opts_default(None)
    # NULL handle / opts / outputs: INVALID ahead of everything else
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert L.pcd_ba_local_bundle_device(None, C.byref(o), p, p, p, None, None, None) == pcdhip.PCD_ERR_INVALID
    assert L.pcd_ba_local_bundle_device(None, None, p, p, p, None, None, None) == pcdhip.PCD_ERR_INVALID
    assert L.pcd_ba_local_bundle(None, C.byref(o), p, p, None, None) == pcdhip.PCD_ERR_INVALID
    assert b"null" in L.pcd_last_error()
    h, info = C.c_void_p(123), pcdhip.BALocalWindowInfo(1, 2, 3, 4, 5, 6, 7.0)
    assert L.pcd_ba_local_window_create_device(None, C.byref(w), None, None, None, C.byref(h),
                                               C.byref(info)) == pcdhip.PCD_ERR_INVALID
    assert h.value is None and (info.num_images_in, info.num_points_fixed, info.num_obs, info.build_ms) == (0, 0, 0, 0.0)
    assert L.pcd_ba_local_window_create_device(None, None, None, None, None, C.byref(h), None) == pcdhip.PCD_ERR_INVALID
    assert L.pcd_ba_local_window_create_device(None, C.byref(w), None, None, None, None, None) == pcdhip.PCD_ERR_INVALID


def test_round_and_percentile_index():
    assert [lb.percentile_index(n) for n in (1, 2, 3, 7)] == [0, 1, 2, 5]     # 0, .75, 1.5, 4.5 rounded
    assert lb.std_round(1.5) == 2 and lb.std_round(4.5) == 5 and lb.std_round(2.5) == 3 and lb.std_round(0.5) == 1
    assert round(4.5) == 4 and int(np.round(2.5)) == 2                         # what the restatement must not use
    assert lb.std_round(0.75) == 1 and lb.std_round(0.25) == 0
    assert lb.percentile([5.0]) == 5.0 and lb.percentile([9.0, 1.0]) == 9.0
    assert lb.percentile([3.0, 1.0, 2.0]) == 3.0
    assert lb.percentile([7.0, 1.0, 6.0, 2.0, 5.0, 3.0, 4.0]) == 6.0           # index 5 of 1 .. 7
    assert lb.percentile([1.0, 2.0, 3.0, 4.0, 5.0]) == 4.0                     # index 3
    assert math.isnan(lb.percentile([1.0, math.nan, 0.5]))                     # index 2: the NaN is last
    assert lb.percentile([1.0, math.nan, 0.5, 0.7, 0.6]) == 1.0                # index 3: the largest number, not the NaN


def test_shared_counts_per_row_and_the_tie_order():
    # image 0 sees point 0 twice and point 1 once (n = 3); image 1 sees point 0 once, image 2 sees point 0 and point 1,
    # image 3 sees point 1 twice, image 4 only point 2
    obs_image = [0, 0, 0, 1, 2, 2, 3, 3, 4]
    obs_point = [0, 0, 1, 0, 0, 1, 1, 1, 2]
    shared, n = lb.shared_counts(obs_image, obs_point, 5, 3, 0)
    assert n == 3 and list(shared) == [0, 2, 3, 2, 0]   # a point seen through two rows counts twice
    assert lb.candidates(shared) == [2, 1, 3]           # the tie of images 1 and 3 goes to the lower index
    assert lb.candidates([0, 4, 4, 4, 9]) == [4, 1, 2, 3] and lb.candidates([0, 0]) == []
    shared, n = lb.shared_counts(obs_image, obs_point, 5, 3, 4)
    assert n == 1 and not shared.any()                  # nobody else sees point 2


def no_angle(j):
    raise AssertionError("no angle is computed on the copy path")


def test_copy_path_below_and_at_num_images():
    shared = {3: 5, 1: 4, 2: 4}
    for num_images in (5, 4):                           # 3 candidates < 4, == 3
        bundle, fired, tri = lb.select([3, 1, 2], shared, 10, no_angle, num_images, 6.0)
        assert bundle == [3, 1, 2] and fired == [] and set(tri.values()) == {-1.0}
    bundle, fired, tri = lb.select([], {}, 0, no_angle, 6, 6.0)
    assert bundle == [] and fired == []


def test_three_passes_append_out_of_count_order():
    """n = 10, num_images = 4.  A (9 shared) never reaches an angle a pass asks for before the bundle is full, B (7) passes
    at once, C (6) only at m / 1.5, D (5) enters with the third pass's bound of 5: B, C, D, not the count order A, B, C"""
    A, B, Cc, D, E = 10, 11, 12, 13, 14
    shared = {A: 9, B: 7, Cc: 6, D: 5, E: 4}
    tri = {A: 0.03, B: 0.2, Cc: 0.08, D: 0.2, E: 0.5}
    assert M / 1.5 < 0.08 < M and 0.03 < M / 3.0
    bundle, fired, got = lb.select([A, B, Cc, D, E], shared, 10, tri.get, 4, 6.0)
    assert bundle == [B, Cc, D] and fired == [0, 1, 2] and bundle != [A, B, Cc]
    assert got == tri                                   # every candidate has shared >= 0.1 * n
    # with room for four, pass 3 (bound 4) takes E, and the bundle is full before A is asked again
    bundle, fired, _ = lb.select([A, B, Cc, D, E], shared, 10, tri.get, 5, 6.0)
    assert bundle == [B, Cc, D, E] and fired == [0, 1, 2, 3]


def test_fill_up_and_the_computed_set():
    # nobody has an angle: the fill-up takes the count order; the candidate below 0.1 * n gets no angle at all
    shared = {1: 50, 2: 40, 3: 30, 4: 9}
    asked = []
    def tri_of(j):
        asked.append(j)
        return 0.001
    bundle, fired, tri = lb.select([1, 2, 3, 4], shared, 100, tri_of, 3, 6.0)
    assert bundle == [1, 2] and fired == [lb.FILL_UP] and asked == [1, 2, 3] and tri[4] == -1.0
    # image 4 (10 shared = 0.1 * n) is reached by pass 6 alone (m / 5, bound 10) and passes; image 3 has exactly m / 6 and
    # passes in pass 7 (>=); the fill-up puts the most connected image behind them
    tri_v = {1: 0.001, 2: 0.001, 3: M / 6.0, 4: 0.5}
    bundle, fired, _ = lb.select([1, 2, 3, 4], {**shared, 4: 10}, 100, tri_v.get, 4, 6.0)
    assert bundle == [4, 3, 1] and fired == [6, 7, lb.FILL_UP]
    # a NaN percentile never passes a >= and is taken by the fill-up only
    bundle, fired, _ = lb.select([1, 2, 3], {1: 9, 2: 8, 3: 7}, 10, {1: math.nan, 2: 0.3, 3: 0.3}.get, 3, 6.0)
    assert bundle == [2, 3] and fired == [0]


def test_a_fractional_bound():
    """shared = 3 of n = 7: 0.5 * 7 = 3.5 > 3 fails pass 2, 0.4 * 7 = 2.8 <= 3 passes pass 3"""
    assert 3.0 < 0.5 * 7 and 3.0 >= 0.4 * 7
    shared = {1: 3, 2: 1, 3: 1}
    tri = {1: M / 2.0, 2: 0.0, 3: 0.0}                  # reaches the angle of pass 2 exactly, but not its bound
    bundle, fired, _ = lb.select([1, 2, 3], shared, 7, tri.get, 3, 6.0)
    assert bundle[0] == 1 and fired[0] == 3
    bundle, fired, _ = lb.select([1, 2, 3], {**shared, 1: 4}, 7, tri.get, 3, 6.0)
    assert bundle[0] == 1 and fired[0] == 2             # 4 >= 3.5: the same image enters one pass earlier


def ident(c):
    return [1.0, 0.0, 0.0, 0.0, -c[0], -c[1], -c[2]]


def test_the_percentile_is_over_every_row_of_the_image():
    """centres 1 apart, points above the middle of the baseline at heights h: the angle is 2 atan(0.5 / h).  Image 0 sees
    seven points, image 1 shares only the farthest: the percentile is still the 6th smallest of all seven"""
    hs = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    points = np.array([[0.5, 0.0, h] for h in hs] + [[0.5, 0.0, 50.0]])
    poses = np.array([ident([0, 0, 0]), ident([1, 0, 0]), ident([2, 0, 0]), ident([3, 0, 0])])
    obs_image = [0] * 7 + [1, 2, 2, 3, 3, 3]
    obs_point = list(range(7)) + [6, 6, 5, 6, 5, 4]
    r = lb.local_bundle(obs_image, obs_point, poses, points, 0, num_images=3)
    assert r["n"] == 7 and list(r["shared"]) == [0, 1, 2, 3] and r["num"] == 2
    angles = sorted(2.0 * math.atan(0.5 / h) for h in hs)
    assert abs(r["tri_angle"][1] - angles[5]) < 1e-15 and r["tri_angle"][1] > 2.0 * math.atan(0.5 / 7.0) * 3
    # the angle to centre 3 apart over the same rows; the duplicated row of the next case enters twice
    X = points[:7]
    t3 = lb.tri_percentile(fr.proj_center(poses[0]), fr.proj_center(poses[3]), X)
    assert r["tri_angle"][3] == t3
    more = lb.tri_percentile(fr.proj_center(poses[0]), fr.proj_center(poses[1]), np.concatenate([X, X[:1], X[:1]]))
    assert lb.percentile_index(9) == 6 and abs(more - angles[6]) < 1e-15     # the nearest point three times: index 6 is its angle
    # the normalised quaternion: scaling a pose's quaternion changes nothing
    scaled = poses.copy(); scaled[1, :4] *= 3.0
    r2 = lb.local_bundle(obs_image, obs_point, scaled, points, 0, num_images=3)
    assert abs(r2["tri_angle"][1] - r["tri_angle"][1]) < 1e-15 and list(r2["bundle"]) == list(r["bundle"])
    assert lb.angle_gap(r["tri_angle"]) > 1e-3 and lb.angle_gap(np.full(4, -1.0)) == math.inf


def test_fresh_args_on_a_hand_case():
    poses = np.array([ident([0, 0, 0]), ident([1, 0, 0]), ident([30, 0, 0]), ident([31, 0, 0])])
    # p0: variable, rows in and out; p1: not variable, wholly inside; p2: not variable, partly inside; p3: keeps nothing;
    # p4: not variable, wholly inside, with a term
    d = dict(poses=poses, points=np.arange(15.0).reshape(5, 3), point_const=np.array([0, 0, 0, 0, 1], np.uint8),
             obs_image=np.array([0, 2, 0, 1, 1, 3, 2, 3, 0, 1], np.int32),
             obs_point=np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4], np.int32), obs_xy=np.arange(20.0).reshape(10, 2),
             lidar_point=np.array([4, 0, 2], np.int32), lidar_abcd=np.arange(12.0).reshape(3, 4),
             lidar_weight=np.array([1.0, 2.0, 3.0]))
    opts = dict(image_set=[1, 1, 0, 0], point_variable=[1, 0, 0, 0, 0])
    kw, obs_map, info, lkeep, inn, V = lb.fresh_args_local(d, poses, d["points"], opts)
    assert list(kw["obs_image"]) == [0, 2, 0, 1, 1, 0, 1] and list(kw["obs_point"]) == [0, 0, 1, 1, 2, 4, 4]
    assert list(obs_map) == [0, 1, 2, 3, 4, lb.NOT_IN, lb.NOT_IN, lb.NOT_IN, 5, 6]
    assert list(kw["point_const"]) == [0, 0, 1, 0, 1]   # p1 stays variable, p2 becomes constant, p4 was constant
    assert list(kw["image_const_pose"]) == [0, 0, 1, 1] and list(lkeep) == [False, True, False]
    assert info == dict(num_images_in=2, num_points_variable=1, num_points_fixed=1, num_obs=7, num_lidar=1, num_pose_rows=6)
    # the rule: observed by image 0 and at most max_track_length rows
    assert list(lb.variable_by_rule(d["obs_image"], d["obs_point"], 5, 0, 2)) == [1, 1, 0, 0, 1]
    long = dict(d, obs_image=np.append(d["obs_image"], 3).astype(np.int32), obs_point=np.append(d["obs_point"], 0).astype(np.int32),
                obs_xy=np.arange(22.0).reshape(11, 2))
    assert list(lb.variable_by_rule(long["obs_image"], long["obs_point"], 5, 0, 2)) == [0, 1, 0, 0, 1]   # 3 rows > 2
    assert list(lb.variable_by_rule(long["obs_image"], long["obs_point"], 5, 0, 3)) == [1, 1, 0, 0, 1]   # == the bound
    kw, _, info, _, _, V = lb.fresh_args_local(long, poses, d["points"], dict(image_set=[1, 1, 0, 0], image=0, max_track_length=2))
    assert list(V) == [0, 1, 0, 0, 1] and list(kw["point_const"]) == [1, 0, 1, 0, 1] and info["num_points_fixed"] == 2
    assert len(d["obs_image"]) == 10                    # the input is left alone


def test_shim_refusals_without_a_gpu():
    """shim/test_ba_local without --gpu: LocalRound without a live handle and the host selection of the mock scene"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_local"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_local")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

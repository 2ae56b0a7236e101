"""The numpy side of the depth-projection route (tests/ba_proj_ref.py): the selection against the hand-computed cases of
shim/test_shim.cc TestMatchVariablePoint, and the scene the GPU tests use against the CPU oracle -- it must exercise the
pick (several candidates from distinct cloud rows, a winner that is not the first), or bit equality there shows little."""
import ctypes as C

import numpy as np

from tests import ba_proj_ref as pr

NEW_SYMBOLS = ["pcd_proj_set_new_images_device", "pcd_ba_proj_opts_default", "pcd_ba_project_lidar_device"]


def test_new_symbols_defaults_and_argument_checks(pcdhip):
    """what needs no device: the symbols, the documented defaults, the checks that come before any device is touched"""
    from tests.test_abi import _declared_symbols
    declared = _declared_symbols()
    L = pcdhip.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and s in pcdhip.ABI_SYMBOLS and hasattr(L, s), s
    o = pcdhip.BAProjOpts()
    C.memset(C.byref(o), 0xAB, C.sizeof(o))
    L.pcd_ba_proj_opts_default(C.byref(o))
    assert o.gate_mode == pcdhip.GATE_MAPPER_LOCAL == 0
    assert (o.proj_weight, o.icp_weight, o.icp_ground_weight) == (1.0, 100.0, 1000.0)
    assert o.cam_width is None and o.cam_height is None and o.d_image_select is None and o.d_point_mode is None
    assert o.d_max_range is None and o.max_range_count == 0 and list(o.reserved) == [0] * 8
    L.pcd_ba_proj_opts_default(None)
    # the structs are the header's: 4 x 8 + 4 (+4) + 8 + 8 + 3 x 8 + 32; 8 x 8 + 3 x 8
    assert C.sizeof(pcdhip.BAProjOpts) == 112 and C.sizeof(pcdhip.BAProjInfo) == 88
    err = lambda: L.pcd_last_error().decode()
    info = pcdhip.BAProjInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    assert L.pcd_ba_project_lidar_device(None, None, None, None, C.byref(info)) == pcdhip.PCD_ERR_INVALID
    assert "null options" in err() and info.num_terms == 0 and info.pairs == 0
    assert L.pcd_ba_project_lidar_device(None, None, C.byref(o), None, None) == pcdhip.PCD_ERR_INVALID
    assert "cam_width" in err()
    wh = (C.c_uint64 * 1)(4032)
    o.cam_width = o.cam_height = C.cast(wh, C.c_void_p)
    assert L.pcd_ba_project_lidar_device(None, None, C.byref(o), None, None) == pcdhip.PCD_ERR_INVALID
    assert "null handle" in err()
    assert L.pcd_proj_set_new_images_device(None, C.c_uint64(0), None, C.c_uint64(0), None, None, None, None, None, None,
                                            None) == pcdhip.PCD_ERR_INVALID


def test_pick_reproduces_the_hand_computed_cases():
    X = [1.0, 2.0, 3.0]
    below = [1.0, 2.0, 2.5, 0, 0, 2.0]          # straight below X along its normal: |cos| = 1
    side = [0.0, 2.0, 2.5, 0, 0, -4.0]          # offset sideways: |cos| = 0.5 / sqrt(1.25)
    which, abcd, xyz = pr.pick(X, [below, side])
    assert which == 1 and xyz[0] == 0.0 and xyz[2] == 2.5
    assert abcd[2] == -1.0 and abcd[3] == 2.5                      # normalised plane z = 2.5
    dist, angle = pr.dist_angle(X, abcd, xyz)
    assert abs(dist - 0.5) < 1e-15 and abs(angle - 0.5 / np.sqrt(1.25)) < 1e-15
    assert pr.pick(X, [])[0] == -1
    which, abcd, xyz = pr.pick(X, [below])
    assert which == 0 and xyz[0] == 1.0 and pr.dist_angle(X, abcd, xyz)[1] == 1.0


def test_pick_ties_nan_and_order():
    X = [0.0, 0.0, 1.0]
    a = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    b = [-1.0, 0.0, 0.0, 0.0, 0.0, 1.0]          # the mirror image: the same |cos|
    assert pr.pick(X, [a, b])[0] == 0 and pr.pick(X, [b, a])[0] == 0            # strict <: the first of a tie stays
    zero_normal = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    on_point = [0.0, 0.0, 1.0, 0.0, 0.0, 1.0]                                    # vn = 0
    assert pr.pick(X, [zero_normal])[0] == -1 and pr.pick(X, [on_point])[0] == -1
    assert pr.pick(X, [zero_normal, a, on_point])[0] == 1


def test_candidates_keep_the_first_found_observation_per_image():
    s = dict(points=np.zeros((2, 3)), obs_image=np.array([0, 0, 1, 0], np.int32), obs_point=np.array([0, 0, 0, 1], np.int32))
    feat_obs = np.array([0, 1, 3, 2])
    l6 = np.arange(24, dtype=np.float64).reshape(4, 6)
    c = pr.candidates(s, feat_obs, [0, 1, 1, 1], l6)                             # observation 0 found nothing
    assert [o for o, _ in c[0]] == [1, 2] and [o for o, _ in c[1]] == [3]
    assert np.array_equal(c[0][1][1], l6[3])                                     # feature 3 is observation 2
    c = pr.candidates(s, feat_obs, [1, 1, 1, 1], l6)
    assert [o for o, _ in c[0]] == [0, 2]                                        # observation 1 is a duplicate in image 0


def test_the_scene_exercises_the_pick(oracle):
    xyz, nrm = pr.cloud()
    s = pr.scene(130)
    assert len(s["points"]) == 130 and len(pr.scene(65)["points"]) == 65
    images, feat, feat_obs = pr.proj_inputs(s)
    oo = oracle.proj_options()
    coeffs = oracle.proj_scale_coeffs(oo, images[0]["params"][0], images[0]["params"][1])
    found, index, _, l6, _, _ = oracle.proj_images(xyz, nrm, oo, coeffs, images, feat)
    row = np.zeros(len(s["obs_image"]), np.int64)
    row[feat_obs] = index
    cands = pr.candidates(s, feat_obs, found, l6)
    several = not_first = 0
    for p in range(130):
        rows = {int(row[o]) for o, _ in cands[p]}
        several += len(rows) >= 2
        which = pr.pick(s["points"][p], [c for _, c in cands[p]])[0]
        not_first += which > 0
    print("found", int(found.sum()), "of", len(found), "several", several, "not_first", not_first)
    assert several >= 40 and not_first >= 15

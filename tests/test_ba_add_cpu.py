"""tests/ba_add_ref.py pinned without a GPU: the merge rule of pcd_ba_add_observations_device equals the
stable counting sort pcd_ba_create runs on the concatenated keys, on the boundary inputs; the concatenated description
and the split the device tests use; the exported symbols and the NULL-handle guard; the shim's bookkeeping."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ba_add_ref as ar


def check_merge(old_image, old_point, new_image, new_point, I, P_old, P_new):
    """both CSRs of the concatenated rows, by the merge rule and by the counting sort"""
    for old, new, nold, nnew in ((old_point, new_point, P_old, P_new), (old_image, new_image, I, I)):
        old, new = np.asarray(old, np.int64), np.asarray(new, np.int64)
        st0, li0 = ar.build_csr(old, nold)
        st, li = ar.merge_csr(st0, li0, old, new, nnew)
        rst, rli = ar.build_csr(np.concatenate([old, new]), nnew)
        assert np.array_equal(st, rst) and np.array_equal(li, rli), (old, new)


OLD_IMAGE, OLD_POINT = [0, 1, 2, 0, 1, 2, 2], [0, 0, 1, 2, 2, 3, 0]
BOUNDARY = {
    "no new rows": (OLD_IMAGE, OLD_POINT, [], [], 3, 4, 4),
    "no new rows, new points": (OLD_IMAGE, OLD_POINT, [], [], 3, 4, 7),
    "no old rows": ([], [], [2, 0, 1, 0], [1, 3, 0, 3], 3, 4, 4),
    "no old rows, new points": ([], [], [2, 0, 1, 0], [4, 3, 5, 3], 3, 4, 6),
    "all new rows on one key": (OLD_IMAGE, OLD_POINT, [1, 1, 1], [2, 2, 2], 3, 4, 4),
    "all new rows on the first key": (OLD_IMAGE, OLD_POINT, [0, 0], [0, 0], 3, 4, 4),
    "all new rows on the last key": (OLD_IMAGE, OLD_POINT, [2, 2], [3, 3], 3, 4, 4),
    "new rows only on new points": (OLD_IMAGE, OLD_POINT, [0, 2, 1, 0], [5, 4, 5, 6], 3, 4, 7),
    "duplicated rows": (OLD_IMAGE, OLD_POINT, [0, 0, 2, 2], [0, 0, 0, 0], 3, 4, 4),      # (0, 0) and (2, 0) exist already
    # key 1 has old rows and no new ones, between keys 0 and 2 that have both (points and images alike)
    "a key without new rows between two with": ([0, 1, 2, 1], [0, 1, 2, 1], [2, 0, 0, 2], [2, 0, 0, 2], 3, 3, 3),
    "a key without any row": ([0, 2], [0, 3], [2, 0], [3, 0], 3, 4, 5),
}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_merge_rule_equals_the_counting_sort_on_the_boundaries(name):
    check_merge(*BOUNDARY[name])


def test_merge_rule_equals_the_counting_sort_on_random_rows():
    rng = np.random.default_rng(5)
    for _ in range(30):
        I, P_old, Pn = int(rng.integers(1, 6)), int(rng.integers(1, 9)), int(rng.integers(0, 4))
        O, A = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        check_merge(rng.integers(0, I, O), rng.integers(0, P_old, O), rng.integers(0, I, A), rng.integers(0, P_old + Pn, A),
                    I, P_old, P_old + Pn)


def test_merge_rule_written_out():
    # point 0: rows 0, 1; point 1: row 2; new rows 3 (point 1), 4 (point 2, new), 5 (point 0), 6 (point 1)
    st0, li0 = ar.build_csr([0, 0, 1], 2)
    st, li = ar.merge_csr(st0, li0, [0, 0, 1], [1, 2, 0, 1], 3)
    assert list(st) == [0, 3, 6, 7] and list(li) == [0, 1, 5, 2, 3, 6, 4]


def hand_scene():
    return dict(points=np.arange(9.0).reshape(3, 3), poses=np.zeros((2, 7)), point_const=np.array([0, 1, 0], np.uint8),
                image_const_pose=np.array([0, 1], np.uint8), obs_image=np.array([0, 1, 0, 1], np.int32),
                obs_point=np.array([0, 0, 1, 2], np.int32), obs_xy=np.arange(8.0).reshape(4, 2),
                lidar_point=np.array([2, 0], np.int32), lidar_abcd=np.arange(8.0).reshape(2, 4), lidar_weight=np.array([1.0, 2.0]))


def test_fresh_args_after_add_on_a_hand_case():
    s = hand_scene()
    moved = s["points"] + 100.0                           # the points as a solve left them on the device
    new = dict(obs_image=np.array([1, 0], np.int32), obs_point=np.array([3, 1], np.int32), obs_xy=np.array([[8.0, 9.0], [10.0, 11.0]]))
    kw, info = ar.fresh_args_after_add(s, moved, new, np.array([[-1.0, -2.0, -3.0]]))
    assert list(kw["obs_image"]) == [0, 1, 0, 1, 1, 0] and list(kw["obs_point"]) == [0, 0, 1, 2, 3, 1]
    assert np.array_equal(kw["obs_xy"], np.arange(12.0).reshape(6, 2))
    assert np.array_equal(kw["points"], [[100, 101, 102], [103, 104, 105], [106, 107, 108], [-1, -2, -3]])
    assert list(kw["point_const"]) == [0, 1, 0, 0] and kw["point_const"].dtype == np.uint8
    assert kw["obs_image"].dtype == np.int32 and kw["obs_point"].dtype == np.int32
    for k in ("lidar_point", "lidar_abcd", "lidar_weight", "poses", "image_const_pose"):
        assert kw[k] is s[k]
    # rows 0, 2, 5 are on the variable image 0
    assert info == dict(num_obs=6, num_obs_added=2, num_points=4, num_points_added=1, num_pose_rows=3)
    assert len(s["obs_image"]) == 4 and len(s["points"]) == 3           # the inputs are left alone
    # nothing added; no masks
    bare = {k: v for k, v in s.items() if k not in ("point_const", "image_const_pose")}
    kw0, info0 = ar.fresh_args_after_add(bare, s["points"], dict(obs_image=[], obs_point=[], obs_xy=np.zeros((0, 2))))
    assert "point_const" not in kw0 and np.array_equal(kw0["obs_xy"], s["obs_xy"]) and np.array_equal(kw0["points"], s["points"])
    assert info0 == dict(num_obs=4, num_obs_added=0, num_points=3, num_points_added=0, num_pose_rows=4)


@pytest.mark.parametrize("shuffle", [False, True])
def test_split_then_add_is_a_permutation_of_the_scene(shuffle):
    from pcdhip import synth
    s = synth.ba_scene(6, 200, seed=4)
    s["point_const"] = (np.arange(200) % 5 == 2).astype(np.uint8)
    base, add = ar.split(s, 0.3, 7, seed=9, shuffle=shuffle)
    Pb = 193
    assert len(base["points"]) == Pb == len(base["point_const"]) and len(add["new_points"]) == 7
    assert (base["obs_point"] < Pb).all() and (base["lidar_point"] < Pb).all()
    assert len(base["lidar_point"]) == int((s["lidar_point"] < Pb).sum()) == len(base["lidar_abcd"]) == len(base["lidar_weight"])
    A, O = len(add["obs_image"]), len(s["obs_image"])
    assert 0.2 * O < A < 0.45 * O and (add["obs_point"] >= Pb).sum() == (s["obs_point"] >= Pb).sum() > 0
    kw, info = ar.fresh_args_after_add(base, base["points"], add, add["new_points"])
    assert info["num_obs"] == O and info["num_obs_added"] == A and info["num_points"] == 200 and info["num_points_added"] == 7
    assert np.array_equal(kw["points"], s["points"])
    assert np.array_equal(kw["point_const"][:Pb], s["point_const"][:Pb]) and not kw["point_const"][Pb:].any()

    def rows(d):                                          # the rows as a sorted list: equal lists = a permutation
        r = np.concatenate([np.stack([d["obs_image"], d["obs_point"]], 1).astype(np.float64), d["obs_xy"]], axis=1)
        return r[np.lexsort(r.T[::-1])]
    assert np.array_equal(rows(kw), rows(s))              # hence the same multiset per point and per image
    in_order = np.array_equal(kw["obs_xy"][len(base["obs_xy"]):], s["obs_xy"][np.isin(s["obs_xy"][:, 0], add["obs_xy"][:, 0])])
    assert in_order == (not shuffle)


def test_symbols_and_the_null_handle(pcdhip):
    L = pcdhip.lib()
    for name in ("pcd_ba_add_observations_device", "pcd_ba_add_observations"):
        assert hasattr(L, name) and name in pcdhip.ABI_SYMBOLS
    assert callable(pcdhip.BA.add_observations) and C.sizeof(pcdhip.BAAddInfo) == 48
    assert L.pcd_ba_add_observations(None, None, 0, None, None, None, 0, None) == pcdhip.PCD_ERR_INVALID
    assert L.pcd_ba_add_observations_device(None, None, 0, None, None, None, 0, None, None) == pcdhip.PCD_ERR_INVALID
    info = pcdhip.BAAddInfo(1, 2, 3, 4, 5, 6.0)
    assert L.pcd_ba_add_observations(None, None, 0, None, None, None, 0, C.byref(info)) == pcdhip.PCD_ERR_INVALID
    assert (info.num_obs, info.num_points_added, info.rebuild_ms) == (0, 0, 0.0)          # cleared on every return
    import inspect
    assert inspect.signature(pcdhip.refine_filter).parameters["complete"].default is None


def test_shim_bookkeeping_and_refusals_without_a_gpu():
    """shim/test_ba_add without --gpu: AddObservations without a live handle, with an image or a point the problem does
    not have, and the order of the rows it appends to the shim's flat arrays"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_add"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_add")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

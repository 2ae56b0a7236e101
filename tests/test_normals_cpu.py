"""The numpy reference of the normal estimation (tests/normals_ref.py) checked on its own, without a GPU: its neighbour
sets against scipy's k-d tree, its sensitivity to the summation order against the tolerances the device test uses, the
eigenvalue gaps of the parity clouds those tolerances rely on, the hand cases, and the entry point's refusal on a box
without a device."""
import ctypes as C

import numpy as np
import pytest

from tests import normals_ref as nr

PARITY = [("planes", r) for r in nr.PLANES_RADII] + [("uniform", r) for r in nr.UNIFORM_RADII]


@pytest.mark.parametrize("name,r", PARITY)
def test_bruteforce_neighbours_equal_kdtree(name, r):
    xyz, pairs = nr.parity_pairs(name)
    I, J = pairs[r]
    Ik, Jk = nr.pairs_kdtree(xyz, r)
    assert np.array_equal(I, Ik) and np.array_equal(J, Jk)
    assert np.all(np.bincount(I, minlength=xyz.shape[0]) >= 1)      # every row is its own neighbour


@pytest.mark.parametrize("name,r", PARITY)
def test_summation_order_stays_within_the_device_tolerances(name, r):
    """the tolerances of tests/test_normals_gpu.py are about the order of the fp64 sums only: the reference with its pair
    list shuffled stays inside them"""
    xyz, ref = nr.parity_ref(name, r)
    I, J = nr.parity_pairs(name)[1][r]
    perm = np.random.default_rng(5).permutation(I.shape[0])
    alt = nr.from_pairs(xyz, I, J, perm=perm)
    assert np.array_equal(alt["count"], ref["count"])
    assert np.array_equal(alt["ok"], ref["ok"])
    dc = np.abs(alt["curvature"] - ref["curvature"])
    print("max curvature move / tol", float(np.max(dc / nr.curvature_tol(ref))))
    assert np.all(dc <= nr.curvature_tol(ref))
    wide = ref["ok"] & (ref["gap"] >= nr.GAP_MIN)
    dn = np.abs(alt["normal"].astype(np.float32).astype(np.float64) - ref["normal"].astype(np.float32))
    print("max normal move", float(dn[wide].max()))
    assert np.all(dn[wide] <= nr.normal_tol(ref)[wide, None])


@pytest.mark.parametrize("name,r", PARITY)
def test_parity_clouds_have_the_gaps_the_device_test_relies_on(name, r):
    xyz, ref = nr.parity_ref(name, r)
    narrow = ref["ok"] & (ref["gap"] < nr.GAP_MIN)
    k = ref["count"]
    print(name, r, "mean k %.1f max k %d, k<3: %d, gap<1e-3: %.3f %%, gap<1e-2: %.3f %%" % (
        k.mean(), k.max(), int((k < 3).sum()), 100.0 * narrow.mean(), 100.0 * (ref["ok"] & (ref["gap"] < 1e-2)).mean()))
    assert narrow.mean() <= 0.01
    # no row within a factor 100 of the rank rule l1 <= 1e-10 l2
    assert not np.any((ref["rank"] > 1e-12) & (ref["rank"] < 1e-8))


def test_lattice_hand_cases():
    xyz = nr.lattice()
    idx = np.arange(12 ** 3).reshape(12, 12, 12)
    for r, interior, corner in ((0.125, 7, 4), (0.25, 33, 11)):
        ref = nr.estimate(xyz, r)
        assert np.all(ref["count"][idx[2:-2, 2:-2, 2:-2].ravel()] == interior)      # the boundary `<=` is included
        assert ref["count"][idx[0, 0, 0]] == corner
        assert np.allclose(ref["curvature"][idx[2:-2, 2:-2, 2:-2].ravel()], 1.0 / 3.0, rtol=0, atol=1e-14)


def test_plane_hand_cases():
    xyz = nr.plane_lattice()
    for vp, orient, nz in (((0, 0, 10), nr.ORIENT_VIEWPOINT, 1.0), ((0, 0, 0), nr.ORIENT_NONE, 1.0),
                           ((0, 0, -10), nr.ORIENT_VIEWPOINT, -1.0)):
        ref = nr.estimate(xyz, 0.1, orient=orient, viewpoint=vp)
        assert ref["ok"].all()
        assert np.allclose(ref["normal"], [0.0, 0.0, nz], rtol=0, atol=1e-12)
        assert np.all(np.abs(ref["curvature"]) <= 1e-15)


@pytest.mark.parametrize("scene", nr.degenerate_scenes(), ids=lambda s: s[0])
def test_degenerate_hand_cases(scene):
    name, xyz, r, min_nb, (est, few, deg), bare = scene
    ref = nr.estimate(xyz, r, min_neighbors=min_nb)
    assert (int(ref["ok"].sum()), int(ref["too_few"].sum()), int(ref["degenerate"].sum())) == (est, few, deg)
    assert np.all(ref["normal"][bare] == 0) and np.all(ref["curvature"][bare] == 0)


def test_orientation_tie_rule():
    """a dot product of exactly 0 falls back to the largest component, ties to the lowest axis"""
    xyz = nr.plane_lattice(n=9, spacing=0.125, z=0.0)     # the viewpoint (0,0,0) lies in the plane: n . (v - p) = 0
    ref = nr.estimate(xyz, 0.3)
    assert ref["ok"].all() and np.allclose(ref["normal"], [0, 0, 1], atol=1e-12)


def test_entry_point_refuses_without_a_device(pcdhip):
    L = pcdhip.lib()
    if pcdhip.device_count() > 0:
        # on a GPU box the argument checks come first: a null handle is invalid
        assert L.pcd_cloud_estimate_normals(None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
        assert L.pcd_cloud_estimate_normals_device(None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
        return
    # "no gfx950 device" is the first guard: no handle can exist on this box, so every call ends there
    o = pcdhip.normals_options()
    assert (o.radius, o.min_neighbors, o.orient, list(o.viewpoint), o.only_missing) == (
        np.float32(0.15), 3, pcdhip.NORMALS_ORIENT_VIEWPOINT, [0.0, 0.0, 0.0], 0)
    assert L.pcd_cloud_estimate_normals(None, C.byref(o), None, None, None) == pcdhip.PCD_ERR_NO_DEVICE
    assert L.pcd_cloud_estimate_normals_device(None, C.byref(o), None, None, None) == pcdhip.PCD_ERR_NO_DEVICE
    assert b"no HIP device" in L.pcd_last_error()
    with pytest.raises(pcdhip.PcdError) as e:
        pcdhip.Cloud(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), raw_lidar_frame=False)
    assert e.value.status == pcdhip.PCD_ERR_NO_DEVICE

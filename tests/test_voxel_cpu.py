"""The numpy reference of the voxel-grid downsampling (tests/voxel_ref.py) against hand-computed cases, and the
condition the device test puts on its inputs: on every cloud whose vectors it compares, at most 1 % of the voxels have
a normal sum too weak to compare as a vector."""
import numpy as np
import pytest

from tests import voxel_ref as vr

Z = np.zeros((1, 3), np.float32)


def test_negative_coordinates_floor_not_truncate():
    # -0.01 at leaf 0.05 lies in voxel -1, 0.01 in voxel 0: two voxels, the negative one first
    xyz = np.array([[0.01, 0.01, 0.01], [-0.01, 0.01, 0.01]], np.float32)
    ref = vr.voxelize(xyz, np.zeros_like(xyz), 0.05)
    assert ref["min_b"] == [-1, 0, 0] and ref["dims"] == [2, 1, 1]
    assert ref["num_voxels"] == 2 and list(ref["row_voxel"]) == [1, 0] and ref["keys"] == [0, 1]
    assert np.array_equal(ref["pos32"], xyz[::-1])


def test_point_on_a_face_belongs_to_the_upper_voxel():
    # 0.125 is exact in float32: 0.25 / 0.125 = 2 exactly -> voxel 2, not 1
    xyz = np.array([[0.25, 0, 0], [0.2499, 0, 0], [0.126, 0, 0], [0.0, 0, 0]], np.float32)
    ref = vr.voxelize(xyz, np.zeros_like(xyz), 0.125)
    assert ref["min_b"] == [0, 0, 0] and ref["dims"] == [3, 1, 1]
    assert list(ref["row_voxel"]) == [2, 1, 1, 0] and list(ref["counts"]) == [1, 2, 1]
    m = (np.float64(np.float32(0.2499)) + np.float64(np.float32(0.126))) / 2
    assert ref["c_ref"][1, 0] == m and ref["pos32"][1, 0] == np.float32(m)
    # at 0.05 the float32 product decides: float32(0.15) * float32(20) rounds to 3.0000002 or 2.9999998?  whatever
    # numpy's float32 multiply gives is the definition; the reference must agree with a direct evaluation
    g = (np.arange(10, dtype=np.float32) - 3) * np.float32(0.05)
    inv = np.float32(1.0) / np.float32(0.05)
    want = np.floor((g * inv).astype(np.float32)).astype(np.int64)
    xyz = np.stack([g, np.zeros(10, np.float32), np.zeros(10, np.float32)], axis=1)
    ref = vr.voxelize(xyz, np.zeros_like(xyz), 0.05)
    ids = want - want.min()
    assert ref["min_b"][0] == want.min() and ref["dims"][0] == want.max() - want.min() + 1
    assert np.array_equal(np.asarray(ref["keys"])[ref["row_vid"]], ids)


def test_key_order_is_x_fastest_and_rows_ascend_inside_a_voxel():
    xyz = np.array([[0.5, 0.5, 1.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.5, 1.5], [0.5, 0.5, 0.5]], np.float32)
    ref = vr.voxelize(xyz, np.zeros_like(xyz), 1.0)
    assert ref["dims"] == [2, 2, 2] and ref["keys"] == [0, 1, 2, 4]
    assert list(ref["row_voxel"]) == [3, 1, 2, 3, 0]
    assert list(ref["rows_sorted"]) == [4, 1, 2, 0, 3]
    assert ref["pos32"][3, 0] == np.float32((np.float64(np.float32(0.5)) + np.float64(np.float32(0.6))) / 2)


def test_normals_sum_then_normalise_and_opposed_normals_vanish():
    xyz = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.1, 0.1, 0.1], [1.2, 0.1, 0.1], [2.5, 0.1, 0.1]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32)
    ref = vr.voxelize(xyz, nrm, 1.0)
    assert np.array_equal(ref["nrm32"][0], [0, 0, 0])                         # two opposed normals
    r = np.float32(1 / np.sqrt(2.0))
    assert np.array_equal(ref["nrm32"][1], np.array([r, r, 0], np.float32))   # sum, then normalise
    assert np.array_equal(ref["nrm32"][2], [0, 0, 0])                         # no normal stays no normal
    strong, zero, rest = vr.normal_classes(ref)
    assert list(zero) == [True, False, True] and list(strong) == [False, True, False] and not rest.any()


def test_min_points_drops_voxels_and_keeps_key_order():
    xyz = np.array([[0.5, 0, 0], [1.5, 0, 0], [1.6, 0, 0], [2.5, 0, 0], [3.5, 0, 0], [3.6, 0, 0], [3.7, 0, 0],
                    [np.inf, 0, 0]], np.float32)
    z = np.zeros_like(xyz)
    for mp, rv, nout, dropped in ((0, [0, 1, 1, 2, 3, 3, 3], 4, 0), (1, [0, 1, 1, 2, 3, 3, 3], 4, 0),
                                  (2, [vr.NONE, 0, 0, vr.NONE, 1, 1, 1], 2, 2),
                                  (3, [vr.NONE] * 4 + [0, 0, 0], 1, 4), (5, [vr.NONE] * 7, 0, 7)):
        ref = vr.voxelize(xyz, z, 1.0, min_points=mp)
        assert list(ref["row_voxel"]) == rv + [vr.NONE], mp
        assert (ref["num_input"], ref["num_voxels"], ref["num_output"], ref["num_dropped_rows"]) == (7, 4, nout, dropped)
        assert ref["max_points"] == 3


def test_refusals_and_empty_inputs():
    xyz = np.array([[-50, -50, -50], [50, 50, 50]], np.float32)
    z = np.zeros_like(xyz)
    assert vr.voxelize(xyz, z, 0.01)["keys"][-1] > 2 ** 32                    # large keys are ordinary
    with pytest.raises(ValueError, match="2\\^63"):
        vr.voxelize(xyz, z, 1e-6)
    with pytest.raises(ValueError, match="int32"):
        vr.voxelize(xyz, z, (1e-8, 1.0, 1.0))
    for cloud in (np.zeros((0, 3), np.float32), np.full((4, 3), np.inf, np.float32)):
        ref = vr.voxelize(cloud, np.zeros_like(cloud), 0.05)
        assert ref["num_input"] == ref["num_voxels"] == ref["num_output"] == 0
        assert np.all(ref["row_voxel"] == vr.NONE) and ref["row_voxel"].shape[0] == cloud.shape[0]


def test_crafted_clouds_are_what_they_claim():
    xyz, nrm = vr.segments_cloud()
    ref = vr.voxelize(xyz, nrm, 1.0)
    assert tuple(ref["counts"]) == vr.SEGMENT_LENGTHS and xyz.shape[0] < 50000
    xyz, nrm = vr.sparse_cloud()
    ref = vr.voxelize(xyz, nrm, 0.01)
    assert max(ref["keys"]) > 2 ** 32 and 2000 < ref["num_voxels"] < 5000
    xyz, nrm = vr.mixed_normals_cloud()
    strong, zero, rest = vr.normal_classes(vr.voxelize(xyz, nrm, 1.0))
    assert zero.sum() == 43 and strong.sum() >= 250
    xyz, nrm = vr.straddle_cloud()
    assert vr.voxelize(xyz, nrm, 0.05)["min_b"] == [-6, -6, -6]
    from tests import normals_ref as nr
    assert np.array_equal(vr.planes_cloud()[0], nr.planes_cloud())
    assert np.array_equal(vr.uniform_cloud()[0], nr.uniform_cloud())


@pytest.mark.parametrize("scene", vr.reference_scenes(), ids=lambda s: s[0])
def test_weak_normal_sums_stay_below_the_cap(scene):
    name, xyz, nrm, leaf = scene
    ref = vr.voxelize(xyz, nrm, leaf)
    share = vr.rest_share(ref)
    print("%s: %d voxels, share of weak normal sums %.4f" % (name, ref["num_voxels"], share))
    assert share <= 0.01

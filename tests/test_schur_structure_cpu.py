"""CPU checks of the co-visibility structure: the contract's restatement (tests/schur_structure_ref.py) on a scene
worked by hand, and the two entry points of the device build, which refuse to run without a gfx950 device.

The scene: 3 images, image 1 with a constant pose, so slot 0 = image 0 and slot 1 = image 2; 4 points, point 2
constant.  Observations (image, point) in the caller's order:
    o0 (2,0)  o1 (0,0)  o2 (0,1)  o3 (1,0)  o4 (2,1)  o5 (0,1)  o6 (2,2)  o7 (0,3)  o8 (1,3)
Point 1 is seen twice by image 0 (o2, o5); point 3 by image 0 and the constant-pose image only.
Image-major positions e: image 0 holds o1 o2 o5 o7 = e0..e3, image 1 holds o3 o8 = e4 e5, image 2 holds o0 o4 o6 =
e6 e7 e8, so obs_pos = [6 0 1 4 7 2 8 3 5].
Eliminated: e0 (p0, s0), e1 e2 (p1, s0), e3 (p3, s0), e6 (p0, s1), e7 (p1, s1); not e4 e5 (constant pose), not e8
(constant point).  Lists: p0 = [0 6], p1 = [1 2 7], p3 = [3].
Diagonal block 0: (0,0) (1,1) (1,2) (2,1) (2,2) (3,3).  Diagonal block 1: (6,6) (7,7).  Pair block (0,1): (0,6) (1,7)
(2,7).  blk_start = [0 6 8 11].
Row 0: the diagonal (block 0, col 0 << 1 = 0), then (0,1) (block 2, col 1 << 1 = 2).  Row 1: the transposed (0,1)
(block 2, col 0 << 1 | 1 = 1), then the diagonal (block 1, col 1 << 1 = 2)."""
import ctypes as C

import numpy as np

from tests import schur_structure_ref as ref

SCENE = dict(
    poses=np.zeros((3, 7)), points=np.zeros((4, 3)),
    obs_image=np.array([2, 0, 0, 1, 2, 0, 2, 0, 1], np.int32), obs_point=np.array([0, 0, 1, 0, 1, 1, 2, 3, 3], np.int32),
    image_const_pose=np.array([0, 1, 0], np.uint8), point_const=np.array([0, 0, 1, 0], np.uint8))

WANT = dict(
    slot_image=[0, 2], obs_pos=[6, 0, 1, 4, 7, 2, 8, 3, 5], blk_start=[0, 6, 8, 11],
    ent_a=[0, 1, 1, 2, 2, 3, 6, 7, 0, 1, 2], ent_b=[0, 1, 2, 1, 2, 3, 6, 7, 6, 7, 7], pair_ij=[0, 1],
    row_start=[0, 2, 4], row_blk=[0, 2, 2, 1], row_col=[0, 2, 1, 2])


def test_reference_on_the_hand_worked_scene():
    got = ref.structure(SCENE)
    assert (got["num_slots"], got["num_pairs"], got["num_entries"]) == (2, 1, 11)
    assert got["image_slot"].tolist() == [0, -1, 1]
    for k in ref.LISTS:
        assert got[k].tolist() == WANT[k], k
        assert got[k].dtype == (np.int32 if k == "slot_image" else np.uint32), k


def test_reference_without_masks_and_without_observations():
    s = {k: v for k, v in SCENE.items() if not k.endswith("const") and k != "image_const_pose"}
    got = ref.structure(s)
    assert got["num_slots"] == 3 and got["slot_image"].tolist() == [0, 1, 2]
    # every track now spans its images: p0 {0, 1, 2}, p1 {0, 2}, p2 {2}, p3 {0, 1}
    assert got["pair_ij"].reshape(-1, 2).tolist() == [[0, 1], [0, 2], [1, 2]]
    assert got["num_entries"] == (6 + 2 + 3) + (2 + 3 + 1)      # the diagonal blocks, then the pair blocks
    empty = ref.structure(dict(SCENE, obs_image=np.zeros(0, np.int32), obs_point=np.zeros(0, np.int32)))
    assert empty["num_entries"] == 0 and empty["blk_start"].tolist() == [0, 0, 0]
    assert empty["row_start"].tolist() == [0, 1, 2] and empty["row_blk"].tolist() == [0, 1]


def test_build_entry_points_without_a_handle(pcdhip):
    """the two new entry points are exported and take the guards of the other pcd_ba_schur* calls in their order: no
    gfx950 device -> NO_DEVICE (there is no CPU route), then a NULL handle -> INVALID"""
    L = pcdhip.lib()
    info, lists = pcdhip.BASchurBuildInfo(), pcdhip.BASchurLists()
    want = pcdhip.PCD_ERR_INVALID if pcdhip.device_count() > 0 else pcdhip.PCD_ERR_NO_DEVICE
    assert L.pcd_ba_schur_build_device(None, None, C.byref(info)) == want
    assert L.pcd_ba_schur_build_device(None, None, None) == want
    assert L.pcd_ba_schur_structure_lists(None, C.byref(lists)) == want
    assert (info.build_ms, info.num_slots, info.num_syncs, info.num_pairs, info.num_entries) == (0.0, 0, 0, 0, 0)

"""The co-visibility structure built on the device (pcd_ba_schur_build_device, pcd_ba_schur_structure_lists) against
the contract's restatement in tests/schur_structure_ref.py.  Every comparison is np.array_equal on every list and count:
the order of the lists is the order of every sum downstream, so there is nothing to tolerate."""
import ctypes as C

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_filter_ref as fr
from tests import schur_structure_ref as ref
from tests.test_ba_schur_gpu import _scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _bare(I, P, obs_image, obs_point, const_pose=None, const_point=None):
    """a scene with the given observation lists; the geometry is arbitrary (the structure does not read it)"""
    rng = np.random.default_rng(5)
    poses = np.zeros((I, 7)); poses[:, 0] = 1.0; poses[:, 4:] = rng.normal(0, 0.1, (I, 3))
    points = np.stack([rng.uniform(-2, 2, P), rng.uniform(-2, 2, P), rng.uniform(6, 20, P)], axis=1)
    O = len(obs_image)
    s = dict(cam_model=np.array([4], np.int32), cam_params_list=[synth.OPENCV_PARAMS], poses=poses,
             image_camera=np.zeros(I, np.int32), points=points, obs_image=np.asarray(obs_image, np.int32),
             obs_point=np.asarray(obs_point, np.int32), obs_xy=rng.uniform(0, 3000, (O, 2)))
    if const_pose is not None:
        s["image_const_pose"] = np.asarray(const_pose, np.uint8)
    if const_point is not None:
        s["point_const"] = np.asarray(const_point, np.uint8)
    return s


def _unmasked(seed):
    s = _scene(seed, const=False, tvec=False)
    s.pop("image_const_pose")
    return s


def _duplicated(seed):
    s = _scene(seed, I=10, P=400)
    rng = np.random.default_rng(seed)
    dup = rng.choice(len(s["obs_image"]), 5, replace=False)          # five (image, point) observations once more
    for k in ("obs_image", "obs_point", "obs_xy"):
        s[k] = np.concatenate([s[k], s[k][dup]])
    return s


def _all_const_poses(seed):
    s = _scene(seed)
    s["image_const_pose"][:] = 1
    return s


def _all_const_points(seed):
    s = _scene(seed)
    s["point_const"][:] = 1
    return s


def _empty_image():
    s = _scene(7, const=False, tvec=False)
    s.pop("image_const_pose")
    keep = s["obs_image"] != 2                                        # image 2 keeps its slot and loses every observation
    for k in ("obs_image", "obs_point", "obs_xy"):
        s[k] = s[k][keep]
    return s


def _one_image():
    return _bare(1, 30, np.zeros(40, np.int32), np.arange(40) % 30)


def _no_observations():
    return _bare(4, 10, [], [], const_pose=[0, 1, 0, 0])


def _tracks_of_one():
    rng = np.random.default_rng(3)
    return _bare(5, 300, rng.integers(0, 5, 300), rng.permutation(300))


def _long_track():
    """point 0 seen by all of 40 images and three times by image 17, next to short tracks: a list longer than a
    wavefront, 780 pair blocks from one point"""
    rng = np.random.default_rng(11)
    oi = list(range(40)) + [17, 17]
    op = [0] * 42
    for p in range(1, 120):
        for i in rng.choice(40, rng.integers(1, 4), replace=False):
            oi.append(int(i)); op.append(p)
    perm = rng.permutation(len(oi))
    return _bare(40, 120, np.asarray(oi)[perm], np.asarray(op)[perm])


def _two_lists_of_3000():
    """one point seen 3000 times by each of two images and nothing else: three blocks of 9 M entries, which cross every
    tile boundary of the expansion"""
    return _bare(2, 1, np.repeat([1, 0], 3000), np.zeros(6000, np.int32))


def _many_workgroups():
    s = synth.ba_scene(40, 20_000, seed=4, const_pose_frac=0.2, order="point")
    s["point_const"] = (np.random.default_rng(4).random(20_000) < 0.1).astype(np.uint8)
    s["image_const_pose"][3] = 1
    return s


def _mostly_constant_points():
    """97 % of the points constant: the rows of a tile of the expansion are thousands of observations apart, more than
    the kernel stages in LDS"""
    s = synth.ba_scene(40, 20_000, seed=6, order="image")
    s["point_const"] = (np.random.default_rng(6).random(20_000) < 0.97).astype(np.uint8)
    return s


def _70k_images():
    """more than 2^16 slots: the keys of the pair entries no longer fit 32 bits"""
    rng = np.random.default_rng(8)
    oi = np.concatenate([rng.choice(70_000, 3, replace=False) for _ in range(500)])
    s = _bare(70_000, 500, oi, np.repeat(np.arange(500), 3), const_pose=np.arange(70_000) % 997 == 0)
    return s


SCENES = {
    "masks-point-order": lambda: _scene(31, order="point"),
    "masks-image-order": lambda: _scene(31, order="image"),
    "no-mask": lambda: _unmasked(31),
    "duplicates": lambda: _duplicated(32),
    "every-pose-constant": lambda: _all_const_poses(33),
    "every-point-constant": lambda: _all_const_points(34),
    "image-without-observations": _empty_image,
    "one-image": _one_image,
    "no-observations": _no_observations,
    "tracks-of-one": _tracks_of_one,
    "track-through-40-images": _long_track,
    "two-lists-of-3000": _two_lists_of_3000,
    "72k-observations": _many_workgroups,
    "mostly-constant-points": _mostly_constant_points,
    "70k-images": _70k_images,
}


@pytest.mark.parametrize("name", list(SCENES))
def test_lists_equal_the_contract(gpu, name):
    s = SCENES[name]()
    want = ref.structure(s)
    ba = gpu.BA(**s)
    info = ba.schur_build()
    assert info["num_syncs"] <= 2
    got = ba.schur_lists()
    ref.assert_equal(got, want, name)
    assert (info["num_slots"], info["num_pairs"], info["num_entries"]) == (want["num_slots"], want["num_pairs"], want["num_entries"])
    st = ba.schur_structure()
    assert np.array_equal(st["image_slot"], want["image_slot"]) and st["num_slots"] == want["num_slots"]
    assert np.array_equal(st["pairs"].reshape(-1), want["pair_ij"].astype(np.int32))
    ba.close()
    # what each shape is there for
    if name == "duplicates":
        diag = slice(0, int(want["blk_start"][want["num_slots"]]))
        assert (want["ent_a"][diag] != want["ent_b"][diag]).sum() >= 2
    if name == "every-pose-constant":
        assert want["num_slots"] == 0 and want["num_entries"] == 0
    if name == "every-point-constant":
        assert want["num_slots"] > 0 and want["num_entries"] == 0 and want["num_pairs"] == 0
        assert np.array_equal(want["row_blk"], np.arange(want["num_slots"]))
    if name == "image-without-observations":
        assert want["blk_start"][2] == want["blk_start"][3] and want["num_slots"] == 6
    if name == "tracks-of-one":
        assert want["num_pairs"] == 0 and want["num_entries"] > 0
    if name == "track-through-40-images":
        assert want["num_pairs"] == 780
    if name == "two-lists-of-3000":
        assert np.array_equal(want["blk_start"], [0, 9_000_000, 18_000_000, 27_000_000])
    if name == "mostly-constant-points":
        assert 0 < want["num_entries"] < len(s["obs_image"]) // 8
    if name == "70k-images":
        assert want["num_slots"] > 1 << 16 and want["num_pairs"] > 1000
    if name == "72k-observations":
        assert len(s["obs_image"]) > 70_000 and want["num_pairs"] > 100


def test_after_an_edit(gpu):
    s = _scene(35, I=10, P=400)
    rng = np.random.default_rng(35)
    erase = (rng.random(len(s["obs_image"])) < 0.1).astype(np.uint8)
    pdel = np.zeros(400, np.uint8)
    pdel[[5, 77, 301]] = 1
    kw, obs_map, _, _ = fr.fresh_args_after_remove(s, erase, pdel)
    a = gpu.BA(**s)
    before = a.schur_lists()
    info = a.remove_observations(erase, pdel, want_map=True)
    assert np.array_equal(info["obs_map"].cpu().numpy().view(np.uint32), obs_map)
    assert a.schur_stats()["num_entries"] == 0                        # the edit dropped the structure
    got = a.schur_lists()
    want = ref.structure(kw)
    assert want["num_entries"] < before["num_entries"]
    ref.assert_equal(got, want, "edited handle")
    b = gpu.BA(**kw)
    ref.assert_equal(b.schur_lists(), got, "fresh handle")
    ra, rb = a.schur(1e-3, dense=True), b.schur(1e-3, dense=True)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    a.close(); b.close()


def test_explicit_build(gpu):
    s = _scene(36, I=10, P=400)
    ba = gpu.BA(**s)
    assert ba.schur_stats()["num_entries"] == 0
    side = torch.cuda.Stream()
    first = ba.schur_build(stream=side)
    side.synchronize()
    assert first["num_syncs"] in (1, 2) and first["build_ms"] > 0
    again = ba.schur_build(stream=side)
    assert again["build_ms"] == 0 and again["num_syncs"] == 0
    for k in ("num_slots", "num_pairs", "num_entries"):
        assert again[k] == first[k]
    st, stats = ba.schur_structure(), ba.schur_stats()
    assert st["num_slots"] == first["num_slots"] and len(st["pairs"]) == first["num_pairs"]
    assert stats["num_entries"] == first["num_entries"] and stats["build_ms"] > 0
    lists = ba.schur_lists()
    ref.assert_equal(lists, ref.structure(s), "explicit build")
    bytes_before = ba.schur_stats()["scratch_bytes"]
    # drop and rebuild: an edit that flags nothing still rebuilds the handle's layouts
    info = ba.remove_observations(np.zeros(len(s["obs_image"]), np.uint8), None)
    assert info["num_obs_removed"] == 0 and ba.schur_stats()["num_entries"] == 0
    rebuilt = ba.schur_build()
    assert rebuilt["build_ms"] > 0 and rebuilt["num_syncs"] <= 2
    ref.assert_equal(ba.schur_lists(), lists, "rebuild")
    assert ba.schur_stats()["scratch_bytes"] == bytes_before          # the rebuild allocates nothing new
    ba.close()


def test_layout_guard(gpu):
    """one point seen 40 000 times by each of two variable-pose images: 3 x 40 000^2 = 4.8e9 entries from 80 000
    observations.  The refusal comes from the 64-bit count, before an entry buffer (38 GB) exists."""
    s = _bare(2, 1, np.repeat([0, 1], 40_000), np.zeros(80_000, np.int32))
    ba = gpu.BA(**s)
    base = ba.schur_stats()["scratch_bytes"]
    for call in (ba.schur_build, lambda: ba.schur(1e-3)):
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "32-bit layout" in str(e.value)
    assert ba.schur_stats()["scratch_bytes"] - base < 64e6
    assert ba.schur_stats()["num_entries"] == 0
    cost = ba.evaluate(("cost",))["cost"]
    assert np.isfinite(cost).all() and cost[0] > 0
    ba.close()


def test_guards(gpu):
    L = gpu.lib()
    info, lists = gpu.BASchurBuildInfo(), gpu.BASchurLists()
    assert L.pcd_ba_schur_build_device(None, None, C.byref(info)) == gpu.PCD_ERR_INVALID
    assert L.pcd_ba_schur_structure_lists(None, C.byref(lists)) == gpu.PCD_ERR_INVALID
    s = _scene(37)
    refine = np.zeros(len(synth.OPENCV_PARAMS), np.uint8)
    refine[0] = 1
    ba = gpu.BA(camera_refine=refine, **s)
    for call in (ba.schur_build, ba.schur_lists):
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "camera_refine" in str(e.value)
    ba.close()


def test_capture_refused_then_eager_works(gpu):
    s = _scene(19)
    ba = gpu.BA(**s)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                ba.schur_build()
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
        assert ba.schur_stats() == dict(build_ms=0.0, num_entries=0, scratch_bytes=0)   # nothing was allocated
        info = ba.schur_build()
        side.synchronize()
        assert info["build_ms"] > 0
    ref.assert_equal(ba.schur_lists(), ref.structure(s), "eager build after the refusal")
    ba.close()

"""The local round's start on the device (pcd_ba_local_bundle_device, pcd_ba_local_window_create_device).

The bundle is compared with tests/ba_local_ref.py: bundle, num, image_set and shared for equality, tri_angle for equality
where the restatement has -1 and within MAX_ULP elsewhere.  Selection equality is a property of the INPUTS: every case
asserts on the CPU that no computed percentile lies within GAP = 1e-9 rad of a pass threshold (the margin
tests/test_ba_filter_gpu.py uses for the same acos); the device's acos differs from libm's by a few ulp of ~0.1 rad, eight
orders of magnitude below that.

The window's contract is equality with a FRESH handle: it has the bits of a handle pcd_ba_create builds from the
description ba_local_ref.fresh_args_local states, every result of tests/test_ba_filter_gpu.all_results, solves included.
point_variable, obs_map and the counts are compared for equality with the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_filter_ref as fr
from tests import ba_lidar_ref as lr
from tests import ba_local_ref as lb
from tests import ba_proj_ref as pr
from tests import test_ba_filter_gpu as bf
from tests import test_ba_lidar_gpu as bl

pytestmark = pytest.mark.gpu
WEIGHT = bl.WEIGHT
GAP = 1e-9
# The largest distance between the device's percentile and the restatement's (libm acos) over every case of this file,
# in units of the last place, is MEASURED_ULP (printed by check_bundle; see test_squeezed_scene_fires_every_pass); the
# bound asserted is twice that.
MEASURED_ULP = 1
MAX_ULP = 2 * MEASURED_ULP
_CACHE = {}


def no_ms(d):
    return {k: v for k, v in d.items() if not k.endswith("_ms")}


def base_scene():
    if "base" not in _CACHE:
        _CACHE["base"] = synth.ba_scene(40, 3000, seed=11)
    return _CACHE["base"]


def squeezed(s, image, f):
    """every camera centre pulled towards that of `image` by the factor f (rotations kept): small baselines, small angles"""
    poses = s["poses"].copy()
    c = np.array([fr.proj_center(p) for p in poses])
    c = c[image] + f * (c - c[image])
    q = poses[:, :4] / np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    poses[:, 4:] = -synth._quat_rotate(q, c)
    return dict(s, poses=poses)


def ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def check_bundle(a, desc, image, num_images=6, deg=6.0):
    """the device's bundle of `image` on handle `a` (rows `desc`) against the restatement at the handle's parameters"""
    poses, points = a.get_parameters()
    ref = lb.local_bundle(desc["obs_image"], desc["obs_point"], poses, points, image, num_images, deg)
    assert lb.angle_gap(ref["tri_angle"], deg) > GAP                # a property of the inputs, checked on the CPU
    bundle, info = a.local_bundle(image, num_images, deg, want=("shared", "tri_angle", "bundle"))
    tri = info["tri_angle"].cpu().numpy()
    computed = ref["tri_angle"] >= 0
    worst = int(ulps(tri[computed], ref["tri_angle"][computed]).max()) if computed.any() else 0
    print("local_bundle image %d: n %d, %d angles, fired %s, gap %.3g rad, worst ulp distance %d"
          % (image, ref["n"], int(computed.sum()), ref["fired"], lb.angle_gap(ref["tri_angle"], deg), worst))
    assert np.array_equal(info["shared"].cpu().numpy().view(np.uint32), ref["shared"])
    assert np.array_equal(tri[~computed], ref["tri_angle"][~computed]) and (tri[~computed] == -1.0).all()
    assert worst <= MAX_ULP
    assert list(bundle) == list(ref["bundle"]) and info["num"] == ref["num"]
    full = info["bundle"].cpu().numpy()
    assert list(full[:ref["num"]]) == list(ref["bundle"]) and (full[ref["num"]:] == -1).all()
    assert np.array_equal(info["image_set"].cpu().numpy(), ref["image_set"])
    return ref, info


FIRED = {0.3: [0, 1, 2, 3], 0.1: [2, 3, 4, 5], 0.05: [3, 4, 5], 0.03: [5, 6], 0.02: [5, 6, 7], 0.005: [lb.FILL_UP]}


@pytest.mark.parametrize("f", sorted(FIRED))
def test_squeezed_scene_fires_every_pass(gpu, f):
    """synth.ba_scene(40, 3000, seed=11), image 20 (358 rows, 19 candidates), the centres squeezed: between them the six
    cases append in every pass and in the fill-up, in orders that differ from the count order.  Measured on an MI355X: the
    device's percentile is at most MEASURED_ULP = 1 ulp from the restatement's
    (0 or 1 in every case of this file)."""
    s = squeezed(base_scene(), 20, f)
    a = gpu.BA(**s)
    ref, _ = check_bundle(a, s, 20)
    assert ref["fired"] == FIRED[f] and ref["n"] == 358 and ref["num"] == 5
    if f in (0.1, 0.05, 0.03, 0.02):
        assert list(ref["bundle"]) != lb.candidates(ref["shared"])[:5]
    a.close()


@pytest.mark.parametrize("image", [0, 128, 256])
def test_257_images(gpu, image):
    """more than one workgroup of images (k_lb_shared handles four per workgroup, the sort and the head 257)"""
    if "big" not in _CACHE:
        _CACHE["big"] = synth.ba_scene(257, 20000, seed=3)
    s = _CACHE["big"]
    a = gpu.BA(**s)
    ref, _ = check_bundle(a, s, image)
    assert ref["num"] == 5 and lb.angle_gap(ref["tri_angle"]) > 0.02
    a.close()


@pytest.mark.parametrize("image,ncand", [(0, 4), (6, 5), (11, 3)])
def test_copy_path(gpu, image, ncand):
    s = synth.ba_scene(12, 600, seed=5)
    a = gpu.BA(**s)
    ref, info = check_bundle(a, s, image)
    assert ref["num"] == ncand and ref["fired"] == [] and (info["tri_angle"].cpu().numpy() == -1.0).all()
    a.close()


def drop_rows(s, image, keep_n):
    """the scene with only the first keep_n rows of `image`, and the erase flags that make it from s"""
    rows = np.flatnonzero(s["obs_image"] == image)
    erase = np.zeros(len(s["obs_image"]), np.uint8)
    erase[rows[keep_n:]] = 1
    k = erase == 0
    return dict(s, obs_image=s["obs_image"][k], obs_point=s["obs_point"][k], obs_xy=s["obs_xy"][k]), erase


@pytest.mark.parametrize("n", [63, 64, 65, 256, 257, 1, 0])
def test_row_counts_at_the_wavefront_and_workgroup_edges(gpu, n):
    """n rows on the image, left by remove_observations on the live handle: one short of, exactly and one past a wavefront
    and a workgroup of the angle kernel; one row (percentile index 0); no row (num = 0, only the image in the set)"""
    s = squeezed(base_scene(), 20, 0.1)
    d, erase = drop_rows(s, 20, n)
    a = gpu.BA(**s)
    a.remove_observations(erase, None)
    ref, info = check_bundle(a, d, 20)
    assert ref["n"] == n
    if n == 0:
        assert ref["num"] == 0 and list(np.flatnonzero(info["image_set"].cpu().numpy())) == [20]
    a.close()


@pytest.mark.parametrize("n", [2047, 2048, 2049, 3601])
def test_row_counts_around_and_beyond_the_lds_cache(gpu, n):
    """k_lb_angles keeps the first 2048 angles in LDS and computes the others again in every digit pass: n one short of,
    exactly, one past and far beyond that, on synth.ba_scene(10, 15000, seed=7), image 6 (3601 rows), squeezed by 0.03 so
    that the bundle comes from two late passes and differs from the count order"""
    if "wide" not in _CACHE:
        _CACHE["wide"] = squeezed(synth.ba_scene(10, 15000, seed=7), 6, 0.03)
    s = _CACHE["wide"]
    d, erase = drop_rows(s, 6, n)
    a = gpu.BA(**s)
    if erase.any():
        a.remove_observations(erase, None)
    ref, info = check_bundle(a, d, 6, num_images=3)
    tri = ref["tri_angle"]
    assert ref["n"] == n and ref["fired"] == [4, 5] and int((tri >= 0).sum()) == 3
    assert list(ref["bundle"]) != lb.candidates(ref["shared"])[:2]
    a.close()


def test_a_duplicated_row_counts_twice(gpu):
    s = squeezed(base_scene(), 20, 0.1)
    d, erase = drop_rows(s, 20, 3)
    a = gpu.BA(**s)
    a.remove_observations(erase, None)
    before, _ = check_bundle(a, d, 20)
    p = int(d["obs_point"][d["obs_image"] == 20][0])
    add = dict(obs_image=np.array([20], np.int32), obs_point=np.array([p], np.int32), obs_xy=np.array([[700.0, 500.0]]))
    a.add_observations(**add)
    d2 = dict(d, obs_image=np.append(d["obs_image"], 20).astype(np.int32), obs_point=np.append(d["obs_point"], p).astype(np.int32),
              obs_xy=np.concatenate([d["obs_xy"], add["obs_xy"]]))
    after, _ = check_bundle(a, d2, 20)
    others = np.flatnonzero((d["obs_point"] == p) & (d["obs_image"] != 20))
    assert after["n"] == 4 and len(others) > 0
    j = int(d["obs_image"][others[0]])
    assert after["shared"][j] == before["shared"][j] + 1            # the point's second row on the image counts again
    a.close()


def test_num_images_2_and_a_repeated_call(gpu):
    s = squeezed(base_scene(), 20, 0.05)
    a = gpu.BA(**s)
    ref, _ = check_bundle(a, s, 20, num_images=2)
    assert ref["num"] == 1
    ref, _ = check_bundle(a, s, 20, num_images=20)                   # room for all 19: the copy path
    assert ref["num"] == 19 and ref["fired"] == []
    ref, _ = check_bundle(a, s, 20, num_images=19, deg=2.0)          # one short of all
    assert ref["num"] == 18 and lb.FILL_UP in ref["fired"]
    want = ("shared", "tri_angle", "bundle")
    one = a.local_bundle(20, 6, 6.0, want=want)[1]
    a.local_bundle(3, 4, 1.0, want=want)                             # another call in between, on the same scratch
    two = a.local_bundle(20, 6, 6.0, want=want)[1]
    for k in ("image_set", "shared", "tri_angle", "bundle"):
        assert lr.same_bits(one[k].cpu().numpy(), two[k].cpu().numpy()), k
    a.close()


# ---- the window ---------------------------------------------------------------------------------------------------
def derive(gpu, a, desc, opts):
    """the local window of `a` (description `desc`) and what the restatement expects of it; flags, map and counts compared"""
    poses, points = a.get_parameters()
    kw, obs_map, info_ref, lkeep, inn, V = lb.fresh_args_local(desc, poses, points, opts)
    w, info = a.local_window(opts["image_set"], point_variable=opts.get("point_variable"), image=opts.get("image"),
                             max_track_length=opts.get("max_track_length", 1000),
                             extra_const_pose=opts.get("extra_const_pose"), want=("point_variable", "obs_map"))
    assert {k: info[k] for k in info_ref} == info_ref
    assert (w.O, w.L, w.I, w.P) == (info_ref["num_obs"], info_ref["num_lidar"], a.I, a.P)
    assert np.array_equal(info["point_variable"].cpu().numpy(), V)
    assert np.array_equal(info["obs_map"].cpu().numpy().view(np.uint32), obs_map)
    assert np.array_equal(w.image_const_pose, kw["image_const_pose"])
    return w, kw, lkeep, info


def fresh(gpu, kw, meta=None, lkeep=None):
    if meta is None:
        return gpu.BA(**kw)
    m = {k: v[lkeep] for k, v in meta.items()}
    b = gpu.BA(**{k: v for k, v in kw.items() if not k.startswith("lidar_")})
    b.set_lidar_device(m["type"], kw.get("lidar_abcd", np.zeros((0, 4))), WEIGHT,
                       point=kw.get("lidar_point", np.zeros(0, np.int32)), lidar_xyz=m["lidar_xyz"])
    return b


def check_window(gpu, a, desc, opts, meta=None, solves=True, keep=False):
    w, kw, lkeep, info = derive(gpu, a, desc, opts)
    b = fresh(gpu, kw, meta, lkeep)
    if meta is not None:
        t = w.get_lidar()
        assert lr.same_bits(t["type"], meta["type"][lkeep]) and lr.same_bits(t["lidar_xyz"], meta["lidar_xyz"][lkeep])
    bl.assert_same(bf.all_results(gpu, w, kw, solves), bf.all_results(gpu, b, kw, solves))
    if keep:
        return w, b, kw, info
    w.close(); b.close()
    return None, None, kw, info


def local_opts(s, image, num_images=4):
    """the bundle of `image` by the restatement, and the track-length rule at the median length of the image's points: some
    of them variable, some not"""
    r = lb.local_bundle(s["obs_image"], s["obs_point"], s["poses"], s["points"], image, num_images)
    length = np.bincount(s["obs_point"], minlength=len(s["points"]))
    mine = np.unique(s["obs_point"][s["obs_image"] == image])
    return dict(image_set=r["image_set"], image=image, max_track_length=int(np.median(length[mine])))


def variant(gpu, oracle, cams, name):
    """(live handle, its description, meta) of the source variants of tests/test_ba_window_gpu.py"""
    s0, many = bl.scene(oracle, cams)
    s = dict(bf.filter_scene(oracle, cams))
    I = len(s["poses"])
    meta = None
    if name == "plain":                                 # no mask at all
        s.pop("image_const_pose"); s.pop("point_const")
    elif name == "masks":
        tv = np.zeros(I, np.uint8); tv[[1, 4, 8]] = [0b001, 0b110, 0b101]
        s["image_const_tvec"] = tv
    elif name == "noterms":
        for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
            s.pop(k)
    if name == "meta":                                  # terms with type / lidar_xyz, from set_lidar_device
        base = {k: v for k, v in s.items() if not k.startswith("lidar_")}
        point, typ, abcd, xyz = bl.make_rows(s0, 200, "shuffled", 5, False)
        y = lr.terms(typ, abcd, WEIGHT, point, xyz)
        s = dict(base, lidar_point=y["lidar_point"], lidar_abcd=y["lidar_abcd"], lidar_weight=y["lidar_weight"])
        meta = dict(type=y["type"], lidar_xyz=y["lidar_xyz"])
        a = gpu.BA(**base)
        a.set_lidar_device(typ, abcd, WEIGHT, point=point, lidar_xyz=xyz)
    else:
        a = gpu.BA(**s)
    return a, s, meta


@pytest.mark.parametrize("cams", ["shared", "two"])
@pytest.mark.parametrize("name", ["plain", "masks", "meta", "noterms"])
def test_window_equals_a_fresh_handle(gpu, oracle, cams, name):
    a, s, meta = variant(gpu, oracle, cams, name)
    bf.in_use(gpu, a)
    opts = local_opts(s, 6)
    _, _, kw, info = check_window(gpu, a, s, opts, meta=meta)
    assert info["num_images_in"] == 4 and 0 < info["num_points_variable"] < a.P and 0 < info["num_obs"] < a.O
    assert info["num_points_fixed"] > 0 and info["num_pose_rows"] < info["num_obs"]
    if name != "noterms":
        assert 0 < info["num_lidar"] < a.L               # the terms of the non-variable points are gone
    else:
        assert info["num_lidar"] == 0
    a.close()


def hand(terms=True):
    """four images (0, 1 in; 2, 3 out), five points: p0 variable with a row outside; p1 not variable, wholly inside; p2 not
    variable, partly inside; p3 outside alone; p4 not variable, wholly inside, with a term"""
    centers = [[0, 0, 0], [1, 0, 0], [30, 0, 0], [31, 0, 0]]
    points = [[0.2, 0.1, 9.0], [0.4, -0.2, 11.0], [0.6, 0.3, 10.0], [30.2, 0.1, 9.5], [0.5, 0.0, 12.0]]
    obs_image = [0, 2, 0, 1, 1, 3, 2, 3, 0, 1]
    obs_point = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    s = bf.hand_scene(centers, points, obs_image, obs_point)
    if terms:
        s.update(lidar_point=np.array([4, 0, 2], np.int32), lidar_weight=np.array([100.0, 100.0, 1000.0]),
                 lidar_abcd=np.array([[0.0, 0, 1, -12.01], [0, 0, 1, -9.02], [0, 1, 0, -0.31]]))
    return s


def test_hand_cases(gpu):
    s = hand()
    a = gpu.BA(**s)
    opts = dict(image_set=np.array([1, 1, 0, 0], np.uint8), point_variable=np.array([1, 0, 0, 0, 0], np.uint8))
    w, b, kw, info = check_window(gpu, a, s, opts, solves=False, keep=True)
    # p0 keeps its outside row (image 2: a constant pose); p2 keeps its inside row alone and is constant now; p3 keeps
    # nothing; p1 and p4 stay variable; the terms of p4 and p2 (kept, not variable) are dropped, p0's stays
    assert list(info["obs_map"].cpu().numpy()) == [0, 1, 2, 3, 4, -1, -1, -1, 5, 6]
    assert list(kw["point_const"]) == [0, 0, 1, 0, 0] and list(kw["image_const_pose"]) == [0, 0, 1, 1]
    assert (info["num_points_variable"], info["num_points_fixed"], info["num_lidar"], info["num_obs"]) == (1, 1, 1, 7)
    assert list(w.get_lidar()["point"]) == [0]
    blocks = w.evaluate_blocks(True, False)
    assert list(blocks["pose_row"]) == [0, 0xFFFFFFFF, 1, 2, 3, 4, 5] and blocks["num_pose_rows"] == 6
    w.close(); b.close()
    # a source mask: p4 constant before, p2 constant by the rule: one point fixed by the call
    sc = dict(s, point_const=np.array([0, 0, 0, 0, 1], np.uint8))
    c = gpu.BA(**sc)
    _, _, kw, info = check_window(gpu, c, sc, opts, solves=False)
    assert list(kw["point_const"]) == [0, 0, 1, 0, 1] and info["num_points_fixed"] == 1
    c.close()
    # the rule: observed by image 0 with at most max_track_length rows.  p0, p1, p4 have 2 rows each
    for bound, V in ((2, [1, 1, 0, 0, 1]), (1, [0, 0, 0, 0, 0])):
        _, _, kw, info = check_window(gpu, a, s, dict(image_set=opts["image_set"], image=0, max_track_length=bound), solves=False)
        assert list(info["point_variable"].cpu().numpy()) == V
    # one row more on p0 (length 3): equal to the bound 3 it is variable, one above the bound 2 it is not and becomes
    # constant, keeping its inside row alone
    a.add_observations(np.array([3], np.int32), np.array([0], np.int32), np.array([[400.0, 300.0]]))
    s3 = dict(s, obs_image=np.append(s["obs_image"], 3).astype(np.int32), obs_point=np.append(s["obs_point"], 0).astype(np.int32),
              obs_xy=np.concatenate([s["obs_xy"], [[400.0, 300.0]]]))
    _, _, kw, info = check_window(gpu, a, s3, dict(image_set=opts["image_set"], image=0, max_track_length=3), solves=False)
    assert list(info["point_variable"].cpu().numpy()) == [1, 1, 0, 0, 1] and kw["point_const"][0] == 0
    _, _, kw, info = check_window(gpu, a, s3, dict(image_set=opts["image_set"], image=0, max_track_length=2), solves=False)
    assert list(info["point_variable"].cpu().numpy()) == [0, 1, 0, 0, 1] and kw["point_const"][0] == 1
    assert list(info["obs_map"].cpu().numpy()) == [0, -1, 1, 2, 3, -1, -1, -1, 4, 5, -1]
    a.close()


def test_every_image_in_only_the_image_in_and_no_variable_pose(gpu, oracle):
    s = bf.filter_scene(oracle, "shared")
    I, P = len(s["poses"]), len(s["points"])
    a = gpu.BA(**s)
    before = bf.all_results(gpu, a, s)
    a.schur(1e-3, want=("cost",))                       # a Schur state from before the derivations
    opts = local_opts(s, 6)
    # every image in, every point variable: the source's own fresh handle (its masks passed as arrays)
    _, _, kw, info = check_window(gpu, a, s, dict(image_set=np.ones(I, np.uint8), point_variable=np.ones(P, np.uint8)))
    assert info["num_obs"] == a.O and info["num_lidar"] == a.L and info["num_points_fixed"] == 0
    assert np.array_equal(kw["image_const_pose"], s["image_const_pose"]) and np.array_equal(kw["point_const"], s["point_const"])
    # only the image in
    only = np.zeros(I, np.uint8); only[6] = 1
    _, _, _, info = check_window(gpu, a, s, dict(opts, image_set=only))
    assert info["num_images_in"] == 1 and info["num_obs"] > int((s["obs_image"] == 6).sum())
    # every "in" image fixed by the caller: no variable pose (evaluate only)
    _, _, _, info = check_window(gpu, a, s, dict(opts, extra_const_pose=opts["image_set"]), solves=False)
    assert info["num_pose_rows"] == 0 and info["num_obs"] > 0
    # no image in, no variable point: O == 0, L == 0
    _, _, _, info = check_window(gpu, a, s, dict(image_set=np.zeros(I, np.uint8), point_variable=np.zeros(P, np.uint8)),
                                 solves=False)
    assert (info["num_obs"], info["num_lidar"], info["num_points_variable"], info["num_points_fixed"]) == (0, 0, 0, 0)
    # two derivations give the same window; the source is untouched and its Schur state still solves
    w1, _, _, i1 = derive(gpu, a, s, opts)
    w2, _, _, i2 = derive(gpu, a, s, opts)
    bl.assert_same(bf.all_results(gpu, w1, s), bf.all_results(gpu, w2, s))
    assert np.array_equal(i1["obs_map"].cpu().numpy(), i2["obs_map"].cpu().numpy())
    w1.close(); w2.close()
    a.schur_solve_pcg()
    bl.assert_same(bf.all_results(gpu, a, s), before)
    a.close()


def test_either_handle_outlives_the_other(gpu, oracle):
    s = bf.filter_scene(oracle, "shared")
    opts = local_opts(s, 3)
    a = gpu.BA(**s)
    w, kw, _, _ = derive(gpu, a, s, opts)
    a.close()                                           # the window owns its buffers
    b = gpu.BA(**kw)
    bl.assert_same(bf.all_results(gpu, w, kw), bf.all_results(gpu, b, kw))
    w.close(); b.close()
    a = gpu.BA(**s)
    before = bf.all_results(gpu, a, s)
    w, _, _, _ = derive(gpu, a, s, opts)
    w.close()
    bl.assert_same(bf.all_results(gpu, a, s), before)
    a.close()


def test_follow_up_edits_on_the_window(gpu, oracle):
    s = pr.scene(65)
    xyz, nrm = pr.cloud()
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    a = gpu.BA(**s)
    w, kw, _, info = derive(gpu, a, s, local_opts(s, 12, 3))
    assert 0 < w.O < a.O
    b = gpu.BA(**kw)
    for h in (w, b):
        h.associate_lidar(cloud, max_range=0.5, select=info["point_variable"])
    assert w.L > 0
    bl.assert_same(w.get_lidar(), b.get_lidar())
    erase, pdel = bf.random_flags(kw, 31, 0.3, 3)
    iw, ib = w.remove_observations(erase, pdel), b.remove_observations(erase, pdel)
    bl.assert_same(no_ms(iw), no_ms(ib))
    bl.assert_same(w.evaluate(bl.EVERY), b.evaluate(bl.EVERY))
    kept = np.flatnonzero(pdel == 0)[:4]
    add = dict(obs_image=np.array([3, 9, 3, 20], np.int32), obs_point=kept.astype(np.int32),
               obs_xy=np.array([[100.0, 200.0], [300.0, 50.0], [1000.0, 900.0], [2000.0, 1500.0]]))
    iw, ib = w.add_observations(**add), b.add_observations(**add)
    bl.assert_same(no_ms(iw), no_ms(ib))
    bl.assert_same(bf.all_results(gpu, w, kw), bf.all_results(gpu, b, kw))
    w.close(); b.close(); a.close(); cloud.close()


def test_commit_carries_the_parameters_back(gpu, oracle):
    s = bf.filter_scene(oracle, "two")
    a = gpu.BA(**s)
    a.schur(1e-3, want=("cost",))
    st0 = a.schur_structure()
    w, kw, _, info = derive(gpu, a, s, local_opts(s, 3))
    summary, _ = gpu.ba_solve(w, max_num_iterations=3, linear_solver="cholesky")
    assert summary["num_accepted"] > 0
    poses, points = w.get_parameters()
    cp, cx = np.asarray(kw["image_const_pose"]) != 0, np.asarray(kw["point_const"]) != 0
    kept = np.bincount(kw["obs_point"], minlength=a.P) > 0
    still = cx | ~kept                                  # the new constant points and the points without a row never move
    assert lr.same_bits(poses[cp], s["poses"][cp]) and lr.same_bits(points[still], s["points"][still])
    assert not lr.same_bits(poses, s["poses"]) and not lr.same_bits(points, s["points"])
    a.commit_window(w)
    got = a.get_parameters()
    assert lr.same_bits(got[0], poses) and lr.same_bits(got[1], points)
    with pytest.raises(gpu.PcdError) as e:              # the numeric Schur state belonged to the old parameters
        a.schur_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    bl.assert_same(a.schur_structure(), st0)            # the co-visibility structure is still there
    moved = dict(s, poses=poses, points=points)
    b = gpu.BA(**moved)
    bl.assert_same(bf.all_results(gpu, a, moved), bf.all_results(gpu, b, moved))
    w.close(); b.close(); a.close()


def test_local_round_equals_the_host_route(gpu, oracle):
    s = pr.scene(200)
    xyz, nrm = pr.cloud()
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    opts = dict(max_num_iterations=3, linear_solver="cholesky")
    I, P = len(s["poses"]), len(s["points"])
    extra = np.zeros(I, np.uint8); extra[10] = 1
    num = np.arange(P, dtype=np.int32) % 5
    images = (8, 11)
    # the host route: download, select, a fresh handle, associate, solve, upload
    h = gpu.BA(**s)
    host = []
    for image in images:
        poses, points = h.get_parameters()
        r = lb.local_bundle(s["obs_image"], s["obs_point"], poses, points, image, 3)
        assert lb.angle_gap(r["tri_angle"]) > GAP
        o = dict(image_set=r["image_set"], image=image, max_track_length=3, extra_const_pose=extra)
        kw, _, info, _, _, V = lb.fresh_args_local(s, poses, points, o)
        f = gpu.BA(**kw)
        ainfo = f.associate_lidar(cloud, max_range=gpu.search_range_schedule(num), gate_mode=gpu.GATE_MAPPER_LOCAL, select=V)
        summary, its = gpu.ba_solve(f, **opts)
        h.set_parameters(*f.get_parameters())
        f.close()
        host.append((list(r["bundle"]), info, no_ms(ainfo), no_ms(summary), its))
    # the device route on one live handle
    a = gpu.BA(**s)
    a.schur_build()
    for image, (bundle, info, ainfo, summary, its) in zip(images, host):
        dbundle, winfo, dinfo, dsummary, dits = gpu.local_round(a, cloud, image, num_images=3, max_track_length=3,
                                                                extra_const_pose=extra, opt_num=num, **opts)
        assert list(dbundle) == bundle and {k: winfo[k] for k in info} == info
        assert info["num_lidar"] == 0 and 0 < info["num_points_variable"] and info["num_points_fixed"] > 0
        bl.assert_same(no_ms(dinfo), ainfo)
        assert dinfo["num_terms"] > 0 and dsummary["num_accepted"] > 0
        bl.assert_same(no_ms(dsummary), summary)
        bl.assert_same([no_ms(i) for i in dits], [no_ms(i) for i in its])
    bl.assert_same(a.get_parameters(), h.get_parameters())
    assert a.O == len(s["obs_point"]) and a.schur_build()["build_ms"] == 0       # rows and structure of the source stay
    a.close(); h.close(); cloud.close()


def test_refusals(gpu, oracle):
    import torch
    s = bf.filter_scene(oracle, "shared")
    a = gpu.BA(**s)
    full = bf.all_results(gpu, a, s)
    before = a.evaluate(bl.EVERY)
    I, P = a.I, a.P
    for kw in (dict(image=I), dict(image=-1), dict(image=0, num_images=1), dict(image=0, num_images=0),
               dict(image=0, min_tri_angle=-1.0), dict(image=0, min_tri_angle=float("nan"))):
        with pytest.raises(gpu.PcdError) as e:
            a.local_bundle(**kw)
        assert e.value.status == gpu.PCD_ERR_INVALID, kw
    iset, var = np.ones(I, np.uint8), np.ones(P, np.uint8)
    for kw in (dict(image_set=None, image=0),                                               # no set
               dict(image_set=iset), dict(image_set=iset, image=0, point_variable=var),     # neither; both
               dict(image_set=iset, image=I), dict(image_set=iset, image=-2)):
        with pytest.raises(gpu.PcdError) as e:
            a.local_window(**kw)
        assert e.value.status == gpu.PCD_ERR_INVALID, kw
        bl.assert_same(a.evaluate(bl.EVERY), before)
    L = gpu.lib()                                       # NULL outputs on a live handle
    o = gpu.BALocalBundleOpts()
    L.pcd_ba_local_bundle_opts_default(C.byref(o))
    o.image = 0
    t = torch.empty(64, dtype=torch.int32, device="cuda")
    for args in ((None, t.data_ptr(), t.data_ptr()), (t.data_ptr(), None, t.data_ptr()), (t.data_ptr(), t.data_ptr(), None)):
        assert L.pcd_ba_local_bundle_device(a._h, C.byref(o), *args, None, None, None) == gpu.PCD_ERR_INVALID
    w, _ = a.local_window(iset, image=0)
    d_set = torch.from_numpy(iset).cuda()              # staged ahead of the capture: a copy from the host cannot be captured
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            for call in (lambda: a.local_bundle(0), lambda: a.local_window(d_set, image=0), lambda: a.commit_window(w)):
                with pytest.raises(gpu.PcdError) as e:
                    call()
                assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
    bl.assert_same(a.evaluate(bl.EVERY), before)
    bundle, _ = a.local_bundle(0)                       # the handle works as before
    assert len(bundle) > 0
    bl.assert_same(bf.all_results(gpu, a, s), full)     # every result, the solves and the structure included
    w.close(); a.close()


def test_shim_local_round(gpu):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_local"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_local"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

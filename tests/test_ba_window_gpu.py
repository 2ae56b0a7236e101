"""The sphere window of a global round derived on the device (pcd_ba_window_create_device, pcd_ba_window_commit_device,
DESIGN 4.3f).

The contract is equality with a FRESH handle: the window has the bits of a handle pcd_ba_create builds from the
description tests/ba_window_ref.fresh_args_window states (the source's cameras and masks, its parameters as they are on
the device, the window's pose mask, the rows and terms of the active points in their old order): every result of
tests/test_ba_filter_gpu.all_results, solves included.  image_in, point_active, obs_map and the counts are compared for
equality with the numpy restatement.

Radii sit in the middle of a gap of the restatement's sorted distances, and the tests assert on the CPU that no image
centre lies within 1e-9 * radius of the boundary: sqrt and the products are correctly rounded on both sides, so the
margin is far above anything the two could differ by.  The exact-equality cases use integer inputs."""
import os
import subprocess

import numpy as np
import pytest

from tests import ba_lidar_ref as lr
from tests import ba_proj_ref as pr
from tests import ba_window_ref as wr
from tests import test_ba_filter_gpu as bf
from tests import test_ba_lidar_gpu as bl

pytestmark = pytest.mark.gpu
WEIGHT = bl.WEIGHT
MARGIN = 1e-9
CENTERS = (8, 11)                        # of test_global_round: two overlapping spheres, the centre moving


def sphere(poses, center, k):
    """options of a sphere around `center` holding its k nearest images, the boundary in a gap"""
    r, rel = wr.gap_radius(poses, center, k)
    assert rel > MARGIN
    return dict(center_image=center, radius=r)


def no_ms(d):
    return {k: v for k, v in d.items() if not k.endswith("_ms")}


def derive(gpu, a, desc, opts):
    """the window of `a` (description `desc`) and what the restatement expects of it; flags, map and counts compared"""
    poses, points = a.get_parameters()
    kw, obs_map, info_ref, lkeep, inn, act = wr.fresh_args_window(desc, poses, points, opts)
    w, info = a.sphere_window(opts.get("center_image"), opts.get("radius", 40.0), image_set=opts.get("image_set"),
                              extra_const_pose=opts.get("extra_const_pose"), want=("image_in", "point_active", "obs_map"))
    assert {k: info[k] for k in info_ref} == info_ref
    assert (w.O, w.L, w.I, w.P) == (info_ref["num_obs"], info_ref["num_lidar"], a.I, a.P)
    assert np.array_equal(info["image_in"].cpu().numpy(), inn)
    assert np.array_equal(info["point_active"].cpu().numpy(), act)
    assert np.array_equal(info["obs_map"].cpu().numpy().view(np.uint32), obs_map)
    return w, kw, lkeep, info


def fresh(gpu, kw, meta=None, lkeep=None):
    """the fresh handle of the description; terms that came from set_lidar_device are installed that way (their meta)"""
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


def variant(gpu, oracle, cams, name):
    """(live handle, its description, meta) of the source variants the issue names"""
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
    opts = sphere(s["poses"], 6, 3)
    _, _, kw, info = check_window(gpu, a, s, opts, meta=meta)
    assert info["num_images_in"] == 3 and 0 < info["num_points_active"] < a.P and 0 < info["num_obs"] < a.O
    assert info["num_pose_rows"] < info["num_obs"]      # active points keep their rows on outside images
    assert (info["num_lidar"] == 0) == (name == "noterms")
    a.close()


def test_refine_mask_travels_and_commits_camera_parameters(gpu, oracle):
    s = dict(bf.filter_scene(oracle, "two"))
    ref = np.zeros(sum(len(c) for c in s["cam_params_list"]), np.uint8)
    ref[0] = ref[len(s["cam_params_list"][0])] = 1      # the focal length of both cameras
    s["camera_refine"] = ref
    a = gpu.BA(**s)
    opts = sphere(s["poses"], 2, 4)
    w, b, kw, _ = check_window(gpu, a, s, opts, solves=False, keep=True)
    # the camera rows through the Python layer: its tensors are sized from the handle's host mirror of the pose mask,
    # which on a window is the window's (most images constant), not the source's
    ns = int((np.asarray(kw["image_const_pose"]) == 0).sum())
    assert 0 < ns < int((np.asarray(s["image_const_pose"]) == 0).sum())
    cam = []
    for h in (w, b):
        assert h._cam_dims() == (ns, 2) and np.array_equal(h.image_const_pose, kw["image_const_pose"])
        r = h.schur_cam(1e-4, dense=True)
        assert r["S_diag"].shape[0] == ns and r["B"].shape[:2] == (ns, 2) and r["S"].shape == (6 * ns + 24, 6 * ns + 24)
        got = {k: v.cpu().numpy() for k, v in r.items()}
        h.schur_cam(1e-4, want=("cost", "num_skipped"))     # the direct solve reads the handle's own blocks
        delta, ci = h.schur_cam_solve_cholesky()
        assert ci["n"] == 6 * ns + 24 and ci["status"] == gpu.CHOL_OK and delta.shape == (6 * ns + 24,)
        got.update(delta=delta.cpu().numpy(), chol={k: v for k, v in ci.items() if not k.endswith("_ms")})
        cam.append(got)
    bl.assert_same(cam[0], cam[1])
    S = cam[0]["S"]
    assert np.array_equal(S[6 * ns:, :6 * ns], S[:6 * ns, 6 * ns:].T) and S[6 * ns:, 6 * ns:].any()   # the border where it belongs
    assert cam[0]["delta"][6 * ns:].any()
    out = []
    for h in (w, b):
        summary, its = gpu.ba_solve(h, max_num_iterations=3, linear_solver="cholesky", refine_intrinsics=True)
        out.append(dict(summary=no_ms(summary), params=h.get_parameters(), cam=h.get_camera_parameters()))
    bl.assert_same(out[0], out[1])
    assert not lr.same_bits(out[0]["cam"], a.get_camera_parameters()) and out[0]["summary"]["num_accepted"] > 0
    a.commit_window(w)
    assert lr.same_bits(a.get_camera_parameters(), out[0]["cam"]) and lr.same_bits(a.cam_params, out[0]["cam"])
    bl.assert_same(a.get_parameters(), out[0]["params"])
    w.close(); b.close(); a.close()


def hand(gpu, centers, quats=None, radius=5.0, center=0):
    """identity rotations at integer centres (quats: replacements), a point per image pair; the window around image 0"""
    I = len(centers)
    points = [[0.1 * i, 0.2, 10.0 + i] for i in range(I)]
    obs_image = [i for i in range(I)] + [(i + 1) % I for i in range(I)]
    obs_point = list(range(I)) * 2
    s = bf.hand_scene(centers, points, obs_image, obs_point)
    for i, q in (quats or {}).items():
        s["poses"][i, :4] = q
    a = gpu.BA(**s)
    w, b, kw, info = check_window(gpu, a, s, dict(center_image=center, radius=radius), keep=True)
    w.close(); b.close(); a.close()
    return info


def test_equality_is_in_and_the_quaternion_is_not_normalised(gpu):
    centers = [[1, 2, 3], [4, 6, 3], [1, 7, 15], [4, 6, 4], [1, 7, 16]]
    assert list(hand(gpu, centers, radius=5.0)["image_in"].cpu().numpy()) == [1, 1, 0, 0, 0]       # 3-4-5
    assert list(hand(gpu, centers, radius=13.0)["image_in"].cpu().numpy()) == [1, 1, 1, 1, 0]      # 5-12-13
    assert list(hand(gpu, centers, radius=float(np.nextafter(5.0, 0)))["image_in"].cpu().numpy()) == [1, 0, 0, 0, 0]
    assert list(hand(gpu, centers, radius=0.0)["image_in"].cpu().numpy()) == [1, 0, 0, 0, 0]       # the centre image alone
    assert list(hand(gpu, centers, radius=float("inf"))["image_in"].cpu().numpy()) == [1] * 5
    # t = (3, 4, 0) under q = 2 * (0, 0, 0, 1): the stored quaternion gives the centre (21, 28, 0), 35 away; the unit
    # quaternion (3, 4, 0), 5 away
    centers = [[0, 0, 0], [-3, -4, 0], [0, 0, 100]]
    q = {1: [0.0, 0.0, 0.0, 2.0]}
    assert list(hand(gpu, centers, q, radius=5.0)["image_in"].cpu().numpy()) == [1, 0, 0]
    assert list(hand(gpu, centers, q, radius=35.0)["image_in"].cpu().numpy()) == [1, 1, 0]
    assert list(hand(gpu, centers, {1: [0.0, 0.0, 0.0, 1.0]}, radius=5.0)["image_in"].cpu().numpy()) == [1, 1, 0]


def test_a_point_seen_from_inside_and_outside_keeps_every_row(gpu):
    centers = [[0, 0, 0], [1, 0, 0], [50, 0, 0], [51, 0, 0]]
    points = [[0.0, 0.1, 9.0], [0.3, 0.0, 11.0], [50.0, 0.2, 10.0]]
    obs_point = [0, 0, 0, 1, 1, 2, 2]                   # point 0: in, in, out; point 1: in, out; point 2: out, out
    obs_image = [0, 1, 2, 1, 3, 2, 3]
    s = bf.hand_scene(centers, points, obs_image, obs_point)
    a = gpu.BA(**s)
    w, b, kw, info = check_window(gpu, a, s, dict(center_image=0, radius=2.0), keep=True)
    assert list(info["point_active"].cpu().numpy()) == [1, 1, 0]
    assert list(info["obs_map"].cpu().numpy()) == [0, 1, 2, 3, 4, -1, -1]
    blocks = w.evaluate_blocks(True, False)
    assert list(blocks["pose_row"]) == [0, 1, 0xFFFFFFFF, 2, 0xFFFFFFFF] and blocks["num_pose_rows"] == 3
    assert blocks["jac_q"].shape[0] == 3 and blocks["jac_X"].shape[0] == 5      # the outside rows still move the point
    w.close(); b.close(); a.close()


def segment_source(oracle, ndrop):
    """tests/test_ba_filter_gpu.segment_scene (image 0 sees points 0 .. 1029, point p is also seen by images 1 + p % 3 and
    1 + (p + 1) % 3) without the image-1 rows of ndrop points with p % 3 == 2: those are left to images 0 and 3, so a
    window of images {1, 2} drops them and image 0 keeps 1030 - ndrop rows"""
    s = bf.segment_scene(oracle)
    lose = np.flatnonzero(np.arange(1030) % 3 == 2)[::40][:ndrop]
    assert len(lose) == ndrop
    rows = ~((s["obs_image"] == 1) & np.isin(s["obs_point"], lose))
    return dict(s, obs_image=s["obs_image"][rows], obs_point=s["obs_point"][rows], obs_xy=s["obs_xy"][rows]), lose


@pytest.mark.parametrize("ndrop", [6, 4])
def test_image_segments_of_the_window(gpu, oracle, ndrop):
    """image 0 has 1030 observations (two segments of 1024); the window keeps 1024 (one segment) or 1026 (two, the edge
    of the second moved)"""
    src, lose = segment_source(oracle, ndrop)
    iset = np.array([0, 1, 1, 0], np.uint8)
    kw, _, info, _, _, act = wr.fresh_args_window(src, src["poses"], src["points"], dict(image_set=iset))
    assert int((src["obs_image"] == 0).sum()) == 1030 and int((kw["obs_image"] == 0).sum()) == 1030 - ndrop
    assert (1030 - ndrop <= 1024) == (ndrop == 6) and not act[lose].any() and act.sum() == len(act) - ndrop
    a = gpu.BA(**src)
    bf.in_use(gpu, a)
    check_window(gpu, a, src, dict(image_set=iset))
    a.close()


@pytest.mark.parametrize("cams", ["shared", "two"])
def test_tracks_reorder_across_the_slice_edge(gpu, oracle, cams):
    s = bf.filter_scene(oracle, cams)
    P = len(s["points"])
    iset = np.zeros(len(s["poses"]), np.uint8)
    iset[[4] if cams == "shared" else [2]] = 1
    kw, _, info, _, _, act = wr.fresh_args_window(s, s["poses"], s["points"], dict(image_set=iset))
    before, after = np.bincount(s["obs_point"], minlength=P), np.bincount(kw["obs_point"], minlength=P)
    order0, order1 = np.argsort(before, kind="stable"), np.argsort(after, kind="stable")
    assert not np.array_equal(order0, order1) and set(order0[:64]) != set(order1[:64])
    if cams == "two":                                   # a first slice that is all empty tracks
        assert (after[order1[:64]] == 0).all() and after[order1[-1]] > 0
    a = gpu.BA(**s)
    bf.in_use(gpu, a)
    check_window(gpu, a, s, dict(image_set=iset))
    a.close()


def test_every_image_in_no_image_in_and_no_variable_pose(gpu, oracle):
    s = bf.filter_scene(oracle, "shared")
    I = len(s["poses"])
    a = gpu.BA(**s)
    before = bf.all_results(gpu, a, s)
    a.schur(1e-3, want=("cost",))                       # a Schur state from before the derivations
    # radius = +inf: the source's own fresh handle (its mask passed as an array)
    _, _, kw, info = check_window(gpu, a, s, dict(center_image=0, radius=float("inf")))
    seen = np.zeros(a.P, bool); seen[s["obs_point"]] = True
    assert info["num_images_in"] == I and info["num_obs"] == a.O and info["num_points_active"] == int(seen.sum())
    assert np.array_equal(kw["image_const_pose"], s["image_const_pose"])
    # radius = 0: the centre image alone
    _, _, _, info = check_window(gpu, a, s, dict(center_image=4, radius=0.0))
    assert info["num_images_in"] == 1 and list(np.flatnonzero(info["image_in"].cpu().numpy())) == [4]
    # the caller's set equals the sphere given the sphere's flags
    opts = sphere(s["poses"], 7, 4)
    w1, _, _, i1 = derive(gpu, a, s, opts)
    w2, _, _, i2 = derive(gpu, a, s, dict(image_set=i1["image_in"].cpu().numpy()))
    bl.assert_same(bf.all_results(gpu, w1, s), bf.all_results(gpu, w2, s))
    assert np.array_equal(i1["obs_map"].cpu().numpy(), i2["obs_map"].cpu().numpy())
    # two derivations give the same window
    w3, _, _, i3 = derive(gpu, a, s, opts)
    bl.assert_same(bf.all_results(gpu, w1, s), bf.all_results(gpu, w3, s))
    for w in (w1, w2, w3):
        w.close()
    # every "in" image fixed by the caller: no variable pose (evaluate only)
    extra = i1["image_in"].cpu().numpy()
    _, _, _, info = check_window(gpu, a, s, dict(opts, extra_const_pose=extra), solves=False)
    assert info["num_pose_rows"] == 0 and info["num_obs"] > 0
    # no image in: O == 0, L == 0
    _, _, _, info = check_window(gpu, a, s, dict(image_set=np.zeros(I, np.uint8)), solves=False)
    assert (info["num_obs"], info["num_lidar"], info["num_points_active"], info["num_images_in"]) == (0, 0, 0, 0)
    # the source is untouched: its results, and the Schur state made before the derivations still solves
    a.schur_solve_pcg()
    bl.assert_same(bf.all_results(gpu, a, s), before)
    a.close()


def test_257_images(gpu, oracle):
    """more than one workgroup of the per-image kernels (and of their per-workgroup counts): 257 images on a line, two
    observations per point"""
    rng = np.random.default_rng(9)
    I, P = 257, 300
    centers = np.stack([np.arange(I) * 0.5, np.zeros(I), np.zeros(I)], axis=1) + rng.uniform(-0.1, 0.1, (I, 3))
    img = rng.integers(0, I - 1, P)
    img[:2] = [255, 0]
    points = np.stack([centers[img, 0] + 0.2, rng.uniform(-1, 1, P), rng.uniform(6, 12, P)], axis=1)
    s = bf.hand_scene(centers, points, np.concatenate([img, img + 1]), np.concatenate([np.arange(P), np.arange(P)]))
    cpose = np.zeros(I, np.uint8); cpose[[3, 250]] = 1  # one constant pose outside the sphere, one inside
    s["image_const_pose"] = cpose
    a = gpu.BA(**s)
    _, _, _, info = check_window(gpu, a, s, sphere(s["poses"], 256, 9))      # structure and solves included
    inn = info["image_in"].cpu().numpy()
    assert inn[256] == 1 and inn[255] == 1 and inn[:240].sum() == 0 and info["num_images_in"] == 9
    assert info["point_active"].cpu().numpy()[0] == 1
    a.close()


def test_either_handle_outlives_the_other(gpu, oracle):
    s = bf.filter_scene(oracle, "shared")
    opts = sphere(s["poses"], 1, 5)
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
    w, kw, _, info = derive(gpu, a, s, sphere(s["poses"], 12, 8))
    assert 0 < w.O < a.O
    b = gpu.BA(**kw)
    for h in (w, b):
        h.associate_lidar(cloud, max_range=0.5)
    assert w.L > 0
    bl.assert_same(w.get_lidar(), b.get_lidar())
    fw, fb = w.filter_points_device(4.0, 1.5), b.filter_points_device(4.0, 1.5)
    for k in fw:
        assert lr.same_bits(fw[k].cpu().numpy(), fb[k].cpu().numpy()), k
    erase, pdel = bf.random_flags(kw, 31, 0.3, 3)
    iw, ib = w.remove_observations(erase, pdel), b.remove_observations(erase, pdel)
    bl.assert_same(no_ms(iw), no_ms(ib))
    bl.assert_same(w.evaluate(bl.EVERY), b.evaluate(bl.EVERY))
    kept = np.flatnonzero(pdel == 0)[:4]
    add = dict(obs_image=np.array([3, 9, 3, 20], np.int32), obs_point=kept.astype(np.int32),
               obs_xy=np.array([[100.0, 200.0], [300.0, 50.0], [1000.0, 900.0], [2000.0, 1500.0]]))
    iw, ib = w.add_observations(**add), b.add_observations(**add)
    bl.assert_same(no_ms(iw), no_ms(ib))
    desc = dict(kw)
    bl.assert_same(bf.all_results(gpu, w, desc), bf.all_results(gpu, b, desc))
    w.close(); b.close(); a.close(); cloud.close()


def test_commit_carries_the_parameters_back(gpu, oracle):
    s = bf.filter_scene(oracle, "two")
    a = gpu.BA(**s)
    a.schur(1e-3, want=("cost",))
    st0 = a.schur_structure()
    w, kw, _, info = derive(gpu, a, s, sphere(s["poses"], 3, 4))
    summary, _ = gpu.ba_solve(w, max_num_iterations=3, linear_solver="cholesky")
    assert summary["num_accepted"] > 0
    poses, points = w.get_parameters()
    act = info["point_active"].cpu().numpy() != 0
    cp = np.asarray(kw["image_const_pose"]) != 0
    assert lr.same_bits(poses[cp], s["poses"][cp]) and lr.same_bits(points[~act], s["points"][~act])   # why the commit is exact
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


def test_global_round_equals_the_host_route(gpu, oracle):
    s = pr.scene(200)
    xyz, nrm = pr.cloud()
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    opts = dict(max_num_iterations=3, linear_solver="cholesky")
    extra = np.zeros(len(s["poses"]), np.uint8); extra[10] = 1
    # the host route: download, select, a fresh handle, associate, solve, upload
    h = gpu.BA(**s)
    num_h = np.zeros(len(s["points"]), np.int32)
    host = []
    for center in CENTERS:
        poses, points = h.get_parameters()
        o = dict(sphere(poses, center, 7), extra_const_pose=extra)
        kw, _, info, _, _, act = wr.fresh_args_window(s, poses, points, o)
        f = gpu.BA(**kw)
        ainfo = f.associate_lidar(cloud, max_range=gpu.search_range_schedule(num_h), select=act)
        summary, its = gpu.ba_solve(f, **opts)
        h.set_parameters(*f.get_parameters())
        f.close()
        num_h += act.astype(np.int32)
        host.append((o["radius"], info, no_ms(ainfo), no_ms(summary), its))
    # the device route on one live handle
    a = gpu.BA(**s)
    a.schur_build()
    num_d = np.zeros(len(s["points"]), np.int32)
    for center, (radius, info, ainfo, summary, its) in zip(CENTERS, host):
        winfo, dinfo, dsummary, dits = gpu.global_round(a, cloud, center, radius, num_d, extra_const_pose=extra, **opts)
        assert {k: winfo[k] for k in info} == info and info["num_lidar"] == 0
        bl.assert_same(no_ms(dinfo), ainfo)
        assert dinfo["num_terms"] > 0 and dsummary["num_accepted"] > 0
        bl.assert_same(no_ms(dsummary), summary)
        bl.assert_same([no_ms(i) for i in dits], [no_ms(i) for i in its])
    assert np.array_equal(num_d, num_h) and set(num_d.tolist()) == {0, 1, 2}
    bl.assert_same(a.get_parameters(), h.get_parameters())
    assert a.O == len(s["obs_point"]) and a.schur_build()["build_ms"] == 0       # rows and structure of the source stay
    a.close(); h.close(); cloud.close()


def test_refusals(gpu, oracle):
    import torch
    s = bf.filter_scene(oracle, "shared")
    a = gpu.BA(**s)
    full = bf.all_results(gpu, a, s)
    before = a.evaluate(bl.EVERY)
    I = a.I
    iset = np.ones(I, np.uint8)
    bad = [dict(center_image=I), dict(center_image=-2), dict(center_image=None),            # out of range; neither
           dict(center_image=0, image_set=iset),                                            # both
           dict(center_image=0, radius=-1.0), dict(center_image=0, radius=float("nan"))]
    for kw in bad:
        with pytest.raises(gpu.PcdError) as e:
            a.sphere_window(**kw)
        assert e.value.status == gpu.PCD_ERR_INVALID, kw
        bl.assert_same(a.evaluate(bl.EVERY), before)
    other = gpu.BA(**dict(s, points=s["points"][:-1], obs_point=np.minimum(s["obs_point"], a.P - 2),
                          lidar_point=np.minimum(s["lidar_point"], a.P - 2), point_const=s["point_const"][:-1]))
    with pytest.raises(gpu.PcdError) as e:              # a commit between handles of different P
        a.commit_window(other)
    assert e.value.status == gpu.PCD_ERR_INVALID
    bl.assert_same(a.evaluate(bl.EVERY), before)
    bl.assert_same(other.get_parameters(), (s["poses"], s["points"][:-1]))
    w, _ = a.sphere_window(0, float("inf"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            for call in (lambda: a.sphere_window(0, 1.0), lambda: a.commit_window(w)):
                with pytest.raises(gpu.PcdError) as e:
                    call()
                assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
    bl.assert_same(a.evaluate(bl.EVERY), before)
    bl.assert_same(bf.all_results(gpu, a, s), full)     # every result, the solves and the structure included
    w.close(); other.close(); a.close()


def test_shim_global_round(gpu):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_window"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_window"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

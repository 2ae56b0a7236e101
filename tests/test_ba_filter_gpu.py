"""FilterPoints3D on the device (pcd_ba_filter_points) and observations dropped from a live handle
(pcd_ba_remove_observations_device).

The filter is compared with tests/ba_filter_ref.py.  Stage 1 has the bits of filter_tracks on the same handle.  acos differs
between libm and the device library, so before stage 2 is compared the test asserts, on the CPU reference, that every
point's largest pair angle lies at least 1e-9 rad from the threshold (a condition on the inputs: the libraries agree to a
few ulp of an angle of order 0.05); with the same decisions point_delete, obs_erase, point_error and the summary are
equal exactly.

The removal's contract is equality with a FRESH handle built from the compacted description
(ba_filter_ref.fresh_args_after_remove): every result of tests/test_ba_lidar_gpu.results, and schur_structure, get_lidar
and filter_points, bit for bit."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import ba_filter_ref as fr
from tests import ba_lidar_ref as lr
from tests import ba_proj_ref as pr
from tests import ba_schur_ref as sr
from tests import test_ba_lidar_gpu as bl
from tests import test_ba_load_order_gpu as lo

pytestmark = pytest.mark.gpu
MARGIN = 1e-9
WEIGHT = bl.WEIGHT
_CACHE = {}


def perturbed_points(s):
    """half the points moved by N(0, 2 cm): reprojection errors on both sides of 8 px; the scenes' 0.3 m baselines at
    5-12 m give pair angles on both sides of 1.5 and 2.5 degrees"""
    rng = np.random.default_rng(1)
    P = len(s["points"])
    return s["points"] + rng.normal(0, 0.02, (P, 3)) * (rng.random((P, 1)) < 0.5)


def filter_scene(oracle, cams):
    if cams not in _CACHE:
        s, many = bl.scene(oracle, cams)
        s = dict(s, **many)
        _CACHE[cams] = dict(s, points=perturbed_points(s))
    return _CACHE[cams]


def summary_keys(d):
    return {k: d[k] for k in ("num_filtered", "mean_reproj_error", "num_points_with_error", "num_negative_depth")}


# ---- the filter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cams", ["shared", "two"])
@pytest.mark.parametrize("min_angle", [1.5, 2.5])
def test_filter_points_equals_the_reference(gpu, oracle, cams, min_angle):
    s = filter_scene(oracle, cams)
    ba = gpu.BA(**s)
    sq, depth = ba.observation_errors()
    ref = fr.filter_points(sq, depth, s["obs_image"], s["obs_point"], s["poses"], s["points"], 8.0, min_angle)
    ran = ref["max_angle"] >= 0
    assert ran.sum() > 20 and (np.abs(ref["max_angle"][ran] - min_angle * fr.DEG) >= MARGIN).all()    # no point left out
    stage1 = ba.filter_tracks(8.0)
    got0 = ba.filter_points(8.0, 0.0)                   # <= 0: stage 1 alone, bit for bit
    bl.assert_same(got0, stage1)
    bl.assert_same(ba.filter_points(8.0, -1.0), stage1)
    got = ba.filter_points(8.0, min_angle)
    # both stages fire, on points and on single elements
    two = (got["point_delete"] == 1) & (stage1["point_delete"] == 0)
    assert two.sum() >= 1 and stage1["point_delete"].sum() >= 1 and (stage1["point_delete"] == 0).sum() > two.sum()
    assert (stage1["obs_erase"][~np.isin(s["obs_point"], np.flatnonzero(stage1["point_delete"]))] == 1).any()
    assert got["num_filtered"] == stage1["num_filtered"] + int(two.sum())
    assert lr.same_bits(got["obs_negative_depth"], stage1["obs_negative_depth"])
    assert got["num_negative_depth"] == stage1["num_negative_depth"]
    for k in ("obs_erase", "point_delete", "point_error", "obs_negative_depth"):
        assert lr.same_bits(got[k], ref[k]), k
    bl.assert_same(summary_keys(got), summary_keys(ref))
    bl.assert_same(ba.filter_points(8.0, min_angle), got)          # a repeated call
    # the device form with only the summary asked for: the per-track outputs live in the handle's scratch
    import torch
    sm = torch.empty(4, dtype=torch.float64, device="cuda")
    ba.filter_points_device(8.0, min_angle, out=dict(summary=sm))
    d = ba.filter_points_device(8.0, min_angle)
    torch.cuda.synchronize()
    assert lr.same_bits(sm.cpu().numpy(), d["summary"].cpu().numpy())
    assert int(sm[0]) == got["num_filtered"] and float(sm[1]) == got["mean_reproj_error"]
    assert lr.same_bits(d["obs_erase"].cpu().numpy(), got["obs_erase"])
    ba.close()


def hand_scene(centers, points, obs_image, obs_point, bad=()):
    """identity rotations at the given centres, one camera, exact observations; those in `bad` moved by 100 px"""
    I = len(centers)
    poses = np.array([[1.0, 0, 0, 0, -c[0], -c[1], -c[2]] for c in centers], np.float64)
    s = dict(cam_model=np.array([0], np.int32), cam_params_list=[np.array([1000.0, 500.0, 400.0])], poses=poses,
             image_camera=np.zeros(I, np.int32), points=np.asarray(points, np.float64),
             obs_image=np.asarray(obs_image, np.int32), obs_point=np.asarray(obs_point, np.int32))
    X = s["points"][s["obs_point"]] - np.asarray(centers, np.float64)[s["obs_image"]]
    z = np.where(X[:, 2] == 0, 1.0, X[:, 2])            # a point on a centre has no projection: any observation will do
    xy = np.stack([1000.0 * X[:, 0] / z + 500.0, 1000.0 * X[:, 1] / z + 400.0], axis=1)
    xy[list(bad)] += 100.0
    s["obs_xy"] = xy
    return s


def test_hand_cases_on_the_device(gpu):
    h = 10.0
    b_hi, b_lo = (h * math.tan(math.radians(1.5 + 1e-6) / 2), h * math.tan(math.radians(1.5 - 1e-6) / 2))
    centers = [[b_hi, 0, 0], [-b_hi, 0, 0], [b_lo, 1, 0], [-b_lo, 1, 0],      # 0-1 above, 2-3 below the threshold
               [0, 0, 0], [0.01, 0, 0], [5.0, 0, 0],                          # 4-5 close together, 6 far away
               [0.3, 0.1, 4.0]]                                               # 7: point 5 sits on it
    points = [[0, 0, h], [0, 1, h], [0, 0, h], [0, 0, h], [0.7, 0.2, 9.0], [0.3, 0.1, 4.0]]
    #          p0 kept   p1 deleted  p2: survivors 4, 5 only   p3: 4, 5, 6 kept   p4: image 4 twice   p5: on centre 7
    obs_point = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5]
    obs_image = [0, 1, 2, 3, 4, 5, 6, 4, 5, 6, 4, 4, 7, 6]
    s = hand_scene(centers, points, obs_image, obs_point, bad=(6,))
    ba = gpu.BA(**s)
    sq, depth = ba.observation_errors()
    assert sq[6] > 64 and (np.delete(sq, [6, 12]) < 1e-12).all()               # observation 12: depth 0, DBL_MAX
    got = ba.filter_points(8.0, 1.5)
    ref = fr.filter_points(sq, depth, s["obs_image"], s["obs_point"], s["poses"], s["points"], 8.0, 1.5)
    assert list(got["point_delete"]) == [0, 1, 1, 0, 1, 1] == list(ref["point_delete"])
    assert list(got["obs_erase"]) == [0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    # elements in stage 1: observation 6, and both of point 5 (one behind the camera: at most one survives); one per
    # point in stage 2: points 1, 2, 4
    assert got["num_filtered"] == 1 + 2 + 3 == ref["num_filtered"]
    assert got["num_points_with_error"] == 2 and got["num_negative_depth"] == 1
    assert list(got["point_error"] >= 0) == [True, False, False, True, False, False]
    stage1 = ba.filter_points(8.0, 0.0)
    bl.assert_same(stage1, ba.filter_tracks(8.0))
    assert list(stage1["point_delete"]) == [0, 0, 0, 0, 0, 1] and stage1["num_filtered"] == 3
    ba.close()


# ---- the removal ----------------------------------------------------------------------------------------------------
def all_results(gpu, ba, s, solves=True):
    out = bl.results(gpu, ba, s) if solves else dict(
        evaluate=ba.evaluate(bl.EVERY), cost_only=ba.evaluate(("cost",)), filter=ba.filter_tracks(4.0))
    out.update(structure=ba.schur_structure() if solves else None, lidar=ba.get_lidar(), points_filter=ba.filter_points(4.0, 2.5))
    return out


def check_removed(gpu, a, desc, erase, pdel, meta=None, solves=True):
    """remove on the live handle `a` (whose description is `desc`, its set_lidar_device rows' meta in `meta`), build the
    fresh handle, compare everything; returns (fresh description, fresh meta, obs_map)"""
    kw, obs_map, info_ref, lkeep = fr.fresh_args_after_remove(desc, erase, pdel)
    info = a.remove_observations(erase, pdel, want_map=True)
    assert {k: info[k] for k in info_ref} == info_ref
    assert (a.O, a.L) == (info_ref["num_obs"], info_ref["num_lidar"])
    assert np.array_equal(info["obs_map"].cpu().numpy().view(np.uint32), obs_map)
    new_meta = None
    if meta is not None:                                # terms that came from set_lidar_device keep type / lidar_xyz
        new_meta = {k: v[lkeep] for k, v in meta.items()}
        b = gpu.BA(**{k: v for k, v in kw.items() if not k.startswith("lidar_")})
        b.set_lidar_device(new_meta["type"], kw.get("lidar_abcd", np.zeros((0, 4))), WEIGHT,
                           point=kw.get("lidar_point", np.zeros(0, np.int32)), lidar_xyz=new_meta["lidar_xyz"])
        t = a.get_lidar()
        assert lr.same_bits(t["type"], new_meta["type"]) and lr.same_bits(t["lidar_xyz"], new_meta["lidar_xyz"])
    else:
        b = gpu.BA(**kw)
    bl.assert_same(all_results(gpu, a, kw, solves), all_results(gpu, b, kw, solves))
    b.close()
    return kw, new_meta, obs_map


def in_use(gpu, a):
    a.evaluate(("cost", "H_pt"))
    a.evaluate_blocks(True, False)                      # h_pose_row and vobs of the handle as it is
    a.schur(1e-3, want=("cost",))


def random_flags(s, seed, frac, npoints):
    rng = np.random.default_rng(seed)
    erase = (rng.random(len(s["obs_point"])) < frac).astype(np.uint8)
    pdel = np.zeros(len(s["points"]), np.uint8)
    pdel[rng.choice(len(s["points"]), npoints, replace=False)] = 1
    return erase, pdel


def test_nothing_flagged_changes_nothing(gpu, oracle):
    s = filter_scene(oracle, "shared")
    a = gpu.BA(**s)
    before = all_results(gpu, a, s)
    a.schur(1e-3, want=("cost",))
    L0, ptrs = a.lidar_device()
    info = a.remove_observations()                      # both pointers NULL
    assert (info["num_obs"], info["num_obs_removed"], info["num_lidar"], info["num_lidar_removed"]) == (a.O, 0, a.L, 0)
    assert a.lidar_device() == (L0, ptrs)
    a.schur_solve_pcg()                                 # the Schur state is still there
    bl.assert_same(all_results(gpu, a, s), before)
    # flags that are all zero go through the rebuild and give the same handle
    check_removed(gpu, a, s, np.zeros(a.O, np.uint8), np.zeros(a.P, np.uint8))
    a.close()


@pytest.mark.parametrize("cams", ["shared", "two"])
def test_random_removal_equals_a_fresh_handle(gpu, oracle, cams):
    s = filter_scene(oracle, cams)
    P = len(s["points"])
    erase, pdel = random_flags(s, 11, 0.3, 4)
    if cams == "two":                                   # every second point loses its whole track: 65 empty tracks
        erase[s["obs_point"] % 2 == 0] = 1
    kw, _, _, _ = fr.fresh_args_after_remove(s, erase, pdel)
    before, after = np.bincount(s["obs_point"], minlength=P), np.bincount(kw["obs_point"], minlength=P)
    order0, order1 = np.argsort(before, kind="stable"), np.argsort(after, kind="stable")
    # lengths tie and the tracks reorder across the 64-track slice edge; with two cameras the first slice is all padding
    assert not np.array_equal(order0, order1) and set(order0[:64]) != set(order1[:64])
    assert len(set(after.tolist())) < P and 0.2 < 1 - after.sum() / before.sum()
    if cams == "two":
        assert (after[order1[:64]] == 0).all() and after[order1[64]] == 0 and after[order1[128]] > 0
    a = gpu.BA(**s)
    in_use(gpu, a)
    check_removed(gpu, a, s, erase, pdel)
    a.schur(1e-3, want=("cost",))
    a.remove_observations(np.zeros(a.O, np.uint8))      # any call with flags drops the Schur state and the structure
    with pytest.raises(gpu.PcdError) as e:
        a.schur_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    a.close()


def segment_scene(oracle):
    """image 0 sees points 0 .. 1029 (1030 observations: two segments of kImgSeg = 1024), images 1-3 see every point
    twice; observations shuffled"""
    if "seg" not in _CACHE:
        rng = np.random.default_rng(77)
        P = 1100
        s = lo._base(rng, 4, P, (4,))
        p = np.arange(P)
        obs_point = np.concatenate([np.arange(1030), p, p])
        obs_image = np.concatenate([np.zeros(1030, np.int64), 1 + p % 3, 1 + (p + 1) % 3])
        perm = rng.permutation(len(obs_point))
        s.update(obs_image=obs_image[perm].astype(np.int32), obs_point=obs_point[perm].astype(np.int32))
        cpose = np.zeros(4, np.uint8); cpose[2] = 1
        s.update(image_const_pose=cpose)
        _CACHE["seg"] = sr.reproject(oracle, s, rng)
    return _CACHE["seg"]


@pytest.mark.parametrize("ndrop,which", [(10, "spread"), (5, "head"), (4, "tail")])
def test_image_segments_after_a_removal(gpu, oracle, ndrop, which):
    s = segment_scene(oracle)
    of0 = np.flatnonzero(s["obs_image"] == 0)
    assert len(of0) == 1030
    pick = {"spread": of0[::103][:ndrop], "head": of0[:ndrop], "tail": of0[-ndrop:]}[which]
    erase = np.zeros(len(s["obs_image"]), np.uint8)
    erase[pick] = 1
    assert (1030 - ndrop <= 1024) == (ndrop == 10)      # two segments become one / stay two with the boundary moved
    a = gpu.BA(**s)
    in_use(gpu, a)
    check_removed(gpu, a, s, erase, None)
    a.close()


def test_an_image_without_observations_and_a_handle_without(gpu, oracle):
    s = filter_scene(oracle, "two")
    a = gpu.BA(**s)
    in_use(gpu, a)
    erase = (s["obs_image"] == 4).astype(np.uint8)      # a middle image loses its segment
    kw, _, _ = check_removed(gpu, a, s, erase, None)
    assert not (kw["obs_image"] == 4).any()
    check_removed(gpu, a, kw, np.ones(a.O, np.uint8), None, solves=False)       # O = 0: only LiDAR residuals are left
    assert a.O == 0 and a.L == len(s["lidar_point"])
    got = a.evaluate(("cost", "residuals"))
    assert got["residuals"].shape == (a.L,) and got["cost"][0] > 0
    a.close()


@pytest.mark.parametrize("source", ["set_lidar_device", "create"])
def test_point_delete_drops_the_terms_of_the_point(gpu, oracle, source):
    s0, many = bl.scene(oracle, "shared")
    P = len(s0["points"])
    meta = None
    if source == "create":
        s = dict(s0, **many)
        a = gpu.BA(**s)
    else:
        point, typ, abcd, xyz = bl.make_rows(s0, 200, "shuffled", 5, False)
        y = lr.terms(typ, abcd, WEIGHT, point, xyz)
        s = dict(s0, lidar_point=y["lidar_point"], lidar_abcd=y["lidar_abcd"], lidar_weight=y["lidar_weight"])
        meta = dict(type=y["type"], lidar_xyz=y["lidar_xyz"])
        a = gpu.BA(**s0)
        a.set_lidar_device(typ, abcd, WEIGHT, point=point, lidar_xyz=xyz)
    per = np.bincount(s["lidar_point"], minlength=P)
    pdel = np.zeros(P, np.uint8)
    for n in (0, 1, 3):                                 # two points of each kind, and the last point
        pdel[np.flatnonzero(per == n)[:2]] = 1
    pdel[P - 1] = 1
    assert {0, 1, 3} <= set(per[pdel == 1].tolist()) and {0, 1, 3} <= set(per[pdel == 0].tolist())
    in_use(gpu, a)
    L0, _ = a.lidar_device()
    kw, _, _ = check_removed(gpu, a, s, None, pdel, meta=meta)
    assert a.L == L0 - int(per[pdel == 1].sum()) > 0
    a.close()


def test_two_removals_equal_one_of_the_union(gpu, oracle):
    s = filter_scene(oracle, "two")
    e1, p1 = random_flags(s, 21, 0.15, 3)
    a = gpu.BA(**s)
    in_use(gpu, a)
    kw1, _, map1 = check_removed(gpu, a, s, e1, p1)
    e2, p2 = random_flags(kw1, 22, 0.15, 3)
    in_use(gpu, a)
    kw2, _, _ = check_removed(gpu, a, kw1, e2, p2)      # the swapped buffers of the first call are the second's scratch
    union = e1.copy()
    kept = map1 != fr.DROPPED
    union[kept] |= e2[map1[kept]]
    c = gpu.BA(**s)
    c.remove_observations(union, p1 | p2)
    bl.assert_same(all_results(gpu, c, kw2), all_results(gpu, a, kw2))
    a.close(); c.close()


def test_follow_up_calls_on_the_edited_handle(gpu, oracle):
    s = pr.scene(65)
    xyz, nrm = pr.cloud()
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    pj = gpu.Projector(cloud)
    erase, pdel = random_flags(s, 31, 0.3, 3)
    kw, _, _, _ = fr.fresh_args_after_remove(s, erase, pdel)
    a, b = gpu.BA(**s), gpu.BA(**kw)
    a.remove_observations(erase, pdel)
    size = (pr.WIDTH, pr.HEIGHT)
    ia, ib = a.project_lidar(pj, size), b.project_lidar(pj, size)              # reads h_img_obs_start
    assert ia["num_terms"] > 0 and ia["num_features"] == a.O
    bl.assert_same({k: v for k, v in ia.items() if not k.endswith("_ms")}, {k: v for k, v in ib.items() if not k.endswith("_ms")})
    bl.assert_same(a.get_lidar(), b.get_lidar())
    ia, ib = a.associate_lidar(cloud, max_range=0.5), b.associate_lidar(cloud, max_range=0.5)
    bl.assert_same({k: v for k, v in ia.items() if not k.endswith("_ms")}, {k: v for k, v in ib.items() if not k.endswith("_ms")})
    bl.assert_same(a.get_lidar(), b.get_lidar())
    bl.assert_same(a.evaluate(bl.EVERY), b.evaluate(bl.EVERY))
    a.close(); b.close(); pj.close(); cloud.close()


def test_refusals(gpu, oracle):
    import ctypes as C
    import torch
    assert gpu.lib().pcd_ba_remove_observations_device(None, None, None, None, None, None) == gpu.PCD_ERR_INVALID
    s = filter_scene(oracle, "shared")
    ba = gpu.BA(**s)
    before = ba.evaluate(bl.EVERY)
    erase = torch.ones(ba.O, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            for call in (lambda: ba.remove_observations(erase), lambda: ba.filter_points_device(8.0, 1.5, out={})):
                with pytest.raises(gpu.PcdError) as e:
                    call()
                assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
    assert ba.O == len(s["obs_point"])
    bl.assert_same(ba.evaluate(bl.EVERY), before)
    ba.close()
    assert C.sizeof(gpu.BAFilterOpts) == 48 and C.sizeof(gpu.BARemoveInfo) == 48


# ---- the loop -------------------------------------------------------------------------------------------------------
def test_refine_filter_equals_a_new_handle_per_round(gpu, oracle):
    s = filter_scene(oracle, "two")
    opts = dict(max_num_iterations=4, linear_solver="cholesky")
    desc, manual = dict(s), []
    for _ in range(8):
        h = gpu.BA(**desc)
        num_obs = h.O
        summary, _its = gpu.ba_solve(h, **opts)
        f = h.filter_points(8.0, 1.5)
        poses, points = h.get_parameters()
        h.close()
        desc, _, info, _ = fr.fresh_args_after_remove(dict(desc, poses=poses, points=points), f["obs_erase"], f["point_delete"])
        manual.append((summary, f, info))
        if f["num_filtered"] / num_obs < 0.0005:
            break
    ba = gpu.BA(**s)
    rounds = gpu.refine_filter(ba, max_refinements=8, **opts)
    assert len(rounds) == len(manual) <= 8 and rounds[-1][1]["changed"] < 0.0005         # ended by the change rule
    assert rounds[0][2]["num_obs_removed"] > 0 and rounds[0][1]["changed"] >= 0.0005
    for (sm, fl, info), (msm, mf, minfo) in zip(rounds, manual):
        bl.assert_same({k: v for k, v in sm.items() if not k.endswith("_ms")}, {k: v for k, v in msm.items() if not k.endswith("_ms")})
        bl.assert_same(summary_keys(fl), summary_keys(mf))
        assert {k: info[k] for k in minfo} == minfo
    poses, points = ba.get_parameters()
    assert lr.same_bits(poses, desc["poses"]) and lr.same_bits(points, desc["points"])
    assert ba.O == len(desc["obs_point"])
    # the flags of the last round on the live handle are those of a fresh handle at the same parameters
    h = gpu.BA(**desc)
    bl.assert_same(ba.filter_points(8.0, 1.5), h.filter_points(8.0, 1.5))
    h.close(); ba.close()


def test_shim_filter_points(gpu):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_filter"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_filter"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

"""Depth-projection (Proj) terms installed on a live BA handle (pcd_proj_set_new_images_device,
pcd_ba_project_lidar_device).

Expected values come from the host route that exists without the call: BA.get_parameters -> Projector.set_new_images
(host buffers) -> the numpy selection of tests/ba_proj_ref.py -> Cloud.associate for the nearest-neighbour points -> the
term rule of tests/ba_lidar_ref.py -> a FRESH handle.  Equality is on bit patterns throughout (ba_lidar_ref.same_bits;
results / assert_same of tests/test_ba_lidar_gpu.py).

Scene: tests/ba_proj_ref.scene at P = 130 and P = 65 (three and two 64-track slices) over synth.cloud_planes(400_000,
seed=5); tests/test_ba_proj_cpu.py shows that its picks have several candidates and winners that are not the first."""
import os
import subprocess

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_lidar_ref as lr
from tests import ba_proj_ref as pr
from tests import test_ba_lidar_gpu as bl

pytestmark = pytest.mark.gpu
SIZE = (pr.WIDTH, pr.HEIGHT)
WEIGHT = [0.0, 70.0, 900.0, 3.0]
KW = dict(proj_weight=3.0, icp_weight=70.0, icp_ground_weight=900.0)
GATE_LOCAL = 0    # PCD_GATE_MAPPER_LOCAL


@pytest.fixture(scope="module")
def world(gpu):
    xyz, nrm = pr.cloud()
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    pj = gpu.Projector(cloud)
    yield cloud, pj
    pj.close()
    cloud.close()


def host_route(cloud, pj, s, poses, points, image_select=None, point_mode=None, max_range=None, gate=0, weight=WEIGHT):
    """the term list of the host route at (poses, points), and what the projector found on the way"""
    images, feat, feat_obs = pr.proj_inputs(s, poses, image_select)
    if images:
        found, index, _, l6, _ = pj.set_new_images(images, feat)
    else:
        found, index, l6 = np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros((0, 6))
    pairs = pj.last_pairs if images else 0
    proj = pr.proj_rows(s, points, feat_obs, found, l6, point_mode)
    assoc = cloud.associate(points, max_range, gate) if point_mode is not None else None
    typ, abcd, xyz = pr.merge_rows(proj, assoc, point_mode)
    y = lr.terms(typ, abcd, weight, None, xyz)
    return y, dict(found=found, index=index, l6=l6, feat_obs=feat_obs, n_images=len(images), pairs=pairs)


def assert_terms(ba, y):
    t = ba.get_lidar()
    for k, ky in (("point", "lidar_point"), ("abcd", "lidar_abcd"), ("weight", "lidar_weight"), ("type", "type"),
                  ("lidar_xyz", "lidar_xyz")):
        assert lr.same_bits(t[k], y[ky]), k
    assert ba.L == len(y["rows"])


# ---- 1. the device form of the projector ----------------------------------------------------------------------------
def test_set_new_images_device_equals_the_host_form(gpu, world):
    import torch
    _, pj = world
    images, feat = synth.proj_scene(6, 300, seed=2)
    inside = (feat[:, 0] >= 0) & (feat[:, 0] < 4032) & (feat[:, 1] >= 0) & (feat[:, 1] < 3024)
    assert 0 < (~inside).sum() < len(feat)                      # out-of-image features ride along
    exp = pj.set_new_images(images, feat)
    exp_pairs = pj.last_pairs
    assert 0 < exp[0].sum() < len(feat)
    d_feat = torch.from_numpy(feat).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = pj.set_new_images_device(images, d_feat, stream=side.cuda_stream)
        only = pj.set_new_images_device(images, d_feat, want=("lidar6",), stream=side.cuda_stream)   # NULL outputs
    assert pj.last_pairs == exp_pairs
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert lr.same_bits(got["found"], exp[0]) and lr.same_bits(got["lidar_index"].view(np.uint32), exp[1])
    assert lr.same_bits(got["dist"], exp[2]) and lr.same_bits(got["lidar6"], exp[3]) and lr.same_bits(got["cam_xyz"], exp[4])
    assert list(only) == ["lidar6"] and lr.same_bits(only["lidar6"].cpu().numpy(), exp[3])
    g = torch.cuda.CUDAGraph()                                   # a capturing stream is refused
    with torch.cuda.stream(side):
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                pj.set_new_images_device(images, d_feat, stream=side.cuda_stream)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
    bad = [dict(im) for im in images]
    bad[2]["params"] = [0.0] + list(images[2]["params"][1:])
    with pytest.raises(gpu.PcdError) as e:
        pj.set_new_images_device(bad, d_feat)
    assert e.value.status == gpu.PCD_ERR_INVALID


# ---- 2. project_lidar against a fresh handle ------------------------------------------------------------------------
def case_args(which, s):
    P, I = len(s["points"]), len(s["poses"])
    if which == "all_proj":
        return dict()
    if which == "mixed":
        mr = np.where(np.arange(P) % 2 == 0, 0.03, 0.5)        # a per-point range: some mode-2 points are rejected
        return dict(point_mode=(np.arange(P) % 3).astype(np.uint8), max_range=mr, gate=GATE_LOCAL)
    if which == "third_image_off":
        return dict(image_select=(np.arange(I) % 3 != 2).astype(np.uint8))
    return dict(image_select=np.zeros(I, np.uint8))


@pytest.mark.parametrize("which,P", [("all_proj", 130), ("mixed", 130), ("third_image_off", 65), ("no_image", 65)])
def test_project_lidar_equals_a_fresh_handle(gpu, world, which, P):
    cloud, pj = world
    assert gpu.GATE_MAPPER_LOCAL == GATE_LOCAL
    s = pr.scene(P)
    a = case_args(which, s)
    y, seen = host_route(cloud, pj, s, s["poses"], s["points"], a.get("image_select"), a.get("point_mode"),
                         a.get("max_range"), a.get("gate", 0))
    ba = gpu.BA(**s)
    ba.evaluate(("cost", "H_pt"))                      # a handle in use
    ba.schur(1e-3, want=("cost",))
    info = ba.project_lidar(pj, SIZE, image_select=a.get("image_select"), point_mode=a.get("point_mode"),
                            max_range=a.get("max_range"), gate_mode=a.get("gate", 0), **KW)
    with pytest.raises(gpu.PcdError) as e:             # the same invalidation as set_lidar_device
        ba.schur_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    n = {t: int((y["type"] == t).sum()) for t in (1, 2, 3)}
    assert (info["num_terms"], info["num_icp"], info["num_icp_ground"], info["num_proj"]) == (len(y["rows"]), n[1], n[2], n[3])
    assert info["num_images"] == seen["n_images"] and info["num_features"] == len(seen["found"])
    assert info["num_found"] == int(seen["found"].sum()) and info["pairs"] == seen["pairs"] == pj.last_pairs
    if which == "all_proj":
        assert n[3] > 100 and n[1] == n[2] == 0
    elif which == "mixed":
        mode = a["point_mode"]
        assert n[3] > 20 and 0 < n[1] + n[2] < int((mode == 2).sum())
        assert not np.isin(y["lidar_point"], np.flatnonzero(mode == 0)).any()
    elif which == "third_image_off":
        full, _ = host_route(cloud, pj, s, s["poses"], s["points"])
        assert 0 < n[3] and not lr.same_bits(full["lidar_abcd"], y["lidar_abcd"])     # the selection changes the terms
    else:
        assert info["num_terms"] == 0 and info["num_images"] == 0
    assert_terms(ba, y)
    fresh = bl.handle(gpu, s, y)
    bl.assert_same(bl.results(gpu, ba, s), bl.results(gpu, fresh, s))
    ba.close(); fresh.close()


# ---- 3. the records follow the moved poses --------------------------------------------------------------------------
def test_project_lidar_after_a_solve_uses_the_current_poses(gpu, world):
    cloud, pj = world
    s = pr.scene(130)
    # start a decimetre off the poses the observations were made with, so that two LM iterations move the cameras by more
    # than a pixel of the depth image (5 full-resolution pixels) and the features find other winners
    poses0 = s["poses"].copy()
    poses0[:, 4:] += np.random.default_rng(1).normal(0, 0.1, (len(poses0), 3))
    s = dict(s, poses=poses0)
    ba = gpu.BA(**s)
    ba.project_lidar(pj, SIZE, **KW)
    first = ba.get_lidar()
    summary, _ = gpu.ba_solve(ba, max_num_iterations=2, linear_solver="cholesky")
    assert summary["num_accepted"] >= 1
    poses, points = ba.get_parameters()
    assert not lr.same_bits(poses, s["poses"]) and not lr.same_bits(points, s["points"])
    y, _ = host_route(cloud, pj, s, poses, points)
    y0, _ = host_route(cloud, pj, s, s["poses"], s["points"])
    assert not lr.same_bits(y["lidar_abcd"], y0["lidar_abcd"])           # the move changes the expected terms
    info = ba.project_lidar(pj, SIZE, **KW)
    assert info["num_terms"] == len(y["rows"])
    assert_terms(ba, y)
    assert not lr.same_bits(ba.get_lidar()["abcd"], first["abcd"])
    s2 = dict(s, poses=poses, points=points)
    fresh = bl.handle(gpu, s2, y)
    bl.assert_same(bl.results(gpu, ba, s2), bl.results(gpu, fresh, s2))
    ba.close(); fresh.close()


# ---- 4. edges in one hand-made scene --------------------------------------------------------------------------------
def edge_world():
    """six isolated cloud rows 10 m in front of three cameras (0 and 2 at the origin, 1 half a metre to the side): A, B,
    C with normals, Z with a zero normal, far from everything else of the cloud"""
    rows = np.array([[-2.0, 0.0, 10.0], [0.0, 0.0, 10.0], [2.0, 0.0, 10.0], [4.0, 0.0, 10.0]], np.float32)   # A B C Z
    nrm = np.array([[0.0, 0.0, -1.0], [0.6, 0.0, -0.8], [0.0, 0.6, -0.8], [0.0, 0.0, 0.0]], np.float32)
    fx, fn = synth.cloud_planes(2000, seed=3)
    xyz = np.concatenate([rows, fx + np.float32([0, 200, 0])]).astype(np.float32)
    nrm = np.concatenate([nrm, fn]).astype(np.float32)
    poses = np.array([[1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, -0.5, 0, 0], [1, 0, 0, 0, 0, 0, 0]], np.float64)
    A, B, C_, Z = range(4)

    def px(img, row):
        pc = rows[row].astype(np.float64) + poses[img, 4:]
        return list(synth._opencv_project(synth.OPENCV_PARAMS, pc[0] / pc[2], pc[1] / pc[2]))

    # (point, image, the row its pixel shows)
    obs = [(0, 0, A), (0, 0, B), (0, 1, C_),       # point 0: a second observation in image 0, which must not count
           (1, 0, Z), (1, 1, A),                   # point 1: a zero normal beside a valid candidate
           (2, 0, Z), (2, 1, Z),                   # point 2: zero normals alone
           (3, 0, A),                              # point 3: ON its candidate (vn = 0)
           (4, 2, B), (4, 2, C_)]                  # point 4: seen only by image 2, which is not selected
    points = np.array([[-1.9, 0.3, 9.0],           # |cos| to A, B, C: 0.95, 0.16, 0.24
                       [-1.5, 0.2, 9.5], [3.5, 0.1, 9.5], rows[A].astype(np.float64), [1.0, 0.0, 9.5]])
    s = dict(cam_model=np.array([4], np.int32), cam_params_list=[list(synth.OPENCV_PARAMS)], poses=poses,
             image_camera=np.zeros(3, np.int32), points=points, obs_image=np.array([o[1] for o in obs], np.int32),
             obs_point=np.array([o[0] for o in obs], np.int32), obs_xy=np.array([px(o[1], o[2]) for o in obs]))
    return xyz, nrm, s, np.array([o[2] for o in obs])


def test_project_lidar_edges(gpu):
    xyz, nrm, s, want_row = edge_world()
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    pj = gpu.Projector(cloud)
    select = np.array([1, 1, 0], np.uint8)
    y, seen = host_route(cloud, pj, s, s["poses"], s["points"], image_select=select)
    # the scene is what its comments say: every feature of the two selected images shows its row
    assert seen["found"].all() and np.array_equal(seen["index"], want_row[seen["feat_obs"]])
    l6 = np.zeros((len(want_row), 6)); l6[seen["feat_obs"]] = seen["l6"]
    X0 = s["points"][0]
    assert pr.pick(X0, [l6[0], l6[1], l6[2]])[0] == 1          # the duplicate WOULD win ...
    assert pr.pick(X0, [l6[0], l6[2]])[0] == 1                 # ... without it the pick is row C in image 1
    assert y["lidar_point"].tolist() == [0, 1]                 # points 2, 3, 4 get no term
    assert lr.same_bits(y["lidar_xyz"][0], xyz[2].astype(np.float64)) and lr.same_bits(y["lidar_xyz"][1], xyz[0].astype(np.float64))
    ba = gpu.BA(**s)
    info = ba.project_lidar(pj, SIZE, image_select=select, **KW)
    assert (info["num_terms"], info["num_proj"], info["num_images"], info["num_features"]) == (2, 2, 2, 8)
    assert_terms(ba, y)
    fresh = bl.handle(gpu, s, y)
    bl.assert_same(bl.results(gpu, ba, s), bl.results(gpu, fresh, s))
    # with image 2 selected as well, point 4 gets a term
    y3, _ = host_route(cloud, pj, s, s["poses"], s["points"])
    assert y3["lidar_point"].tolist() == [0, 1, 4]
    ba.project_lidar(pj, SIZE, **KW)
    assert_terms(ba, y3)
    ba.close(); fresh.close(); pj.close(); cloud.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_untouched(gpu, world):
    import torch
    cloud, pj = world
    s = pr.scene(65)
    P = len(s["points"])
    ba = gpu.BA(**s)
    ba.project_lidar(pj, SIZE, **KW)
    before = ba.get_lidar()
    assert len(before["point"]) > 30
    mode3 = np.ones(P, np.uint8); mode3[40] = 3
    calls = [lambda: ba.project_lidar(pj, SIZE, point_mode=mode3, max_range=0.3, **KW),
             lambda: ba.project_lidar(pj, None, **KW)]                       # no size arrays
    for call in calls:
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_INVALID, str(e.value)
        bl.assert_same(ba.get_lidar(), before)
    params = np.array(s["cam_params_list"][0], np.float64)
    zero_f = params.copy(); zero_f[1] = 0.0
    ba.set_camera_parameters(zero_f)
    with pytest.raises(gpu.PcdError) as e:
        ba.project_lidar(pj, SIZE, **KW)
    assert e.value.status == gpu.PCD_ERR_INVALID and "focal" in str(e.value)
    ba.set_camera_parameters(params)
    bl.assert_same(ba.get_lidar(), before)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                ba.project_lidar(pj, SIZE, **KW)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
    bl.assert_same(ba.get_lidar(), before)
    # the handle still solves, as a fresh one with these terms does
    y = dict(lidar_point=before["point"], lidar_abcd=before["abcd"], lidar_weight=before["weight"])
    fresh = bl.handle(gpu, s, y)
    bl.assert_same(bl.results(gpu, ba, s), bl.results(gpu, fresh, s))
    ba.close(); fresh.close()


# ---- 6. repeatability -----------------------------------------------------------------------------------------------
def test_two_identical_calls_give_identical_handles(gpu, world):
    cloud, shared = world
    s = pr.scene(130)
    P = len(s["points"])
    pj = gpu.Projector(cloud)                          # not latched yet: the call latches on the camera of image 0
    assert not pj.scale_coeffs()[1]
    mode = ((np.arange(P) + 1) % 3).astype(np.uint8)
    ba = gpu.BA(**s)
    i1 = ba.project_lidar(pj, SIZE, point_mode=mode, max_range=0.4, **KW)
    c4, latched = pj.scale_coeffs()
    shared.set_new_images(*pr.proj_inputs(s)[:2])
    assert latched and lr.same_bits(c4, shared.scale_coeffs()[0])
    t1, r1 = ba.get_lidar(), bl.results(gpu, ba, s)
    i2 = ba.project_lidar(pj, SIZE, point_mode=mode, max_range=0.4, **KW)
    assert {k: v for k, v in i1.items() if not k.endswith("_ms")} == {k: v for k, v in i2.items() if not k.endswith("_ms")}
    assert i1["num_proj"] > 0 and i1["num_icp"] + i1["num_icp_ground"] > 0
    bl.assert_same(ba.get_lidar(), t1)
    bl.assert_same(bl.results(gpu, ba, s), r1)
    ba.close(); pj.close()


def test_no_observations_installs_no_terms(gpu, world):
    _, pj = world
    s = pr.scene(65)
    empty = dict(s, obs_image=np.zeros(0, np.int32), obs_point=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2)))
    t = lr.terms(np.ones(65, np.uint8), np.tile([0.0, 0.0, 1.0, -5.0], (65, 1)), [0.0, 1.0, 1.0, 1.0])
    ba = gpu.BA(**lr.fresh_args(empty, t))             # 65 terms, no observation
    info = ba.project_lidar(pj, SIZE, **KW)
    assert (info["num_terms"], info["num_features"], info["num_found"], info["num_images"]) == (0, 0, 0, 24)
    assert ba.L == 0 and len(ba.get_lidar()["point"]) == 0
    ba.close()


def test_register_refine_with_a_projector_is_project_then_solve(gpu, world):
    cloud, pj = world
    s = pr.scene(65)
    mode = (np.arange(65) % 2 + 1).astype(np.uint8)    # Proj and nearest neighbour in turn
    opts = dict(max_num_iterations=3, linear_solver="cholesky")
    sched = dict(kd_max=0.4, kd_min=0.1, drop=0.2)
    a, b = gpu.BA(**s), gpu.BA(**s)
    (info, summary, _), = gpu.register_refine(a, cloud, 1, gate_mode=GATE_LOCAL, projector=pj, cam_size=SIZE, point_mode=mode,
                                               proj_weight=3.0, **sched, **opts)
    rng = float(gpu.search_range_schedule(np.array([0], np.int32), **sched)[0])
    manual = b.project_lidar(pj, SIZE, point_mode=mode, max_range=rng, gate_mode=GATE_LOCAL, proj_weight=3.0)
    bl.assert_same(a.get_lidar(), b.get_lidar())
    gpu.ba_solve(b, **opts)
    assert info["max_range"] == rng and info["num_terms"] == manual["num_terms"]
    assert info["num_proj"] > 0 and info["num_icp"] + info["num_icp_ground"] > 0 and summary["num_iterations"] >= 1
    for x, y in zip(a.get_parameters(), b.get_parameters()):
        assert lr.same_bits(x, y)
    a.close(); b.close()


# ---- 7. shim --------------------------------------------------------------------------------------------------------
def test_shim_project_lidar(gpu):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_proj"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_proj")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

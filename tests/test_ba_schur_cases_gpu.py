"""GPU parity of the point elimination (pcd_ba_schur*) beyond the single-camera scenes of
test_ba_schur_gpu.py: every camera model and a mixed-model scene, shuffled / reversed observation orders, points seen
twice by one image, the edge shapes (ns = 0, ns = 1, ns > 256, O = 0, points seen only by constant poses, images of
several 1024-observation segments), rank-deficient points at mu = 0 and 1e-4, the host-copy entry pcd_ba_schur and
ba_solve_lm.  Every case compares cost, S_diag, S_off, rhs, the dense S, num_skipped and the set of skipped points,
back-substitution, the model decrease and plus with the bounds of test_ba_schur_gpu.py.

Seeds: the blocks of S are differences of large terms, so the 1e-9 bound holds only where S is insensitive to the
ulp-level differences between the device's and the oracle's sums of H_pt and W.  The seeds below were chosen where a
relative perturbation of 1e-15 of those inputs moves S and rhs by less than 1e-12 relative (some other seeds of the same
generators move them by 1e-9)."""
import ctypes as C

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_schur_ref as ref
from tests.test_ba_schur_gpu import _check_blocks, _close, _scene, _step

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _skipped_on_device(ba, ne, ns):
    """the device's skipped set: points whose step is exactly 0 for a random pose step (V^-1 = 0); kept points move"""
    dpose = torch.from_numpy(np.random.default_rng(1).normal(size=(ns, 6))).cuda(ba.device)
    x, _ = ba.back_substitute(dpose)
    zero = ~x.cpu().numpy().any(axis=1)
    elim = ne.pr["point_const"] == 0
    got = np.flatnonzero(zero & elim)
    assert np.array_equal(got, np.flatnonzero(ne.skipped)), (got, np.flatnonzero(ne.skipped))


def _full(gpu, oracle, s, mu, mode="marquardt", wc=False):
    """every output of the elimination, the step and plus against the reference"""
    ba = gpu.BA(**s)
    out = ba.schur(mu, damping=mode, dense=True)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    ne = ref.NormalEquations(oracle, s, mu, mode)
    np.testing.assert_allclose(res["cost"][0], ne.cost, rtol=1e-9)
    st = ba.schur_structure()
    assert np.array_equal(st["image_slot"], ne.pr["slot"])
    _check_blocks(ne, st, res)
    ns = st["num_slots"]
    _skipped_on_device(ba, ne, ns)
    dpose, dpoint = _step(ba, res, ne, wc)
    dev = torch.device("cuda", ba.device)
    poses, points = ba.plus(torch.from_numpy(dpose).to(dev), torch.from_numpy(dpoint).to(dev))
    rp, rx = ref.plus(s, dpose, dpoint)
    _close(poses.cpu().numpy(), rp, 1e-14, "plus (poses)")
    _close(points.cpu().numpy(), rx, 1e-14, "plus (points)")
    return ba, res, ne, dpose, dpoint


def _permuted(s, perm):
    s = dict(s)
    for k in ("obs_image", "obs_point", "obs_xy"):
        s[k] = np.ascontiguousarray(np.asarray(s[k])[perm])
    return s


# ---------------------------------------------------------------------------------------------- camera models ----
@pytest.mark.parametrize("model", range(11))
def test_camera_model(gpu, oracle, model):
    """three cameras of one model with different parameters, image i on camera i % 3: models 0-4 take the compiled-in
    instantiations of the Schur pass, 5-10 the generic one"""
    s = ref.camera_scene(oracle, [model] * 3, 400 + model)
    assert s["cam_model"].tolist() == [model] * 3 and set(s["image_camera"].tolist()) == {0, 1, 2}
    assert len({tuple(c) for c in s["cam_params_list"]}) == 3
    ba, *_ = _full(gpu, oracle, s, 1e-4, wc=model in (0, 1))
    ba.close()


MIXED = [0, 3, 4, 6, 9]     # 3, 5, 8, 12 and 5 parameters: the per-camera offsets differ


def test_mixed_camera_models(gpu, oracle):
    s = ref.camera_scene(oracle, MIXED, 410, I=10, P=250)
    assert s["cam_model"].tolist() == MIXED and set(s["image_camera"].tolist()) == set(range(5))
    assert len({len(c) for c in s["cam_params_list"]}) == 4
    ba, *_ = _full(gpu, oracle, s, 1e-4, wc=True)
    ba.close()


# ----------------------------------------------------------------------------------- orders and duplicates ----
@pytest.mark.parametrize("order", ["shuffled", "reversed"])
def test_observation_order(gpu, oracle, order):
    s = _scene(420, I=8, P=200)
    O = len(s["obs_image"])
    perm = np.random.default_rng(7).permutation(O) if order == "shuffled" else np.arange(O)[::-1]
    s = _permuted(s, perm)
    for key in ("obs_image", "obs_point"):          # neither image-major nor point-major
        assert (np.diff(s[key]) < 0).any()
    ba, *_ = _full(gpu, oracle, s, 1e-4, wc=True)
    ba.close()


def test_shuffled_order_bitwise_repeatable(gpu):
    s = _scene(421, I=8, P=300)
    s = _permuted(s, np.random.default_rng(8).permutation(len(s["obs_image"])))
    ba = gpu.BA(**s)
    a = ba.schur(1e-3, dense=True)
    dpose = torch.linalg.solve(a["S"], a["rhs"].reshape(-1)).reshape(-1, 6)
    x1, m1 = ba.back_substitute(dpose)
    x1, m1 = x1.clone(), m1.clone()
    b = ba.schur(1e-3, dense=True)
    x2, m2 = ba.back_substitute(dpose)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(x1, x2) and torch.equal(m1, m2)
    ba.close()


def test_duplicate_observations(gpu, oracle):
    """points seen twice by one variable-pose image (cross entries in its diagonal block, doubled pair entries) and
    twice by one constant-pose image (no part in S)"""
    s = _scene(422, I=8, P=300)
    cpose = s["image_const_pose"].astype(bool)
    oi, op = np.asarray(s["obs_image"]), np.asarray(s["obs_point"])
    elim = s["point_const"][op] == 0
    var_o = np.flatnonzero(~cpose[oi] & elim)[:12]
    const_o = np.flatnonzero(cpose[oi] & elim)[:12]
    extra = np.concatenate([var_o, const_o])
    s["obs_image"] = np.concatenate([oi, oi[extra]]).astype(np.int32)
    s["obs_point"] = np.concatenate([op, op[extra]]).astype(np.int32)
    s["obs_xy"] = np.concatenate([s["obs_xy"], s["obs_xy"][extra] + 3.0])
    pairs = np.stack([s["obs_image"], s["obs_point"]], 1)
    _, cnt = np.unique(pairs, axis=0, return_counts=True)
    assert (cnt == 2).sum() == 24 and var_o.size == 12 and const_o.size == 12
    # the variable images with a duplicate also share that point with another variable image: a doubled pair entry
    shared = [p for p in op[var_o] if (~cpose[s["obs_image"][s["obs_point"] == p]]).sum() >= 3]
    assert shared
    ba, *_ = _full(gpu, oracle, s, 1e-4, wc=True)
    ba.close()


# -------------------------------------------------------------------------------------------------- shapes ----
def test_all_poses_constant(gpu, oracle):
    """ns = 0: only the points move, the model decrease is the points' share"""
    s = _scene(430, I=6, P=150)
    s["image_const_pose"][:] = 1
    ba, res, ne, dpose, dpoint = _full(gpu, oracle, s, 1e-4, wc=True)
    assert ba.schur_structure()["num_slots"] == 0 and res["S"].shape == (0, 0) and dpose.shape == (0, 6)
    elim = ne.pr["point_const"] == 0
    want = -np.einsum("pij,pj->pi", ne.Vinv, ne.gpt)
    _close(dpoint[elim], want[elim], 1e-8, "dpoint = -V^-1 g")
    ba.close()


def test_single_variable_pose(gpu, oracle):
    s = _scene(431, I=6, P=150)
    s["image_const_pose"][:] = 1
    s["image_const_pose"][3] = 0
    ba, res, ne, _, _ = _full(gpu, oracle, s, 1e-4, wc=True)
    st = ba.schur_structure()
    assert st["num_slots"] == 1 and st["pairs"].shape == (0, 2) and res["S_off"].shape == (0, 6, 6)
    ba.close()


def test_many_variable_poses(gpu, oracle):
    """ns > 256: the strided slot loop of k_schur_model_decrease"""
    s = synth.ba_scene(310, 1500, seed=436, const_pose_frac=0.0, lidar_frac=1.0)
    s["image_const_pose"][[0, 5]] = 1
    ba, res, ne, dpose, _ = _full(gpu, oracle, s, 1e-4)
    ns = ba.schur_structure()["num_slots"]
    assert ns >= 300 and np.abs(dpose[256:]).max() > 0
    per_image = np.bincount(s["obs_image"], minlength=310)
    assert per_image.max() <= 64                                # few points each
    ba.close()


def test_lidar_terms_only(gpu, oracle):
    """O = 0: three LiDAR planes per point, no observation; S is the pose damping alone"""
    s = synth.ba_scene(5, 120, seed=433, const_pose_frac=0.3)
    rng = np.random.default_rng(433)
    P = s["points"].shape[0]
    n = rng.normal(size=(3 * P, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    lp = np.repeat(np.arange(P), 3)
    X = s["points"][lp] + rng.normal(0, 0.05, (3 * P, 3))
    s.update(obs_image=np.zeros(0, np.int32), obs_point=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2)),
             lidar_point=lp.astype(np.int32), lidar_abcd=np.concatenate([n, -np.sum(n * X, 1, keepdims=True)], 1),
             lidar_weight=np.full(3 * P, 100.0))
    s["image_const_pose"][0] = 1
    ba, res, ne, dpose, dpoint = _full(gpu, oracle, s, 1e-4, wc=True)
    assert len(s["obs_image"]) == 0 and ba.schur_structure()["pairs"].shape == (0, 2)
    assert not dpose.any() and np.abs(dpoint).max() > 0 and not ne.skipped.any()
    ba.close()


def test_points_seen_only_by_constant_poses(gpu, oracle):
    """synth tracks stay on images of one parity: with the even images constant, the points of even anchors have only
    constant-pose observations.  They get dpoint = -V^-1 g and nothing of them enters S"""
    s = _scene(434, I=8, P=200, tvec=False)
    s["image_const_pose"] = (np.arange(8) % 2 == 0).astype(np.uint8)
    oi, op = np.asarray(s["obs_image"]), np.asarray(s["obs_point"])
    var_seen = np.zeros(200, bool)
    var_seen[op[s["image_const_pose"][oi] == 0]] = True
    only = np.flatnonzero(~var_seen & (np.bincount(op, minlength=200) > 0) & (s["point_const"] == 0))
    assert only.size >= 20
    ba, res, ne, _, dpoint = _full(gpu, oracle, s, 1e-4, wc=True)
    _close(dpoint[only], -np.einsum("pij,pj->pi", ne.Vinv[only], ne.gpt[only]), 1e-8, "dpoint = -V^-1 g")
    # S without these points is the same S: compare against a reference in which they are constant
    s2 = dict(s, point_const=s["point_const"].copy())
    s2["point_const"][only] = 1
    sb2 = ref.NormalEquations(oracle, s2, 1e-4).schur_blocks()
    _close(res["S"], sb2["S"], 1e-9, "S without the constant-pose-only points")
    _close(res["rhs"], sb2["rhs"], 1e-9, "rhs without the constant-pose-only points")
    ba.close()


def test_images_span_several_segments(gpu, oracle):
    """4 images, 9000 points: every image holds several 1024-observation segments; every block, rhs and the step"""
    s = synth.ba_scene(4, 9000, seed=435, const_pose_frac=0.0, lidar_frac=1.0, order="image")
    s["image_const_pose"][1] = 1
    per_image = np.bincount(s["obs_image"], minlength=4)
    var = np.flatnonzero(s["image_const_pose"] == 0)
    assert (per_image[var] > 2 * 1024).all()
    ba, *_ = _full(gpu, oracle, s, 1e-4)
    ba.close()


# -------------------------------------------------------------------------------------- degenerate points ----
@pytest.mark.parametrize("mu", [0.0, 1e-4])
def test_rank_deficient_points(gpu, oracle, mu):
    """one observation without a LiDAR term (rank 2), only a LiDAR term (rank 1, generic and axis-aligned normals):
    skipped at mu = 0 on both sides, kept at a 1e-4 Marquardt damping with their values compared"""
    s, deg = ref.degenerate_scene(oracle, 443)
    ba, res, ne, _, dpoint = _full(gpu, oracle, s, mu)
    if mu == 0.0:
        assert np.array_equal(np.flatnonzero(ne.skipped), deg) and int(res["num_skipped"][0]) == deg.size
        assert not dpoint[deg].any()
    else:
        assert not ne.skipped.any() and int(res["num_skipped"][0]) == 0
        assert np.abs(dpoint[deg]).max() > 0
    ba.close()


# ------------------------------------------------------------------------------------------ host entry ----
def _host_schur(gpu, ba, mu, ns, npair, keys):
    shapes = dict(cost=(1,), S_diag=(ns, 6, 6), S_off=(npair, 6, 6), rhs=(ns, 6), S=(6 * ns, 6 * ns))
    out = {k: np.full(shapes[k], np.nan) for k in keys if k in shapes}
    if "num_skipped" in keys:
        out["num_skipped"] = np.full(1, 2 ** 63, np.uint64)
    o = gpu.BASchurOut(*[gpu._ptr(out.get(n)) for n, _ in gpu.BASchurOut._fields_])
    gpu._check(gpu.lib().pcd_ba_schur(ba._h, C.byref(gpu.BASchurOpts(mu, gpu.DAMP_MARQUARDT)), C.byref(o)))
    return out


def test_host_entry_matches_device_form(gpu):
    s = _scene(450, I=8, P=300)
    probe = gpu.BA(**s)
    st = probe.schur_structure()
    probe.close()
    ns, npair = st["num_slots"], st["pairs"].shape[0]
    assert ns > 1 and npair > 0
    ba = gpu.BA(**s)                                   # fresh handle: the host entry builds the structure
    assert ba.schur_stats()["num_entries"] == 0
    keys = ("cost", "S_diag", "S_off", "rhs", "S", "num_skipped")
    host = _host_schur(gpu, ba, 1e-4, ns, npair, keys)
    assert ba.schur_stats()["num_entries"] > 0
    dev = {k: v.cpu().numpy() for k, v in ba.schur(1e-4, dense=True).items()}
    for k in keys:
        if k == "num_skipped":
            assert int(host[k][0]) == int(dev[k][0])
        else:
            assert np.array_equal(host[k].view(np.uint64), dev[k].view(np.uint64)), k
    for sub in (("rhs",), ("S",), ("num_skipped", "S_off")):
        part = _host_schur(gpu, ba, 1e-4, ns, npair, sub)
        for k in sub:
            assert np.array_equal(part[k].view(np.uint64), host[k].view(np.uint64)), (sub, k)
    ba.close()


# ------------------------------------------------------------------------------------------ LM and cost ----
def _lm_case(oracle, kind, seed):
    models = {"radial": [2, 2, 2], "mixed": MIXED, "const": [4]}[kind]
    s = ref.camera_scene(oracle, models, seed, I=10, P=400)
    if kind == "const":
        s["image_const_pose"][:] = 1
    s["points"] = s["points"] + np.random.default_rng(seed + 1000).normal(0, 0.05, s["points"].shape)
    return s


@pytest.mark.parametrize("kind,seed", [("radial", 64), ("mixed", 64), ("const", 62)])
def test_solve_lm_camera_models_and_constant_poses(gpu, oracle, kind, seed):
    """ba_solve_lm against ref.lm on a SIMPLE_RADIAL scene, the mixed scene and a scene with every pose constant;
    the seeds keep every rho far from 1e-3 and include a rejected step"""
    s = _lm_case(oracle, kind, seed)
    if kind == "radial":
        assert s["cam_model"].tolist() == [2, 2, 2]
    if kind == "const":
        assert s["image_const_pose"].all()
    want, final = ref.lm(oracle, s, 6)
    ba = gpu.BA(**s)
    got = gpu.ba_solve_lm(ba, max_iterations=6)
    assert [r["accepted"] for r in got] == [r["accepted"] for r in want]
    assert any(r["accepted"] for r in want) and not all(r["accepted"] for r in want)
    for g, w in zip(got, want):
        assert abs(w["rho"] - 1e-3) > 0.05
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
    cost_final = ba.evaluate(("cost",))["cost"][0]
    np.testing.assert_allclose(cost_final, oracle.BA(**final).normal_equations()[0], rtol=1e-8)
    assert cost_final < got[0]["cost"]
    ba.close()


def test_cost_device_equals_evaluate(gpu, oracle):
    s = ref.camera_scene(oracle, MIXED, 410, I=10, P=250)
    ba = gpu.BA(**s)
    a = ba.cost_device().cpu().numpy()[0]
    b = ba.evaluate(("cost",))["cost"][0]
    assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    ba.close()

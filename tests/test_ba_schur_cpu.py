"""CPU checks of the point elimination: the numpy reference (tests/ba_schur_ref.py) agrees with itself -- block-wise
Schur complement + back-substitution against the dense solve of the whole damped system -- on synthetic scenes and
hand-made edge cases, and the library exports the new entry points, which refuse to run without a gfx950 device."""
import ctypes as C

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_schur_ref as ref

NEW_SYMBOLS = ["pcd_ba_schur_structure", "pcd_ba_schur_device", "pcd_ba_schur", "pcd_ba_schur_back_substitute_device",
               "pcd_ba_plus_device", "pcd_ba_set_parameters_device", "pcd_ba_schur_stats"]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def _block_step(ne):
    sb = ne.schur_blocks()
    dpose = np.linalg.solve(sb["S"], sb["rhs"].reshape(-1)).reshape(-1, 6)
    return sb, dpose, ne.back_substitute(dpose)


def _check_routes(ne, tol=1e-10):
    sb, dpose, dpoint = _block_step(ne)
    dp_ref, dx_ref = ne.dense_solve()
    assert _rel(dpose, dp_ref) < tol, _rel(dpose, dp_ref)
    assert _rel(dpoint, dx_ref) < tol, _rel(dpoint, dx_ref)
    # the step solves (H + D) delta = -g: the model decrease is positive
    assert ne.model_decrease(dpose, dpoint) > 0
    return sb, dpose, dpoint


# damping strong enough for the system to be well conditioned (cond(S) ~ 1e10): weakly damped points of two-view
# tracks make the undamped system too ill-conditioned for any two solvers to agree to 1e-10
@pytest.mark.parametrize("mu,mode", [(1e-4, "marquardt"), (1.0, "marquardt"), (10.0, "levenberg"), (100.0, "levenberg")])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_block_schur_equals_dense_solve(oracle, seed, mu, mode):
    s = synth.ba_scene(6, 80, seed=seed, const_pose_frac=0.3, lidar_frac=1.0)
    rng = np.random.default_rng(seed)
    s["image_const_tvec"] = rng.integers(0, 8, 6).astype(np.uint8) * (rng.random(6) < 0.4)
    s["point_const"] = (rng.random(80) < 0.1).astype(np.uint8)
    _check_routes(ref.NormalEquations(oracle, s, mu, mode))


@pytest.mark.parametrize("loss", [0, 1, 2])
def test_block_schur_equals_dense_solve_losses(oracle, loss):
    s = synth.ba_scene(5, 60, seed=7 + loss, order="image")
    s["loss_type"], s["loss_scale"] = loss, 2.0
    _check_routes(ref.NormalEquations(oracle, s, 1e-2))


def _tiny(extra_obs=False):
    """2 images looking along +z, 1 point in front of both (OPENCV camera of synth.ba_scene)"""
    cx, cy = synth.OPENCV_PARAMS[2], synth.OPENCV_PARAMS[3]
    obs_image, obs_xy = [0, 1], [[cx + 30.0, cy - 20.0], [cx - 200.0, cy + 10.0]]
    if extra_obs:                      # the point observed twice in image 0
        obs_image.append(0)
        obs_xy.append([cx + 35.0, cy - 12.0])
    return dict(cam_model=np.array([4], np.int32), cam_params_list=[synth.OPENCV_PARAMS],
                poses=np.array([[1, 0, 0, 0, 0, 0, 0], [0.999, 0.02, -0.03, 0.01, -1.0, 0.05, 0.1]], np.float64),
                image_camera=np.zeros(2, np.int32), points=np.array([[0.2, 0.1, 5.0]]),
                obs_image=np.array(obs_image, np.int32), obs_point=np.zeros(len(obs_image), np.int32),
                obs_xy=np.array(obs_xy, np.float64))


def test_two_images_one_point_by_hand(oracle):
    ne = ref.NormalEquations(oracle, _tiny(), 0.5)
    sb, _, _ = _check_routes(ne)
    Wa, Wb = ne.W[0], ne.W[1]
    Vinv = np.linalg.inv(ne.Hpt[0] + np.diag(0.5 * np.clip(np.diag(ne.Hpt[0]), 1e-6, 1e32)))
    np.testing.assert_allclose(sb["S_off"][(0, 1)], -Wa @ Vinv @ Wb.T, rtol=1e-12, atol=1e-12 * np.abs(Wa).max() ** 2)
    D0 = 0.5 * np.clip(np.diag(ne.Himg[0]), 1e-6, 1e32)
    np.testing.assert_allclose(sb["S_diag"][0], ne.Himg[0] + np.diag(D0) - Wa @ Vinv @ Wa.T, rtol=1e-10,
                               atol=1e-10 * np.abs(ne.Himg[0]).max())
    np.testing.assert_allclose(sb["rhs"][1], -ne.gimg[1] + Wb @ Vinv @ ne.gpt[0], rtol=1e-10,
                               atol=1e-10 * np.abs(ne.gimg[1]).max())
    assert sb["pairs"].tolist() == [[0, 1]]


def test_point_observed_twice_in_one_image(oracle):
    ne = ref.NormalEquations(oracle, _tiny(extra_obs=True), 1e-3)
    sb, _, _ = _check_routes(ne)
    Z0 = ne.W[0] + ne.W[2]               # both observations of image 0 land in its diagonal block
    blk = ne.Himg[0] + np.diag(ne.Dimg[0]) - Z0 @ ne.Vinv[0] @ Z0.T
    np.testing.assert_allclose(sb["S_diag"][0], blk, rtol=1e-10, atol=1e-10 * np.abs(blk).max())
    np.testing.assert_allclose(sb["S_off"][(0, 1)], -Z0 @ ne.Vinv[0] @ ne.W[1].T, rtol=1e-10,
                               atol=1e-10 * np.abs(Z0).max() ** 2)


def test_constant_tvec_component(oracle):
    s = _tiny()
    s["image_const_tvec"] = np.array([0, 0b101], np.uint8)   # tx and tz of image 1 held constant
    ne = ref.NormalEquations(oracle, s, 1e-2)
    sb, dpose, _ = _check_routes(ne)
    for k in (3, 5):
        assert dpose[1, k] == 0.0 and sb["rhs"][1, k] == 0.0
        e = np.zeros(6); e[k] = 1.0
        assert np.array_equal(sb["S_diag"][1][k], e) and np.array_equal(sb["S_diag"][1][:, k], e)
        assert not sb["S_off"][(0, 1)][:, k].any()
    poses, _ = ref.plus(s, dpose, np.zeros((1, 3)))
    assert poses[1, 4] == s["poses"][1, 4] and poses[1, 6] == s["poses"][1, 6] and poses[1, 5] != s["poses"][1, 5]


def test_constant_point(oracle):
    s = synth.ba_scene(4, 30, seed=5)
    s["point_const"] = np.zeros(30, np.uint8)
    s["point_const"][[0, 3, 7]] = 1
    ne = ref.NormalEquations(oracle, s, 1e-3)
    _, _, dpoint = _check_routes(ne)
    assert not dpoint[[0, 3, 7]].any()
    _, points = ref.plus(s, np.zeros((4, 6)), dpoint + 1.0)
    assert np.array_equal(points[[0, 3, 7]], s["points"][[0, 3, 7]])


def test_quaternion_plus_matches_manifold_jacobian():
    """Plus(q, d) - q = PlusJacobian(q) d + O(|d|^2) with the PlusJacobian of csrc/ba_math.h quat_tangent"""
    q = np.array([0.9, 0.1, -0.3, 0.2]); q /= np.linalg.norm(q)
    J = np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])
    d = np.array([1e-6, -2e-6, 0.5e-6])
    np.testing.assert_allclose(ref.quat_plus(q, d) - q, J @ d, rtol=1e-5, atol=1e-16)
    assert np.array_equal(ref.quat_plus(q, np.zeros(3)), q)
    assert abs(np.linalg.norm(ref.quat_plus(q, np.array([0.3, -0.2, 0.1]))) - 1.0) < 1e-15


def test_new_symbols_exported(pcdhip):
    L = pcdhip.lib()
    missing = [s for s in NEW_SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert set(NEW_SYMBOLS) <= set(pcdhip.ABI_SYMBOLS)
    for m in ("schur", "back_substitute", "plus", "schur_structure"):
        assert callable(getattr(pcdhip.BA, m))
    assert callable(pcdhip.ba_solve_lm)


def test_no_device_refusal(pcdhip):
    """without a gfx950 device every new entry point returns PCD_ERR_NO_DEVICE (there is no CPU route)"""
    if pcdhip.device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is exercised on CPU-only boxes")
    L = pcdhip.lib()
    opts, out = pcdhip.BASchurOpts(1e-3, 0), pcdhip.BASchurOut()
    ns, npair = C.c_int32(0), C.c_uint64(0)
    calls = [
        L.pcd_ba_schur_structure(None, None, C.byref(ns), C.byref(npair), None, None),
        L.pcd_ba_schur_device(None, C.byref(opts), C.byref(out), None),
        L.pcd_ba_schur(None, C.byref(opts), C.byref(out)),
        L.pcd_ba_schur_back_substitute_device(None, None, None, None, None),
        L.pcd_ba_plus_device(None, None, None, None, None, None),
        L.pcd_ba_set_parameters_device(None, None, None, None),
        L.pcd_ba_schur_stats(None, None),
    ]
    assert calls == [pcdhip.PCD_ERR_NO_DEVICE] * len(calls)
    with pytest.raises(pcdhip.PcdError) as e:
        pcdhip.BA(**synth.ba_scene(3, 10, seed=1))
    assert e.value.status == pcdhip.PCD_ERR_NO_DEVICE


@pytest.mark.parametrize("seed", [50, 51, 52])
def test_pivot_rule_is_stable_under_rounding(oracle, seed):
    """the skip decision of point_inverse (the rule of k_schur_points) does not depend on the last bits of H_pt: the
    device sums H_pt in another order than the oracle, so the two agree only to a few ulp.  Rank-deficient points of
    ref.degenerate_scene (one observation without a LiDAR term, only a LiDAR term) are skipped at mu = 0 and kept at a
    1e-4 Marquardt damping, and no decision flips under a symmetric relative perturbation of 4e-16 N(0, 1); full-rank
    points (two or more observations, or one observation plus a LiDAR term) are never skipped."""
    s, deg = ref.degenerate_scene(oracle, seed)
    ne0 = ref.NormalEquations(oracle, s, 0.0)
    P = s["points"].shape[0]
    nobs = np.bincount(s["obs_point"], minlength=P)
    nlid = np.bincount(s["lidar_point"], minlength=P)
    assert (nobs[deg[:8]] == 1).all() and (nlid[deg[:8]] == 0).all()
    assert (nobs[deg[8:]] == 0).all() and (nlid[deg[8:]] == 1).all()
    full = np.flatnonzero((nobs >= 2) | ((nobs == 1) & (nlid >= 1)))
    assert full.size > 100 and not np.isin(full, deg).any()
    rng = np.random.default_rng(seed)
    H = ne0.Hpt
    pc = np.zeros(P, np.uint8)
    for mu in (0.0, 1e-16, 1e-4):
        D = ref.damping(np.diagonal(H, axis1=1, axis2=2), mu, "marquardt")
        _, skip = ref.point_inverse(H, D, pc)
        if mu == 0.0:
            assert np.array_equal(np.flatnonzero(skip), deg)
        elif mu == 1e-16:   # axis-aligned LiDAR-only points: exactly diagonal V, kept (pivots = diagonal)
            assert np.array_equal(np.flatnonzero(skip), deg[:-3])
        else:
            assert not skip.any()
        for _ in range(200):
            E = rng.normal(size=H.shape)
            E = 0.5 * (E + E.transpose(0, 2, 1))
            Hp = H * (1.0 + 4e-16 * E)
            Dp = ref.damping(np.diagonal(Hp, axis1=1, axis2=2), mu, "marquardt")
            _, sp = ref.point_inverse(Hp, Dp, pc)
            assert np.array_equal(sp, skip), (mu, np.flatnonzero(sp != skip))
        assert not skip[full].any()


def test_shared_launch_scene_skips_no_point(oracle):
    """ref.shared_launch_scene is what its docstring says, and the reference elimination skips none of its points at
    mu = 0: the GPU comparison on it (test_ba_schur_gpu.py) covers all 70"""
    s = ref.shared_launch_scene()
    assert s["poses"].shape == (3, 7) and s["points"].shape == (70, 3)
    assert s["image_const_pose"].tolist() == [1, 0, 0] and np.flatnonzero(s["point_const"]).tolist() == [5]
    per_image = np.bincount(s["obs_image"], minlength=3)
    assert per_image.tolist() == [70, 70, 1050] and 1024 < per_image[2] <= 2 * 1024
    assert 0 < s["lidar_point"].size < 10
    assert not np.array_equal(np.argsort(s["obs_image"], kind="stable"), np.arange(s["obs_image"].size))
    ne = ref.NormalEquations(oracle, s, 0.0)
    assert not ne.skipped.any()
    assert ne.elig.sum() == 69 * 16 and np.isfinite(ne.schur_blocks()["S"]).all()


def test_pivot_rule_is_scale_invariant():
    """scaling a point's coordinates (V -> S V S, S diagonal) does not change the decision"""
    rng = np.random.default_rng(3)
    J = rng.normal(size=(500, 2, 3))
    H = np.einsum("pki,pkj->pij", J, J)                       # rank 2
    Hf = H + np.einsum("pi,pj->pij", *(2 * [rng.normal(size=(500, 3))]))   # + a rank-1 term: full rank
    pc = np.zeros(500, np.uint8)
    for scale in (1e-6, 1.0, 1e8):
        Sc = np.diag([scale, 1.0, 1.0 / scale])
        for A, want in ((H, True), (Hf, False)):
            As = Sc @ A @ Sc
            for mu, w in ((0.0, want), (1e-4, False)):
                _, skip = ref.point_inverse(As, ref.damping(np.diagonal(As, axis1=1, axis2=2), mu, "marquardt"), pc)
                assert (skip == w).all(), (scale, mu, want, int(skip.sum()))

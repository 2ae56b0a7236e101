"""GPU parity of the reduced system with refined intrinsics (pcd_ba_schur_cam*, pcd_ba_solve with refine_intrinsics;
DESIGN 4.3a) against the numpy reference built from the oracle's blocks (tests/ba_schur_cam_ref.py).

Bounds: B, S_cam, rhs_cam and the dense S within 1e-9 relative (scale-aware floor, as test_ba_schur_gpu.py), the pose
part (cost, S_diag, S_off, rhs) bit-identical to the plain call on the same scene without camera_refine; the direct solve
of the bordered system within ETA_CAM_BOUND (tests/test_ba_schur_cam_cpu.py: taken from the reference alone) in backward
error against the device's own dense S; back-substitution and model decrease within 1e-8 of the reference for the same
delta; plus within 1e-14; on the well-conditioned settings the step within 1e-8 of the solve of the whole damped system.
The chunk of the camera point sums is 256 points: the 300-point scenes cross it."""
import numpy as np
import pytest

from tests import ba_schur_cam_ref as cref
from tests import ba_schur_ref as ref
from tests.test_ba_chol_cpu import eta
from tests.test_ba_schur_cam_cpu import ETA_CAM_BOUND

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S12 = 12


def _close(a, b, rtol, what):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, err_msg=what)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _parity(gpu, oracle, s, refine, mu, mode, well_conditioned):
    """every check of one (scene, refine, damping): blocks, pose part, solve, back-substitution, plus.  Returns the
    reference; its attribute `device` holds the direct solve's info and step, the device's dense S and right-hand side"""
    base = cref.without_refine(s)
    ne = cref.CamNormalEquations(oracle, base, refine, mu, mode)
    sb = ne.schur_cam_blocks()
    ns, ncs = ne.pr["slot_img"].size, ne.ncs
    n = 6 * ns + S12 * ncs
    plain = gpu.BA(**base)
    p = _np(plain.schur(mu, damping=mode))
    ba = gpu.BA(**base, camera_refine=refine)
    slots = ba.camera_slots()
    assert slots["num_slots"] == ncs and np.array_equal(slots["camera_slot"], ne.cam_slot)
    assert np.array_equal(slots["active"].astype(bool), ne.cam_active)
    want = ("cost", "S_diag", "S_off", "rhs", "B", "S_cam", "rhs_cam", "num_skipped")
    r = _np(ba.schur_cam(mu, damping=mode, dense=True, want=want, num_pairs=p["S_off"].shape[0]))
    # the pose part must not move
    for k in ("cost", "S_diag", "S_off", "rhs", "num_skipped"):
        assert np.array_equal(r[k], p[k]), k
    assert int(r["num_skipped"][0]) == int(ne.skipped.sum())
    np.testing.assert_allclose(r["cost"][0], ne.cost, rtol=1e-9)
    _close(r["B"], sb["B"], 1e-9, "B")
    _close(r["S_cam"], sb["S_cam"], 1e-9, "S_cam")
    _close(r["rhs_cam"], sb["rhs_cam"], 1e-9, "rhs_cam")
    _close(r["S"], sb["S"], 1e-9, "dense S")
    S = r["S"]
    assert S.shape == (n, n)
    n0 = 6 * ns     # the camera part is exactly symmetric; the pose part is the plain call's, entry by entry
    assert np.array_equal(S[n0:, n0:], S[n0:, n0:].T) and np.array_equal(S[n0:, :n0], S[:n0, n0:].T)
    assert np.array_equal(S[:n0, :n0], _np(plain.schur(mu, damping=mode, dense=True, want=("cost",)))["S"])
    dead = np.concatenate([~ne.pr["active"].reshape(-1), ~ne.cam_active.reshape(-1)])
    assert np.array_equal(S[dead][:, dead], np.eye(int(dead.sum()))) and not S[dead][:, ~dead].any()
    rhs = np.concatenate([r["rhs"].reshape(-1), r["rhs_cam"].reshape(-1)])
    assert not rhs[dead].any()
    # the direct solve reads the handle's own blocks
    ba.schur_cam(mu, damping=mode, want=("cost", "num_skipped"))
    delta, info = ba.schur_cam_solve_cholesky()
    delta = delta.cpu().numpy()
    assert info["n"] == n
    ne.device = dict(info=info, S=S, rhs=rhs, delta=delta.copy(), slots=slots)      # for the caller's own assertions
    if info["status"] == gpu.CHOL_OK:
        e = eta(S, rhs, delta)
        print(f"n {n} ncs {ncs} eta {e:.3e} (bound {ETA_CAM_BOUND:.3e})")
        assert e <= ETA_CAM_BOUND
        assert not delta[dead].any()
    else:   # S is not numerically positive definite (Levenberg at mu = 0 on a scene with a free gauge)
        assert not well_conditioned and not delta.any()
    if well_conditioned:
        assert info["status"] == gpu.CHOL_OK
        dpose, dcam = ne.split(delta)
    else:   # the same linear maps, on a step of moderate size; inactive camera coordinates carry garbage on purpose
        rng = np.random.default_rng(7)
        dpose = rng.normal(0, 1e-3, (ns, 6)) * ne.pr["active"]
        dcam = rng.normal(0, 1e-3, (ncs, S12))
        delta = np.concatenate([dpose.reshape(-1), dcam.reshape(-1)])
    dpoint, md = ba.back_substitute_cam(_dev(delta))
    dpoint = dpoint.cpu().numpy()
    _close(dpoint, ne.back_substitute_cam(dpose, dcam), 1e-8, "back-substitution")
    _close(md.cpu().numpy()[0], ne.model_decrease_cam(dpose, dcam, dpoint), 1e-8, "model decrease")
    assert not dpoint[ne.skipped | (ne.pr["point_const"] == 1)].any()
    if well_conditioned:
        rp, rc, rx = ne.dense_solve_cam()
        _close(dpose, rp, 1e-8, "pose step vs the whole system")
        _close(dcam, rc, 1e-8, "camera step vs the whole system")
        _close(dpoint, rx, 1e-8, "point step vs the whole system")
    poses, points, cams = ba.plus_cam(_dev(delta), _dev(dpoint))
    wp, wx, wc = cref.plus_cam(base, refine, dpose, dcam, dpoint)
    _close(poses.cpu().numpy(), wp, 1e-14, "plus (poses)")
    _close(points.cpu().numpy(), wx, 1e-14, "plus (points)")
    cams = cams.cpu().numpy()
    _close(cams, np.concatenate(wc), 1e-14, "plus (cameras)")
    flat = np.concatenate([np.asarray(c, np.float64) for c in base["cam_params_list"]])
    fixed = np.asarray(refine) == 0
    assert np.array_equal(cams[fixed], flat[fixed]) and (ncs == 0 or not np.array_equal(cams, flat))
    assert np.array_equal(ba.get_camera_parameters(), flat)        # plus writes candidates, not the handle
    plain.close(); ba.close()
    return ne


@pytest.mark.parametrize("damping", range(len(cref.DAMPINGS)))
@pytest.mark.parametrize("case", range(len(cref.CAM_CASES)))
def test_block_parity(gpu, oracle, case, damping):
    mode, mu = cref.DAMPINGS[damping]
    s, refine = cref.cam_case_scene(oracle, case)
    ne = _parity(gpu, oracle, s, refine, mu, mode, mode in cref.WELL_CONDITIONED)
    if case == 4:      # two slots whose images share points: the off-diagonal block is not zero
        assert np.abs(ne.schur_cam_blocks()["S_cam"][0, 1]).max() > 0


def test_shared_launch_scene(gpu, oracle):
    """70 points (two 64-track slices, the second partial), an image of 1050 observations (two segments), a constant-pose
    image whose observations still feed Wc_p, a constant point; one shared camera: the kernel without a camera test"""
    s = ref.shared_launch_scene()
    ne = _parity(gpu, oracle, s, cref.refine_mask(s, None, (0, 1)), 1e-4, "marquardt", True)
    const_img = ne.pr["slot"][ne.pr["obs_image"]] < 0
    assert np.abs(ne.Wcam[const_img & (ne.obs_cam_slot >= 0)]).max() > 0


@pytest.mark.parametrize("models", [[4], [4, 2]])
def test_points_cross_a_chunk(gpu, oracle, models):
    """300 points: two chunks of the camera point sums, the second one partial"""
    s = cref.camera_scene(oracle, models, 61, I=6, P=300)
    _parity(gpu, oracle, s, cref.refine_mask(s), 1e-4, "marquardt", True)


def test_degenerate_points_are_skipped(gpu, oracle):
    s, bad = ref.degenerate_scene(oracle, 71)
    s["cam_params_list"] = [np.asarray(s["cam_params_list"][0], np.float64)]
    ne = _parity(gpu, oracle, s, cref.refine_mask(s, None, (0, 1)), 0.0, "marquardt", False)
    assert ne.skipped.sum() > 0 and ne.skipped[bad].sum() == ne.skipped.sum()


def test_every_pose_constant(gpu, oracle):
    """ns = 0, n = 12 ncs: cameras and points alone"""
    s = cref.camera_scene(oracle, [4, 2], 81)
    s["image_const_pose"][:] = 1
    ne = _parity(gpu, oracle, s, cref.refine_mask(s), 1e-4, "marquardt", True)
    assert ne.pr["slot_img"].size == 0 and ne.ncs == 2


def test_without_camera_slots_the_calls_are_the_plain_ones(gpu, oracle):
    s = ref.camera_scene(oracle, [4, 2], 91)
    a, b = gpu.BA(**s), gpu.BA(**s)
    assert a.camera_slots()["num_slots"] == 0
    pa = a.schur(1e-4, dense=True)
    pb = b.schur_cam(1e-4, dense=True, want=("cost", "S_diag", "S_off", "rhs", "num_skipped"), num_pairs=pa["S_off"].shape[0])
    for k in ("cost", "S_diag", "S_off", "rhs", "S", "num_skipped"):
        assert torch.equal(pa[k], pb[k]), k
    a.schur(1e-4, want=("cost",)); b.schur_cam(1e-4, want=("cost",))
    xa, ia = a.schur_solve_cholesky()
    xb, ib = b.schur_cam_solve_cholesky()
    assert ia == ib and ia["status"] == gpu.CHOL_OK and torch.equal(xa.reshape(-1), xb)
    da, ma = a.back_substitute(xa)
    db, mb = b.back_substitute_cam(xb)
    assert torch.equal(da, db) and torch.equal(ma, mb)
    qa, ya = a.plus(xa, da)
    qb, yb, cb = b.plus_cam(xb, db)
    assert torch.equal(qa, qb) and torch.equal(ya, yb)
    assert np.array_equal(cb.cpu().numpy(), a.cam_params)
    sa, ha = gpu.ba_solve(a, max_num_iterations=4, linear_solver="cholesky")
    sb, hb = gpu.ba_solve(b, max_num_iterations=4, linear_solver="cholesky", refine_intrinsics=True)
    assert ha == hb and sa["final_cost"] == sb["final_cost"] and sa["num_accepted"] == sb["num_accepted"] >= 1
    for u, v in zip(a.get_parameters(), b.get_parameters()):
        assert np.array_equal(u, v)
    sc, hc = gpu.ba_solve(b, max_num_iterations=2, refine_intrinsics=True)      # the PCG is fine without camera slots
    assert sc["num_iterations"] == 2
    a.close(); b.close()


def test_bitwise_repeatable(gpu, oracle):
    s, refine = cref.cam_case_scene(oracle, 4)
    ba = gpu.BA(**s, camera_refine=refine)
    want = ("cost", "B", "S_cam", "rhs_cam", "num_skipped")
    a = {k: v.clone() for k, v in ba.schur_cam(1e-4, dense=True, want=want).items()}
    xa, ia = ba.schur_cam_solve_cholesky()
    xa = xa.clone()
    b = ba.schur_cam(1e-4, dense=True, want=want)
    xb, ib = ba.schur_cam_solve_cholesky()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(xa, xb) and ia == ib and ia["status"] == gpu.CHOL_OK
    ba.close()


# ---- the LM loop ------------------------------------------------------------------------------------------------------
def _lm_scene(oracle):
    s = ref.camera_scene(oracle, [4], seed=25, I=8, P=200)
    s["points"] = s["points"] + np.random.default_rng(1025).normal(0, 1.0, s["points"].shape)
    cp = np.array(s["cam_params_list"][0], np.float64)
    cp[:2] *= 1.05
    s["cam_params_list"] = [cp]
    return s, cref.refine_mask(s)


def _cost(oracle, s, poses, points, cams):
    return oracle.BA(**dict(s, poses=poses, points=points, cam_params_list=[np.asarray(cams)])).normal_equations()[0]


def test_lm_parity(gpu, oracle):
    """pcd_ba_solve with refine_intrinsics and the direct solver against the same loop on the oracle.  The reference:
    accepted TTTTFFTT, min |rho - 1e-3| = 0.40, cost 5.58e7 -> 6.10e6"""
    s, refine = _lm_scene(oracle)
    want, final = cref.lm_cam(oracle, s, refine, 8, initial_radius=1e4)
    assert "".join("T" if w["accepted"] else "F" for w in want) == "TTTTFFTT"
    for w in want:
        assert abs(w["rho"] - 1e-3) > 0.05
    cost_final = oracle.BA(**final).normal_equations()[0]
    ba = gpu.BA(**s, camera_refine=refine)
    summary, got = gpu.ba_solve(ba, max_num_iterations=8, initial_radius=1e4, linear_solver="cholesky",
                                refine_intrinsics=True)
    print(summary, "accepted", "".join("T" if r["accepted"] else "F" for r in got), "costs", [r["cost"] for r in got])
    assert summary["num_iterations"] == 8 and summary["termination"] == gpu.SOLVE_MAX_ITERATIONS
    assert [r["accepted"] for r in got] == [w["accepted"] for w in want]
    for g, w in zip(got, want):
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
        assert g["linear_iterations"] == 0 and g["linear_termination"] == gpu.CHOL_OK
    np.testing.assert_allclose(summary["final_cost"], cost_final, rtol=1e-8)
    poses, points = ba.get_parameters()
    cams = ba.get_camera_parameters()
    np.testing.assert_allclose(_cost(oracle, s, poses, points, cams), cost_final, rtol=1e-8)
    assert not np.array_equal(cams, s["cam_params_list"][0])
    ba.close()


def test_focal_length_is_recovered(gpu, oracle):
    """focal x 1.02, focal only refined.  The reference: six accepted steps, cost 3.32e5 -> 2.39e4 in the first, fx and fy
    within 0.1 % of the truth; the constant-intrinsics solve ends at 6.5e4"""
    s = ref.camera_scene(oracle, [4], seed=23, I=8, P=200)
    truth = np.array(s["cam_params_list"][0], np.float64)
    cp = truth.copy()
    cp[:2] *= 1.02
    s["cam_params_list"] = [cp]
    refine = cref.refine_mask(s, None, (0, 1))
    want, final = cref.lm_cam(oracle, s, refine, 6)
    assert all(w["accepted"] for w in want)
    assert np.abs(final["cam_params_list"][0][:2] / truth[:2] - 1).max() < 1e-3
    ba = gpu.BA(**s, camera_refine=refine)
    summary, got = gpu.ba_solve(ba, max_num_iterations=6, linear_solver="cholesky", refine_intrinsics=True)
    assert [r["accepted"] for r in got] == [True] * 6
    for g, w in zip(got, want):
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["candidate_cost"], w["candidate_cost"], rtol=1e-8)
    cams = ba.get_camera_parameters()
    assert np.abs(cams[:2] / truth[:2] - 1).max() < 1e-3 and np.array_equal(cams[2:], cp[2:])
    fixed = gpu.BA(**s)
    sf, _ = gpu.ba_solve(fixed, max_num_iterations=6, linear_solver="cholesky")
    print("refined", summary["final_cost"], "constant intrinsics", sf["final_cost"])
    assert summary["final_cost"] < sf["final_cost"]
    ba.close(); fixed.close()


def test_after_a_refining_solve_the_handle_is_a_fresh_one(gpu):
    """evaluate on the solved handle equals evaluate on a handle created from the returned poses, points and camera
    parameters bit for bit; project_lidar installs the same terms on both: the host mirror of the camera parameters
    (focal lengths of the depth projection) followed the solve"""
    from tests import ba_lidar_ref as lr
    from tests import ba_proj_ref as pr
    from tests.test_ba_proj_gpu import KW, SIZE
    s = dict(pr.scene(130))
    cp = np.array(s["cam_params_list"][0], np.float64)
    cp[:2] *= 1.02
    s["cam_params_list"] = [cp]
    refine = cref.refine_mask(s, None, (0, 1))
    ba = gpu.BA(**s, camera_refine=refine)
    summary, _ = gpu.ba_solve(ba, max_num_iterations=3, linear_solver="cholesky", refine_intrinsics=True)
    assert summary["num_accepted"] >= 1
    poses, points = ba.get_parameters()
    cams = ba.get_camera_parameters()
    assert not np.array_equal(cams[:2], cp[:2]) and np.array_equal(cams[2:], cp[2:])
    fresh = gpu.BA(**dict(s, poses=poses, points=points, cam_params_list=[cams]), camera_refine=refine)
    want = ("cost", "residuals", "H_img", "g_img", "H_pt", "g_pt", "H_cam", "g_cam", "E_cam")
    a, b = ba.evaluate(want), fresh.evaluate(want)
    for k in want:
        assert lr.same_bits(a[k], b[k]), k
    xyz, nrm = pr.cloud()
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    # a projector of its own for each handle: its scale coefficients are latched from the focal lengths of the first
    # call, which project_lidar takes from the handle's host mirror
    pa, pb = gpu.Projector(cloud), gpu.Projector(cloud)
    ia, ib = ba.project_lidar(pa, SIZE, **KW), fresh.project_lidar(pb, SIZE, **KW)
    assert ia["num_terms"] == ib["num_terms"] > 0
    (ca, la), (cb, lb) = pa.scale_coeffs(), pb.scale_coeffs()
    assert la and lb and lr.same_bits(ca, cb)
    ta, tb = ba.get_lidar(), fresh.get_lidar()
    for k in ("point", "abcd", "weight", "type", "lidar_xyz"):
        assert lr.same_bits(ta[k], tb[k]), k
    for h in (ba, fresh, pa, pb, cloud):
        h.close()


# ---- guards -----------------------------------------------------------------------------------------------------------
def test_guards(gpu, oracle):
    s, refine = cref.cam_case_scene(oracle, 0)
    ba = gpu.BA(**s, camera_refine=refine)
    with pytest.raises(gpu.PcdError) as e:                     # no _cam Schur call yet
        ba.schur_cam_solve_cholesky()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    with pytest.raises(gpu.PcdError) as e:                     # the PCG knows no border
        gpu.ba_solve(ba, max_num_iterations=2, refine_intrinsics=True)
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "PCD_LINEAR_CHOLESKY" in str(e.value)
    with pytest.raises(gpu.PcdError) as e:                     # without the flag a refined handle is refused as before
        gpu.ba_solve(ba, max_num_iterations=2, linear_solver="cholesky")
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    with pytest.raises(gpu.PcdError) as e:
        ba.schur(1e-4)
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    ba.schur_cam(1e-4, want=("cost", "S_diag"))                # S_diag went to caller memory
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_cam_solve_cholesky()
    assert e.value.status == gpu.PCD_ERR_INVALID and "S_diag" in str(e.value)
    summary, _ = gpu.ba_solve(ba, max_num_iterations=2, linear_solver="cholesky", refine_intrinsics=True)
    assert summary["num_iterations"] == 2
    with pytest.raises(gpu.PcdError) as e:                     # the loop has moved on from its last Schur state
        ba.schur_cam_solve_cholesky()
    assert e.value.status == gpu.PCD_ERR_INVALID
    ba.close()
    # one refined camera per image, nine of them: more than the bordered system carries
    s9 = ref.camera_scene(oracle, [1] * 9, 33, I=9, P=60)
    ba = gpu.BA(**s9, camera_refine=cref.refine_mask(s9, None, (0, 1)))
    assert ba.camera_slots()["num_slots"] == 9 > gpu.MAX_CAMERA_SLOTS
    for call in (lambda: ba.schur_cam(1e-4), lambda: ba.schur_cam_solve_cholesky(),
                 lambda: gpu.ba_solve(ba, linear_solver="cholesky", refine_intrinsics=True)):
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "PCD_BA_MAX_CAMERA_SLOTS" in str(e.value)
    got = ba.evaluate(("cost", "H_cam"))                       # the handle is usable afterwards
    assert np.isfinite(got["cost"][0]) and np.abs(got["H_cam"]).max() > 0
    ba.close()


def test_capture_refused_then_eager_works(gpu, oracle):
    s, refine = cref.cam_case_scene(oracle, 1)
    ba = gpu.BA(**s, camera_refine=refine)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ba.schur_cam(1e-3, want=("cost", "num_skipped"))
        x0, i0 = ba.schur_cam_solve_cholesky()
        x0 = x0.clone()
        buf = torch.empty_like(x0)
        dpt = torch.empty((ba.P, 3), dtype=torch.float64, device="cuda")
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            for call in (lambda: ba.schur_cam_solve_cholesky(delta=buf), lambda: ba.back_substitute_cam(x0, dpoint=dpt, model_decrease=False)):
                with pytest.raises(gpu.PcdError) as e:
                    call()
                assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
        x1, i1 = ba.schur_cam_solve_cholesky()
        side.synchronize()
        assert torch.equal(x1, x0) and i1 == i0 and i0["status"] == gpu.CHOL_OK
    ba.close()

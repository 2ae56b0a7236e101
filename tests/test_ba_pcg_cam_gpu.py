"""GPU parity of the bordered PCG (pcd_ba_schur_cam_solve_pcg*, pcd_ba_solve with PCD_LINEAR_PCG_CAM)
against the numpy references of tests/ba_pcg_cam_ref.py.

Fixed-iteration parity: 8 iterations with the tolerances off against pcg_cam_device_order (every sum in the order
csrc/ba_pcg.hip states) on the device's own blocks; x, Q and ||r|| / ||rhs|| within PARITY_BOUND = 100 x the
reference's own ascending / descending sensitivity, measured and re-measured in tests/test_ba_pcg_cam_cpu.py (1.6584e-03
on the gauge-free Levenberg mu = 0 systems, hence 1.6584e-01); rhs_norm within 1e-14, precond_fallbacks equal, inactive
camera coordinates and constant-tvec coordinates exactly 0.  Every test prints its figures before it asserts.
Measured on gfx950: the library is built without fused multiply-add (-ffp-contract=off), so the device follows the stated
order exactly and dx = dQ = d|r| = 0 on all 60 cases of test_fixed_iteration_parity and all 12 of test_shapes; the tight
solves stop after 7, 30, 10, 23, 24 and 17 iterations on cases 0 .. 5 with true residuals 2.6e-14 .. 7.2e-13.

The tight solve is compared with the direct solve of the same handle state, the LM loop with lm_cam_pcg and with the
Cholesky route.  Shapes: ns = 0, a constant-pose image on a refined camera, 8 camera slots, ns = 65 with 65 blocks in
every row (one above a wavefront's lanes: the second trip of the row list and of the camera-row sum over the slots),
ns = 257 (one above k_pcg_cam_update's workgroup), a camera block that takes the identity fallback."""
import numpy as np
import pytest

from pcdhip import synth
from tests import ba_pcg_cam_ref as pc
from tests import ba_schur_cam_ref as cref
from tests import ba_schur_ref as ref
from tests.test_ba_pcg_cam_cpu import FIXED8, PARITY_BOUND, TIGHT, lm_scene, rel, unused_camera_scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S12 = 12
KIND = {"identity": pc.IDENTITY, "schur_jacobi": pc.SCHUR_JACOBI}
WANT = ("cost", "S_diag", "S_off", "rhs", "B", "S_cam", "rhs_cam", "num_skipped")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _handle(gpu, s, refine, mu, mode="marquardt"):
    """(handle, block lists, dead coordinates [n]): schur_cam with the blocks downloaded, then once more with the blocks
    left in the handle, which is the state the solver reads (as test_ba_pcg_gpu._blocks)"""
    base = cref.without_refine(s)
    plain = gpu.BA(**base)
    pairs = plain.schur_structure()["pairs"].astype(np.int64).reshape(-1, 2)
    plain.close()
    ba = gpu.BA(**base, camera_refine=refine)
    r = _np(ba.schur_cam(mu, damping=mode, want=WANT, num_pairs=pairs.shape[0]))
    ba.schur_cam(mu, damping=mode, want=("cost", "num_skipped"))
    active = ba.camera_slots()["active"].astype(bool)
    dead = np.concatenate([~ref.problem(base)["active"].reshape(-1), ~active.reshape(-1)])
    return ba, (r["S_diag"], r["S_off"], pairs, r["rhs"], r["B"], r["S_cam"], r["rhs_cam"]), dead


def _solve(ba, **opts):
    x, info = ba.schur_cam_solve_pcg(**opts)
    return dict(info, x=x.cpu().numpy())


def _parity(ba, bl, dead, precond, what):
    got = _solve(ba, preconditioner=precond, **FIXED8)
    want = pc.pcg_cam_device_order(*bl, preconditioner=KIND[precond], **FIXED8)
    dx, dq, dr = rel(got, want, want["rhs_norm"])
    print(f"{what} {precond}: n {got['x'].size}, device {got['iterations']} its term {got['termination']}, reference "
          f"{want['iterations']} its term {want['termination']}, fallbacks {got['precond_fallbacks']} / "
          f"{want['precond_fallbacks']}; dx {dx:.3e} dQ {dq:.3e} d|r| {dr:.3e} (bound {PARITY_BOUND:.4e})")
    assert (got["iterations"], got["termination"]) == (want["iterations"], want["termination"])
    np.testing.assert_allclose(got["rhs_norm"], want["rhs_norm"], rtol=1e-14)
    assert got["precond_fallbacks"] == want["precond_fallbacks"]
    assert max(dx, dq, dr) <= PARITY_BOUND, (dx, dq, dr)
    assert dead.size == got["x"].size and not got["x"][dead].any()
    return got, want


@pytest.mark.parametrize("precond", ["identity", "schur_jacobi"])
@pytest.mark.parametrize("damping", range(len(cref.DAMPINGS)))
@pytest.mark.parametrize("case", range(len(cref.CAM_CASES)))
def test_fixed_iteration_parity(gpu, oracle, case, damping, precond):
    mode, mu = cref.DAMPINGS[damping]
    s, refine = cref.cam_case_scene(oracle, case)
    ba, bl, dead = _handle(gpu, s, refine, mu, mode)
    _parity(ba, bl, dead, precond, f"case {case} {mode} {mu}")
    if case in (2, 4):
        assert dead[6 * bl[3].shape[0]:].any()          # PINHOLE / SIMPLE_RADIAL leave inactive camera rows
    if case == 3:
        assert not dead[6 * bl[3].shape[0]:].any()      # FULL_OPENCV: none
    ba.close()


def line_scene(I, P, seed):
    """I images 0.1 m apart looking along +z, image 0 with a constant pose, P points in front of all of them and seen by
    every image: every slot row of S holds ns = I - 1 blocks"""
    rng = np.random.default_rng(seed)
    poses = np.zeros((I, 7))
    poses[:, 0] = 1.0
    poses[:, 4] = -0.1 * np.arange(I)
    points = np.stack([rng.uniform(-3, 9, P), rng.uniform(-2, 2, P), rng.uniform(6, 20, P)], axis=1)
    obs_image = np.tile(np.arange(I), P).astype(np.int32)
    obs_point = np.repeat(np.arange(P), I).astype(np.int32)
    Pc = points[obs_point] + poses[obs_image, 4:]
    x, y = synth._opencv_project(synth.OPENCV_PARAMS, Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2])
    obs_xy = np.stack([x, y], axis=1) + rng.uniform(-2, 2, (obs_image.size, 2))
    poses[:, 1:4] = rng.normal(0, 0.004, (I, 3))
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    poses[:, 4:] += rng.normal(0, 0.02, (I, 3))
    const = np.zeros(I, np.uint8)
    const[0] = 1
    return dict(cam_model=np.array([4], np.int32), cam_params_list=[synth.OPENCV_PARAMS], poses=poses,
                image_camera=np.zeros(I, np.int32), points=points, obs_image=obs_image, obs_point=obs_point, obs_xy=obs_xy,
                image_const_pose=const)


@pytest.mark.parametrize("precond", ["identity", "schur_jacobi"])
@pytest.mark.parametrize("shape", ["no_slots", "const_pose_image", "eight_cameras", "row_of_65", "slots_257", "fallback"])
def test_shapes(gpu, oracle, shape, precond):
    mode, mu = "marquardt", 1e-4
    if shape == "no_slots":                 # every pose constant: the system is S_cam alone
        s = cref.camera_scene(oracle, [4, 2], 81)
        s["image_const_pose"][:] = 1
        refine = cref.refine_mask(s)
    elif shape == "const_pose_image":       # image 0 is constant, its camera refined: no slot, but it feeds S_cam
        s = ref.shared_launch_scene()
        refine = cref.refine_mask(s, None, (0, 1))
    elif shape == "eight_cameras":          # 16 images dealt out in pairs over 8 PINHOLE cameras
        s = cref.camera_scene(oracle, [1] * 8, 33, I=16, P=150)
        refine = cref.refine_mask(s)
    elif shape == "row_of_65":
        s = line_scene(66, 40, 5)
        refine = cref.refine_mask(s)
    elif shape == "slots_257":              # tracks of at most 3 images: a narrow co-visibility window
        s = synth.ba_scene(257, 1500, seed=17, max_track=3, lidar_frac=0.5)
        refine = cref.refine_mask(s, None, (0, 1))
    else:
        s, refine = unused_camera_scene(oracle)
        mode, mu = "levenberg", 0.0
    ba, bl, dead = _handle(gpu, s, refine, mu, mode)
    ns, ncs = bl[3].shape[0], bl[6].shape[0]
    print(f"{shape}: ns {ns} ncs {ncs} pairs {bl[2].shape[0]}")
    got, want = _parity(ba, bl, dead, precond, shape)
    assert (ns, ncs) == {"no_slots": (0, 2), "const_pose_image": (2, 1), "eight_cameras": (ns, 8), "row_of_65": (65, 1),
                         "slots_257": (257, 1), "fallback": (ns, 2)}[shape]
    if shape == "row_of_65":
        assert bl[2].shape[0] == 65 * 64 // 2
    if shape == "fallback":
        assert got["precond_fallbacks"] == (1 if precond == "schur_jacobi" else 0) and not got["x"][6 * ns + S12:].any()
    ba.close()


@pytest.mark.parametrize("case", range(len(cref.CAM_CASES)))
def test_tight_solve_matches_the_direct_solve(gpu, oracle, case):
    """the same handle state solved twice; then back-substitution and model decrease from both steps.  Tolerance of
    test_ba_pcg_gpu.test_tight_step_matches_dense_solve (1e-8 relative, floor 1e-8 x the group's scale), per group"""
    s, refine = cref.cam_case_scene(oracle, case)
    for mode, mu in [d for d in cref.DAMPINGS if d[0] in cref.WELL_CONDITIONED]:
        ba, bl, dead = _handle(gpu, s, refine, mu, mode)
        ns = bl[3].shape[0]
        x, info = ba.schur_cam_solve_pcg(max_iterations=500, **TIGHT)
        x = x.clone()
        assert info["termination"] == gpu.PCG_R_TOLERANCE and info["precond_fallbacks"] == 0
        xc, ci = ba.schur_cam_solve_cholesky()
        assert ci["status"] == gpu.CHOL_OK
        true = pc.true_residual(bl, x.cpu().numpy())
        print(f"case {case}: {info['iterations']} iterations, true residual {true:.3e}")
        dp, mdp = ba.back_substitute_cam(x)
        dp, mdp = dp.clone(), mdp.clone()
        dc, mdc = ba.back_substitute_cam(xc)
        a, b = x.cpu().numpy(), xc.cpu().numpy()
        for u, v, what in ((a[:6 * ns], b[:6 * ns], "pose step"), (a[6 * ns:], b[6 * ns:], "camera step"),
                           (dp.cpu().numpy(), dc.cpu().numpy(), "point step"),
                           (mdp.cpu().numpy(), mdc.cpu().numpy(), "model decrease")):
            scale = max(1.0, float(np.abs(v).max()))
            np.testing.assert_allclose(u, v, rtol=1e-8, atol=1e-8 * scale, err_msg=what)
        assert not a[dead].any()
        ba.close()


def test_bitwise_repeatable(gpu, oracle):
    s, refine = cref.cam_case_scene(oracle, 4)
    ba, _, _ = _handle(gpu, s, refine, 1e-4)
    for o in (FIXED8, dict(max_iterations=500, **TIGHT), dict()):
        xa, ia = ba.schur_cam_solve_pcg(**o)
        xa = xa.clone()
        xb, ib = ba.schur_cam_solve_pcg(**o)
        assert torch.equal(xa, xb) and ia == ib
        ba.schur_cam(1e-4, want=("cost", "num_skipped"))
        xc, ic = ba.schur_cam_solve_pcg(**o)
        assert torch.equal(xa, xc) and ia == ic
        xh, ih = ba.schur_cam_solve_pcg_host(**o)
        assert np.array_equal(xa.cpu().numpy(), xh) and ia == ih
    ba.close()


def test_without_camera_slots_it_is_the_plain_pcg(gpu, oracle):
    s = ref.camera_scene(oracle, [4, 2], 91)
    a, b = gpu.BA(**s), gpu.BA(**s)
    assert b.camera_slots()["num_slots"] == 0
    a.schur(1e-4, want=("cost", "num_skipped")); b.schur_cam(1e-4, want=("cost", "num_skipped"))
    for o in (FIXED8, dict(), dict(preconditioner="identity", max_iterations=300, **TIGHT)):
        xa, ia = a.schur_solve_pcg(**o)
        xb, ib = b.schur_cam_solve_pcg(**o)
        assert ia == ib and ia["iterations"] > 0 and torch.equal(xa.reshape(-1), xb)
        xh, ih = b.schur_cam_solve_pcg_host(**o)
        assert ih == ia and np.array_equal(xh, xa.cpu().numpy().reshape(-1))
    sa, ha = gpu.ba_solve(a, max_num_iterations=3)
    sb, hb = gpu.ba_solve(b, max_num_iterations=3, linear_solver="pcg_cam", refine_intrinsics=True)
    assert ha == hb and sa["final_cost"] == sb["final_cost"]
    a.close(); b.close()


# ---- the LM loop ------------------------------------------------------------------------------------------------------
def test_lm_matches_numpy_lm(gpu, oracle):
    """pcd_ba_solve(PCD_LINEAR_PCG_CAM, refine_intrinsics) at the default PCG options against lm_cam_pcg; the margins of
    the reference (tests/test_ba_pcg_cam_cpu.py: rho 0.61 from min_relative_decrease, zeta 0.0278 from q_tolerance) are
    asserted first, so rounding cannot decide an accept or an iteration count"""
    s, refine = lm_scene(oracle)
    want, final = pc.lm_cam_pcg(oracle, s, refine, 6)
    assert min(abs(w["rho"] - 1e-3) for w in want) > 0.5
    assert min(abs(z - 0.1) for w in want for z in w["zetas"]) > 0.02
    assert "".join("T" if w["accepted"] else "F" for w in want) == "TTFTTT"
    ba = gpu.BA(**s, camera_refine=refine)
    summary, got = gpu.ba_solve(ba, max_num_iterations=6, linear_solver="pcg_cam", refine_intrinsics=True)
    print(summary, [(g["accepted"], g["linear_iterations"], g["cost"]) for g in got])
    assert summary["num_iterations"] == 6
    assert [g["accepted"] for g in got] == [w["accepted"] for w in want]
    assert [g["linear_iterations"] for g in got] == [w["linear_iterations"] for w in want]
    for g, w in zip(got, want):
        assert g["linear_termination"] == w["linear_termination"] == gpu.PCG_Q_TOLERANCE
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["candidate_cost"], w["candidate_cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
    np.testing.assert_allclose(summary["final_cost"], oracle.BA(**final).normal_equations()[0], rtol=1e-8)
    cams = ba.get_camera_parameters()
    np.testing.assert_allclose(cams, final["cam_params_list"][0], rtol=1e-8)
    ba.close()


def test_tight_pcg_lm_is_the_cholesky_lm(gpu, oracle):
    s, refine = lm_scene(oracle)
    a, b = gpu.BA(**s, camera_refine=refine), gpu.BA(**s, camera_refine=refine)
    sa, ha = gpu.ba_solve(a, max_num_iterations=6, linear_solver="pcg_cam", refine_intrinsics=True,
                          linear=dict(max_iterations=500, **TIGHT))
    sb, hb = gpu.ba_solve(b, max_num_iterations=6, linear_solver="cholesky", refine_intrinsics=True)
    print([(g["accepted"], g["linear_iterations"]) for g in ha])
    assert [g["accepted"] for g in ha] == [g["accepted"] for g in hb] and sa["num_accepted"] >= 1
    for g, w in zip(ha, hb):
        assert g["linear_termination"] == gpu.PCG_R_TOLERANCE and g["linear_iterations"] > 8      # more than one batch
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
    np.testing.assert_allclose(sa["final_cost"], sb["final_cost"], rtol=1e-8)
    a.close(); b.close()


def test_refined_parameters_move_and_constant_ones_do_not(gpu, oracle):
    s, _ = lm_scene(oracle)
    refine = cref.refine_mask(s, None, (0, 1))
    cp = np.asarray(s["cam_params_list"][0], np.float64)
    ba = gpu.BA(**s, camera_refine=refine)
    summary, _ = gpu.ba_solve(ba, max_num_iterations=4, linear_solver="pcg_cam", refine_intrinsics=True)
    cams = ba.get_camera_parameters()
    assert summary["num_accepted"] >= 1 and np.all(cams[:2] != cp[:2]) and np.array_equal(cams[2:], cp[2:])
    assert np.abs(cams[:2] / (cp[:2] / 1.02) - 1).max() < 5e-3       # towards the true focal length
    poses, _ = ba.get_parameters()
    const = np.asarray(s["image_const_pose"]) == 1
    assert const.any() and np.array_equal(poses[const], np.asarray(s["poses"])[const])
    ba.close()


# ---- guards -----------------------------------------------------------------------------------------------------------
def test_guards(gpu, oracle):
    s, refine = cref.cam_case_scene(oracle, 0)
    ba = gpu.BA(**s, camera_refine=refine)
    for call in (ba.schur_cam_solve_pcg, ba.schur_cam_solve_pcg_host):
        with pytest.raises(gpu.PcdError) as e:                 # no _cam Schur call yet
            call()
        assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    with pytest.raises(gpu.PcdError) as e:                     # the plain call is refused on a refined handle ...
        ba.schur(1e-4)
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    with pytest.raises(gpu.PcdError) as e:                     # ... and leaves nothing to solve from
        ba.schur_cam_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID
    ba.schur_cam(1e-4, want=("cost", "S_diag"))                # S_diag went to caller memory
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_cam_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "S_diag" in str(e.value)
    ba.schur_cam(1e-4, want=("cost",))
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_cam_solve_pcg(preconditioner=7)
    assert e.value.status == gpu.PCD_ERR_INVALID
    x, info = ba.schur_cam_solve_pcg()
    assert info["iterations"] > 0 and np.isfinite(x.cpu().numpy()).all()
    with pytest.raises(gpu.PcdError) as e:                     # the pose-only PCG still refuses camera rows
        gpu.ba_solve(ba, max_num_iterations=2, refine_intrinsics=True)
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "PCD_LINEAR_CHOLESKY" in str(e.value)
    with pytest.raises(gpu.PcdError) as e:
        gpu.ba_solve(ba, max_num_iterations=2, refine_intrinsics=True, linear_solver=7)
    assert e.value.status == gpu.PCD_ERR_INVALID
    summary, _ = gpu.ba_solve(ba, max_num_iterations=2, linear_solver="pcg_cam", refine_intrinsics=True)
    assert summary["num_iterations"] == 2
    with pytest.raises(gpu.PcdError) as e:                     # the loop has moved on from its last Schur state
        ba.schur_cam_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID
    ba.close()
    s9 = ref.camera_scene(oracle, [1] * 9, 33, I=9, P=60)     # nine slots: more than the bordered system carries
    ba = gpu.BA(**s9, camera_refine=cref.refine_mask(s9, None, (0, 1)))
    for call in (ba.schur_cam_solve_pcg, ba.schur_cam_solve_pcg_host,
                 lambda: gpu.ba_solve(ba, linear_solver="pcg_cam", refine_intrinsics=True)):
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "PCD_BA_MAX_CAMERA_SLOTS" in str(e.value)
    assert np.isfinite(ba.evaluate(("cost",))["cost"][0])     # the handle is usable afterwards
    ba.close()


def test_capture_refused_then_eager_works(gpu, oracle):
    s, refine = cref.cam_case_scene(oracle, 1)
    ba = gpu.BA(**s, camera_refine=refine)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ba.schur_cam(1e-3, want=("cost", "num_skipped"))
        x0, i0 = ba.schur_cam_solve_pcg()
        x0 = x0.clone()
        buf = torch.empty_like(x0)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                ba.schur_cam_solve_pcg(delta=buf)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
        x1, i1 = ba.schur_cam_solve_pcg()
        side.synchronize()
        assert torch.equal(x1, x0) and i1 == i0 and i0["iterations"] > 0
    ba.close()

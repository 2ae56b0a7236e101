"""GPU parity of the reduced solve (pcd_ba_schur_solve_pcg*, pcd_ba_get_parameters, pcd_ba_solve) against
the numpy PCG / LM of tests/ba_pcg_ref.py.

Fixed-iteration parity.  The bound is the reference's own sensitivity to the order of the sums: the numpy PCG with
the rows added in ascending and in descending partner order, 8 iterations with the tolerances off, both
preconditioners, on the ten scene shapes of CASES with the oracle's blocks.  Relative differences as _rel() defines
them: x by max |dx| / max |x|, Q by |dQ| / |Q|, ||r|| by |d||r||| / ||rhs|| (||r|| is a sum of rounding errors once a
six-image system has converged inside the 8 iterations -- down to 1e-107 ||rhs|| with block-Jacobi on the cases whose
images share no point -- so its own size is no scale; ||rhs|| is).  Largest value measured: 5.4345e-13 (x, case 4,
block-Jacobi); most of these small systems have at most two blocks per row and show no difference at all.
PARITY_BOUND = 100 x 5.4345e-13 = 5.4345e-11 for device against reference.

The device is compared with ba_pcg_ref.pcg_device_order: the same algorithm with every sum in the order csrc/ba_pcg.hip
states (as ba_schur_ref.point_inverse follows k_schur_points).  With pcg(), whose sums round in the order numpy and
its BLAS choose, the check cannot be met by any implementation: on these systems (cond(S) 1e7 ... 1e19) pcg() and
pcg_device_order() -- two roundings of the same arithmetic on the CPU alone -- differ in x by up to 7.3e-10 with the
tolerances off (case 2, identity; 7.0e-11 on case 1, identity, where the device stood 1.0e-10 from pcg()) and by
8.7e-8 on case 7 with block-Jacobi, while Q and ||r|| agree to 1e-14.  The row-order switch does not show this
because a row of these systems rarely has more than two blocks.  tests/test_ba_pcg_cpu.py::test_reference_roundings_agree holds the
two references together where rounding is not amplified.

The true-residual and x.r bounds are the ones tests/test_ba_pcg_cpu.py records.  Every bound here comes from the
reference alone; the device's own figures (each test prints them before it asserts) have not been recorded yet."""
import os
import subprocess

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_pcg_ref as pr
from tests import ba_schur_ref as ref
from tests.test_ba_pcg_cpu import SCENES, TRUE_RESIDUAL_BOUND, XR_BOUND_TIGHT, table_scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PARITY_BOUND = 5.4345e-11        # 100 x 5.4345e-13, see above

CASES = [  # (loss, order, lidar, const, mode, mu, well conditioned): tests/test_ba_schur_gpu.py's
    (0, "point", True, True, "marquardt", 1e-4, True),
    (1, "point", True, True, "marquardt", 1e-4, True),
    (2, "image", True, True, "marquardt", 1e-4, True),
    (0, "image", False, True, "marquardt", 1.0, True),
    (1, "point", True, False, "levenberg", 1.0, False),
    (2, "point", True, True, "levenberg", 1e-4, False),
    (0, "image", True, True, "marquardt", 0.0, False),
    (0, "point", True, True, "levenberg", 0.0, False),
    (0, "point", True, True, "marquardt", 1.0, True),
    (2, "image", True, True, "levenberg", 1.0, False),
]


def _scene(seed, I=6, P=150, order="point", loss=0, lidar=True, const=True, tvec=True):
    s = synth.ba_scene(I, P, seed=seed, const_pose_frac=0.3 if const else 0.0, order=order,
                       lidar_frac=1.0 if lidar else 0.0)
    if not lidar:
        for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
            s.pop(k)
    rng = np.random.default_rng(seed)
    if tvec:
        s["image_const_tvec"] = (rng.integers(1, 8, I) * (rng.random(I) < 0.4)).astype(np.uint8)
    if const:
        s["point_const"] = (rng.random(P) < 0.1).astype(np.uint8)
        s["image_const_pose"][0] = 1
    s["loss_type"], s["loss_scale"] = loss, 2.0
    return s


def _case_scene(case):
    loss, order, lidar, const, mode, mu, wc = CASES[case]
    return _scene(30 + case, order=order, loss=loss, lidar=lidar, const=const), mode, mu, wc


def _lm_scene():
    s = synth.ba_scene(12, 3000, seed=5, const_pose_frac=0.25)
    rng = np.random.default_rng(1005)
    s["points"] = s["points"] + rng.normal(0, 0.05, s["points"].shape)
    return s


def _blocks(ba, mu, mode="marquardt"):
    """the device's own blocks, downloaded (a first Schur call into caller memory), then the same call once more with
    the blocks left in the handle, which is the state the solver reads; the two calls are bitwise identical"""
    out = ba.schur(mu, damping=mode)
    st = ba.schur_structure()
    res = (out["S_diag"].cpu().numpy(), out["S_off"].cpu().numpy(), st["pairs"].astype(np.int64),
           out["rhs"].cpu().numpy())
    ba.schur(mu, damping=mode, want=("cost", "num_skipped"))
    return res


def _rel(got, want, rhs_norm):
    dx = np.abs(got["x"] - want["x"]).max() / max(np.abs(want["x"]).max(), 1e-300)
    dq = abs(got["q"] - want["q"]) / max(abs(want["q"]), 1e-300)
    dr = abs(got["residual_norm"] - want["residual_norm"]) / rhs_norm
    return dx, dq, dr


def _solve(ba, **opts):
    x, info = ba.schur_solve_pcg(**opts)
    return dict(info, x=x.cpu().numpy())


def test_reference_order_sensitivity(oracle):
    """the measurement PARITY_BOUND comes from, repeated: ascending against descending row order"""
    worst = 0.0
    for case in range(len(CASES)):
        s, mode, mu, _ = _case_scene(case)
        bl = pr.block_lists(ref.NormalEquations(oracle, s, mu, mode).schur_blocks())
        for pc in (pr.IDENTITY, pr.SCHUR_JACOBI):
            o = dict(q_tolerance=-1.0, r_tolerance=-1.0, max_iterations=8, preconditioner=pc)
            a, d = pr.pcg(*bl, **o), pr.pcg(*bl, descending=True, **o)
            worst = max(worst, *_rel(d, a, a["rhs_norm"]))
    print(f"largest ascending / descending difference {worst:.3e}")
    assert 0.0 < worst <= PARITY_BOUND / 100


@pytest.mark.parametrize("precond", ["identity", "schur_jacobi"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_fixed_iteration_parity(gpu, case, precond):
    s, mode, mu, _ = _case_scene(case)
    ba = gpu.BA(**s)
    bl = _blocks(ba, mu, mode)
    got = _solve(ba, max_iterations=8, q_tolerance=-1.0, r_tolerance=-1.0, preconditioner=precond)
    want = pr.pcg_device_order(*bl, max_iterations=8, q_tolerance=-1.0, r_tolerance=-1.0,
                               preconditioner=pr.SCHUR_JACOBI if precond == "schur_jacobi" else pr.IDENTITY)
    dx, dq, dr = _rel(got, want, want["rhs_norm"])
    print(f"case {case} {precond}: device {got['iterations']} its term {got['termination']}, reference "
          f"{want['iterations']} its term {want['termination']}; dx {dx:.3e} dQ {dq:.3e} d|r| {dr:.3e}")
    np.testing.assert_allclose(got["rhs_norm"], want["rhs_norm"], rtol=1e-14)
    assert got["precond_fallbacks"] == want["precond_fallbacks"]
    assert max(dx, dq, dr) <= PARITY_BOUND, (dx, dq, dr)
    pr_ = ref.problem(s)
    assert not got["x"][~pr_["active"]].any()           # constant-tvec coordinates: exactly 0
    ba.close()


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_stopping_rule(gpu, k):
    """at the defaults device and reference stop at the same iteration for the same reason; the reference's zeta_k keep
    their distance from q_tolerance, so rounding cannot decide (12-image scene: mu 1e-2, at 1e-4 one sits at 0.002)"""
    s = table_scene(k)
    ba = gpu.BA(**s)
    for mu in ((1e-2,) if k == 0 else (1e-4, 1e-2)):
        bl = _blocks(ba, mu)
        want = pr.pcg(*bl)
        got = _solve(ba)
        margin = min(abs(z - 0.1) for z in want["zetas"])
        print(f"scene {SCENES[k][0]} mu {mu}: {want['iterations']} iterations, nearest zeta {margin:.4f} from q_tolerance")
        assert margin > 0.005
        assert (got["iterations"], got["termination"]) == (want["iterations"], want["termination"])
        assert want["termination"] == pr.Q_TOLERANCE
        np.testing.assert_allclose(got["x"], want["x"], rtol=0, atol=1e-9 * np.abs(want["x"]).max())
        np.testing.assert_allclose(got["q"], want["q"], rtol=1e-9)
    ba.close()


@pytest.mark.parametrize("k", range(len(SCENES)))
@pytest.mark.parametrize("mu", [1e-4, 1e-2])
def test_tight_solve(gpu, k, mu):
    s = table_scene(k)
    ba = gpu.BA(**s)
    Sd, So, pairs, rhs = _blocks(ba, mu)
    got = _solve(ba, r_tolerance=1e-12, q_tolerance=-1.0, max_iterations=2000)
    assert got["termination"] == gpu.PCG_R_TOLERANCE
    assert got["residual_norm"] <= 1e-12 * got["rhs_norm"]
    true = pr.true_residual(Sd, So, pairs, rhs, got["x"])
    xr = abs(got["step_dot_residual"]) / (np.linalg.norm(got["x"]) * got["residual_norm"])
    print(f"scene {SCENES[k][0]} mu {mu}: {got['iterations']} iterations, true residual {true:.3e}, x.r {xr:.3e}")
    assert true <= TRUE_RESIDUAL_BOUND
    assert xr <= XR_BOUND_TIGHT
    assert got["precond_fallbacks"] == 0
    ba.close()


@pytest.mark.parametrize("case", [c for c in range(len(CASES)) if CASES[c][6]])
def test_tight_step_matches_dense_solve(gpu, oracle, case):
    """tight PCG, then the GPU back-substitution of that dpose, against the dense solve of the whole damped system
    (the bound tests/test_ba_schur_gpu.py applies to the numpy solve of the same well-conditioned systems)"""
    s, mode, mu, _ = _case_scene(case)
    ba = gpu.BA(**s)
    ba.schur(mu, damping=mode, want=("cost", "num_skipped"))
    x, info = ba.schur_solve_pcg(r_tolerance=1e-12, q_tolerance=-1.0, max_iterations=200)
    assert info["termination"] == gpu.PCG_R_TOLERANCE
    dpoint, _ = ba.back_substitute(x)
    ne = ref.NormalEquations(oracle, s, mu, mode)
    dp_ref, dx_ref = ne.dense_solve()
    for a, b, what in ((x.cpu().numpy(), dp_ref, "pose step"), (dpoint.cpu().numpy(), dx_ref, "point step")):
        scale = max(1.0, float(np.abs(b).max()))
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-8 * scale, err_msg=what)
    ba.close()


def test_no_slots(gpu):
    s = _scene(41)
    s["image_const_pose"][:] = 1
    ba = gpu.BA(**s)
    ba.schur(1e-3, want=("cost", "num_skipped"))
    x, info = ba.schur_solve_pcg()
    assert x.shape == (0, 6) and info["iterations"] == 0 and info["termination"] == gpu.PCG_ZERO_RHS
    xh, ih = ba.schur_solve_pcg_host()
    assert xh.shape == (0, 6) and ih["iterations"] == 0
    ba.close()


def test_zero_rhs(gpu):
    """every observation on constant-pose images, three variable-pose images without observations, Levenberg damping:
    S = mu I and rhs = 0 exactly"""
    s = _scene(43, tvec=False)
    I = s["poses"].shape[0]
    s["image_const_pose"][:] = 1
    s["poses"] = np.concatenate([s["poses"], s["poses"][:3]])
    s["image_camera"] = np.concatenate([s["image_camera"], s["image_camera"][:3]]).astype(np.int32)
    s["image_const_pose"] = np.concatenate([s["image_const_pose"], [0, 0, 0]]).astype(np.uint8)
    s["image_const_tvec"] = np.zeros(I + 3, np.uint8)
    ba = gpu.BA(**s)
    out = ba.schur(0.5, damping="levenberg")
    assert np.array_equal(out["S_diag"].cpu().numpy(), np.tile(0.5 * np.eye(6), (3, 1, 1)))
    assert not out["rhs"].cpu().numpy().any()
    ba.schur(0.5, damping="levenberg", want=("cost", "num_skipped"))
    x, info = ba.schur_solve_pcg()
    assert info["termination"] == gpu.PCG_ZERO_RHS and info["iterations"] == 0 and info["rhs_norm"] == 0.0
    assert x.shape == (3, 6) and not x.cpu().numpy().any()
    ba.close()


def test_state_guards(gpu):
    s = _scene(17)
    ba = gpu.BA(**s)
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    ba.schur(1e-3, want=("cost", "S_diag", "num_skipped"))          # S_diag went to caller memory
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "S_diag" in str(e.value) and "S_off" not in str(e.value)
    ba.schur(1e-3, want=("cost", "num_skipped"))
    _, info = ba.schur_solve_pcg()
    assert info["iterations"] > 0
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_solve_pcg(preconditioner=7)
    assert e.value.status == gpu.PCD_ERR_INVALID
    ba.close()
    s["camera_refine"] = gpu.camera_refine_mask(s["cam_model"], True, False, False)
    ba = gpu.BA(**s)
    for call in (lambda: ba.schur_solve_pcg(dpose=torch.zeros((6, 6), dtype=torch.float64, device="cuda")),
                 lambda: ba.schur_solve_pcg_host(), lambda: gpu.ba_solve(ba)):
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    ba.close()


def test_capture_refused_then_eager_works(gpu):
    s = _scene(19)
    ba = gpu.BA(**s)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ba.schur(1e-3, want=("cost", "num_skipped"))
        x0, i0 = ba.schur_solve_pcg()
        x0 = x0.clone()
        buf = torch.empty_like(x0)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                ba.schur_solve_pcg(dpose=buf)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
        x1, i1 = ba.schur_solve_pcg()
        side.synchronize()
        assert torch.equal(x1, x0) and i1 == i0
    ba.close()


def test_bitwise_repeatable(gpu):
    s = table_scene(0)
    ba = gpu.BA(**s)
    ba.schur(1e-3, want=("cost", "num_skipped"))
    a, ia = ba.schur_solve_pcg(r_tolerance=1e-10, q_tolerance=-1.0)
    a = a.clone()
    b, ib = ba.schur_solve_pcg(r_tolerance=1e-10, q_tolerance=-1.0)
    assert torch.equal(a, b) and ia == ib and ia["iterations"] > 8
    ba.schur(1e-3, want=("cost", "num_skipped"))
    c, ic = ba.schur_solve_pcg(r_tolerance=1e-10, q_tolerance=-1.0)
    assert torch.equal(a, c) and ia == ic
    xh, ih = ba.schur_solve_pcg_host(r_tolerance=1e-10, q_tolerance=-1.0)
    assert np.array_equal(xh, a.cpu().numpy()) and ih == ia
    assert ba.schur_stats()["scratch_bytes"] > 0
    ba.close()


def _check_lm(got, want):
    assert [r["accepted"] for r in got] == [r["accepted"] for r in want]
    assert [r["linear_iterations"] for r in got] == [r["linear_iterations"] for r in want]
    for g, w in zip(got, want):
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
    costs = [r["cost"] for r in got]
    assert all(b <= a for a, b in zip(costs, costs[1:]))


def test_lm_matches_numpy_lm(gpu, oracle):
    """pcd_ba_solve and ba_solve_lm(linear_solver="pcg") at the PCG defaults against the same loop on the oracle"""
    s = _lm_scene()
    want, final = pr.lm_pcg(oracle, s, 8)
    rho_margin = min(abs(r["rho"] - 1e-3) for r in want)
    zeta_margin = min(abs(z - 0.1) for r in want for z in r["zetas"])
    print("accepted", "".join("T" if r["accepted"] else "F" for r in want), "linear iterations",
          [r["linear_iterations"] for r in want], f"rho margin {rho_margin:.3f} zeta margin {zeta_margin:.2e}")
    assert rho_margin > 0.05 and zeta_margin > 1e-4
    assert any(r["accepted"] for r in want) and not all(r["accepted"] for r in want)
    cost_final = oracle.BA(**final).normal_equations()[0]

    ba = gpu.BA(**s)
    summary, got = gpu.ba_solve(ba, max_num_iterations=8)
    assert summary["num_iterations"] == 8 and summary["termination"] == gpu.SOLVE_MAX_ITERATIONS
    assert summary["num_accepted"] == sum(r["accepted"] for r in want)
    _check_lm(got, want)
    poses, points = ba.get_parameters()
    np.testing.assert_allclose(oracle.BA(**dict(s, poses=poses, points=points)).normal_equations()[0], cost_final, rtol=1e-8)
    np.testing.assert_allclose(summary["final_cost"], cost_final, rtol=1e-8)
    np.testing.assert_allclose(summary["initial_cost"], want[0]["cost"], rtol=1e-8)
    assert np.array_equal(ba.evaluate(("cost",))["cost"][0] < got[0]["cost"], True)
    cpose = np.flatnonzero(s["image_const_pose"])
    assert np.array_equal(poses[cpose], np.asarray(s["poses"])[cpose])
    assert all(r["gradient_max_norm"] > 0 for r in got) and summary["linear_solver_ms"] > 0
    ba.close()

    ba = gpu.BA(**s)
    got = gpu.ba_solve_lm(ba, max_iterations=8, linear_solver="pcg")
    _check_lm(got, want)
    poses, points = ba.get_parameters()
    np.testing.assert_allclose(oracle.BA(**dict(s, poses=poses, points=points)).normal_equations()[0], cost_final, rtol=1e-8)
    ba.close()


def test_lm_tight_pcg_matches_cholesky(gpu):
    """r_tolerance 1e-12 with the Q test off: the PCG steps are the Cholesky steps, so accept sequence, costs and radii
    equal the dense route's within the tolerances of test_solve_lm_matches_numpy_lm"""
    s = _lm_scene()
    ba = gpu.BA(**s)
    want = gpu.ba_solve_lm(ba, max_iterations=8)
    ba.close()
    tight = dict(r_tolerance=1e-12, q_tolerance=-1.0)
    for run in ("library", "python"):
        ba = gpu.BA(**s)
        if run == "library":
            _, got = gpu.ba_solve(ba, max_num_iterations=8, linear=tight)
        else:
            got = gpu.ba_solve_lm(ba, max_iterations=8, linear_solver="pcg", pcg=tight)
        assert [r["accepted"] for r in got] == [r["accepted"] for r in want], run
        assert all(r["linear_termination"] == gpu.PCG_R_TOLERANCE for r in got)
        assert max(r["linear_iterations"] for r in got) > 8          # past the first batch
        for g, w in zip(got, want):
            np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
            np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
        ba.close()


def test_solve_stopping_tests(gpu):
    s = _lm_scene()
    ba = gpu.BA(**s)
    summary, got = gpu.ba_solve(ba, max_num_iterations=8, function_tolerance=0.9)
    assert summary["termination"] == gpu.SOLVE_FUNCTION_TOLERANCE and summary["num_iterations"] == len(got) < 8
    assert got[-1]["accepted"] and abs(got[-1]["cost"] - got[-1]["candidate_cost"]) <= 0.9 * got[-1]["cost"]
    p0, x0 = ba.get_parameters()
    summary, got = gpu.ba_solve(ba, max_num_iterations=8, gradient_tolerance=1e300)
    assert summary["termination"] == gpu.SOLVE_GRADIENT_TOLERANCE and summary["num_iterations"] == 0
    p1, x1 = ba.get_parameters()
    assert np.array_equal(p0, p1) and np.array_equal(x0, x1)
    summary, got = gpu.ba_solve(ba, max_num_iterations=8, initial_radius=1e-3, min_radius=1.0)
    assert summary["termination"] == gpu.SOLVE_MIN_RADIUS and summary["num_iterations"] == 0
    ba.close()


def test_config_b_sized_solve(gpu):
    """450 images / 400 k points: PCG to r_tolerance 1e-10, the true residual by a numpy block product over the
    downloaded blocks (no dense S)"""
    s = synth.ba_scene(450, 400_000, seed=23, const_pose_frac=0.1, order="image")
    ba = gpu.BA(**s)
    Sd, So, pairs, rhs = _blocks(ba, 1e-4)
    got = _solve(ba, r_tolerance=1e-10, q_tolerance=-1.0, max_iterations=2000)
    assert got["termination"] == gpu.PCG_R_TOLERANCE and got["residual_norm"] <= 1e-10 * got["rhs_norm"]
    true = pr.true_residual(Sd, So, pairs, rhs, got["x"])
    print(f"{Sd.shape[0]} slots, {len(pairs)} pairs: {got['iterations']} iterations, true residual {true:.3e}")
    assert true <= 1e-9          # 10 x the tolerance asked for: the drift of the recurrence, as in the CPU test
    ba.close()


def test_above_the_dense_switch(gpu):
    """1500 images (the reference goes iterative above 1000; the dense S would be 648 MB): three LM iterations"""
    s = synth.ba_scene(1500, 150_000, seed=29, const_pose_frac=0.05, order="image")
    s["points"] = s["points"] + np.random.default_rng(1029).normal(0, 0.05, s["points"].shape)
    ba = gpu.BA(**s)
    summary, got = gpu.ba_solve(ba, max_num_iterations=3)
    print(summary, [(r["accepted"], r["linear_iterations"], r["cost"]) for r in got])
    assert summary["num_iterations"] == 3 and summary["num_accepted"] >= 1
    assert summary["final_cost"] < summary["initial_cost"]
    assert ba.evaluate(("cost",))["cost"][0] < got[0]["cost"]
    ba.close()


def test_shim_solve(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_solve"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_solve"), "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout

"""CPU checks of the reduced solve: the numpy PCG of tests/ba_pcg_ref.py on the oracle's own reduced
systems, and the ABI surface of pcd_ba_schur_solve_pcg* / pcd_ba_get_parameters / pcd_ba_solve.

Measured with the reference on the six systems below (scene x mu; SCHUR_JACOBI, r_tolerance 1e-12, q_tolerance off):

  scene (images, points, seed, const_pose_frac)  mu     iterations  true residual  |x.r|/(|x||r|) at 3 its   at the end
  12, 3000, 5, 0.25                              1e-4   36          5.72e-13       2.9e-15                   1.4e-10
                                                 1e-2   26          5.33e-13       1.5e-16                   5.7e-13
  40, 6000, 9, 0.1                               1e-4   51          8.80e-13       1.4e-17                   2.0e-05
                                                 1e-2   41          6.49e-13       1.4e-17                   9.1e-09
  80, 8000, 3, 0.0                               1e-4   68          9.12e-13       3.1e-14                   1.9e-05
                                                 1e-2   46          9.79e-13       2.4e-18                   3.2e-15

True residual ||rhs - S x|| / ||rhs|| with the dense S: largest 9.79e-13, bound TRUE_RESIDUAL_BOUND = 1e-11 (10 x: the
recurrence residual, which the stopping test sees, drifts from the true one by rounding that grows with the iteration
count).  x.r: for CG from x = 0 the residual is orthogonal to the iterate up to rounding.  After 3 iterations (the
inexact step of the LM loop) the largest normalised value is 3.1e-14, bound XR_BOUND_INEXACT = 3.1e-13.  At the end of
a tight solve ||r|| is 1e-12 ||rhs||, so the same rounding in x.r is a far larger fraction of |x||r|: largest 2.0e-05,
bound XR_BOUND_TIGHT = 2e-4.  The identity preconditioner needs 845 / 366 iterations on the 12-image scene and does
not converge in 2000 on the others."""
import ctypes as C

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_pcg_ref as pr
from tests import ba_schur_ref as ref

TRUE_RESIDUAL_BOUND = 1e-11      # 10 x 9.79e-13, see above
XR_BOUND_INEXACT = 3.1e-13       # 10 x 3.1e-14
XR_BOUND_TIGHT = 2e-4            # 10 x 2.0e-05

SCENES = [(12, 3000, 5, 0.25), (40, 6000, 9, 0.1), (80, 8000, 3, 0.0)]
MUS = (1e-4, 1e-2)
JACOBI_ITERATIONS = {(12, 1e-4): 36, (12, 1e-2): 26, (40, 1e-4): 51, (40, 1e-2): 41, (80, 1e-4): 68, (80, 1e-2): 46}


def table_scene(k):
    I, P, seed, frac = SCENES[k]
    s = synth.ba_scene(I, P, seed=seed, const_pose_frac=frac)
    s["points"] = s["points"] + np.random.default_rng(1000 + seed).normal(0, 0.05, s["points"].shape)
    return s


@pytest.fixture(scope="module")
def systems(oracle):
    out = {}
    for k in range(len(SCENES)):
        s = table_scene(k)
        for mu in MUS:
            ne = ref.NormalEquations(oracle, s, mu)
            out[(k, mu)] = (ne, ne.schur_blocks())
    return out


@pytest.mark.parametrize("k", range(len(SCENES)))
@pytest.mark.parametrize("mu", MUS)
def test_tight_solve_true_residual(systems, k, mu):
    _, sb = systems[(k, mu)]
    sol = pr.pcg(*pr.block_lists(sb), r_tolerance=1e-12, q_tolerance=-1.0, max_iterations=2000)
    assert sol["termination"] == pr.R_TOLERANCE
    assert sol["residual_norm"] <= 1e-12 * sol["rhs_norm"]
    rhs = sb["rhs"].reshape(-1)
    true = np.linalg.norm(rhs - sb["S"] @ sol["x"].reshape(-1)) / np.linalg.norm(rhs)
    print(f"scene {SCENES[k][0]} mu {mu}: {sol['iterations']} iterations, true residual {true:.3e}")
    assert true <= TRUE_RESIDUAL_BOUND
    assert sol["iterations"] == JACOBI_ITERATIONS[(SCENES[k][0], mu)]
    xr = abs(sol["step_dot_residual"]) / (np.linalg.norm(sol["x"]) * sol["residual_norm"])
    assert xr <= XR_BOUND_TIGHT
    xs = np.linalg.solve(sb["S"], rhs)
    assert np.linalg.norm(sol["x"].reshape(-1) - xs) <= 1e-9 * np.linalg.norm(xs)
    assert sol["precond_fallbacks"] == 0


@pytest.mark.parametrize("k", range(len(SCENES)))
@pytest.mark.parametrize("mu", MUS)
def test_block_jacobi_beats_identity(systems, k, mu):
    _, sb = systems[(k, mu)]
    bl = pr.block_lists(sb)
    jac = pr.pcg(*bl, r_tolerance=1e-12, q_tolerance=-1.0, max_iterations=2000)
    idn = pr.pcg(*bl, r_tolerance=1e-12, q_tolerance=-1.0, max_iterations=2000, preconditioner=pr.IDENTITY)
    assert jac["termination"] == pr.R_TOLERANCE
    assert idn["termination"] in (pr.R_TOLERANCE, pr.MAX_ITERATIONS)
    assert 4 * jac["iterations"] <= idn["iterations"], (jac["iterations"], idn["iterations"])


@pytest.mark.parametrize("k", range(len(SCENES)))
@pytest.mark.parametrize("mu", MUS)
def test_inexact_step_is_orthogonal_to_its_residual(systems, k, mu):
    _, sb = systems[(k, mu)]
    sol = pr.pcg(*pr.block_lists(sb), q_tolerance=-1.0, max_iterations=3)
    assert sol["iterations"] == 3 and sol["termination"] == pr.MAX_ITERATIONS
    xr = abs(sol["step_dot_residual"]) / (np.linalg.norm(sol["x"]) * sol["residual_norm"])
    print(f"scene {SCENES[k][0]} mu {mu}: |x.r| / (|x||r|) = {xr:.3e}")
    assert xr <= XR_BOUND_INEXACT
    # the recurrence's x.r is the true one
    rhs = sb["rhs"].reshape(-1)
    x = sol["x"].reshape(-1)
    r = rhs - sb["S"] @ x
    assert abs(x @ r) <= 1e-9 * np.linalg.norm(x) * np.linalg.norm(r)


@pytest.mark.parametrize("mu", MUS)
def test_model_decrease_of_an_inexact_step(systems, mu):
    """1/2 (-d^T g + d^T D d), what the back-substitution reports, is the decrease -g^T d - 1/2 d^T H d of the
    undamped model for the step after 3 PCG iterations (pose rows inexact, point rows exact)"""
    ne, sb = systems[(0, mu)]
    sol = pr.pcg(*pr.block_lists(sb), q_tolerance=-1.0, max_iterations=3)
    dpose = sol["x"]
    dpoint = ne.back_substitute(dpose)
    A, b, ns, pts = ne.dense_system()
    d = ne.dense_vector(dpose, dpoint)
    D = np.concatenate([ne.Dimg.reshape(-1), ne.Dpt[pts].reshape(-1)])
    quad = d @ (A @ d) - d @ (D * d)                       # d^T H d, the damping removed
    want = b @ d - 0.5 * quad                              # b = -g
    got = ne.model_decrease(dpose, dpoint)
    assert want > 0
    np.testing.assert_allclose(got, want, rtol=1e-8)


def test_default_rule_stops_early(systems):
    """Ceres' inexact-step rule (q_tolerance 0.1): a handful of iterations, a few percent of residual"""
    for (k, mu), (_, sb) in systems.items():
        sol = pr.pcg(*pr.block_lists(sb))
        assert sol["termination"] == pr.Q_TOLERANCE and 2 <= sol["iterations"] <= 5
        assert 0.01 < sol["residual_norm"] / sol["rhs_norm"] < 0.1


def test_row_order_changes_rounding_only(systems):
    _, sb = systems[(0, 1e-2)]
    bl = pr.block_lists(sb)
    a = pr.pcg(*bl, q_tolerance=-1.0, max_iterations=8)
    d = pr.pcg(*bl, q_tolerance=-1.0, max_iterations=8, descending=True)
    assert not np.array_equal(a["x"], d["x"])
    np.testing.assert_allclose(a["x"], d["x"], rtol=0, atol=1e-9 * np.abs(a["x"]).max())


@pytest.mark.parametrize("k", range(len(SCENES)))
@pytest.mark.parametrize("mu", MUS)
def test_reference_roundings_agree(systems, k, mu):
    """pcg() (numpy's summation orders) and pcg_device_order() (every sum in the order csrc/ba_pcg.hip states) are the same
    algorithm: same iteration counts and terminations at the defaults and to r_tolerance 1e-12, the tight solutions
    equal to 1e-9 (both are within that of numpy.linalg.solve)"""
    _, sb = systems[(k, mu)]
    bl = pr.block_lists(sb)
    for opts in (dict(), dict(r_tolerance=1e-12, q_tolerance=-1.0, max_iterations=2000)):
        a, d = pr.pcg(*bl, **opts), pr.pcg_device_order(*bl, **opts)
        assert (a["iterations"], a["termination"]) == (d["iterations"], d["termination"])
        np.testing.assert_allclose(d["x"], a["x"], rtol=0, atol=1e-9 * np.abs(a["x"]).max())
        np.testing.assert_allclose(d["q"], a["q"], rtol=1e-12)
        np.testing.assert_allclose(d["zetas"], a["zetas"], rtol=0, atol=1e-9)


def test_zero_rhs_and_singular_block():
    Sd = np.tile(np.eye(6), (3, 1, 1))
    So = np.zeros((1, 6, 6))
    pairs = np.array([[0, 2]])
    sol = pr.pcg(Sd, So, pairs, np.zeros((3, 6)))
    assert sol["termination"] == pr.ZERO_RHS and sol["iterations"] == 0 and not sol["x"].any()
    Sd[1][2, 2] = -100.0                                   # fails its Cholesky: identity for that slot, counted
    Minv, fb = pr.preconditioner(Sd, pr.SCHUR_JACOBI)
    assert fb == 1 and np.array_equal(Minv[1], np.eye(6))
    rhs = np.ones((3, 6))
    sol = pr.pcg(Sd, So, pairs, rhs)
    assert sol["termination"] == pr.BREAKDOWN              # p.w <= 0 on the indefinite system


def test_shim_solve_refusals():
    """BundleAdjusterHip::Solve returns false without residuals and with refined intrinsics (no GPU needed)"""
    import os
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_solve"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_solve")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


# ---- ABI surface ----
NEW_SYMBOLS = ["pcd_ba_pcg_opts_default", "pcd_ba_schur_solve_pcg_device", "pcd_ba_schur_solve_pcg",
               "pcd_ba_get_parameters", "pcd_ba_solve_opts_default", "pcd_ba_solve"]


def test_new_symbols_declared_and_exported(pcdhip):
    from tests.test_abi import _declared_symbols
    declared = _declared_symbols()
    lib = pcdhip.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/pcdhip.h"
        assert hasattr(lib, s), f"{s} is not exported by libpcdhip.so"
        assert s in pcdhip.ABI_SYMBOLS
    assert lib.pcd_version() == 1


def test_option_defaults(pcdhip):
    o = pcdhip.pcg_opts()
    assert (o.max_iterations, o.min_iterations, o.preconditioner, o.q_tolerance, o.r_tolerance) == \
        (100, 0, pcdhip.PRECOND_SCHUR_JACOBI, 0.1, -1.0)
    s = pcdhip.BASolveOpts()
    pcdhip.lib().pcd_ba_solve_opts_default(C.byref(s))
    assert (s.max_num_iterations, s.damping, s.initial_radius, s.max_radius, s.min_radius, s.min_relative_decrease,
            s.function_tolerance, s.gradient_tolerance) == (10, pcdhip.DAMP_MARQUARDT, 1e4, 1e16, 1e-32, 1e-3, 0.0, 0.0)
    assert (s.linear.max_iterations, s.linear.preconditioner, s.linear.q_tolerance, s.linear.r_tolerance) == \
        (100, pcdhip.PRECOND_SCHUR_JACOBI, 0.1, -1.0)
    # the layouts the binding assumes
    assert C.sizeof(pcdhip.BAPcgOpts) == 64 and C.sizeof(pcdhip.BAPcgInfo) == 48
    assert C.sizeof(pcdhip.BASolveOpts) == 152 and C.sizeof(pcdhip.BASolveIteration) == 72
    assert C.sizeof(pcdhip.BASolveSummary) == 48


def test_no_device_no_fallback(pcdhip):
    """without a gfx950 device every new computing entry point refuses with NO_DEVICE (no host solve behind it)"""
    if pcdhip.device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is exercised on CPU-only machines")
    lib = pcdhip.lib()
    o, so = pcdhip.pcg_opts(), pcdhip.BASolveOpts()
    lib.pcd_ba_solve_opts_default(C.byref(so))
    x = np.zeros(6)
    info, sm = pcdhip.BAPcgInfo(), pcdhip.BASolveSummary()
    vp = x.ctypes.data_as(C.c_void_p)
    assert lib.pcd_ba_schur_solve_pcg_device(None, C.byref(o), vp, None, None) == pcdhip.PCD_ERR_NO_DEVICE
    assert lib.pcd_ba_schur_solve_pcg(None, C.byref(o), vp, C.byref(info)) == pcdhip.PCD_ERR_NO_DEVICE
    assert lib.pcd_ba_get_parameters(None, vp, vp) == pcdhip.PCD_ERR_NO_DEVICE
    assert lib.pcd_ba_solve(None, C.byref(so), C.byref(sm), None) == pcdhip.PCD_ERR_NO_DEVICE

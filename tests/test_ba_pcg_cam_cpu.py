"""CPU checks of the bordered PCG's numpy reference (tests/ba_pcg_cam_ref.py; pcd_ba_schur_cam_solve_pcg*)
on the oracle's own bordered systems (ba_schur_cam_ref.CAM_CASES x DAMPINGS).

Order sensitivity and the parity bound.  Method of tests/test_ba_pcg_gpu.py: pcg_cam with the sums walked in ascending
and in descending order (pose row lists, the pose slots of the camera-row sum, the camera slots of the border term), 8
iterations with the tolerances off, both preconditioners, relative differences as rel() defines them (x by
max |dx| / max |x|, Q by |dQ| / |Q|, ||r|| by |d||r||| / ||rhs||).  Largest value measured: 1.6584e-03 (x, case 3
FULL_OPENCV, Levenberg mu = 0, block-Jacobi; 6.5e-04 on case 0 and 1.3e-04 on case 3 at mu = 1e-4).  These are the
settings whose gauge is nearly free (cond(S) up to 1e20, ba_schur_cam_ref) and whose camera rows mix focal-length and
distortion scales: the plain systems' 5.4345e-13 does not carry over.  On the Marquardt 1e-4 systems (cond 1e10 .. 1e11)
the largest value is 1.4e-10.  PARITY_BOUND = 100 x 1.6584e-03 = 1.6584e-01 for device against pcg_cam_device_order.

Tight solves (Marquardt 1e-4, r_tolerance 1e-12, Q test off), iterations identity / block-Jacobi and the true residual
||b - S x|| / ||b|| with the dense S:

  case                                  identity  block-Jacobi  true residual (identity, block-Jacobi)
  0  OPENCV, focal only                 252       6             3.19e-13  2.16e-13
  1  OPENCV, all 8                      386       30            7.70e-13  1.14e-14
  2  PINHOLE, all 4                     93        10            8.29e-14  7.18e-13
  3  FULL_OPENCV, all 12                248       23            4.58e-13  7.03e-14
  4  OPENCV + SIMPLE_RADIAL             253       25            5.74e-13  1.46e-13
  5  the same, camera 1 refined alone   230       17            9.47e-13  1.96e-13

Block-Jacobi with the 12 x 12 camera blocks buys a factor 8 to 42 in iterations on these systems.  Largest true residual
9.47e-13, bound TRUE_RESIDUAL_CAM_BOUND = 1e-11 (10 x, as tests/test_ba_pcg_cpu.py).  The block-Jacobi solve stands
within 8.7e-13 of numpy.linalg.solve(S, rhs_full) in norm (bound 1e-9, as there).

LM (lm_scene: 8 images, 200 points, one OPENCV camera with focal x 1.02, all 8 parameters refined, seed 30): the tight
PCG reproduces lm_cam's six accepted steps with costs within 1e-12 and radii within 1e-9; at the default options the
loop runs 3, 4, 2, 2, 2, 2 PCG iterations and accepts TTFTTT (the inexact third step is rejected), min |rho - 1e-3| =
0.61 and the nearest zeta stands 0.0278 from q_tolerance."""
import numpy as np
import pytest

from tests import ba_pcg_cam_ref as pc
from tests import ba_pcg_ref as pr
from tests import ba_schur_cam_ref as cref
from tests import ba_schur_ref as ref

ORDER_SENSITIVITY = 1.6584e-03               # measured, see above; re-measured by test_reference_order_sensitivity
PARITY_BOUND = 100 * ORDER_SENSITIVITY       # 1.6584e-01
TRUE_RESIDUAL_CAM_BOUND = 1e-11              # 10 x 9.47e-13
TIGHT_ITERATIONS = {0: (252, 6), 1: (386, 30), 2: (93, 10), 3: (248, 23), 4: (253, 25), 5: (230, 17)}   # identity, Jacobi
TIGHT = dict(r_tolerance=1e-12, q_tolerance=-1.0)
FIXED8 = dict(q_tolerance=-1.0, r_tolerance=-1.0, max_iterations=8)


def rel(got, want, rhs_norm):
    dx = np.abs(got["x"] - want["x"]).max() / max(np.abs(want["x"]).max(), 1e-300)
    dq = abs(got["q"] - want["q"]) / max(abs(want["q"]), 1e-300)
    dr = abs(got["residual_norm"] - want["residual_norm"]) / rhs_norm
    return dx, dq, dr


def lm_scene(oracle, seed=30):
    """focal x 1.02 on a clean 8-image scene, every OPENCV parameter refined"""
    s = ref.camera_scene(oracle, [4], seed=seed, I=8, P=200)
    cp = np.array(s["cam_params_list"][0], np.float64)
    cp[:2] *= 1.02
    s["cam_params_list"] = [cp]
    return s, cref.refine_mask(s)


def unused_camera_scene(oracle):
    """two cameras, every image on camera 0, both refined: at Levenberg mu = 0 the diagonal block of camera 1's slot is 0
    on its active coordinates (no observation, no damping), so its first pivot is not positive -- the identity fallback
    of the camera preconditioner, reached by input values; its right-hand side is 0 and so is its step"""
    s = cref.camera_scene(oracle, [4, 2], 77)
    s["image_camera"][:] = 0
    ref.reproject(oracle, s, np.random.default_rng(5))
    s["loss_type"], s["loss_scale"] = 2, 2.0
    return s, cref.refine_mask(s)


@pytest.fixture(scope="module")
def systems(oracle):
    out = {}
    for case in range(len(cref.CAM_CASES)):
        s, refine = cref.cam_case_scene(oracle, case)
        for d, (mode, mu) in enumerate(cref.DAMPINGS):
            ne = cref.CamNormalEquations(oracle, cref.without_refine(s), refine, mu, mode)
            out[(case, d)] = (ne, ne.schur_cam_blocks())
    return out


MARQUARDT = [d for d, (mode, _) in enumerate(cref.DAMPINGS) if mode in cref.WELL_CONDITIONED]


def test_reference_order_sensitivity(systems):
    """the measurement PARITY_BOUND comes from, repeated: ascending against descending order of the sums"""
    worst, where = 0.0, None
    for (case, d), (_, sb) in systems.items():
        bl = pc.cam_block_lists(sb)
        for kind in (pc.IDENTITY, pc.SCHUR_JACOBI):
            a, b = pc.pcg_cam(*bl, preconditioner=kind, **FIXED8), pc.pcg_cam(*bl, preconditioner=kind, descending=True, **FIXED8)
            m = max(rel(b, a, a["rhs_norm"]))
            if m > worst:
                worst, where = m, (case, cref.DAMPINGS[d], kind)
    print(f"largest ascending / descending difference {worst:.4e} at {where}; PARITY_BOUND {PARITY_BOUND:.4e}")
    assert 0.0 < worst <= ORDER_SENSITIVITY * 1.0001      # the recorded figure, to its printed digits


def test_without_camera_slots_both_references_are_the_plain_ones(oracle):
    s = ref.camera_scene(oracle, [4, 2], 91)
    sb = ref.NormalEquations(oracle, s, 1e-4).schur_blocks()
    bl = pr.block_lists(sb)
    ns = sb["rhs"].shape[0]
    empty = (np.zeros((ns, 0, 12, 6)), np.zeros((0, 0, 12, 12)), np.zeros((0, 12)))
    for o in (FIXED8, dict(), dict(preconditioner=pc.IDENTITY, **FIXED8)):
        for mine, plain in ((pc.pcg_cam, pr.pcg), (pc.pcg_cam_device_order, pr.pcg_device_order)):
            a, b = mine(*bl, *empty, **o), plain(*bl, **o)
            assert np.array_equal(a["x"], b["x"].reshape(-1)) and a["zetas"] == b["zetas"]
            for k in ("iterations", "termination", "q", "residual_norm", "rhs_norm", "step_dot_residual", "precond_fallbacks"):
                assert a[k] == b[k], k


@pytest.mark.parametrize("case", range(len(cref.CAM_CASES)))
def test_tight_solve_matches_the_dense_solve(systems, case):
    for d in MARQUARDT:
        ne, sb = systems[(case, d)]
        bl = pc.cam_block_lists(sb)
        S, b = pc.dense_system(*bl)
        assert np.array_equal(S, sb["S"]) and np.array_equal(b, sb["rhs_full"])
        its = []
        for kind in (pc.IDENTITY, pc.SCHUR_JACOBI):
            sol = pc.pcg_cam(*bl, preconditioner=kind, max_iterations=5000, **TIGHT)
            assert sol["termination"] == pc.R_TOLERANCE and sol["precond_fallbacks"] == 0
            true = pc.true_residual(bl, sol["x"])
            print(f"case {case} preconditioner {kind}: {sol['iterations']} iterations, true residual {true:.3e}")
            assert true <= TRUE_RESIDUAL_CAM_BOUND
            assert not sol["x_cam"][~ne.cam_active].any() and not sol["x_pose"][~ne.pr["active"]].any()
            its.append(sol["iterations"])
        assert tuple(its) == TIGHT_ITERATIONS[case]
        xs = np.linalg.solve(sb["S"], sb["rhs_full"])
        assert np.linalg.norm(sol["x"] - xs) <= 1e-9 * np.linalg.norm(xs)


@pytest.mark.parametrize("kind", [pc.IDENTITY, pc.SCHUR_JACOBI])
def test_inactive_coordinates_are_exactly_zero(systems, kind):
    """in both references, at every damping, after 8 iterations: identity rows with a zero right-hand side never move"""
    seen = 0
    for (case, d), (ne, sb) in systems.items():
        for solve in (pc.pcg_cam, pc.pcg_cam_device_order):
            sol = solve(*pc.cam_block_lists(sb), preconditioner=kind, **FIXED8)
            assert not sol["x_cam"][~ne.cam_active].any() and not sol["x_pose"][~ne.pr["active"]].any()
        seen += int((~ne.cam_active).sum())
    assert seen > 0


def test_block_inverse_keeps_identity_rows(systems):
    _, sb = systems[(4, MARQUARDT[0])]              # slot 1 is SIMPLE_RADIAL: 4 active coordinates, 8 identity rows
    ne = systems[(4, MARQUARDT[0])][0]
    dead = ~ne.cam_active[1]
    assert dead.sum() == 8
    for order in (False, True):
        inv = pc.block_inverse_n(sb["S_cam"][1, 1], device_order=order)
        assert np.array_equal(inv[dead][:, dead], np.eye(8)) and not inv[dead][:, ~dead].any() and not inv[~dead][:, dead].any()
        np.testing.assert_allclose(inv[~dead][:, ~dead], np.linalg.inv(sb["S_cam"][1, 1][~dead][:, ~dead]), rtol=1e-9)
    a, b = pc.block_inverse_n(sb["S_cam"][0, 0]), pc.block_inverse_n(sb["S_cam"][0, 0], device_order=True)
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12 * np.abs(b).max())
    for n in (6, 12):                               # the 6 x 6 of ba_pcg_ref is the same code at n = 6
        A = np.random.default_rng(n).normal(size=(n, 20))
        A = A @ A.T
        assert np.array_equal(pc.block_inverse_n(A[:6, :6], True), pr._block_inverse_device_order(A[:6, :6]))
    assert pc.block_inverse_n(np.zeros((12, 12))) is None and pc.block_inverse_n(-np.eye(12), True) is None


def test_unused_refined_camera_takes_the_fallback(oracle):
    s, refine = unused_camera_scene(oracle)
    ne = cref.CamNormalEquations(oracle, s, refine, 0.0, "levenberg")
    sb = ne.schur_cam_blocks()
    assert ne.ncs == 2 and not np.diag(sb["S_cam"][1, 1])[ne.cam_active[1]].any() and not sb["rhs_cam"][1].any()
    assert pr.preconditioner(sb["S_diag"], pr.SCHUR_JACOBI)[1] == 0
    for solve in (pc.pcg_cam, pc.pcg_cam_device_order):
        sol = solve(*pc.cam_block_lists(sb), **FIXED8)
        assert sol["precond_fallbacks"] == 1 and sol["iterations"] == 8 and not sol["x_cam"][1].any()


def test_lm_with_the_tight_pcg_is_the_cholesky_lm(oracle):
    s, refine = lm_scene(oracle)
    want, _ = cref.lm_cam(oracle, s, refine, 6)
    got, _ = pc.lm_cam_pcg(oracle, s, refine, 6, linear=dict(max_iterations=500, **TIGHT))
    assert all(w["accepted"] for w in want)
    assert [g["accepted"] for g in got] == [w["accepted"] for w in want]
    for g, w in zip(got, want):
        assert g["linear_termination"] == pc.R_TOLERANCE
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-12)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-9)


def test_lm_margins_at_the_defaults(oracle):
    """what tests/test_ba_pcg_cam_gpu.py relies on: no rho near min_relative_decrease, no zeta near q_tolerance"""
    s, refine = lm_scene(oracle)
    hist, _ = pc.lm_cam_pcg(oracle, s, refine, 6)
    assert [h["linear_iterations"] for h in hist] == [3, 4, 2, 2, 2, 2]
    assert "".join("T" if h["accepted"] else "F" for h in hist) == "TTFTTT"
    assert min(abs(h["rho"] - 1e-3) for h in hist) > 0.5
    assert min(abs(z - 0.1) for h in hist for z in h["zetas"]) > 0.02

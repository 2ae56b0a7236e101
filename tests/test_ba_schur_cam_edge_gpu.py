"""The camera rows of the reduced system (pcd_ba_schur_cam*, pcd_ba_solve with refine_intrinsics) pinned
at the boundaries of their kernels, against the numpy reference built from the oracle's blocks
(tests/ba_schur_cam_ref.py).  What each scene reaches, and every condition that makes it bite, is asserted on the
reference alone in tests/test_ba_schur_cam_edge_cpu.py:

  slot pairs       three and eight camera slots: the pair decode from q = 3 on, 36 pairs with several chunks, K = 3 and
                   K = 5 on the dead-row logic, every camera model the older cases leave out;
  64 coordinates   12 ncs = 96: the second trip of the one-wavefront loops of the model decrease and of the gradient
                   maximum (slots 5 .. 7);
  64 chunks        16 700 points: 66 chunks, two partials on lanes 0 and 1 of the chunk reduction;
  panel edges      n = 96 exactly, camera rows astride the first edge of the bordered Cholesky, camera rows opening
                   panel 1, camera rows across the edge at 192 behind 28 pose slots;
  masks            refine masks with holes, two cameras with different masks;
  degenerate       every point constant, a refined camera on constant-pose images only, a refined camera nobody
                   observes (Marquardt: step exactly 0; Levenberg 0: the factorisation fails at that slot's first column);
  gradient         gradient_max_norm against the reference with the maximum in a camera coordinate of slot 7, a pose
                   coordinate and the last point, and the gradient-tolerance exit on both sides of that value.

Bounds are those of tests/test_ba_schur_cam_gpu.py (_parity is that module's): blocks 1e-9 relative with the
scale-aware floor, pose part bit-identical to the plain call, back-substitution and model decrease 1e-8, plus 1e-14, the
step against the whole damped system 1e-8 (100 x the reference's own two-route agreement), eta <= ETA_CAM_BOUND; pivots
at 1e-10 as tests/test_ba_chol_gpu.py; gradient_max_norm at 1e-9.  Every test prints its figures before it asserts.

Measured on gfx950: eta 3.6e-20 .. 8.6e-16 over all cases (bound 2.26e-13); the bordered info fills min_pivot and
max_pivot, equal to numpy's on the device's own S to the printed six digits; chunks_65 blocks within 2.5e-13 of the
reference, its back-substitution within 1.1e-12; the diagonal of S_cam with every point constant equals H_cam plus the
damping exactly; gradient_max_norm differs from the reference in the last digit at most; the loop at eight slots
accepts TTTTFF with costs within 2e-10 of the reference, the tight PCG takes 65 .. 70 iterations per step."""
import numpy as np
import pytest

from tests import ba_schur_cam_ref as cref
from tests import ba_schur_ref as ref
from tests.test_ba_chol_cpu import eta, first_failing_column
from tests.test_ba_pcg_cam_cpu import TIGHT
from tests.test_ba_schur_cam_cpu import ETA_CAM_BOUND
from tests.test_ba_schur_cam_edge_cpu import LM_ACCEPTED
from tests.test_ba_schur_cam_gpu import _close, _dev, _np, _parity

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S12, NB = 12, 96
MU, MODE = 1e-4, "marquardt"


def _shape(ne, ns, ncs, what):
    """ns, ncs, n and the panel count of the direct solve that _parity ran"""
    info, n = ne.device["info"], 6 * ns + S12 * ncs
    print(f"{what}: ns {ne.pr['slot_img'].size} ncs {ne.ncs} n {info['n']} panels {info['panels']} status {info['status']} "
          f"pivots {info['min_pivot']:.6g} .. {info['max_pivot']:.6g}")
    assert (ne.pr["slot_img"].size, ne.ncs) == (ns, ncs)
    assert info["n"] == n and info["panels"] == -(-n // NB) and info["n_padded"] == NB * info["panels"]
    return info


# ---- 1. slot counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_slots", "eight_wide"])
def test_slot_counts(gpu, oracle, name):
    s, refine = cref.slot_scene(oracle, name)
    ne = _parity(gpu, oracle, s, refine, MU, MODE, True)
    info = _shape(ne, *cref.SLOT_CASES[name][5:7], name)
    assert info["status"] == gpu.CHOL_OK and info["panels"] == {"three_slots": 2, "eight_wide": 3}[name]


@pytest.mark.parametrize("damping", range(len(cref.DAMPINGS)))
def test_eight_mixed(gpu, oracle, damping):
    mode, mu = cref.DAMPINGS[damping]
    s, refine = cref.slot_scene(oracle, "eight_mixed")
    ne = _parity(gpu, oracle, s, refine, mu, mode, mode in cref.WELL_CONDITIONED)
    _shape(ne, 15, 8, f"eight_mixed {mode} {mu}")
    assert ne.device["slots"]["active"].sum(axis=1).tolist() == [3, 5, 8, 5, 4, 5, 12, 8]


# ---- 2. panel edges of the bordered Cholesky --------------------------------------------------------------------------
@pytest.mark.parametrize("ncs,ns", cref.PANEL_CASES)
def test_panel_edges(gpu, oracle, ncs, ns):
    s, refine = cref.panel_scene(oracle, ncs, ns)
    ne = _parity(gpu, oracle, s, refine, MU, MODE, True)
    info = _shape(ne, ns, ncs, f"panel ({ncs}, {ns})")
    assert info["status"] == gpu.CHOL_OK and info["failed_column"] == -1
    d = np.diag(np.linalg.cholesky(ne.device["S"]))        # the pivots: L's diagonal, of the device's own S
    print(f"pivots of numpy on the device's S {d.min():.6g} .. {d.max():.6g}")
    np.testing.assert_allclose([info["min_pivot"], info["max_pivot"]], [d.min(), d.max()], rtol=1e-10)
    ba = gpu.BA(**cref.without_refine(s), camera_refine=refine)
    ba.schur_cam(MU, damping=MODE, want=("cost", "num_skipped"))
    xa, ia = ba.schur_cam_solve_cholesky()
    xa = xa.clone()
    xb, ib = ba.schur_cam_solve_cholesky()
    assert torch.equal(xa, xb) and ia == ib == info and np.array_equal(xa.cpu().numpy(), ne.device["delta"])
    ba.close()


# ---- 3. more than 64 chunks -------------------------------------------------------------------------------------------
def test_chunks_65(gpu, oracle):
    s, refine = cref.chunks_65_scene(oracle)
    base = cref.without_refine(s)
    ne = cref.CamNormalEquations(oracle, base, refine, MU, MODE)
    sb = ne.schur_cam_blocks()
    ns, ncs = ne.pr["slot_img"].size, ne.ncs
    n = 6 * ns + S12 * ncs
    assert (ns, ncs, ne.pr["P"]) == (5, 2, 16700)
    ba = gpu.BA(**base, camera_refine=refine)
    r = _np(ba.schur_cam(MU, damping=MODE, dense=True, want=("cost", "rhs", "B", "S_cam", "rhs_cam", "num_skipped")))
    for k in ("B", "S_cam", "rhs_cam", "S"):
        print(f"{k}: max |device - reference| / scale {np.abs(r[k] - sb[k]).max() / max(1.0, np.abs(sb[k]).max()):.3e}")
    np.testing.assert_allclose(r["cost"][0], ne.cost, rtol=1e-9)
    assert int(r["num_skipped"][0]) == int(ne.skipped.sum())
    _close(r["B"], sb["B"], 1e-9, "B")
    _close(r["S_cam"], sb["S_cam"], 1e-9, "S_cam")
    _close(r["rhs_cam"], sb["rhs_cam"], 1e-9, "rhs_cam")
    _close(r["rhs"], sb["rhs"], 1e-9, "rhs")
    _close(r["S"], sb["S"], 1e-9, "dense S")
    ba.schur_cam(MU, damping=MODE, want=("cost", "num_skipped"))
    delta, info = ba.schur_cam_solve_cholesky()
    rhs = np.concatenate([r["rhs"].reshape(-1), r["rhs_cam"].reshape(-1)])
    e = eta(r["S"], rhs, delta.cpu().numpy())
    print(f"n {n} panels {info['panels']} eta {e:.3e} (bound {ETA_CAM_BOUND:.3e})")
    assert info["status"] == gpu.CHOL_OK and info["n"] == n == 54 and info["panels"] == 1
    assert e <= ETA_CAM_BOUND
    rng = np.random.default_rng(7)      # a step of moderate size; inactive camera coordinates carry garbage on purpose
    dpose = rng.normal(0, 1e-3, (ns, 6)) * ne.pr["active"]
    dcam = rng.normal(0, 1e-3, (ncs, S12))
    dpoint, md = ba.back_substitute_cam(_dev(np.concatenate([dpose.reshape(-1), dcam.reshape(-1)])))
    dpoint = dpoint.cpu().numpy()
    want = ne.back_substitute_cam(dpose, dcam)
    print(f"back-substitution: max |d| / scale {np.abs(dpoint - want).max() / max(1.0, np.abs(want).max()):.3e}")
    _close(dpoint, want, 1e-8, "back-substitution")
    _close(md.cpu().numpy()[0], ne.model_decrease_cam(dpose, dcam, dpoint), 1e-8, "model decrease")
    assert not dpoint[ne.skipped | (ne.pr["point_const"] == 1)].any()
    ba.close()


# ---- 4. masks with holes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cref.MASK_CASES))
def test_masks_with_holes(gpu, oracle, name):
    s, refine = cref.mask_scene(oracle, name)
    ne = _parity(gpu, oracle, s, refine, MU, MODE, True)       # camera_slots()["active"] against the reference's in there
    _shape(ne, 5, len(cref.MASK_CASES[name][0]), name)
    assert int(ne.cam_active.sum()) == int(refine.sum())
    base = cref.without_refine(s)
    ba = gpu.BA(**base, camera_refine=refine)
    ba.schur_cam(MU, damping=MODE, want=("cost", "num_skipped"))
    delta, _ = ba.schur_cam_solve_cholesky()
    dpoint, _ = ba.back_substitute_cam(delta)
    cams = ba.plus_cam(delta, dpoint)[2].cpu().numpy()
    flat = np.concatenate([np.asarray(c, np.float64) for c in base["cam_params_list"]])
    print(f"{name}: moved {np.flatnonzero(cams != flat).tolist()}, masked {np.flatnonzero(refine).tolist()}")
    assert np.array_equal(cams != flat, refine != 0)           # exactly the masked parameters move
    ba.close()


# ---- 5. degenerate couplings ------------------------------------------------------------------------------------------
def test_every_point_constant(gpu, oracle):
    """nothing is eliminated: the camera rows are the handle's own evaluation"""
    s, refine = cref.const_points_scene(oracle)
    base = cref.without_refine(s)
    ne = cref.CamNormalEquations(oracle, base, refine, MU, MODE)
    ba = gpu.BA(**base, camera_refine=refine)
    ev = ba.evaluate(("cost", "H_cam", "g_cam", "E_cam"))
    r = _np(ba.schur_cam(MU, damping=MODE, want=("cost", "B", "S_cam", "rhs_cam", "num_skipped")))
    active = ba.camera_slots()["active"].astype(bool)
    assert np.array_equal(active, ne.cam_active) and (ne.pr["slot_img"].size, ne.ncs) == (7, 2)
    assert not r["S_cam"][0, 1].any() and not r["S_cam"][1, 0].any() and int(r["num_skipped"][0]) == 0
    worst = 0.0
    for q, c in enumerate(ne.slot_cam):
        a = active[q]
        H, S = ev["H_cam"][c][np.ix_(a, a)], r["S_cam"][q, q][np.ix_(a, a)]
        offd = ~np.eye(int(a.sum()), dtype=bool)
        assert np.array_equal(S[offd], H[offd])
        want = np.diag(H) + ref.damping(np.diag(H), MU, MODE)
        worst = max(worst, float(np.abs(np.diag(S) / want - 1).max()))
        assert np.array_equal(r["rhs_cam"][q][a], -ev["g_cam"][c][a]) and not r["rhs_cam"][q][~a].any()
    print(f"diagonal of S_cam against H_cam + damping: {worst:.3e} relative")
    assert worst <= 1e-15
    for i, im in enumerate(ne.pr["slot_img"]):
        q = ne.img_cam_slot[im]
        keep = np.outer(active[q], ne.pr["active"][i])
        assert np.array_equal(r["B"][i, q][keep], ev["E_cam"][im][keep]) and np.abs(ev["E_cam"][im][keep]).max() > 0
        assert not r["B"][i, q][~keep].any() and not r["B"][i, 1 - q].any()
    sb = ne.schur_cam_blocks()
    for k in ("B", "S_cam", "rhs_cam"):
        _close(r[k], sb[k], 1e-9, k)
    ba.close()


def test_refined_camera_on_constant_poses_only(gpu, oracle):
    s, refine = cref.const_pose_camera_scene(oracle)
    ne = _parity(gpu, oracle, s, refine, MU, MODE, True)
    _shape(ne, 4, 2, "const_pose_camera")
    n0 = 6 * 4
    assert np.abs(ne.device["S"][n0 + S12:, :n0]).max() > 0 and np.abs(ne.device["S"][n0 + S12:, n0:n0 + S12]).max() > 0


def test_unused_refined_camera(gpu, oracle):
    """Marquardt: the unused slot's step is exactly 0.  Levenberg at mu = 0: its first coordinate is the column at which
    the factorisation fails, the step is all zeros, and the same handle solves the Marquardt system right after."""
    s, refine = cref.unused_camera_scene(oracle)
    ne = _parity(gpu, oracle, s, refine, MU, MODE, True)
    info = _shape(ne, 4, 2, "unused_camera")
    ns = 4
    assert info["status"] == gpu.CHOL_OK
    assert not ne.device["delta"][6 * ns + S12:].any() and ne.device["delta"][6 * ns:6 * ns + S12].any()
    base = cref.without_refine(s)
    want = first_failing_column(cref.CamNormalEquations(oracle, base, refine, 0.0, "levenberg").schur_cam_blocks()["S"])
    ba = gpu.BA(**base, camera_refine=refine)
    ba.schur_cam(0.0, damping="levenberg", want=("cost", "num_skipped"))
    delta, bad = ba.schur_cam_solve_cholesky()
    print(f"Levenberg 0: status {bad['status']} failed_column {bad['failed_column']} (reference {want})")
    assert want == 6 * ns + S12 == 36
    assert bad["status"] == gpu.CHOL_NOT_POSITIVE_DEFINITE and bad["failed_column"] == want
    assert bad["n"] == 48 and bad["panels"] == 1 and not delta.cpu().numpy().any()
    ba.schur_cam(MU, damping=MODE, want=("cost", "num_skipped"))
    delta, ok = ba.schur_cam_solve_cholesky()
    assert ok == info and np.array_equal(delta.cpu().numpy(), ne.device["delta"])
    ba.close()


# ---- 6. the gradient maximum and its exit -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gradients(oracle):
    """where -> (scene, refine, reference maximum, its parts), computed once"""
    out = {}
    for where in ("camera", "pose", "point"):
        s, refine = cref.gradient_scene(oracle, where)
        ne = ref.NormalEquations(oracle, s, MU) if refine is None else cref.CamNormalEquations(oracle, s, refine, MU)
        out[where] = (s, refine) + cref.gradient_max(ne)
    return out


def _solve(gpu, s, refine, direct, **opts):
    if refine is None:
        ba = gpu.BA(**s)
        out = gpu.ba_solve(ba, linear_solver="cholesky" if direct else "pcg", **opts)
    else:
        ba = gpu.BA(**cref.without_refine(s), camera_refine=refine)
        out = gpu.ba_solve(ba, linear_solver="cholesky" if direct else "pcg_cam", refine_intrinsics=True, **opts)
    ba.close()
    return out


@pytest.mark.parametrize("direct", [True, False], ids=["cholesky", "pcg"])
@pytest.mark.parametrize("where", ["camera", "pose", "point"])
def test_gradient_max_norm(gpu, gradients, where, direct):
    s, refine, want, parts = gradients[where]
    summary, got = _solve(gpu, s, refine, direct, max_num_iterations=1)
    print(f"{where}: gradient_max_norm {got[0]['gradient_max_norm']:.17g}, reference {want:.17g} of {parts}")
    assert summary["num_iterations"] == 1 and want == parts[where]
    np.testing.assert_allclose(got[0]["gradient_max_norm"], want, rtol=1e-9)


@pytest.mark.parametrize("direct", [True, False], ids=["cholesky", "pcg"])
def test_gradient_tolerance_exit(gpu, gradients, direct):
    """on both sides of the reference maximum, which sits in camera slot 7"""
    s, refine, want, _ = gradients["camera"]
    below, _ = _solve(gpu, s, refine, direct, max_num_iterations=2, gradient_tolerance=0.999 * want)
    above, hist = _solve(gpu, s, refine, direct, max_num_iterations=2, gradient_tolerance=1.001 * want)
    print(f"tolerance 0.999 x: {below['num_iterations']} iterations, termination {below['termination']}; 1.001 x: "
          f"{above['num_iterations']} iterations, termination {above['termination']}")
    assert below["num_iterations"] >= 1
    assert above["termination"] == gpu.SOLVE_GRADIENT_TOLERANCE and above["num_iterations"] == 0 and hist == []


# ---- 7. the loop at eight slots ---------------------------------------------------------------------------------------
def test_lm_at_eight_slots(gpu, oracle):
    s, refine, radius = cref.lm_eight_scene(oracle)
    want, final = cref.lm_cam(oracle, s, refine, 6, initial_radius=radius)
    assert "".join("T" if w["accepted"] else "F" for w in want) == LM_ACCEPTED
    assert all(abs(w["rho"] - 1e-3) > 0.05 for w in want)
    base = cref.without_refine(s)
    ba = gpu.BA(**base, camera_refine=refine)
    summary, got = gpu.ba_solve(ba, max_num_iterations=6, initial_radius=radius, linear_solver="cholesky",
                                refine_intrinsics=True)
    print(summary, "accepted", "".join("T" if r["accepted"] else "F" for r in got), "costs", [r["cost"] for r in got],
          "reference", [w["cost"] for w in want])
    assert summary["num_iterations"] == 6 and [r["accepted"] for r in got] == [w["accepted"] for w in want]
    for g, w in zip(got, want):
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
        assert g["linear_iterations"] == 0 and g["linear_termination"] == gpu.CHOL_OK
    np.testing.assert_allclose(summary["final_cost"], oracle.BA(**final).normal_equations()[0], rtol=1e-8)
    ba.close()
    ba = gpu.BA(**base, camera_refine=refine)
    sp, hp = gpu.ba_solve(ba, max_num_iterations=6, initial_radius=radius, linear_solver="pcg_cam", refine_intrinsics=True,
                          linear=dict(max_iterations=2000, **TIGHT))
    print("tight PCG: accepted", "".join("T" if r["accepted"] else "F" for r in hp), "iterations",
          [r["linear_iterations"] for r in hp])
    assert [r["accepted"] for r in hp] == [w["accepted"] for w in want]
    ba.close()

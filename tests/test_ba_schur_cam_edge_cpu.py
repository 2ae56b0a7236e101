"""The conditions that tests/test_ba_schur_cam_edge_gpu.py relies on, asserted on the numpy reference
(tests/ba_schur_cam_ref.py) and the oracle alone; no GPU, and no constant here comes from device output.

The scenes pin the camera rows of the reduced system at the boundaries of its kernels: the slot-pair
decode from q = 3 on (three and eight camera slots, PCD_BA_MAX_CAMERA_SLOTS = 8 gives 36 pairs), the partial index with
many pairs and several chunks together, more than 64 chunks of 256 points in the chunk reduction, more than 64 camera
coordinates in the one-wavefront loops (12 ncs = 96), and camera rows on and across the panel edges of the bordered
Cholesky (kCholNB = 96).

For every new Marquardt 1e-4 system except chunks_65 (whose whole system has 45 000 unknowns) three things are
measured and asserted (test_marquardt_systems): the two routes of the reference (whole damped system; block by block,
then back-substitution) agree within ROUTES_AGREE = 1e-10, which makes the GPU module's 1e-8 the customary 100 x
margin; cond(S) is printed; eta of np.linalg.cholesky plus two substitutions is at most ETA_CAM_REFERENCE, so
ETA_CAM_BOUND keeps its margin on the new sizes.  Measured (ns, ncs, n, non-zero off-diagonal S_cam blocks, cond(S), eta,
route agreement):

  three_slots        11 3 102   3/3   1.07e+11 9.17e-18 2.72e-12
  eight_mixed        15 8 186  21/28  2.20e+12 1.02e-19 9.06e-12   active counts [3, 5, 8, 5, 4, 5, 12, 8]
  eight_wide         28 8 264  28/28  2.02e+11 2.01e-20 1.84e-12   camera rows 168 .. 263 across the edge at 192
  panel (1, 14)      14 1  96   -     5.73e+10 1.37e-17 1.13e-12
  panel (2, 12)      12 2  96   1/1   1.82e+11 1.28e-18 3.96e-12
  panel (1, 15)      15 1 102   -     5.79e+10 4.76e-19 4.29e-13
  panel (2, 13)      13 2 102   1/1   1.67e+11 2.12e-18 1.41e-12
  panel (2, 16)      16 2 120   1/1   8.04e+10 6.22e-20 4.03e-12
  principal_point     5 1  42   -     1.63e+10 4.04e-16 1.46e-11
  distortion_only     5 1  42   -     2.37e+10 1.79e-16 4.88e-12
  one_parameter       5 1  42   -     4.81e+10 1.66e-17 1.13e-12
  thin_prism_ends     5 1  42   -     1.33e+10 7.16e-18 1.24e-12
  two_masks           5 2  54   1/1   1.70e+11 3.30e-19 2.46e-12
  const_points        7 2  66   0/1   1.45e+11 7.20e-21 0
  const_pose_camera   4 2  48   1/1   6.23e+10 1.10e-17 2.16e-11
  unused_camera       4 2  48   0/1   2.12e+20 5.06e-18 1.65e-12   (the unused slot's diagonal is 1e-4 x 1e-6)

chunks_65 (16 700 points, 66 chunks): the points of chunks 64 and 65 hold 3.5 % of the largest S_cam entry, and 97
entries of S_cam receive more from them than the comparison floor of the GPU module (1e-9 x (scale + |entry|)): a
chunk reduction that reads one partial per lane fails parity.  The reference takes 0.5 s there (2 s with the scene), so its
per-observation loops stay as they are.

unused_camera at Levenberg mu = 0: the first failing column of the reference S is 36 = 6 ns + 12, and every pivot before
it is at least 1.2e-3 of its diagonal entry (bound 1e-8): rounding cannot move the failure.

Gradient maximum (gradient_scene): 'camera' 1.77e8 in coordinate 7 of slot 7 (flat coordinate 91 of 96) against 1.46e4
over the coordinates of the first loop trip, 1.99e5 over the poses and 9.9e5 over the points; 'pose' 2.09e5 against 1.0e3
(points) and 9.5 (cameras); 'point' 7.46e8 in the last point against 1.97e5 over the other points and 2.99e6 over the
poses.  Each margin is asserted to be at least 2.

LM at eight slots (lm_eight_scene): the reference accepts TTTTFF, min |rho - 1e-3| = 0.278, cost 1.26e9 -> 3.31e7; the
reference loop with the tight PCG gives the same sequence."""
import numpy as np
import pytest

from tests import ba_pcg_cam_ref as pc
from tests import ba_schur_cam_ref as cref
from tests import ba_schur_ref as ref
from tests.test_ba_chol_cpu import cholesky_solve, eta, first_failing_column
from tests.test_ba_pcg_cam_cpu import TIGHT
from tests.test_ba_schur_cam_cpu import ETA_CAM_REFERENCE

ROUTES_AGREE = 1e-10        # the reference's two routes on every new Marquardt system; the GPU module allows 100 x that
NB = 96                     # kCholNB
CHUNK = 256                 # kCamChunk
PIVOT_MARGIN = 1e-8         # unused_camera: every pivot before the failing column, relative to its diagonal entry
LM_ACCEPTED = "TTTTFF"


def marquardt_scenes(oracle):
    """name -> (scene, refine, ns, ncs) of every new system that is solved at Marquardt 1e-4"""
    out = {}
    for name, case in cref.SLOT_CASES.items():
        out[name] = cref.slot_scene(oracle, name) + case[5:7]
    for ncs, ns in cref.PANEL_CASES:
        out[f"panel_{ncs}_{ns}"] = cref.panel_scene(oracle, ncs, ns) + (ns, ncs)
    for name, (models, _) in cref.MASK_CASES.items():
        out[name] = cref.mask_scene(oracle, name) + (5, len(models))
    out["const_points"] = cref.const_points_scene(oracle) + (7, 2)
    out["const_pose_camera"] = cref.const_pose_camera_scene(oracle) + (4, 2)
    out["unused_camera"] = cref.unused_camera_scene(oracle) + (4, 2)
    return out


@pytest.fixture(scope="module")
def systems(oracle):
    """name -> (CamNormalEquations, its blocks, ns, ncs), computed once"""
    out = {}
    for name, (s, refine, ns, ncs) in marquardt_scenes(oracle).items():
        ne = cref.CamNormalEquations(oracle, s, refine, 1e-4, "marquardt")
        out[name] = (ne, ne.schur_cam_blocks(), ns, ncs)
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _offdiag_nonzero(S_cam):
    ncs = S_cam.shape[0]
    return sum(1 for r in range(ncs) for q in range(r) if np.abs(S_cam[r, q]).max() > 0)


def test_marquardt_systems(systems):
    """two-route agreement, cond(S) and the reference's own eta on every new Marquardt system"""
    for name, (ne, sb, ns, ncs) in systems.items():
        assert (ne.pr["slot_img"].size, ne.ncs) == (ns, ncs), name
        n = 6 * ns + 12 * ncs
        assert sb["S"].shape == (n, n)
        dpose, dcam = ne.split(np.linalg.solve(sb["S"], sb["rhs_full"]))
        dpoint = ne.back_substitute_cam(dpose, dcam)
        rp, rc, rx = ne.dense_solve_cam()
        agree = max(_rel(dpose, rp), _rel(dcam, rc), _rel(dpoint, rx))
        e = eta(sb["S"], sb["rhs_full"], cholesky_solve(sb["S"], sb["rhs_full"]))
        print(f"{name}: ns {ns} ncs {ncs} n {n} panels {-(-n // NB)} off-diagonal blocks {_offdiag_nonzero(sb['S_cam'])} / "
              f"{ncs * (ncs - 1) // 2} cond {np.linalg.cond(sb['S']):.2e} eta {e:.2e} routes {agree:.2e}")
        assert agree <= ROUTES_AGREE, name
        assert e <= ETA_CAM_REFERENCE, name
        assert not dcam[~ne.cam_active].any()


def test_slot_cases(systems):
    ne, sb, _, _ = systems["three_slots"]
    assert ne.pr["P"] == 600 and -(-600 // CHUNK) == 3 and 600 % CHUNK != 0        # three chunks, the third partial
    assert _offdiag_nonzero(sb["S_cam"]) == 3                                      # pairs q = 1, 3, 4
    ne, sb, _, _ = systems["eight_mixed"]
    assert ne.cam_active.sum(axis=1).tolist() == [3, 5, 8, 5, 4, 5, 12, 8]
    assert _offdiag_nonzero(sb["S_cam"]) >= 20
    assert sorted(set(cref.SLOT_CASES["eight_mixed"][0]) | {m for c in cref.CAM_CASES for m in c[0]}) == list(range(11))
    ne, sb, ns, ncs = systems["eight_wide"]
    assert _offdiag_nonzero(sb["S_cam"]) == 28
    n0, n = 6 * ns, 6 * ns + 12 * ncs
    assert (n0, n) == (168, 264) and -(-n // NB) == 3 and NB < n0 < 2 * NB < n     # camera rows across the edge at 192
    for name in ("eight_mixed", "eight_wide"):                                     # the second trip of the 64-lane loops
        assert 12 * systems[name][3] > 64


def test_panel_cases(systems):
    want = {(1, 14): (96, 84), (2, 12): (96, 72), (1, 15): (102, 90), (2, 13): (102, 78), (2, 16): (120, 96)}
    assert sorted(want) == sorted(cref.PANEL_CASES)
    for (ncs, ns), (n, n0) in want.items():
        ne, sb, _, _ = systems[f"panel_{ncs}_{ns}"]
        assert sb["S"].shape[0] == n and 6 * ns == n0 and ne.pr["I"] == ns + 1
        assert np.flatnonzero(ne.pr["slot"] < 0).tolist() == [0]                   # image 0 alone is constant
    assert all(n0 < NB < n for n, n0 in (want[(1, 15)], want[(2, 13)]))            # camera rows astride the first edge
    assert want[(2, 16)][1] == NB                                                  # camera rows open panel 1


def test_chunks_65_later_chunks_matter(oracle):
    """what chunks 64 and 65 add to S_cam exceeds the comparison floor of the GPU module"""
    s, refine = cref.chunks_65_scene(oracle)
    ne = cref.CamNormalEquations(oracle, s, refine, 1e-4)
    P = ne.pr["P"]
    assert P == 16700 and -(-P // CHUNK) == 66 and (ne.pr["slot_img"].size, ne.ncs) == (5, 2)
    sb = ne.schur_cam_blocks()
    Wc = ne.wc()[64 * CHUNK:]
    late = -np.einsum("prak,pkl,psbl->rsab", Wc, ne.Vinv[64 * CHUNK:], Wc)
    scale = max(1.0, np.abs(sb["S_cam"]).max())
    above = int((np.abs(late) > 1e-9 * (scale + np.abs(sb["S_cam"]))).sum())
    print(f"chunks 64, 65 hold {np.abs(late).max() / np.abs(sb['S_cam']).max():.3%} of the largest S_cam entry; "
          f"{above} entries above the comparison floor")
    assert above >= 10
    assert np.abs(sb["S_cam"][1, 0]).max() > 0
    late_rhs = np.einsum("prak,pkl,pl->ra", Wc, ne.Vinv[64 * CHUNK:], ne.gpt[64 * CHUNK:])
    assert (np.abs(late_rhs) > 1e-9 * (max(1.0, np.abs(sb["rhs_cam"]).max()) + np.abs(sb["rhs_cam"]))).any()


def test_mask_cases(systems):
    want = {"principal_point": [[2, 3]], "distortion_only": [[4, 5, 6, 7]], "one_parameter": [[1]],
            "thin_prism_ends": [[0, 11]], "two_masks": [[0, 3, 5], [1, 3]]}
    for name, rows in want.items():
        ne = systems[name][0]
        assert [np.flatnonzero(a).tolist() for a in ne.cam_active] == rows, name


def test_const_points_reference(systems):
    """nothing is eliminated: S_cam is H_cam plus its damping, B is E_cam, rhs_cam is -g_cam"""
    ne, sb, ns, ncs = systems["const_points"]
    assert ne.pr["point_const"].all() and not ne.Vinv.any()
    assert not sb["S_cam"][0, 1].any() and not sb["S_cam"][1, 0].any()
    for r, c in enumerate(ne.slot_cam):
        a = ne.cam_active[r]
        assert np.array_equal(sb["S_cam"][r, r][np.ix_(a, a)], (ne.Hcam[c] + np.diag(ne.Dcam[r]))[np.ix_(a, a)])
        assert np.array_equal(sb["rhs_cam"][r][a], -ne.gcam[c][a])
    seen = 0
    for i, im in enumerate(ne.pr["slot_img"]):
        r = ne.img_cam_slot[im]
        keep = np.outer(ne.cam_active[r], ne.pr["active"][i])
        assert np.array_equal(sb["B"][i, r][keep], ne.Ecam[im][keep]) and not sb["B"][i, 1 - r].any()
        seen += int(np.abs(ne.Ecam[im][keep]).max() > 0)
    assert seen == ns


def test_const_pose_camera_reference(systems):
    ne, sb, ns, ncs = systems["const_pose_camera"]
    assert (ne.img_cam_slot[ne.pr["slot_img"]] == 0).all()          # no pose slot on camera 1: no E_cam term in B[:, 1]
    assert np.abs(sb["B"][:, 1]).max() > 0 and np.abs(sb["S_cam"][1, 0]).max() > 0


def test_unused_camera_reference(oracle, systems):
    ne, sb, ns, ncs = systems["unused_camera"]
    dcam = ne.split(np.linalg.solve(sb["S"], sb["rhs_full"]))[1]
    assert not dcam[1].any() and dcam[0].any()                      # Marquardt: rhs 0 on the unused slot, step exactly 0
    s, refine = cref.unused_camera_scene(oracle)
    S = cref.CamNormalEquations(oracle, s, refine, 0.0, "levenberg").schur_cam_blocks()["S"]
    k = first_failing_column(S)
    assert k == 6 * ns + 12 == 36
    L = np.linalg.cholesky(S[:k, :k])
    margin = (np.diag(L) ** 2 / np.diag(S[:k, :k])).min()
    print(f"first failing column {k}; smallest pivot before it / its diagonal entry {margin:.3e}")
    assert margin > PIVOT_MARGIN


def _gradient(oracle, where):
    s, refine = cref.gradient_scene(oracle, where)
    ne = ref.NormalEquations(oracle, s, 1e-4) if refine is None else cref.CamNormalEquations(oracle, s, refine, 1e-4)
    return ne, cref.gradient_max(ne)


def test_gradient_maximum_sits_where_the_scenes_say(oracle):
    ne, (m, parts) = _gradient(oracle, "camera")
    g = (np.abs(ne.gcam[ne.slot_cam].reshape(-1, 12)) * ne.cam_active).reshape(-1)
    assert ne.ncs == 8 and g.size == 96
    print(f"camera: {parts}, at flat coordinate {g.argmax()}, first trip {g[:64].max():.4g}")
    assert m == parts["camera"] == g.max() and g.argmax() >= 84                    # slot 7
    assert m >= 2 * max(g[:64].max(), parts["pose"], parts["point"])
    ne, (m, parts) = _gradient(oracle, "pose")
    print(f"pose: {parts}")
    assert m == parts["pose"] >= 2 * max(parts["point"], parts["camera"]) and ne.ncs == 8
    ne, (m, parts) = _gradient(oracle, "point")
    P = ne.pr["P"]
    others = np.abs(ne.gpt[:P - 1][ne.pr["point_const"][:P - 1] == 0]).max()
    print(f"point: {parts}, the other points {others:.4g}")
    assert P == 16700 and m == parts["point"] == np.abs(ne.gpt[P - 1]).max() >= 2 * max(others, parts["pose"])


def test_gradient_max_counts_skipped_points_and_no_constants(oracle):
    """the definition itself, on a scene with rank-deficient (skipped) points: they count, constants do not"""
    s, bad = ref.degenerate_scene(oracle, 71)
    ne = ref.NormalEquations(oracle, s, 0.0)
    assert ne.skipped.any()
    m, parts = cref.gradient_max(ne)
    assert parts["point"] == np.abs(ne.gpt).max() >= np.abs(ne.gpt[ne.skipped]).max() > 0 and parts["camera"] == 0.0
    s["point_const"][np.abs(ne.gpt).max(axis=1).argmax()] = 1
    assert cref.gradient_max(ref.NormalEquations(oracle, s, 0.0))[1]["point"] < parts["point"]
    assert parts["pose"] == np.abs(ne.gimg[ne.pr["slot_img"]])[ne.pr["active"]].max()


def test_lm_at_eight_slots_has_margins(oracle):
    s, refine, radius = cref.lm_eight_scene(oracle)
    hist, _ = cref.lm_cam(oracle, s, refine, 6, initial_radius=radius)
    print("accepted", "".join("T" if h["accepted"] else "F" for h in hist), "rho", [h["rho"] for h in hist], "cost",
          [h["cost"] for h in hist])
    assert "".join("T" if h["accepted"] else "F" for h in hist) == LM_ACCEPTED
    assert all(np.isfinite(h["rho"]) and abs(h["rho"] - 1e-3) > 0.05 for h in hist)
    tight, _ = pc.lm_cam_pcg(oracle, s, refine, 6, initial_radius=radius, linear=dict(max_iterations=2000, **TIGHT))
    assert [h["accepted"] for h in tight] == [h["accepted"] for h in hist]
    assert all(h["linear_termination"] == pc.R_TOLERANCE for h in tight)

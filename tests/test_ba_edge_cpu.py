"""The oracle at the camera models' branch points (no GPU): tests/ba_edge_ref.py's catalogue lands where it says,
the Jet oracle is finite there, agrees with a 50-digit evaluation of the same branch formula and its derivatives
(mpmath), and with finite differences taken inside one branch.

Oracle against mpmath, worst |oracle - mpmath| / column scale per branch tag.  Column = d(x, y)/d(u), d/d(v) or
d/d(camera parameter k); column scale = max |mpmath column| over the catalogue entries of the same model (what a
single-model edge scene holds), the scale tests/test_ba_edge_gpu.py applies.  Measured with this file
(test_oracle_vs_mpmath prints the figures); the test holds the oracle to four times these, with one rounding
(2^-53) as the floor for a figure that came out smaller:

    branch tag     worst relative error   in column
    small_omega    1.63e-16               FOV ray (0, 0), d/du
    small_radius   3.24e-16               FOV ray (0, 0), d/dv
    general        1.77e-14               FOV omega = 1.01e-2, ray (2, -1.5), d/d(omega): atan(..)/omega against its own derivative
    r_le_eps       2.4e-36                THIN_PRISM_FISHEYE ray (1e-16, 1e-16), d/du
    r_gt_eps       3.47e-16               THIN_PRISM_FISHEYE ray (1e-12, 2e-12), d/dv
    mid            3.49e-16               OPENCV_FISHEYE ray (0.3, 0.2), d/du
    wide           5.68e-16               SIMPLE_RADIAL_FISHEYE ray (11.4, 0), d/df
    poly           4.04e-16               FULL_OPENCV ray (1.5, -1.2), d/dk5
    pinhole        0                      -

Every figure but one is a few units of double rounding (the FOV general branch at omega just above 1e-2 differentiates
atan(2 r tan(omega / 2)) / (r omega) by omega as a difference of two terms of size 1 / omega).  The cancellation in
u * theta_d / r - u just above r = eps costs an absolute error of eps * |u|, far below any column scale, and the
quotient rule of d(theta_d / r) multiplies its own cancellation (r - theta_d, absolute error eps * r, divided by r^2)
by u ~ r again.  No column needs an allowance
beyond the project's 1e-9 on the device side."""
import numpy as np
import pytest

from tests import ba_edge_ref as er

import mpmath as mp  # noqa: E402

# worst relative error per branch tag, from the table above
MEASURED = {"small_omega": 1.63e-16, "small_radius": 3.24e-16, "general": 1.77e-14, "r_le_eps": 2.4e-36,
            "r_gt_eps": 3.47e-16, "mid": 3.49e-16, "wide": 5.68e-16, "poly": 4.04e-16, "pinhole": 0.0}
ONE_ROUNDING = 2.0 ** -53


def _mp_world_to_image(model, branch, p, u, v):
    """base/camera_models.h WorldToImage on the given branch, in mpmath numbers (p: parameters, u, v: the ray)"""
    def fisheye(k):
        if branch == "r_le_eps":
            return u, v
        r = mp.sqrt(u * u + v * v)
        th = mp.atan(r)
        thd = th * (1 + sum(kj * th ** (2 * j + 2) for j, kj in enumerate(k)))
        return u + (u * thd / r - u), v + (v * thd / r - v)
    if model == 0:
        return p[0] * u + p[1], p[0] * v + p[2]
    if model == 1:
        return p[0] * u + p[2], p[1] * v + p[3]
    if model in (2, 3):
        r2 = u * u + v * v
        rad = p[3] * r2 + (p[4] * r2 * r2 if model == 3 else 0)
        return p[0] * (u + u * rad) + p[1], p[0] * (v + v * rad) + p[2]
    if model in (4, 6):
        r2 = u * u + v * v
        if model == 4:
            rad = 1 + p[4] * r2 + p[5] * r2 ** 2
        else:
            rad = (1 + p[4] * r2 + p[5] * r2 ** 2 + p[8] * r2 ** 3) / (1 + p[9] * r2 + p[10] * r2 ** 2 + p[11] * r2 ** 3)
        xu = u * rad + 2 * p[6] * u * v + p[7] * (r2 + 2 * u * u)
        xv = v * rad + 2 * p[7] * u * v + p[6] * (r2 + 2 * v * v)
        return p[0] * xu + p[2], p[1] * xv + p[3]
    if model == 5:
        xu, xv = fisheye(p[4:8])
        return p[0] * xu + p[2], p[1] * xv + p[3]
    if model == 7:
        om, rad2 = p[4], u * u + v * v
        if branch == "small_omega":
            fac = om * om * rad2 / 3 - om * om / 12 + 1
        elif branch == "small_radius":
            t = mp.tan(om / 2)
            fac = (-2 * t * (4 * rad2 * t * t - 3)) / (3 * om)
        else:
            rad = mp.sqrt(rad2)
            fac = mp.atan(rad * 2 * mp.tan(om / 2)) / (rad * om)
        return p[0] * u * fac + p[2], p[1] * v * fac + p[3]
    if model in (8, 9):
        xu, xv = fisheye(p[3:4] if model == 8 else p[3:5])
        return p[0] * xu + p[1], p[0] * xv + p[2]
    uu, vv = u, v
    if branch != "r_le_eps":
        r = mp.sqrt(u * u + v * v)
        th = mp.atan(r)
        uu, vv = th * u / r, th * v / r
    r2 = uu * uu + vv * vv
    rad = p[4] * r2 + p[5] * r2 ** 2 + p[8] * r2 ** 3 + p[9] * r2 ** 4
    du = uu * rad + 2 * p[6] * uu * vv + p[7] * (r2 + 2 * uu * uu) + p[10] * r2
    dv = vv * rad + 2 * p[7] * uu * vv + p[6] * (r2 + 2 * vv * vv) + p[11] * r2
    return p[0] * (uu + du) + p[2], p[1] * (vv + dv) + p[3]


def _mp_reference(e):
    """(xy [2], J [2][2 + K]) at 50 digits: columns d/du, d/dv, then d/d(parameter k)"""
    K = len(e["cam"])
    branch = er.formula_branch(e["model"], e["cam"], *e["ray"])
    with mp.workdps(50):
        args = [mp.mpf(float(e["ray"][0])), mp.mpf(float(e["ray"][1]))] + [mp.mpf(float(c)) for c in e["cam"]]
        xy = _mp_world_to_image(e["model"], branch, args[2:], args[0], args[1])
        J = np.zeros((2, 2 + K))
        for row in range(2):
            f = lambda *a: _mp_world_to_image(e["model"], branch, a[2:], a[0], a[1])[row]
            for k in range(2 + K):
                order = tuple(1 if j == k else 0 for j in range(2 + K))
                J[row, k] = float(mp.diff(f, tuple(args), order))
        return np.array([float(xy[0]), float(xy[1])]), J


def _oracle_at_identity(oracle, e):
    """the oracle's block at identity pose and depth 4 (u = P.x / 4 exactly): (xy, J [2][2 + K])"""
    u, v = e["ray"]
    r, Jq, Jt, JX, Jc = oracle.reproj_block(e["model"], [1, 0, 0, 0], [0, 0, 0], [4 * u, 4 * v, 4.0], e["cam"], [0, 0])
    return r, np.concatenate([4.0 * JX[:, :2], Jc], axis=1), (Jq, Jt, JX, Jc)


def test_catalogue_covers_the_issue_and_lands_on_its_branches(oracle):
    tags = {(e["model"], e["tag"]) for e in er.CATALOGUE}
    for m in er.FISHEYE:
        assert {(m, "r_le_eps"), (m, "r_gt_eps"), (m, "mid"), (m, "wide")} <= tags
        assert any(e["model"] == m and not e["cam"][-1] and not e["cam"][len(e["cam"]) - len(er.EXTRA[m])] for e in er.CATALOGUE)
    assert {(7, "small_omega"), (7, "small_radius"), (7, "general")} <= tags
    assert {(m, "poly") for m in (2, 3, 4, 6)} | {(0, "pinhole"), (1, "pinhole")} <= tags
    assert {e["cam"][4] for e in er.CATALOGUE if e["model"] == 7} == {0.0, 1e-6, 9.9e-3, 1.01e-2, 0.9}
    # the builder's own assertion (check_branches) on every scene the GPU tests use
    for m in range(11):
        s = er.edge_scene(oracle, models=(m,), seed=m)
        assert len(s["_edge"]) == sum(e["model"] == m for e in er.CATALOGUE)
        assert (np.bincount(s["obs_point"]) >= 2).all()
    for pad in (False, True):
        s = er.edge_scene(oracle, cameras=er.MIXED_CAMERAS, seed=20, padding=pad)
        assert sorted(set(s["cam_model"].tolist())) == [4, 5, 7, 10]
        lanes = {o % 64 for o, _ in s["_edge"]}
        assert not pad or (len(lanes) > len(s["_edge"]) // 2 and np.bincount(s["obs_image"]).max() > 1024)
        sc = np.linalg.norm(s["poses"][:, :4], axis=1)
        assert 0.2 < np.mean(np.abs(sc - 1) > 0.01) < 0.6 and sc.min() >= 0.6 and sc.max() <= 1.7
        assert s["image_const_pose"].sum() == 1 and s["image_const_tvec"].any() and 0 < s["point_const"].mean() < 0.25


def test_oracle_finite_at_every_entry(oracle):
    for e in er.CATALOGUE:
        r, J, blocks = _oracle_at_identity(oracle, e)
        assert np.isfinite(r).all() and all(np.isfinite(b).all() for b in blocks), e
        if e["tag"] == "r_le_eps" and e["model"] != 10:      # theta_d distortion and its derivatives vanish (THIN_PRISM
            # keeps its polynomial in the unmapped ray)
            K0 = len(e["cam"]) - len(er.EXTRA[e["model"]])
            assert not blocks[3][:, K0:].any(), e


def test_oracle_vs_mpmath(oracle):
    ref = [(_mp_reference(e)) for e in er.CATALOGUE]
    worst = {t: (0.0, None) for t in er.TAGS}
    for e, (xy, J) in zip(er.CATALOGUE, ref):
        same = [k for k, f in enumerate(er.CATALOGUE) if f["model"] == e["model"]]
        scale = np.max([np.abs(ref[k][1]) for k in same], axis=(0, 1))            # per column over the model's entries
        xscale = np.max([np.abs(ref[k][0]) for k in same])
        r, Jo, _ = _oracle_at_identity(oracle, e)
        assert np.abs(r - xy).max() <= 16 * ONE_ROUNDING * xscale, (e, r, xy)      # a chain of about ten operations
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(scale > 0, np.abs(Jo - J) / scale, np.where(Jo == J, 0.0, np.inf))
        k = np.unravel_index(np.argmax(rel), rel.shape)
        if rel[k] > worst[e["tag"]][0]:
            worst[e["tag"]] = (float(rel[k]), "model %d ray %r column %d" % (e["model"], e["ray"], k[1]))
    for t in er.TAGS:
        print("%-13s %.3e   %s" % (t, worst[t][0], worst[t][1]))
    for t in er.TAGS:
        assert worst[t][0] <= 4 * max(MEASURED[t], ONE_ROUNDING), (t, worst[t])
    # what the GPU test may add to 1e-9 for a column: four times the measured error -- nothing visible
    assert 4 * max(MEASURED.values()) < 1e-3 * er.REL


def test_fov_omega_column_flips_sign_across_the_threshold(oracle):
    """d(x, y)/d(omega) for the same ray on either side of omega^2 = 1e-4 (camera_models.h:1105-1160): the two
    formulas the reference switches between disagree in sign there, so a device that took the other branch, or tested
    omega instead of omega^2, shows up in the camera column"""
    lo = dict(model=7, cam=er.cam_params(7, extra=[0.0099]), ray=(0.0101, 0.0))
    hi = dict(model=7, cam=er.cam_params(7, extra=[0.0101]), ray=(0.0101, 0.0))
    a, b = _oracle_at_identity(oracle, lo)[1][0, 2 + 4], _oracle_at_identity(oracle, hi)[1][0, 2 + 4]
    assert -0.02 < a < -0.005 and 0.005 < b < 0.02, (a, b)
    assert abs(_mp_reference(lo)[1][0, 6] - a) < 1e-12 and abs(_mp_reference(hi)[1][0, 6] - b) < 1e-12


@pytest.mark.parametrize("tag", er.TAGS)
def test_finite_differences_inside_one_branch(oracle, tag):
    """tests/test_oracle_cpu.py's central differences at one interior entry per branch tag.  A difference is taken only
    when both perturbed arguments evaluate the formula of the entry itself; the r <= eps branch is narrower than any
    usable step in the pose and the point (camera-parameter steps leave the ray alone), so there the camera columns
    are differenced and the pose / point columns are pinned by test_oracle_vs_mpmath alone."""
    pick = {"small_omega": (7, 9.9e-3, (0.3, 0.2)), "small_radius": (7, 0.9, (0.004, -0.006)), "general": (7, 0.9, (0.3, 0.2)),
            "r_le_eps": (5, None, (0.0, 0.0)), "r_gt_eps": (5, None, (1e-8, 0.0)), "mid": (9, None, (0.3, 0.2)), "wide": (10, None, (5.0, 3.0)),
            "poly": (6, None, (1.5, -1.2)), "pinhole": (1, None, (0.0, 0.0))}[tag]
    e = next(f for f in er.CATALOGUE if f["model"] == pick[0] and f["ray"] == pick[2] and f["tag"] == tag
             and (pick[1] is None or f["cam"][4] == pick[1]))
    rng = np.random.default_rng(5)
    model, cam, obs = e["model"], e["cam"].copy(), np.zeros(2)
    if e["exact"]:
        q, t = np.array([1.0, 0, 0, 0]), np.array([0.0, 0, 1.0])
        X = np.array([4 * e["ray"][0], 4 * e["ray"][1], 3.0])
    else:
        pose = er._generic_pose(rng)
        q, t = pose[:4] * 1.3, pose[4:]                       # off-unit: the polynomial's own derivative
        X = np.linalg.solve(er.rotation_matrix_poly(q), np.array([e["ray"][0] * 6.0, e["ray"][1] * 6.0, 6.0]) - t)
    home = er.formula_branch(model, cam, *er.camera_ray(np.concatenate([q, t]), X)[1])
    assert home == er.formula_branch(model, cam, *e["ray"])
    r, Jq, Jt, JX, Jc = oracle.reproj_block(model, q, t, X, cam, obs)
    done = 0
    for J, arg, n in ((Jq, 0, 4), (Jt, 1, 3), (JX, 2, 3), (Jc, 3, len(cam))):
        if tag == "r_le_eps" and arg != 3:
            continue
        ref = np.zeros((2, n))
        for k in range(n):
            h = 1e-6 * max(1.0, abs([q, t, X, cam][arg][k]))
            a = [q.copy(), t.copy(), X.copy(), cam.copy()]; b = [q.copy(), t.copy(), X.copy(), cam.copy()]
            a[arg][k] += h; b[arg][k] -= h
            for side in (a, b):        # never across a threshold
                assert er.formula_branch(model, side[3], *er.camera_ray(np.concatenate(side[:2]), side[2])[1]) == home
            ref[:, k] = (oracle.reproj_residual(model, *a, obs) - oracle.reproj_residual(model, *b, obs)) / (2 * h)
        assert np.allclose(J, ref, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(ref).max())), (tag, arg, J, ref)
        done += 1
    assert done == (1 if tag == "r_le_eps" else 4)

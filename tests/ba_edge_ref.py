"""Edge catalogue of the camera models and the scenes built from it (host only, test infrastructure).

Every BA kernel evaluates base/camera_models.h WorldToImage through csrc/ba_math.h (pose / point Jacobians) and
csrc/ba_cam_jac.h (camera Jacobians).  Both hold data-dependent branches:
  FOV (7)                 omega^2 < 1e-4 | radius^2 < 1e-4 | general          (camera_models.h:1105-1160)
  fisheye (5, 8, 9, 10)   r > DBL_EPSILON | r <= DBL_EPSILON                  (:963-990, :1272-1290, :1348-1370, :1405-1482)
CATALOGUE lists (model, camera parameters, camera-frame ray, branch tag) at and around those thresholds, at the wide
end of a fisheye lens, and one or two rays for the branch-free models.  edge_scene turns the entries of the requested
models into a pcdhip.BA / oracle.BA problem in which every entry is one observation; the builder recomputes
P = R(q) X + t with the rotation polynomial in numpy and asserts that each entry sits on its tagged branch.

Tolerance helpers: the project's 1e-9 relative (tests/test_ba_gpu.py), applied per column -- see col_close."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
NUM_PARAMS = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]
FISHEYE = (5, 8, 9, 10)
F1, F2, CX, CY = 651.123, 655.123, 386.123, 511.123      # the reference test's values (golden/reference_kats.json)
# moderate distortion (tests/ba_schur_ref.camera_params)
EXTRA = {0: [], 1: [], 2: [-0.03], 3: [-0.03, 0.005], 4: [-0.05, 0.01, 1e-4, 1e-4], 5: [0.02, -0.01, 0.003, -0.001],
         6: [-0.05, 0.01, 1e-4, 1e-4, 0.002, 0.01, -0.005, 0.001], 7: [0.4], 8: [0.02], 9: [0.02, -0.004],
         10: [0.02, -0.01, 1e-4, -1e-4, 0.003, -0.001, 2e-4, -1e-4]}
REL = 1e-9                                                # the project's bar


def cam_params(model, variant=0, extra=None):
    """variant 0: the values above; variant k: focal lengths * (1 + 1e-3 k), coefficients * (1 + 0.25 k);
    extra overrides the coefficient vector (FOV omega, all-zero fisheye coefficients)"""
    nf = 1 if model in (0, 2, 3, 8, 9) else 2
    s = 1.0 + 1e-3 * variant
    ex = [c * (1.0 + 0.25 * variant) for c in EXTRA[model]] if extra is None else list(extra)
    p = np.array([F1 * s, F2 * s][:nf] + [CX, CY] + ex, np.float64)
    assert p.shape[0] == NUM_PARAMS[model]
    return p


def formula_branch(model, cam, u, v):
    """which formula WorldToImage evaluates at this ray"""
    if model == 7:
        om2 = cam[4] * cam[4]
        if om2 < 1e-4:
            return "small_omega"
        return "small_radius" if u * u + v * v < 1e-4 else "general"
    if model in FISHEYE:
        return "r_gt_eps" if np.sqrt(u * u + v * v) > EPS else "r_le_eps"
    return "poly" if model in (2, 3, 4, 6) else "pinhole"


def branch_tag(model, cam, u, v):
    """formula_branch, with the r > eps side of the fisheye models split by region: cancellation (r < 1e-6,
    u * theta_d / r - u loses every digit), wide (r > 3, the outer end of a fisheye lens), mid (the rest)"""
    b = formula_branch(model, cam, u, v)
    if b == "r_gt_eps":
        r = np.sqrt(u * u + v * v)
        return "r_gt_eps" if r < 1e-6 else ("wide" if r > 3.0 else "mid")
    return b


def threshold_margin(model, cam, u, v):
    """smallest relative distance of the quantities the branches test to their thresholds"""
    m = np.inf
    if model == 7:
        om2 = cam[4] * cam[4]
        m = abs(om2 / 1e-4 - 1.0)
        if om2 >= 1e-4:
            m = min(m, abs((u * u + v * v) / 1e-4 - 1.0))
    elif model in FISHEYE:
        m = abs(np.sqrt(u * u + v * v) / EPS - 1.0)
    return m


def _entries():
    out = []

    def add(model, cam, ray, tag, exact, cam_name):
        out.append(dict(model=model, cam=np.asarray(cam, np.float64), ray=(float(ray[0]), float(ray[1])), tag=tag,
                        exact=exact, cam_name=cam_name))
    fov = lambda om: cam_params(7, extra=[om])
    for om in (0.0, 1e-6, 9.9e-3):
        for ray in ((0, 0), (0.0099, 0), (0.0101, 0), (0.3, 0.2)):
            add(7, fov(om), ray, "small_omega", ray == (0, 0), "fov_%g" % om)
    for om in (1.01e-2, 0.9):
        for ray in ((0, 0), (0.0099, 0), (0.004, -0.006)):
            add(7, fov(om), ray, "small_radius", ray == (0, 0), "fov_%g" % om)
        for ray in ((0.0101, 0), (0.3, 0.2), (2.0, -1.5)):
            add(7, fov(om), ray, "general", False, "fov_%g" % om)
    for m in FISHEYE:
        cams = [("k0", cam_params(m, 0)), ("k1", cam_params(m, 1)), ("zero", cam_params(m, extra=[0.0] * len(EXTRA[m])))]
        for name, cam in cams:
            for ray in ((0, 0), (1e-17, 0), (1e-16, 1e-16)):
                add(m, cam, ray, "r_le_eps", True, "m%d_%s" % (m, name))
            for ray in ((3e-16, 0), (1e-15, 0), (1e-12, 2e-12), (1e-8, 0)):
                add(m, cam, ray, "r_gt_eps", True, "m%d_%s" % (m, name))
            add(m, cam, (0.3, 0.2), "mid", False, "m%d_%s" % (m, name))
            for ray in ((5, 3), (11.4, 0), (0, -11.4)):
                add(m, cam, ray, "wide", False, "m%d_%s" % (m, name))
    for m in (2, 3, 4, 6):
        for k in (0, 1):
            for ray in ((0, 0), (1.5, -1.2)):
                add(m, cam_params(m, k), ray, "poly", ray == (0, 0), "m%d_k%d" % (m, k))
    for m in (0, 1):
        for k in (0, 1):
            add(m, cam_params(m, k), (0, 0), "pinhole", True, "m%d_k%d" % (m, k))
    for e in out:
        assert branch_tag(e["model"], e["cam"], *e["ray"]) == e["tag"], e
        assert e["exact"] or threshold_margin(e["model"], e["cam"], *e["ray"]) >= 0.01, e
    return out


CATALOGUE = _entries()
TAGS = ("small_omega", "small_radius", "general", "r_le_eps", "r_gt_eps", "mid", "wide", "poly", "pinhole")
# the mixed scene: FOV on its small-omega and on its large-omega branches, two fisheye models and OPENCV in one handle
MIXED_CAMERAS = ("fov_1e-06", "fov_0.9", "m5_k0", "m10_k0", "m4_k0")


# ---------------------------------------------------------------- geometry ---
def rotate_poly(q, X):
    """ceres::UnitQuaternionRotatePoint's polynomial X + 2w (v x X) + 2 v x (v x X), q not normalised"""
    w, v = q[0], np.asarray(q[1:4])
    uv = 2.0 * np.cross(v, X)
    return np.asarray(X) + w * uv + np.cross(v, uv)


def rotation_matrix_poly(q):
    """the same polynomial as a matrix: I + 2w [v]x + 2 (v v^T - |v|^2 I)"""
    w, v = q[0], np.asarray(q[1:4], np.float64)
    vx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + 2.0 * w * vx + 2.0 * (np.outer(v, v) - (v @ v) * np.eye(3))


def camera_ray(pose, X):
    """(u, v) both ways the code under test and the oracle form it: P.xy * (1 / P.z) and P.xy / P.z"""
    P = rotate_poly(pose[:4], X) + pose[4:]
    iz = 1.0 / P[2]
    return (P[0] * iz, P[1] * iz), (P[0] / P[2], P[1] / P[2]), P


def _generic_pose(rng):
    rv = rng.uniform(-0.06, 0.06, 3)
    a = np.linalg.norm(rv)
    q = np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * rv / a])
    return np.concatenate([q, rng.uniform(-0.3, 0.3, 3)])


EXACT_TZ_PZ = ((1.0, 4.0), (5.0, 8.0))       # exact images: identity rotation, t = (0, 0, tz); points at depth Pz - tz


def edge_scene(oracle, models=None, cameras=None, seed=0, padding=False, noise=2.0, loss=None):
    """pcdhip.BA / oracle.BA keyword arguments.  Every catalogue entry of `models` (or of the cameras named in
    `cameras`) is one observation; its point has a second observation from a neighbouring image of the same camera and,
    mostly, a LiDAR term.  Per camera: two exact images (identity rotation, t = (0, 0, tz), points at a depth that makes
    P.z a power of two, so u = P.x / P.z is the catalogue's double exactly) and three generic ones.  One generic image
    per scene has a constant pose, some images constant tvec components, about 10 % of the points are constant, about a
    third of the images carry quaternions scaled by 0.6-1.7 (the Jacobian is that of the unnormalised polynomial).
    padding: adds a synth.ba_scene on two more images of camera 0 (more than 1024 observations each) and shuffles all
    observations, so the edge observations sit at varied lane positions.
    The returned dict carries the key "_edge": per catalogue observation (observation index, entry)."""
    from pcdhip import synth
    from tests import ba_schur_ref
    rng = np.random.default_rng(1000 + seed)
    ents = [e for e in CATALOGUE if (cameras is None or e["cam_name"] in cameras) and (models is None or e["model"] in models)]
    assert ents
    names = []
    for e in ents:
        if e["cam_name"] not in names:
            names.append(e["cam_name"])
    if cameras is not None:
        names = [n for n in cameras if n in names]
    cam_of = {n: k for k, n in enumerate(names)}
    cam_model = np.array([next(e["model"] for e in ents if e["cam_name"] == n) for n in names], np.int32)
    cam_list = [next(e["cam"] for e in ents if e["cam_name"] == n) for n in names]
    poses, image_camera, exact_imgs, generic_imgs = [], [], {}, {}
    for c in range(len(names)):
        exact_imgs[c], generic_imgs[c] = [], []
        for tz, _ in EXACT_TZ_PZ:
            exact_imgs[c].append(len(poses)); poses.append([1, 0, 0, 0, 0, 0, tz]); image_camera.append(c)
        for _ in range(3):
            generic_imgs[c].append(len(poses)); poses.append(_generic_pose(rng)); image_camera.append(c)
    poses = np.array(poses, np.float64)
    I = poses.shape[0]
    scaled = rng.random(I) < 1.0 / 3.0
    scaled[[exact_imgs[0][1], generic_imgs[0][0]]] = True            # at least one of either kind
    poses[scaled, :4] *= rng.uniform(0.6, 1.7, (int(scaled.sum()), 1))
    points, obs_image, obs_point, edge = [], [], [], []
    for k, e in enumerate(ents):
        c = cam_of[e["cam_name"]]
        u, v = e["ray"]
        if e["exact"]:
            j = k % 2
            im = exact_imgs[c][j]
            tz, pz = EXACT_TZ_PZ[j]
            X = np.array([u * pz, v * pz, pz - tz])
        else:
            im = generic_imgs[c][k % 3]
            d = rng.uniform(4.0, 9.0)
            X = np.linalg.solve(rotation_matrix_poly(poses[im, :4]), np.array([u * d, v * d, d]) - poses[im, 4:])
        nb = [g for g in generic_imgs[c] if g != im][k % 2]
        edge.append((len(obs_image), e))
        obs_image += [im, nb]; obs_point += [len(points)] * 2
        points.append(X)
    points = np.array(points, np.float64)
    P = points.shape[0]
    lp = np.flatnonzero(rng.random(P) < 0.85).astype(np.int32)
    nrm = rng.normal(size=(len(lp), 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    near = points[lp] + rng.normal(0, 0.05, (len(lp), 3))
    s = dict(cam_model=cam_model, cam_params_list=cam_list, poses=poses, image_camera=np.array(image_camera, np.int32),
             points=points, obs_image=np.array(obs_image, np.int32), obs_point=np.array(obs_point, np.int32),
             lidar_point=lp, lidar_abcd=np.concatenate([nrm, -np.sum(nrm * near, 1, keepdims=True)], axis=1),
             lidar_weight=np.where(rng.random(len(lp)) < 0.35, 1000.0, 100.0))
    cpose = np.zeros(I, np.uint8); cpose[generic_imgs[len(names) - 1][2]] = 1
    tv = (rng.integers(1, 8, I) * (rng.random(I) < 0.3)).astype(np.uint8); tv[exact_imgs[0][0]] = 0b010
    pc = (rng.random(P) < 0.1).astype(np.uint8); pc[0] = 0; pc[P - 1] = 1
    if padding:
        pad = synth.ba_scene(2, 2600, seed=77 + seed)
        s["poses"] = np.concatenate([s["poses"], pad["poses"]])
        s["image_camera"] = np.concatenate([s["image_camera"], [0, 0]]).astype(np.int32)
        s["obs_image"] = np.concatenate([s["obs_image"], pad["obs_image"] + I]).astype(np.int32)
        s["obs_point"] = np.concatenate([s["obs_point"], pad["obs_point"] + P]).astype(np.int32)
        s["points"] = np.concatenate([s["points"], pad["points"]])
        s["lidar_point"] = np.concatenate([s["lidar_point"], pad["lidar_point"] + P]).astype(np.int32)
        s["lidar_abcd"] = np.concatenate([s["lidar_abcd"], pad["lidar_abcd"]])
        s["lidar_weight"] = np.concatenate([s["lidar_weight"], pad["lidar_weight"]])
        cpose = np.concatenate([cpose, [0, 0]]).astype(np.uint8)
        tv = np.concatenate([tv, [0, 0b100]]).astype(np.uint8)
        pc = np.concatenate([pc, (rng.random(len(pad["points"])) < 0.1)]).astype(np.uint8)
        assert np.bincount(pad["obs_image"]).min() > 1024
    s.update(image_const_pose=cpose, image_const_tvec=tv, point_const=pc)
    if loss is not None:
        s.update(loss_type=loss[0], loss_scale=loss[1])
    ba_schur_ref.reproject(oracle, s, rng, noise=noise)
    if padding:
        perm = rng.permutation(len(s["obs_image"]))
        s["obs_image"], s["obs_point"], s["obs_xy"] = s["obs_image"][perm], s["obs_point"][perm], s["obs_xy"][perm]
        inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
        edge = [(int(inv[o]), e) for o, e in edge]
    check_branches(s, edge)
    s["_edge"] = edge
    return s


def check_branches(s, edge):
    """P = R(q) X + t again with the rotation polynomial: every catalogue observation is on its tagged branch (exact
    entries at exactly the catalogue's ray, the others at least 1 % from every threshold), and no observation of the
    scene sits where P.xy * (1 / P.z) and P.xy / P.z would fall on different branches"""
    for o, e in edge:
        im, pt = s["obs_image"][o], s["obs_point"][o]
        c = s["image_camera"][im]
        assert s["cam_model"][c] == e["model"] and np.array_equal(s["cam_params_list"][c], e["cam"])
        a, b, P = camera_ray(s["poses"][im], s["points"][pt])
        if e["exact"]:
            assert a == e["ray"] and b == e["ray"] and P[2] in (4.0, 8.0), (e, a, b, P)
        else:
            assert np.allclose(a, e["ray"], rtol=1e-12, atol=1e-15), (e, a)
            assert min(threshold_margin(e["model"], e["cam"], *a), threshold_margin(e["model"], e["cam"], *b)) >= 0.01, e
        assert branch_tag(e["model"], e["cam"], *a) == e["tag"] and branch_tag(e["model"], e["cam"], *b) == e["tag"], (e, a, b)
    for o in range(len(s["obs_image"])):
        im = s["obs_image"][o]
        c = s["image_camera"][im]
        m, cam = int(s["cam_model"][c]), s["cam_params_list"][c]
        a, b, P = camera_ray(s["poses"][im], s["points"][s["obs_point"][o]])
        assert formula_branch(m, cam, *a) == formula_branch(m, cam, *b), (o, a, b)
        # neighbours of the wide fisheye rays may see their point near the image plane, which atan keeps bounded; the
        # polynomial models must stay where their distortion means something, and no depth may come close to zero
        assert np.isfinite(a).all() and abs(P[2]) > 1e-4 * np.linalg.norm(P), (o, a, P)
        assert m in FISHEYE or m == 7 or max(abs(a[0]), abs(a[1])) < 4.0, (o, a)


def scene_kwargs(s):
    return {k: v for k, v in s.items() if not k.startswith("_")}


def pz_zero_scene(oracle, seed=0):
    """an OPENCV edge scene plus one point at P.z == 0 exactly in the first exact image (identity rotation,
    t = (0, 0, 1), X.z = -1), with a second observation from a generic image.  Returns (kwargs, observation, image,
    point) of the singular observation."""
    s = edge_scene(oracle, models=(4,), seed=seed)
    kw = scene_kwargs(s)
    P, O = kw["points"].shape[0], len(kw["obs_image"])
    kw["points"] = np.concatenate([kw["points"], [[0.3, 0.2, -1.0]]])
    kw["point_const"] = np.concatenate([kw["point_const"], [0]]).astype(np.uint8)
    kw["obs_image"] = np.concatenate([kw["obs_image"], [0, 2]]).astype(np.int32)
    kw["obs_point"] = np.concatenate([kw["obs_point"], [P, P]]).astype(np.int32)
    kw["obs_xy"] = np.concatenate([kw["obs_xy"], [[400.0, 500.0], [300.0, 600.0]]])
    with np.errstate(divide="ignore"):
        assert camera_ray(kw["poses"][0], kw["points"][P])[2][2] == 0.0
    return kw, O, 0, P


# --------------------------------------------------------------- tolerance ---
def col_close(got, ref, what, rel=REL):
    """|got - ref| <= rel * scale, the scale taken per column over the whole scene:
      [N][K] or [N][R][K] Jacobian blocks   scale_k = max |ref[..., k]|
      1-d (residuals, cost)                 scale   = max |ref|
    so that an error in a column of small magnitude (d/d omega ~ 1e-6) cannot hide behind a focal-length column (~650).
    A column that is zero in the oracle must be exactly zero."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    assert np.isfinite(ref).all(), what + ": oracle not finite"
    assert np.isfinite(got).all(), what + ": not finite"
    if ref.ndim == 1:
        scale = np.abs(ref).max()
    else:
        scale = np.abs(ref).reshape(-1, ref.shape[-1]).max(axis=0)
    err = np.abs(got - ref)
    bad = err > rel * scale
    if bad.any():
        i = np.unravel_index(np.argmax(err / np.maximum(rel * scale, 1e-300) * bad), err.shape)
        raise AssertionError("%s: %d entries off, worst at %s: got %r oracle %r column scale %r"
                             % (what, int(bad.sum()), i, got[i], ref[i], scale if ref.ndim == 1 else scale[i[-1]]))


def block_close(got, ref, what, rel=REL):
    """normal-equation blocks [N][A][B] (H_img, H_pt, W, H_cam, E_cam, W_cam): entry (a, b) is held to both its row's
    and its column's scale over the scene, atol = rel * min(max |ref[:, a, :]|, max |ref[:, :, b]|).  An entry of
    J_a^T J_b carries rounding errors of order eps * |J_a| |J_b|, which both scales dominate (row a holds J_a^T J_a
    or its product with the largest column, likewise column b), so the bound leaves the usual seven orders of margin."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and ref.ndim == 3, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    assert np.isfinite(ref).all(), what + ": oracle not finite"
    assert np.isfinite(got).all(), what + ": not finite"
    row = np.abs(ref).max(axis=(0, 2))[:, None]
    col = np.abs(ref).max(axis=(0, 1))[None, :]
    tol = rel * np.minimum(row, col)
    err = np.abs(got - ref)
    bad = err > tol[None]
    if bad.any():
        i = np.unravel_index(np.argmax(err * bad), err.shape)
        raise AssertionError("%s: %d entries off, largest at %s: got %r oracle %r bound %r"
                             % (what, int(bad.sum()), i, got[i], ref[i], tol[i[1], i[2]]))


# ------------------------------------------------- scenes of the GPU tests ---
SCENES = ["m%d" % m for m in range(11)] + ["mixed", "mixed_padded"]
_SCENE_CACHE = {}


def named_scene(oracle, name):
    """"m0" .. "m10": the single-model scenes; "mixed" / "mixed_padded": MIXED_CAMERAS in one handle (built once)"""
    if name not in _SCENE_CACHE:
        if name.startswith("mixed"):
            _SCENE_CACHE[name] = edge_scene(oracle, cameras=MIXED_CAMERAS, seed=20, padding=name.endswith("padded"))
        else:
            _SCENE_CACHE[name] = edge_scene(oracle, models=(int(name[1:]),), seed=int(name[1:]))
    return _SCENE_CACHE[name]


def scene(oracle, name, **extra):
    kw = dict(scene_kwargs(named_scene(oracle, name)))
    kw.update(extra)
    return kw


def pad12(Jc):
    """the oracle's [O][2][max K] camera block in the C ABI's stride of 12 columns"""
    out = np.zeros(Jc.shape[:2] + (12,))
    out[:, :, :Jc.shape[2]] = Jc
    return out


def check_raw(oracle, kw, got, what=""):
    """raw blocks of pcd_ba_evaluate / pcd_ba_evaluate_blocks (un-packed) against the oracle, per column"""
    res, Jq, Jt, JX, Jc, JL = oracle.BA(**kw).evaluate_raw()
    O = len(kw["obs_image"])
    col_close(got["residuals"][:2 * O], res[:2 * O], what + "residuals")
    col_close(got["residuals"][2 * O:], res[2 * O:], what + "lidar residuals")
    col_close(got["jac_q"], Jq, what + "jac_q")
    col_close(got["jac_t"], Jt, what + "jac_t")
    col_close(got["jac_X"], JX, what + "jac_X")
    col_close(got["jac_lidar"], JL, what + "jac_lidar")
    col_close(got["jac_cam"], pad12(Jc), what + "jac_cam")
    K = np.array([NUM_PARAMS[int(m)] for m in kw["cam_model"]])
    K = K[np.asarray(kw["image_camera"], np.int64)[np.asarray(kw["obs_image"], np.int64)]]
    assert not (got["jac_cam"] * (np.arange(12)[None, None, :] >= K[:, None, None])).any(), what + "jac_cam columns >= K"
    assert np.abs(Jc).max() > 0


def entry_close(got, ref, what, rel=REL):
    """a single residual block: every entry within rel of its own magnitude (an entry that is zero in the oracle must
    be zero).  With one observation there is no larger entry in a column to lend its scale, which is what lets a
    named case tell two branch formulas apart that agree to 1e-7."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(ref).all() and np.isfinite(got).all(), what
    bad = np.abs(got - ref) > rel * np.abs(ref)
    assert not bad.any(), "%s: got %r oracle %r" % (what, got[bad], ref[bad])

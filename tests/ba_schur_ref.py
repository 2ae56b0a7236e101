"""numpy reference of the device point elimination (pcd_ba_schur*), built from the oracle's block-form
normal equations (oracle.BA(...).normal_equations(want_w=True)).

Two independent routes to the LM step of (H + D) delta = -g:
  dense_solve     the full damped system (pose tangents of the variable images, then the points) by numpy.linalg.solve;
  schur_blocks    S / rhs formed block by block from the same blocks (per point and image: Z_pi = sum of W_a), then
                  back_substitute for the points.
plus implements Ceres' QuaternionManifold::Plus; lm runs the trust-region loop of pcdhip.ba_solve_lm on the oracle.
Test infrastructure: small scenes only (dense matrices, Python loops over pairs)."""
import numpy as np

DIAG_MIN, DIAG_MAX = 1e-6, 1e32
PIVOT_TOL = 1e-10          # k_schur_points' kPivotTol: pivot k must exceed PIVOT_TOL * V_kk


def damping(h_diag, mu, mode):
    """mode 'marquardt': mu * clamp(H_kk, 1e-6, 1e32); 'levenberg': mu"""
    if mode == "marquardt":
        return mu * np.clip(h_diag, DIAG_MIN, DIAG_MAX)
    return np.full_like(h_diag, mu)


def problem(scene):
    """constness of the scene dict (pcdhip.BA / oracle.BA keyword arguments) with the defaults filled in"""
    I, P = np.asarray(scene["poses"]).reshape(-1, 7).shape[0], np.asarray(scene["points"]).reshape(-1, 3).shape[0]
    cpose = np.zeros(I, np.uint8) if scene.get("image_const_pose") is None else np.asarray(scene["image_const_pose"], np.uint8)
    ctvec = np.zeros(I, np.uint8) if scene.get("image_const_tvec") is None else np.asarray(scene["image_const_tvec"], np.uint8)
    cpt = np.zeros(P, np.uint8) if scene.get("point_const") is None else np.asarray(scene["point_const"], np.uint8)
    slot = np.full(I, -1, np.int64)
    var = np.flatnonzero(cpose == 0)
    slot[var] = np.arange(var.size)
    active = np.ones((var.size, 6), bool)          # constant-tvec components are inactive coordinates
    for k in range(3):
        active[:, 3 + k] = ((ctvec[var] >> k) & 1) == 0
    return dict(I=I, P=P, slot=slot, slot_img=var, active=active, point_const=cpt,
                obs_image=np.asarray(scene["obs_image"], np.int64), obs_point=np.asarray(scene["obs_point"], np.int64))


def point_inverse(Hpt, Dpt, point_const):
    """V_p^-1 through the same 3x3 Cholesky as the device, with its scale-invariant pivot rule in the same operation
    order: V_00 <= 0 or pivot k <= PIVOT_TOL * V_kk (pivot of the Jacobi-scaled V <= PIVOT_TOL) -> skipped, V^-1 = 0;
    constant points: 0"""
    A = Hpt + Dpt[:, :, None] * np.eye(3)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = A[:, 0, 0] > 0
        l00 = np.sqrt(np.where(ok, A[:, 0, 0], 1.0))
        l10, l20 = A[:, 0, 1] / l00, A[:, 0, 2] / l00
        t1 = A[:, 1, 1] - l10 * l10
        ok &= t1 > PIVOT_TOL * A[:, 1, 1]
        l11 = np.sqrt(np.where(ok, t1, 1.0))
        l21 = (A[:, 1, 2] - l20 * l10) / l11
        t2 = A[:, 2, 2] - l20 * l20 - l21 * l21
        ok &= t2 > PIVOT_TOL * A[:, 2, 2]
        l22 = np.sqrt(np.where(ok, t2, 1.0))
    L = np.zeros_like(A)
    L[:, 0, 0], L[:, 1, 0], L[:, 2, 0], L[:, 1, 1], L[:, 2, 1], L[:, 2, 2] = l00, l10, l20, l11, l21, l22
    elim = point_const == 0
    good = ok & elim
    Vinv = np.zeros_like(A)
    if good.any():
        M = np.linalg.inv(L[good])
        Vinv[good] = np.einsum("pki,pkj->pij", M, M)
    return Vinv, elim & ~ok


class NormalEquations:
    """the oracle's blocks of one scene at its parameters, with the damping of (mu, mode) applied; `blocks` =
    (cost, H_img, g_img, H_pt, g_pt, W) puts blocks from elsewhere (the device's evaluation) in their place"""

    def __init__(self, oracle, scene, mu, mode="marquardt", blocks=None):
        self.pr = problem(scene)
        self.cost, self.Himg, self.gimg, self.Hpt, self.gpt, self.W = \
            blocks if blocks is not None else oracle.BA(**scene).normal_equations(want_w=True)
        pr = self.pr
        self.Dimg = damping(np.diagonal(self.Himg, axis1=1, axis2=2)[pr["slot_img"]], mu, mode) * pr["active"]
        self.Dpt = damping(np.diagonal(self.Hpt, axis1=1, axis2=2), mu, mode)
        self.Vinv, self.skipped = point_inverse(self.Hpt, self.Dpt, pr["point_const"])
        s = pr["slot"][pr["obs_image"]]
        # observations that take part: variable pose, eliminated (non-constant, non-skipped) point
        self.elig = (s >= 0) & (pr["point_const"][pr["obs_point"]] == 0) & ~self.skipped[pr["obs_point"]]
        self.obs_slot = s
        # the co-visibility structure does not depend on the numbers: skipped points still define pairs (zero blocks)
        self.struct_elig = (s >= 0) & (pr["point_const"][pr["obs_point"]] == 0)

    # ---- route 1: the whole damped system ----
    def dense_solve(self):
        A, b, ns, pts = self.dense_system()
        x = np.linalg.solve(A, b)
        dpoint = np.zeros((self.pr["P"], 3))
        dpoint[pts] = x[6 * ns:].reshape(-1, 3)
        return x[:6 * ns].reshape(ns, 6), dpoint

    def dense_vector(self, dpose, dpoint):
        """(dpose, dpoint) in the unknown order of dense_system"""
        _, _, ns, pts = self._layout()
        return np.concatenate([np.asarray(dpose).reshape(-1), np.asarray(dpoint)[pts].reshape(-1)])

    def _layout(self):
        pr = self.pr
        pts = np.flatnonzero((pr["point_const"] == 0) & ~self.skipped)
        return None, None, pr["slot_img"].size, pts

    def dense_system(self):
        """(A, b, ns, eliminated points): (H + D) over the pose tangents of the variable images, then the points"""
        pr = self.pr
        ns, P = pr["slot_img"].size, pr["P"]
        pts = np.flatnonzero((pr["point_const"] == 0) & ~self.skipped)
        col = np.full(P, -1, np.int64)
        col[pts] = 6 * ns + 3 * np.arange(pts.size)
        n = 6 * ns + 3 * pts.size
        A = np.zeros((n, n))
        b = np.zeros(n)
        for i, im in enumerate(pr["slot_img"]):
            A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = self.Himg[im] + np.diag(self.Dimg[i])
            b[6 * i:6 * i + 6] = -self.gimg[im]
        for p in pts:
            c = col[p]
            A[c:c + 3, c:c + 3] = self.Hpt[p] + np.diag(self.Dpt[p])
            b[c:c + 3] = -self.gpt[p]
        for a in np.flatnonzero(self.elig):
            i, c = 6 * self.obs_slot[a], col[pr["obs_point"][a]]
            A[i:i + 6, c:c + 3] += self.W[a]
            A[c:c + 3, i:i + 6] += self.W[a].T
        for i in range(ns):                          # inactive coordinates: identity rows / columns, rhs 0
            for k in np.flatnonzero(~pr["active"][i]):
                r = 6 * i + k
                A[r, :] = 0.0; A[:, r] = 0.0; A[r, r] = 1.0; b[r] = 0.0
        return A, b, ns, pts

    # ---- route 2: block by block ----
    def _z(self, pts=None):
        """Z[(p, slot)] = sum of W_a over the eliminated observations of point p in that slot's image"""
        pr = self.pr
        Z = {}
        for a in np.flatnonzero(self.elig):
            p = int(pr["obs_point"][a])
            if pts is not None and p not in pts:
                continue
            key = (p, int(self.obs_slot[a]))
            Z[key] = Z.get(key, 0.0) + self.W[a]
        return Z

    def schur_blocks(self):
        """dict(S_diag [ns][6][6], S_off {(i, j): 6x6} for i < j, pairs (ascending), rhs [ns][6], S dense)"""
        pr = self.pr
        ns = pr["slot_img"].size
        Z = self._z()
        by_point = {}
        for (p, i), z in Z.items():
            by_point.setdefault(p, []).append((i, z))
        Sd = np.stack([self.Himg[im] + np.diag(self.Dimg[i]) for i, im in enumerate(pr["slot_img"])]) if ns else \
            np.zeros((0, 6, 6))
        rhs = -self.gimg[pr["slot_img"]].copy()
        off = {}
        for p, lst in by_point.items():
            Vi, vg = self.Vinv[p], self.Vinv[p] @ self.gpt[p]
            for i, zi in lst:
                rhs[i] += zi @ vg
                for j, zj in lst:
                    blk = zi @ Vi @ zj.T
                    if i == j:
                        Sd[i] -= blk
                    elif i < j:
                        off[(i, j)] = off.get((i, j), 0.0) - blk
        st = {}
        for a in np.flatnonzero(self.struct_elig):
            st.setdefault(int(pr["obs_point"][a]), set()).add(int(self.obs_slot[a]))
        for sl in st.values():
            sl = sorted(sl)
            for k, i in enumerate(sl):
                for j in sl[k + 1:]:
                    off.setdefault((i, j), np.zeros((6, 6)))
        self._mask(Sd, off, rhs)
        pairs = sorted(off)
        S = np.zeros((6 * ns, 6 * ns))
        for i in range(ns):
            S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Sd[i]
        for (i, j) in pairs:
            S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = off[(i, j)]
            S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = off[(i, j)].T
        return dict(S_diag=Sd, S_off=off, pairs=np.array(pairs, np.int64).reshape(-1, 2), rhs=rhs, S=S)

    def _mask(self, Sd, off, rhs):
        act = self.pr["active"]
        for i in range(Sd.shape[0]):
            for k in np.flatnonzero(~act[i]):
                Sd[i][k, :] = 0.0; Sd[i][:, k] = 0.0; Sd[i][k, k] = 1.0; rhs[i][k] = 0.0
        for (i, j), blk in off.items():
            blk[~act[i], :] = 0.0
            blk[:, ~act[j]] = 0.0

    def pair_block(self, i, j):
        """one block of S (i <= j) without forming the others: the config-B-sized check"""
        pr = self.pr
        ims = pr["slot_img"]
        ob_i = np.flatnonzero(self.elig & (pr["obs_image"] == ims[i]))
        ob_j = np.flatnonzero(self.elig & (pr["obs_image"] == ims[j]))
        common = set(pr["obs_point"][ob_i].tolist()) & set(pr["obs_point"][ob_j].tolist())
        acc = np.zeros((6, 6))
        for p in common:
            zi = self.W[ob_i[pr["obs_point"][ob_i] == p]].sum(0)
            zj = self.W[ob_j[pr["obs_point"][ob_j] == p]].sum(0)
            acc += zi @ self.Vinv[p] @ zj.T
        act = pr["active"]
        if i == j:
            blk = self.Himg[ims[i]] + np.diag(self.Dimg[i]) - acc
            for k in np.flatnonzero(~act[i]):
                blk[k, :] = 0.0; blk[:, k] = 0.0; blk[k, k] = 1.0
            return blk
        blk = -acc
        blk[~act[i], :] = 0.0
        blk[:, ~act[j]] = 0.0
        return blk

    def back_substitute(self, dpose):
        pr = self.pr
        r = self.gpt.copy()
        for a in np.flatnonzero(self.elig):
            r[pr["obs_point"][a]] += self.W[a].T @ dpose[self.obs_slot[a]]
        return -np.einsum("pij,pj->pi", self.Vinv, r)

    def model_decrease(self, dpose, dpoint):
        """1/2 (-delta^T g + delta^T D delta) over the active pose coordinates and the points"""
        pr = self.pr
        dp = np.where(pr["active"], dpose, 0.0)
        g = self.gimg[pr["slot_img"]]
        t = np.sum(-dp * g + self.Dimg * dp * dp) + np.sum(-dpoint * self.gpt + self.Dpt * dpoint * dpoint)
        return 0.5 * t


def quat_plus(q, d):
    """Ceres QuaternionManifold::Plus: [cos|d|, sin|d|/|d| d] * q (q = w x y z)"""
    nd = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if nd == 0.0:
        return np.array(q, np.float64)
    s = np.sin(nd) / nd
    a = np.array([np.cos(nd), s * d[0], s * d[1], s * d[2]])
    return np.array([a[0] * q[0] - a[1] * q[1] - a[2] * q[2] - a[3] * q[3],
                     a[0] * q[1] + a[1] * q[0] + a[2] * q[3] - a[3] * q[2],
                     a[0] * q[2] - a[1] * q[3] + a[2] * q[0] + a[3] * q[1],
                     a[0] * q[3] + a[1] * q[2] - a[2] * q[1] + a[3] * q[0]])


def plus(scene, dpose, dpoint):
    """candidate (poses [I][7], points [P][3]): constant poses, tvec components and points are copied"""
    pr = problem(scene)
    poses = np.array(scene["poses"], np.float64).reshape(-1, 7).copy()
    points = np.array(scene["points"], np.float64).reshape(-1, 3).copy()
    for i, im in enumerate(pr["slot_img"]):
        poses[im, :4] = quat_plus(poses[im, :4], dpose[i, :3])
        for k in range(3):
            if pr["active"][i, 3 + k]:
                poses[im, 4 + k] += dpose[i, 3 + k]
    var = pr["point_const"] == 0
    points[var] += dpoint[var]
    return poses, points


def lm(oracle, scene, max_iterations, initial_radius=1e4, mode="marquardt", min_relative_decrease=1e-3,
       max_radius=1e16):
    """pcdhip.ba_solve_lm's loop on the oracle (Cholesky of the block-wise S).  Returns (history, final scene)."""
    scene = dict(scene)
    radius, factor = float(initial_radius), 2.0
    hist = []
    for _ in range(max_iterations):
        ne = NormalEquations(oracle, scene, 1.0 / radius, mode)
        sb = ne.schur_blocks()
        rec = dict(cost=ne.cost, candidate_cost=np.nan, rho=np.nan, accepted=False)
        try:
            Lc = np.linalg.cholesky(sb["S"])
        except np.linalg.LinAlgError:
            Lc = None
        cand = None
        if Lc is not None:
            y = np.linalg.solve(Lc, sb["rhs"].reshape(-1))
            dpose = np.linalg.solve(Lc.T, y).reshape(-1, 6)
            dpoint = ne.back_substitute(dpose)
            model = ne.model_decrease(dpose, dpoint)
            poses, points = plus(scene, dpose, dpoint)
            cand = dict(scene, poses=poses, points=points)
            new_cost = oracle.BA(**cand).normal_equations()[0]
            rho = (ne.cost - new_cost) / model if model > 0 else -np.inf
            rec.update(candidate_cost=new_cost, rho=rho, accepted=bool(rho > min_relative_decrease))
        if rec["accepted"]:
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rec["rho"] - 1.0) ** 3))
            factor = 2.0
            scene = cand
        else:
            radius /= factor
            factor *= 2.0
        rec["radius"] = radius
        hist.append(rec)
    return hist, scene


# ---- scenes shared by the CPU and GPU tests ----
def camera_params(model, focal_scale=1.0):
    """parameters of camera `model` around synth.OPENCV_PARAMS' focal length and principal point, small distortion"""
    from pcdhip import synth
    fx, fy, cx, cy = synth.OPENCV_PARAMS[:4]
    nf = 1 if model in (0, 2, 3, 8, 9) else 2          # focal lengths: f, or fx fy
    extra = {0: [], 1: [], 2: [-0.03], 3: [-0.03, 0.005], 4: [-0.05, 0.01, 1e-4, 1e-4], 5: [0.02, -0.01, 0.003, -0.001],
             6: [-0.05, 0.01, 1e-4, 1e-4, 0.002, 0.01, -0.005, 0.001], 7: [0.4], 8: [0.02], 9: [0.02, -0.004],
             10: [0.02, -0.01, 1e-4, -1e-4, 0.003, -0.001, 2e-4, -1e-4]}[model]
    return np.array([fx * focal_scale, fy * focal_scale * 1.01][:nf] + [cx, cy] + extra, np.float64)


def reproject(oracle, scene, rng, noise=1.0):
    """observations = projection of each observed point through its image's camera (oracle) + U(-noise, noise) px"""
    models = np.asarray(scene["cam_model"])
    poses, X = np.asarray(scene["poses"]), np.asarray(scene["points"])
    xy = np.empty((len(scene["obs_image"]), 2))
    for o, (i, p) in enumerate(zip(scene["obs_image"], scene["obs_point"])):
        c = int(scene["image_camera"][i])
        xy[o] = oracle.reproj_residual(int(models[c]), poses[i, :4], poses[i, 4:], X[p], scene["cam_params_list"][c],
                                       np.zeros(2))
    scene["obs_xy"] = xy + rng.uniform(-noise, noise, xy.shape)
    assert np.isfinite(scene["obs_xy"]).all()
    return scene


def camera_scene(oracle, models, seed, I=6, P=150, lidar_frac=1.0):
    """synth.ba_scene with cameras of the given models (one camera per entry, parameters differing), image i on camera
    i % len(models), observations re-projected through those cameras; image 0 constant, some constant tvec components
    and constant points"""
    from pcdhip import synth
    s = synth.ba_scene(I, P, seed=seed, const_pose_frac=0.3, lidar_frac=lidar_frac)
    nc = len(models)
    s["cam_model"] = np.array(models, np.int32)
    s["cam_params_list"] = [camera_params(m, 1.0 + 1e-3 * k) for k, m in enumerate(models)]
    s["image_camera"] = (np.arange(I) % nc).astype(np.int32)
    rng = np.random.default_rng(seed)
    s["image_const_pose"][0] = 1
    s["image_const_tvec"] = (rng.integers(1, 8, I) * (rng.random(I) < 0.4)).astype(np.uint8)
    s["point_const"] = (rng.random(P) < 0.1).astype(np.uint8)
    return reproject(oracle, s, rng)


def shared_launch_scene(seed=461):
    """the smallest scene that reaches all four launches of the normal equations (point pass, cost sum, image pass,
    image reduction) with every branch of their grids: 3 images one metre apart looking along +z, image 0 with a constant
    pose; 70 points in front of all three (two 64-track slices, the second partial), point 5 constant, LiDAR terms on 6
    points; every point is observed once in images 0 and 1 and 15 times in image 2, which so holds 1050 observations:
    two image segments of at most 1024.  Observations are grouped by track, so the caller's order is not image-major.
    Three views of every point: no point is rank-deficient at mu = 0."""
    from pcdhip import synth
    rng = np.random.default_rng(seed)
    I, P, rep = 3, 70, 15
    poses = np.zeros((I, 7))
    poses[:, 0] = 1.0
    poses[:, 4] = -np.arange(I)                                   # t = -R C, camera centres (i, 0, 0)
    points = np.stack([rng.uniform(-3, 5, P), rng.uniform(-2, 2, P), rng.uniform(6, 20, P)], axis=1)
    obs_image = np.tile(np.r_[0, 1, np.full(rep, 2)], P).astype(np.int32)
    obs_point = np.repeat(np.arange(P), 2 + rep).astype(np.int32)
    Pc = points[obs_point] + poses[obs_image, 4:]
    x, y = synth._opencv_project(synth.OPENCV_PARAMS, Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2])
    obs_xy = np.stack([x, y], axis=1) + rng.uniform(-2, 2, (obs_image.size, 2))
    poses[:, 1:4] = rng.normal(0, 0.004, (I, 3))                  # what BA starts from: ~0.5 degrees, 5 cm off
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    poses[:, 4:] += rng.normal(0, 0.05, (I, 3))
    lidar_point = np.array([0, 5, 17, 63, 64, 69], np.int32)
    nrm = rng.normal(size=(lidar_point.size, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    lp = points[lidar_point] + rng.normal(0, 0.05, (lidar_point.size, 3))
    point_const = np.zeros(P, np.uint8)
    point_const[5] = 1
    return dict(cam_model=np.array([4], np.int32), cam_params_list=[synth.OPENCV_PARAMS], poses=poses,
                image_camera=np.zeros(I, np.int32), points=points, obs_image=obs_image, obs_point=obs_point, obs_xy=obs_xy,
                lidar_point=lidar_point, lidar_abcd=np.concatenate([nrm, -np.sum(nrm * lp, 1, keepdims=True)], axis=1),
                lidar_weight=np.full(lidar_point.size, 100.0), image_const_pose=np.array([1, 0, 0], np.uint8),
                point_const=point_const)


def degenerate_scene(oracle, seed, n_single=8, n_lidar=6):
    """a well-conditioned base scene (every point has a LiDAR term) plus points whose H_pt is rank-deficient:
    n_single points with one observation near the centre of a variable image at 8-15 m depth and no LiDAR term (rank 2),
    n_lidar points with only a LiDAR term of a generic normal and 3 with axis-aligned normals (rank 1).
    Returns (scene, indices of the rank-deficient points)."""
    from pcdhip import synth
    s = synth.ba_scene(6, 150, seed=seed, const_pose_frac=0.3, lidar_frac=1.0)
    rng = np.random.default_rng(seed)
    s["image_const_pose"][0] = 1
    P0 = s["points"].shape[0]
    var = np.flatnonzero(s["image_const_pose"] == 0)
    pts, oi, op, lp, ab, lw = [], [], [], [], [], []
    for k in range(n_single):
        i = int(var[k % var.size])
        q, t = s["poses"][i, :4], s["poses"][i, 4:]
        pc = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 1.0]) * rng.uniform(8, 15)
        pts.append(synth._quat_rotate(q * np.array([1, -1, -1, -1]), pc - t))
        oi.append(i); op.append(P0 + k)
    normals = [n / np.linalg.norm(n) for n in rng.normal(size=(n_lidar, 3))] + list(np.eye(3))
    for k, n in enumerate(normals):
        X = s["points"][rng.integers(P0)] + rng.normal(0, 0.5, 3)
        pts.append(X)
        lp.append(P0 + n_single + k)
        ab.append(np.r_[n, -n @ (X + rng.normal(0, 0.05, 3))])
        lw.append(100.0)
    s["points"] = np.concatenate([s["points"], pts])
    xy_new = np.array([oracle.reproj_residual(4, s["poses"][i, :4], s["poses"][i, 4:], s["points"][p],
                                              synth.OPENCV_PARAMS, np.zeros(2)) for i, p in zip(oi, op)])
    s["obs_image"] = np.concatenate([s["obs_image"], oi]).astype(np.int32)
    s["obs_point"] = np.concatenate([s["obs_point"], op]).astype(np.int32)
    s["obs_xy"] = np.concatenate([s["obs_xy"], xy_new + rng.uniform(-1, 1, xy_new.shape)])
    s["lidar_point"] = np.concatenate([s["lidar_point"], lp]).astype(np.int32)
    s["lidar_abcd"] = np.concatenate([s["lidar_abcd"], ab])
    s["lidar_weight"] = np.concatenate([s["lidar_weight"], lw])
    s["point_const"] = np.zeros(s["points"].shape[0], np.uint8)
    return s, np.arange(P0, s["points"].shape[0])

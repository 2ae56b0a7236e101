"""numpy reference of the device point elimination with refined intrinsics (pcd_ba_schur_cam*), built by
import on tests/ba_schur_ref.py and the oracle's camera blocks (oracle.BA.camera_blocks).

Unknowns of the reduced system: [6 ns pose tangents | 12 ncs camera coordinates]; camera slots are the cameras with at
least one camera_refine byte set, ascending camera index; of a slot's 12 coordinates the refined entries below the model's
K are active, the others are identity rows / columns with a zero right-hand side.

Two independent routes to the LM step, as in ba_schur_ref:
  dense_solve_cam    the whole damped system (poses, cameras, points) by numpy.linalg.solve;
  schur_cam_blocks   B / S_cam / rhs_cam formed block by block (Wc_p[r], Z_p[r] = Wc_p[r] V_p^-1), the pose part from
                     ba_schur_ref unchanged, then back_substitute_cam for the points.
plus_cam adds the camera step to the active parameters; lm_cam runs the trust-region loop of pcd_ba_solve with
refine_intrinsics on the oracle.  Test infrastructure: small scenes only."""
import numpy as np

from tests import ba_schur_ref as ref

S12 = 12
NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 6: 12, 7: 5, 8: 4, 9: 5, 10: 12}


def refine_mask(scene, cameras=None, groups=None):
    """camera_refine bytes [cam_params_len]: the parameters `groups` (indices within a camera, None = all) of the
    cameras `cameras` (None = all)"""
    out = []
    for c, cp in enumerate(scene["cam_params_list"]):
        m = np.zeros(len(cp), np.uint8)
        if cameras is None or c in cameras:
            m[:] = 1 if groups is None else 0
            if groups is not None:
                m[[k for k in groups if k < len(cp)]] = 1
        out.append(m)
    return np.concatenate(out)


def without_refine(scene):
    return {k: v for k, v in scene.items() if k != "camera_refine"}


def camera_slots(scene, refine):
    """(camera_slot [C] (-1: no refined parameter), slot_cam [ncs], active [ncs][12] bool, offsets [C])"""
    models = np.asarray(scene["cam_model"])
    off = np.concatenate([[0], np.cumsum([len(c) for c in scene["cam_params_list"]])]).astype(np.int64)
    slot = np.full(len(models), -1, np.int64)
    act = []
    for c, m in enumerate(models):
        K = NUM_PARAMS[int(m)]
        r = np.asarray(refine[off[c]:off[c] + K]) != 0
        if r.any():
            slot[c] = len(act)
            a = np.zeros(S12, bool)
            a[:K] = r
            act.append(a)
    return slot, np.flatnonzero(slot >= 0), np.array(act, bool).reshape(-1, S12), off[:-1]


class CamNormalEquations(ref.NormalEquations):
    """ba_schur_ref.NormalEquations plus the oracle's camera blocks of `refine` and their damping"""

    def __init__(self, oracle, scene, refine, mu, mode="marquardt"):
        base = without_refine(scene)
        super().__init__(oracle, base, mu, mode)
        self.refine = np.ascontiguousarray(refine, np.uint8)
        self.Hcam, self.gcam, self.Ecam, self.Wcam = oracle.BA(**base).camera_blocks(self.refine, want_w=True)
        self.cam_slot, self.slot_cam, self.cam_active, self.cam_off = camera_slots(base, self.refine)
        self.ncs = self.slot_cam.size
        self.img_cam_slot = self.cam_slot[np.asarray(base["image_camera"], np.int64)]
        self.obs_cam_slot = self.img_cam_slot[self.pr["obs_image"]]
        hd = np.diagonal(self.Hcam, axis1=1, axis2=2)[self.slot_cam].reshape(-1, S12)
        self.Dcam = ref.damping(hd, mu, mode) * self.cam_active
        # observations whose point is eliminated couple their camera to it, whatever their image's pose is
        self.cam_elig = (self.obs_cam_slot >= 0) & (self.pr["point_const"][self.pr["obs_point"]] == 0) & \
            ~self.skipped[self.pr["obs_point"]]

    # ---- route 1: the whole damped system ----
    def dense_system_cam(self):
        """(A, b, ns, ncs, eliminated points): unknowns = pose tangents, camera coordinates, points"""
        A0, b0, ns, pts = self.dense_system()
        pr, ncs = self.pr, self.ncs
        n0, nc = 6 * ns, S12 * ncs
        n = A0.shape[0] + nc
        A, b = np.zeros((n, n)), np.zeros(n)
        pose = np.arange(n0)
        pt = np.arange(n0, A0.shape[0])
        A[np.ix_(pose, pose)] = A0[:n0, :n0]
        A[np.ix_(pose, pt + nc)] = A0[:n0, n0:]
        A[np.ix_(pt + nc, pose)] = A0[n0:, :n0]
        A[np.ix_(pt + nc, pt + nc)] = A0[n0:, n0:]
        b[pose], b[pt + nc] = b0[:n0], b0[n0:]
        col = np.full(pr["P"], -1, np.int64)
        col[pts] = n0 + nc + 3 * np.arange(pts.size)
        for r, c in enumerate(self.slot_cam):
            k = n0 + S12 * r
            A[k:k + S12, k:k + S12] = self.Hcam[c] + np.diag(self.Dcam[r])
            b[k:k + S12] = -self.gcam[c]
        for i, im in enumerate(pr["slot_img"]):
            r = self.img_cam_slot[im]
            if r >= 0:
                k = n0 + S12 * r
                A[k:k + S12, 6 * i:6 * i + 6] += self.Ecam[im]
                A[6 * i:6 * i + 6, k:k + S12] += self.Ecam[im].T
        for o in np.flatnonzero(self.cam_elig):
            k, c = n0 + S12 * self.obs_cam_slot[o], col[pr["obs_point"][o]]
            A[k:k + S12, c:c + 3] += self.Wcam[o]
            A[c:c + 3, k:k + S12] += self.Wcam[o].T
        dead = [6 * i + k for i in range(ns) for k in np.flatnonzero(~pr["active"][i])] + \
               [n0 + S12 * r + k for r in range(ncs) for k in np.flatnonzero(~self.cam_active[r])]
        for r in dead:
            A[r, :] = 0.0; A[:, r] = 0.0; A[r, r] = 1.0; b[r] = 0.0
        return A, b, ns, ncs, pts

    def dense_solve_cam(self):
        """(dpose [ns][6], dcam [ncs][12], dpoint [P][3])"""
        A, b, ns, ncs, pts = self.dense_system_cam()
        x = np.linalg.solve(A, b)
        n0, nc = 6 * ns, S12 * ncs
        dpoint = np.zeros((self.pr["P"], 3))
        dpoint[pts] = x[n0 + nc:].reshape(-1, 3)
        return x[:n0].reshape(ns, 6), x[n0:n0 + nc].reshape(ncs, S12), dpoint

    # ---- route 2: block by block ----
    def wc(self):
        """Wc [P][ncs][12][3]: sum of W_cam over the observations of each point and camera slot, ascending observation"""
        Wc = np.zeros((self.pr["P"], self.ncs, S12, 3))
        for o in np.flatnonzero(self.obs_cam_slot >= 0):
            Wc[self.pr["obs_point"][o], self.obs_cam_slot[o]] += self.Wcam[o]
        return Wc

    def schur_cam_blocks(self):
        """the blocks of ba_schur_ref.schur_blocks (S_diag, S_off, pairs, rhs) plus B [ns][ncs][12][6],
        S_cam [ncs][ncs][12][12], rhs_cam [ncs][12] and the dense S [n][n], n = 6 ns + 12 ncs"""
        sb = self.schur_blocks()
        pr, ns, ncs = self.pr, self.pr["slot_img"].size, self.ncs
        Wc = self.wc()
        Z = np.einsum("prak,pkl->pral", Wc, self.Vinv)                 # 0 for constant and skipped points
        Scam = -np.einsum("prak,psbk->rsab", Z, Wc)
        rhs_cam = -self.gcam[self.slot_cam].reshape(ncs, S12) + np.einsum("prak,pk->ra", Z, self.gpt)
        for r, c in enumerate(self.slot_cam):
            Scam[r, r] += self.Hcam[c] + np.diag(self.Dcam[r])
        B = np.zeros((ns, ncs, S12, 6))
        for i, im in enumerate(pr["slot_img"]):
            if self.img_cam_slot[im] >= 0:
                B[i, self.img_cam_slot[im]] += self.Ecam[im]
        for e in np.flatnonzero(self.elig):
            B[self.obs_slot[e]] -= np.einsum("rak,ck->rac", Z[pr["obs_point"][e]], self.W[e])
        for i in range(ns):
            B[i][:, :, ~pr["active"][i]] = 0.0
        for r in range(ncs):
            dead = ~self.cam_active[r]
            B[:, r, dead, :] = 0.0
            Scam[r][:, dead, :] = 0.0
            Scam[:, r][:, :, dead] = 0.0
            Scam[r, r][dead, dead] = 1.0
            rhs_cam[r, dead] = 0.0
        n0, nc = 6 * ns, S12 * ncs
        S = np.zeros((n0 + nc, n0 + nc))
        S[:n0, :n0] = sb["S"]
        for i in range(ns):
            for r in range(ncs):
                S[n0 + S12 * r:n0 + S12 * r + S12, 6 * i:6 * i + 6] = B[i, r]
                S[6 * i:6 * i + 6, n0 + S12 * r:n0 + S12 * r + S12] = B[i, r].T
        for r in range(ncs):
            for q in range(ncs):
                S[n0 + S12 * r:n0 + S12 * r + S12, n0 + S12 * q:n0 + S12 * q + S12] = Scam[r, q]
        out = dict(sb)
        out.update(B=B, S_cam=Scam, rhs_cam=rhs_cam, S=S, S_pose=sb["S"],
                   rhs_full=np.concatenate([sb["rhs"].reshape(-1), rhs_cam.reshape(-1)]))
        return out

    def back_substitute_cam(self, dpose, dcam):
        pr = self.pr
        r = self.gpt.copy()
        for a in np.flatnonzero(self.elig):
            r[pr["obs_point"][a]] += self.W[a].T @ dpose[self.obs_slot[a]]
        r += np.einsum("prak,ra->pk", self.wc(), np.where(self.cam_active, dcam, 0.0))
        return -np.einsum("pij,pj->pi", self.Vinv, r)

    def model_decrease_cam(self, dpose, dcam, dpoint):
        dc = np.where(self.cam_active, dcam, 0.0)
        g = self.gcam[self.slot_cam].reshape(-1, S12)
        return self.model_decrease(dpose, dpoint) + 0.5 * np.sum(-dc * g + self.Dcam * dc * dc)

    def split(self, delta):
        """delta [n] -> (dpose [ns][6], dcam [ncs][12])"""
        n0 = 6 * self.pr["slot_img"].size
        delta = np.asarray(delta).reshape(-1)
        return delta[:n0].reshape(-1, 6), delta[n0:].reshape(-1, S12)


def plus_cam(scene, refine, dpose, dcam, dpoint):
    """candidate (poses, points, cam_params_list): ba_schur_ref.plus, and p + dcam on the active camera parameters"""
    base = without_refine(scene)
    poses, points = ref.plus(base, dpose, dpoint)
    slot, slot_cam, active, _ = camera_slots(base, refine)
    cams = [np.array(c, np.float64).copy() for c in base["cam_params_list"]]
    for r, c in enumerate(slot_cam):
        for k in np.flatnonzero(active[r]):
            cams[c][k] += dcam[r][k]
    return poses, points, cams


def lm_cam(oracle, scene, refine, max_iterations, initial_radius=1e4, mode="marquardt", min_relative_decrease=1e-3,
           max_radius=1e16):
    """pcd_ba_solve's loop with refine_intrinsics on the oracle (Cholesky of the block-wise bordered S).  Returns
    (history, final scene)."""
    scene = without_refine(scene)
    radius, factor = float(initial_radius), 2.0
    hist = []
    for _ in range(max_iterations):
        ne = CamNormalEquations(oracle, scene, refine, 1.0 / radius, mode)
        sb = ne.schur_cam_blocks()
        rec = dict(cost=ne.cost, candidate_cost=np.nan, rho=np.nan, accepted=False)
        try:
            Lc = np.linalg.cholesky(sb["S"])
        except np.linalg.LinAlgError:
            Lc = None
        cand = None
        if Lc is not None:
            y = np.linalg.solve(Lc, sb["rhs_full"])
            dpose, dcam = ne.split(np.linalg.solve(Lc.T, y))
            dpoint = ne.back_substitute_cam(dpose, dcam)
            model = ne.model_decrease_cam(dpose, dcam, dpoint)
            poses, points, cams = plus_cam(scene, refine, dpose, dcam, dpoint)
            cand = dict(scene, poses=poses, points=points, cam_params_list=cams)
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


# ---- the camera cases shared by the CPU and GPU tests: (models, refined cameras or None = all, parameters or None) ----
CAM_CASES = [
    ([4], None, (0, 1)),            # shared OPENCV, focal only
    ([4], None, None),              # shared OPENCV, all 8
    ([1], None, None),              # PINHOLE, all 4
    ([6], None, None),              # FULL_OPENCV, all 12: K = S, no padding rows
    ([4, 2], None, None),           # two slots whose images share points; SIMPLE_RADIAL leaves inactive rows
    ([4, 2], (1,), None),           # only camera 1 refined: slot numbering differs from the camera index
]
# Cauchy loss everywhere (cam_case_scene).  Levenberg damping at mu 0, 1e-4, 1: small constant damping leaves the gauge
# directions of these scenes nearly free (cond(S) up to 1e20), so blocks are compared there, steps only against the same
# system; Marquardt at 1e-4 (cond(S) 1e10 .. 1e12) is where a step is compared with the solve of the whole system.
DAMPINGS = [("levenberg", 0.0), ("levenberg", 1e-4), ("levenberg", 1.0), ("marquardt", 1e-4)]
WELL_CONDITIONED = ("marquardt",)


def camera_scene(oracle, models, seed, **kw):
    """ba_schur_ref.camera_scene; with more than one camera the images are dealt out in pairs (0 0 1 1 0 0 ...) and
    re-projected.  synth.ba_scene lets a point be seen by images of one parity only, so with ba_schur_ref's alternating
    deal (image i on camera i % 2) no point would be shared by two cameras and every off-diagonal block of S_cam would
    be exactly zero."""
    s = ref.camera_scene(oracle, models, seed, **kw)
    nc = len(models)
    if nc > 1:
        s["image_camera"] = ((np.arange(len(s["poses"])) // 2) % nc).astype(np.int32)
        ref.reproject(oracle, s, np.random.default_rng(seed + 1000))
    return s


def cam_case_scene(oracle, case, seed=40, **kw):
    """camera_scene of CAM_CASES[case] with Cauchy loss, and its camera_refine bytes"""
    models, cams, groups = CAM_CASES[case]
    s = camera_scene(oracle, models, seed + case, **kw)
    s["loss_type"], s["loss_scale"] = 2, 2.0
    return s, refine_mask(s, cams, groups)


def gradient_max(ne):
    """max |g| as pcd_ba_solve reports it (gradient_max_norm): over the active pose coordinates of the slots, every
    non-constant point (skipped points included, as k_ba_grad_max) and, on a CamNormalEquations, the active camera
    coordinates.  Returns (maximum, dict of the three partial maxima 'pose', 'point', 'camera')"""
    pr = ne.pr
    gp = np.abs(ne.gimg[pr["slot_img"]])[pr["active"]]
    gx = np.abs(ne.gpt[pr["point_const"] == 0])
    parts = dict(pose=float(gp.max()) if gp.size else 0.0, point=float(gx.max()) if gx.size else 0.0, camera=0.0)
    if hasattr(ne, "gcam") and ne.ncs:
        gc = np.abs(ne.gcam[ne.slot_cam].reshape(-1, S12))[ne.cam_active]
        parts["camera"] = float(gc.max()) if gc.size else 0.0
    return max(parts.values()), parts


# ---- the boundary scenes of tests/test_ba_schur_cam_edge_{cpu,gpu}.py.  Every one sets image_const_pose explicitly, so
# ---- that ns is what the case says (ba_schur_ref.camera_scene draws constant poses at random).
def edge_scene(oracle, models, seed, I, P, const=(0,), cauchy=True, **kw):
    """camera_scene (images dealt out in pairs over the cameras) with exactly the images `const` at a constant pose,
    Cauchy loss unless cauchy=False"""
    s = camera_scene(oracle, models, seed, I=I, P=P, **kw)
    s["image_const_pose"] = np.zeros(I, np.uint8)
    s["image_const_pose"][list(const)] = 1
    if cauchy:
        s["loss_type"], s["loss_scale"] = 2, 2.0
    return s


# name -> (models, seed, I, P, constant-pose images, ns, ncs): n = 6 ns + 12 ncs
SLOT_CASES = {
    # three chunks of the camera point sums (the third partial), six slot pairs: the first shape where the pair decode
    # sees q = 3..5; n = 102 (2 panels)
    "three_slots": ([4, 2, 1], 31, 12, 600, (0,), 11, 3),
    # every camera model the other cases leave out; active counts [3, 5, 8, 5, 4, 5, 12, 8]: K = 3 and K = 5 meet the
    # dead-row logic; 36 slot pairs, 96 camera coordinates (two trips of the one-wavefront loops); n = 186 (2 panels)
    "eight_mixed": ([0, 3, 5, 7, 8, 9, 10, 4], 34, 16, 150, (0,), 15, 8),
    # eight PINHOLE cameras, 41 images of which 13 are constant: ns = 28, n = 264 (3 panels), the camera rows occupy
    # 168..263 across the panel edge at 192
    "eight_wide": ([1] * 8, 37, 41, 300, tuple(range(0, 39, 3)), 28, 8),
}


def slot_scene(oracle, name):
    """(scene, refine) of SLOT_CASES[name], every parameter refined"""
    models, seed, I, P, const, _, _ = SLOT_CASES[name]
    s = edge_scene(oracle, models, seed, I, P, const)
    return s, refine_mask(s)


# (ncs, ns): one OPENCV camera or OPENCV + SIMPLE_RADIAL, I = ns + 1 images of which image 0 alone is constant, 150
# points.  n = 96 exactly (one full panel) twice; camera rows astride the first panel edge twice (n = 102: rows 90..101
# and 78..101); camera rows opening panel 1 (6 ns = 96, n = 120)
PANEL_CASES = [(1, 14), (2, 12), (1, 15), (2, 13), (2, 16)]


def panel_scene(oracle, ncs, ns):
    """(scene, refine) of one PANEL_CASES entry"""
    s = edge_scene(oracle, [4] if ncs == 1 else [4, 2], 50 + 7 * ns + ncs, ns + 1, 150)
    return s, refine_mask(s)


def chunks_65_scene(oracle):
    """OPENCV + SIMPLE_RADIAL, 6 images (image 0 constant: ns = 5, n = 54), 16 700 points: 66 chunks of 256 points, so
    lanes 0 and 1 of the chunk reduction take two partials each, and the last chunk is partial (60 points)"""
    s = edge_scene(oracle, [4, 2], 61, 6, 16700, cauchy=False)
    return s, refine_mask(s)


def _mask_of(scene, per_camera):
    """camera_refine bytes from one tuple of parameter indices per camera"""
    out = []
    for cp, g in zip(scene["cam_params_list"], per_camera):
        m = np.zeros(len(cp), np.uint8)
        m[list(g)] = 1
        out.append(m)
    return np.concatenate(out)


# name -> (models, one tuple of refined parameters per camera): masks with holes
MASK_CASES = {
    "principal_point": ([4], [(2, 3)]),
    "distortion_only": ([4], [(4, 5, 6, 7)]),
    "one_parameter": ([4], [(1,)]),
    "thin_prism_ends": ([10], [(0, 11)]),
    "two_masks": ([4, 2], [(0, 3, 5), (1, 3)]),
}


def mask_scene(oracle, name):
    """(scene, refine) of MASK_CASES[name]: 6 images, image 0 constant, 150 points"""
    models, groups = MASK_CASES[name]
    s = edge_scene(oracle, models, 70 + sorted(MASK_CASES).index(name), 6, 150)
    return s, _mask_of(s, groups)


def const_points_scene(oracle):
    """OPENCV + SIMPLE_RADIAL, 8 images, every point constant: nothing is eliminated, so S_cam is H_cam plus its damping,
    B is E_cam, rhs_cam is -g_cam and the off-diagonal blocks of S_cam are zero"""
    s = edge_scene(oracle, [4, 2], 83, 8, 150)
    s["point_const"] = np.ones(150, np.uint8)
    return s, refine_mask(s)


def const_pose_camera_scene(oracle):
    """two cameras, 8 images dealt out in pairs; every image of camera 1 (2, 3, 6, 7) has a constant pose: ns = 4, the
    B column of slot 1 carries no E_cam term, and its S_cam blocks are still non-zero through the shared points"""
    s = edge_scene(oracle, [4, 2], 85, 8, 150, const=(2, 3, 6, 7))
    return s, refine_mask(s)


def unused_camera_scene(oracle):
    """test_ba_pcg_cam_cpu.unused_camera_scene with images 0 and 1 constant (ns = 4): the gauge is fixed, so the pose
    part and camera 0 keep safe pivots without damping, and the first coordinate of the unused slot, 6 ns + 12 = 36, is
    the first column that fails at Levenberg mu = 0"""
    from tests.test_ba_pcg_cam_cpu import unused_camera_scene as base
    s, refine = base(oracle)
    s["image_const_pose"] = np.zeros(len(s["poses"]), np.uint8)
    s["image_const_pose"][:2] = 1
    return s, refine


def gradient_scene(oracle, where):
    """(scene, refine or None) whose largest gradient entry sits
    'camera': in a coordinate of camera slot 7 -- the eight_mixed scene with the trivial loss, the focal lengths of
              camera 7 (OPENCV) x 1.5 and its two images at a constant pose, so that their pose gradients do not count;
              the coordinates 84 .. 95 are read by the second trip of the one-wavefront loops over 12 ncs = 96;
    'pose':   in a pose coordinate -- eight_wide as it is;
    'point':  in the last point of the 16 700-point scene, on a handle without refinement (refine None): the plane of
              its LiDAR term is moved 1000 m away.  The point is read by the last workgroup of the gradient maximum."""
    if where == "camera":
        models, seed, I, P, const, _, _ = SLOT_CASES["eight_mixed"]
        s = edge_scene(oracle, models, seed, I, P, const, cauchy=False)
        s["image_const_pose"][np.asarray(s["image_camera"]) == 7] = 1
        cp = [np.array(c, np.float64) for c in s["cam_params_list"]]
        cp[7][:2] *= 1.5
        s["cam_params_list"] = cp
        return s, refine_mask(s)
    if where == "pose":
        return slot_scene(oracle, "eight_wide")
    s, _ = chunks_65_scene(oracle)
    last = s["points"].shape[0] - 1
    s["point_const"][last] = 0
    k = np.flatnonzero(np.asarray(s["lidar_point"]) == last)
    assert k.size == 1
    s["lidar_abcd"] = np.array(s["lidar_abcd"], np.float64)
    s["lidar_abcd"][k, 3] += 1000.0
    return s, None


def lm_eight_scene(oracle):
    """(scene, refine, initial radius) of the LM loop at eight slots: eight_wide with the trivial loss, the points
    perturbed by N(0, 2 m) and every focal length x 1.05 (as test_ba_schur_cam_gpu._lm_scene), started at radius 1e7"""
    models, seed, I, P, const, _, _ = SLOT_CASES["eight_wide"]
    s = edge_scene(oracle, models, seed, I, P, const, cauchy=False)
    s["points"] = s["points"] + np.random.default_rng(1037).normal(0, 2.0, s["points"].shape)
    s["cam_params_list"] = [np.array(c, np.float64) * np.r_[1.05, 1.05, 1.0, 1.0] for c in s["cam_params_list"]]
    return s, refine_mask(s), 1e7

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

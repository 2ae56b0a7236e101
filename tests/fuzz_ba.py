"""(test infrastructure, run by hand; not collected by pytest)  Randomised parity sweep of the BA evaluation against the Jet oracle: python tests/fuzz_ba.py [seconds] [seed].
Random scene sizes (incl. segments > 1024 observations per image, images without observations, tracks of length 1..max,
points without observations), camera models (one model per scene or mixed), several cameras, constant poses / tvec
masks / points, lidar terms, the three losses, observation order (by track / by image / shuffled), refined-camera
masks.  With probability 0.3 a random subset of the branch-point observations of tests/ba_edge_ref.py's catalogue (for
the scene's models, with their own cameras and images) is appended; FOV omega is drawn from a mixture of 0, 1e-6, values
within 2 % of the 1e-2 threshold and 0.2-0.9; a random third of the quaternions is scaled by 0.6-1.7 (each image
re-centred on the points it sees, see scale_quaternions).  Compared: cost, H_img, g_img, H_pt, g_pt, W (fused and raw),
raw residual / Jacobian blocks, camera blocks."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd")); sys.path.insert(0, ROOT)
import numpy as np
import pcdhip
from pcdhip import synth
from oracle import pyoracle as oracle
from tests import ba_edge_ref as edge

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t_end = time.time() + budget
NP = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]


def close(a, b, rtol, what, ctx):
    a = np.asarray(a); b = np.asarray(b)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    if not np.allclose(a, b, rtol=rtol, atol=rtol * scale, equal_nan=True):
        bad = np.nonzero(~np.isclose(a, b, rtol=rtol, atol=rtol * scale, equal_nan=True))
        print("MISMATCH", what, ctx, "count", len(bad[0]), "first", [x[:3] for x in bad], a[bad][:3], b[bad][:3], flush=True)
        sys.exit(1)


def cam_params(model):
    # plausible parameters for every model: f, (f2), cx, cy, small distortion
    K = NP[model]
    p = np.zeros(K)
    two_f = model in (1, 4, 5, 6, 10)
    p[0] = rng.uniform(900, 1500)
    i = 1
    if two_f:
        p[1] = p[0] * rng.uniform(0.98, 1.02); i = 2
    p[i] = rng.uniform(1900, 2100); p[i + 1] = rng.uniform(1400, 1600)
    p[i + 2:] = rng.normal(0, 5e-3, K - i - 2)
    if model == 7:   # FOV: omega
        p[4] = [0.0, 1e-6, rng.uniform(0.98e-2, 1.02e-2), rng.uniform(0.2, 0.9)][int(rng.integers(0, 4))]
    return p


def scale_quaternions(s):
    """q -> c q, c in 0.6-1.7, on a random third of the images; t moves so that the centroid of the points the image
    sees keeps its camera-frame position.  The scaled polynomial is I + c^2 (R - I): for a camera that faces backwards
    a large c throws part of its points behind it, where the distortion polynomials mean nothing and would set every
    norm of the case, so a draw that leaves a seen point closer than a tenth of the centroid's depth is drawn again
    (five times at most, then the image keeps its unit quaternion)"""
    for i in np.flatnonzero(rng.random(s["poses"].shape[0]) < 1.0 / 3.0):
        seen = s["points"][s["obs_point"][s["obs_image"] == i]]
        if not len(seen):
            s["poses"][i, :4] *= rng.uniform(0.6, 1.7)
            continue
        q, t, mean = s["poses"][i, :4].copy(), s["poses"][i, 4:].copy(), seen.mean(axis=0)
        zbar = (edge.rotation_matrix_poly(q) @ mean + t)[2]
        for _ in range(5):
            q2 = q * rng.uniform(0.6, 1.7)
            D2 = edge.rotation_matrix_poly(q2)
            t2 = t + (edge.rotation_matrix_poly(q) - D2) @ mean
            if zbar > 0 and ((seen @ D2.T + t2)[:, 2] > 0.1 * zbar).all():
                s["poses"][i, :4], s["poses"][i, 4:] = q2, t2
                break


def append_edge_observations(s, models):
    """a random subset of the catalogue's points (their observations and LiDAR terms) for the scene's models, on
    cameras and images of their own appended to the scene"""
    e = edge.scene_kwargs(edge.edge_scene(oracle, models=tuple(set(models)), seed=int(rng.integers(1 << 20))))
    keep = np.flatnonzero(rng.random(e["points"].shape[0]) < rng.uniform(0.2, 1.0))
    if not len(keep):
        return
    new_id = np.full(e["points"].shape[0], -1, np.int64); new_id[keep] = np.arange(len(keep))
    C0, I0, P0 = len(s["cam_model"]), s["poses"].shape[0], s["points"].shape[0]
    ok, lk = new_id[e["obs_point"]] >= 0, new_id[e["lidar_point"]] >= 0
    s["cam_model"] = np.concatenate([s["cam_model"], e["cam_model"]]).astype(np.int32)
    s["cam_params_list"] = list(s["cam_params_list"]) + list(e["cam_params_list"])
    s["poses"] = np.concatenate([s["poses"], e["poses"]])
    s["image_camera"] = np.concatenate([s["image_camera"], e["image_camera"] + C0]).astype(np.int32)
    s["image_const_pose"] = np.concatenate([s["image_const_pose"], e["image_const_pose"]]).astype(np.uint8)
    s["points"] = np.concatenate([s["points"], e["points"][keep]])
    s["obs_image"] = np.concatenate([s["obs_image"], e["obs_image"][ok] + I0]).astype(np.int32)
    s["obs_point"] = np.concatenate([s["obs_point"], new_id[e["obs_point"][ok]] + P0]).astype(np.int32)
    s["obs_xy"] = np.concatenate([s["obs_xy"], e["obs_xy"][ok]])
    s["lidar_point"] = np.concatenate([s["lidar_point"], new_id[e["lidar_point"][lk]] + P0]).astype(np.int32)
    s["lidar_abcd"] = np.concatenate([s["lidar_abcd"], e["lidar_abcd"][lk]])
    s["lidar_weight"] = np.concatenate([s["lidar_weight"], e["lidar_weight"][lk]])


ncase = 0
while time.time() < t_end:
    I = int(rng.choice([1, 2, 5, 17, 40]))
    P = int(rng.choice([1, 30, 500, 4000]))
    if rng.random() < 0.15:
        I, P = 2, 9000           # > 1024 observations per image: several segments
    s = synth.ba_scene(I, P, seed=int(rng.integers(1 << 30)), const_pose_frac=float(rng.choice([0, 0.25, 1.0])),
                       order=str(rng.choice(["point", "image"])))
    mixed = rng.random() < 0.3
    C = int(rng.integers(1, 4))
    models = [int(rng.integers(0, 11)) for _ in range(C)] if mixed else [int(rng.integers(0, 11))] * C
    s["cam_model"] = np.array(models, np.int32)
    s["cam_params_list"] = [cam_params(m) for m in models]
    s["image_camera"] = rng.integers(0, C, I).astype(np.int32)
    scale_quaternions(s)
    with_edges = rng.random() < 0.3
    if with_edges:
        append_edge_observations(s, models)
        I, P, C = s["poses"].shape[0], s["points"].shape[0], len(s["cam_model"])
    O = len(s["obs_image"])
    if O and rng.random() < 0.3:   # shuffled observation order
        perm = rng.permutation(O)
        s["obs_image"], s["obs_point"], s["obs_xy"] = s["obs_image"][perm], s["obs_point"][perm], s["obs_xy"][perm]
    models = [int(m) for m in s["cam_model"]]
    tv = rng.integers(0, 8, I).astype(np.uint8) * (rng.random(I) < 0.3)
    pc = (rng.random(P) < rng.choice([0.0, 0.1, 1.0])).astype(np.uint8)
    loss = [(0, 1.0), (1, 1.0), (2, 2.5), (1, 0.3)][int(rng.integers(0, 4))]
    kw = dict(image_const_tvec=tv.astype(np.uint8), point_const=pc, loss_type=loss[0], loss_scale=loss[1])
    ctx = dict(I=I, P=P, O=O, L=len(s.get("lidar_point", [])), models=models, loss=loss, case=ncase, edges=with_edges)
    ob = oracle.BA(**s, **kw)
    ba = pcdhip.BA(**s, **kw)
    cost, Himg, gimg, Hpt, gpt, W = ob.normal_equations(want_w=True)
    got = ba.evaluate(("cost", "H_img", "g_img", "H_pt", "g_pt", "W"))
    if abs(got["cost"][0] - cost) > 1e-10 * max(abs(cost), 1e-30):
        print("MISMATCH cost", ctx, got["cost"][0], cost); sys.exit(1)
    for k, ref in (("H_img", Himg), ("g_img", gimg), ("H_pt", Hpt), ("g_pt", gpt), ("W", W)):
        close(got[k], ref, 1e-8, k, ctx)
    close(ba.evaluate(("W",))["W"], W, 1e-8, "W raw", ctx)
    c1 = ba.evaluate(("cost",))["cost"][0]
    if abs(c1 - cost) > 1e-10 * max(abs(cost), 1e-30):
        print("MISMATCH cost-only pass", ctx, c1, cost); sys.exit(1)
    res, Jq, Jt, JX, Jc, JL = ob.evaluate_raw()
    raw = ba.evaluate(("residuals", "jac_q", "jac_t", "jac_X", "jac_lidar", "jac_cam"))
    close(raw["residuals"], res, 1e-9, "residuals", ctx)
    close(raw["jac_q"], Jq, 1e-8, "jac_q", ctx); close(raw["jac_t"], Jt, 1e-8, "jac_t", ctx)
    close(raw["jac_X"], JX, 1e-8, "jac_X", ctx); close(raw["jac_lidar"], JL, 1e-11, "jac_lidar", ctx)
    if O:
        Kmax = max(NP[m] for m in models)
        close(raw["jac_cam"][:, :, :Kmax], Jc[:, :, :Kmax], 1e-8, "jac_cam", ctx)
    ba.close()
    if rng.random() < 0.5 and O:
        flags = [bool(rng.integers(0, 2)) for _ in range(3)]
        const_cams = tuple(int(c) for c in range(C) if rng.random() < 0.3)
        mask = pcdhip.camera_refine_mask(s["cam_model"], *flags, constant_cameras=const_cams)
        H, g, E, Wc = ob.camera_blocks(mask, want_w=True)
        bc = pcdhip.BA(**s, **kw, camera_refine=mask)
        gc = bc.evaluate(("H_cam", "g_cam", "E_cam", "W_cam"))
        for k, ref in (("H_cam", H), ("g_cam", g), ("E_cam", E), ("W_cam", Wc)):
            close(gc[k], ref, 1e-8, k, dict(ctx, flags=flags, const_cams=const_cams))
        bc.close()
    ncase += 1
    if ncase % 20 == 0:
        print("cases %d, %.0f s left" % (ncase, t_end - time.time()), flush=True)
print("OK: %d cases, no mismatch" % ncase)

"""One local-BA hand-over between the depth projection and bundle adjustment at workload M (the bench's BA scene and
cloud: synth.ba_scene(1000, 1_000_000, seed=11, order="image") against synth.cloud_planes(10_000_000)), two ways
(DESIGN 4.3c).

  python tools/ba_proj_probe.py [--out profiles/ba_proj_probe.txt] [--reps 3] [--cams N --points N --cloud N]

Both routes start from a live BA handle and end with a handle that carries one Proj term per point that has a candidate
(every point takes the projection route, every image is projected).

  host route     only entry points that exist without pcd_ba_project_lidar_device: BA.get_parameters (poses and points
                 to the host), Projector.set_new_images (features up and 81 B per feature back through pageable host
                 buffers), the selection of shim/lidar_hip.h MatchVariablePoint2LidarPoint vectorised in numpy, the
                 handle destroyed and pcd_ba_create on the whole problem again.
  device route   pcd_ba_project_lidar_device on the live handle: proj_ms (record preparation, splat, read-out, pick),
                 rebuild_ms as the call reports them, the call's wall time, and from one more call with the library's
                 event timers on the time of every scope.

Medians of --reps after one warm-up round; wall times with the device idle before and after.  The two term lists are
compared: same points, same planes."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pcdhip  # noqa: E402
from pcdhip import synth  # noqa: E402

WIDTH, HEIGHT = 4032, 3024


def select(points, obs_point, obs_image, found, l6):
    """MatchVariablePoint2LidarPoint for every point at once; found / l6 per observation (the caller's order).
    Returns (points with a term, abcd, lidar_xyz)."""
    o = np.flatnonzero(found)
    # of several found observations of a point in one image only the first counts
    key = obs_point[o].astype(np.int64) * (int(obs_image.max()) + 1) + obs_image[o]
    _, first = np.unique(key, return_index=True)
    o = o[np.sort(first)]
    c = l6[o]
    v = points[obs_point[o]] - c[:, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        dot = v[:, 0] * c[:, 3] + v[:, 1] * c[:, 4] + v[:, 2] * c[:, 5]
        nn = np.sqrt(c[:, 3] * c[:, 3] + c[:, 4] * c[:, 4] + c[:, 5] * c[:, 5])
        vn = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        a = np.abs(dot / (nn * vn))
    ok = a < 360                                     # a NaN never wins
    o, c, a = o[ok], c[ok], a[ok]
    order = np.lexsort((o, a, obs_point[o]))         # per point: smallest |cos|, ties to the lowest observation
    p_sorted = obs_point[o][order]
    head = np.ones(len(order), bool)
    head[1:] = p_sorted[1:] != p_sorted[:-1]
    win = order[head]
    best = c[win]
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.sqrt(best[:, 3] * best[:, 3] + best[:, 4] * best[:, 4] + best[:, 5] * best[:, 5])
        n = best[:, 3:] / norm[:, None]
        d = 0 - n[:, 0] * best[:, 0] - n[:, 1] * best[:, 1] - n[:, 2] * best[:, 2]
    abcd = np.concatenate([n, d[:, None]], axis=1)
    keep = ~np.isnan(abcd).any(axis=1)
    return obs_point[o][win][keep].astype(np.int32), abcd[keep], best[keep, :3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cams", type=int, default=1000)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--cloud", type=int, default=10_000_000)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    def med(v):
        return "%.2f (%.2f .. %.2f)" % (float(np.median(v)), min(v), max(v))

    have_device_route = hasattr(pcdhip.lib(), "pcd_ba_project_lidar_device") and hasattr(pcdhip.BA, "project_lidar")
    log("# tools/ba_proj_probe.py on %s, torch %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                  os.path.relpath(pcdhip.LIB_PATH, ROOT)))
    xyz, nrm = synth.cloud_planes(a.cloud)
    cloud = pcdhip.Cloud(xyz, nrm, raw_lidar_frame=False)
    pj = pcdhip.Projector(cloud)
    scene = synth.ba_scene(a.cams, a.points, seed=11, order="image")
    base = {k: v for k, v in scene.items() if k not in ("lidar_point", "lidar_abcd", "lidar_weight")}
    P, O, I = len(scene["points"]), len(scene["obs_image"]), len(scene["poses"])
    log("scene: %d images, %d points, %d observations; cloud of %d points, %d submaps" % (I, P, O, len(cloud), pj.num_submaps))
    obs_image, obs_point = scene["obs_image"], scene["obs_point"]
    order = np.argsort(obs_image, kind="stable")          # image-major features, ascending observation index
    start = np.searchsorted(obs_image[order], np.arange(I + 1))
    feat = np.ascontiguousarray(scene["obs_xy"][order])
    prm = list(scene["cam_params_list"][0])

    # ---- host route ----
    ba = pcdhip.BA(**base)
    t = dict(params=[], project=[], select=[], create=[], handover=[])
    host_terms = None
    for rep in range(a.reps + 1):
        (poses, points), t_params = wall(ba.get_parameters)

        def project():
            images = [dict(qvec=poses[i, :4], tvec=poses[i, 4:], params=prm, width=WIDTH, height=HEIGHT,
                           feat_begin=int(start[i]), feat_end=int(start[i + 1])) for i in range(I)]
            return pj.set_new_images(images, feat)
        (found_f, _, _, l6_f, _), t_project = wall(project)

        def pick():
            found, l6 = np.zeros(O, np.uint8), np.zeros((O, 6))
            found[order], l6[order] = found_f, l6_f
            return select(points, obs_point, obs_image, found, l6)
        (lp, abcd, lxyz), t_select = wall(pick)

        def recreate():
            ba.close()
            return pcdhip.BA(**dict(base, poses=poses, points=points), lidar_point=lp, lidar_abcd=abcd,
                             lidar_weight=np.ones(len(lp)))
        ba, t_create = wall(recreate)
        host_terms = (lp, abcd)
        if rep:
            for k, v in (("params", t_params), ("project", t_project), ("select", t_select), ("create", t_create),
                         ("handover", t_params + t_project + t_select + t_create)):
                t[k].append(v)
    log("host route, %d of %d features found, %d terms: get_parameters %s ms | set_new_images (host buffers) %s ms | "
        "selection (numpy) %s ms | destroy + pcd_ba_create %s ms" % (int(found_f.sum()), O, len(host_terms[0]), med(t["params"]),
                                                                    med(t["project"]), med(t["select"]), med(t["create"])))
    log("host route hand-over: %s ms" % med(t["handover"]))

    # ---- device route ----
    if have_device_route:
        r = dict(proj=[], rebuild=[], wall=[])
        info = None
        for rep in range(a.reps + 1):
            info, t_wall = wall(lambda: ba.project_lidar(pj, (WIDTH, HEIGHT)))
            if rep:
                r["proj"].append(info["proj_ms"]); r["rebuild"].append(info["rebuild_ms"]); r["wall"].append(t_wall)
        got = ba.get_lidar()
        same = np.array_equal(got["point"], host_terms[0]) and np.array_equal(got["abcd"], host_terms[1])
        log("device route, %d of %d features found, %d terms, %d (image, submap) pairs: proj_ms %s | rebuild_ms %s | wall "
            "time of the call %s ms" % (info["num_found"], info["num_features"], info["num_terms"], info["pairs"],
                                        med(r["proj"]), med(r["rebuild"]), med(r["wall"])))
        log("device route hand-over (wall time of the call): %s ms; terms equal to the host route's: %s" % (med(r["wall"]), same))
        # where the call's time goes: one more call with the library's per-scope event timers on (not part of the medians)
        pcdhip.profile_reset()
        pcdhip.profile_enable(True)
        ba.project_lidar(pj, (WIDTH, HEIGHT))
        torch.cuda.synchronize()
        prof = pcdhip.profile_get()
        pcdhip.profile_enable(False)
        log("device route, scopes of one call (ms): " + ", ".join(
            "%s %.3f" % (k, prof[k][1]) for k in ("proj_prepare", "proj_feat_init", "proj_cull", "proj_splat", "proj_readout",
                                                   "ba_lidar_proj_pick", "ba_lidar_flag", "ba_lidar_rebuild") if k in prof))
    else:
        log("device route: this library has no pcd_ba_project_lidar_device")
    ba.close()
    pj.close()
    cloud.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

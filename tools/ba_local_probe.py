"""The start of a local round at workload M (the bench's BA scene: synth.ba_scene(1000, 1_000_000, seed=11,
order="image")), two ways.

  python tools/ba_local_probe.py [--out profiles/ba_local_probe.txt] [--reps 3] [--cams N --points N]

Both routes start from a live BA handle that holds the whole map and end with a handle that holds the sub-problem of
IncrementalMapper::AdjustLocalBundle for one image (its bundle of local_ba_num_images - 1 = 5 images by FindLocalBundle,
the points it observes variable), its co-visibility structure built, and with the (here unchanged) parameters back in the
whole-map handle.  Three images: those with the fewest, the median and the most rows.

  host route     what the library offered before: pcd_ba_get_parameters, FindLocalBundle and the selection in numpy
                 (vectorised: bincount for the shared rows, array arithmetic and np.partition for the percentiles),
                 pcd_ba_create on the sub-problem, the structure build of its first Schur call, pcd_ba_set_parameters.
  device route   BA.local_bundle and BA.local_window on the live handle (the bundle's wall time includes reading the
                 bundle back; build_ms as the window call reports it), the same structure build on the window,
                 BA.commit_window.  The device time of the bundle's launches alone is given beside it.

Beside them: one LM iteration (pcd_ba_solve, PCG, max_num_iterations = 1) on the window and on the whole handle, each
after one warm-up solve on the same handle and from the same parameters.
Medians of --reps after one warm-up; wall times with the device idle before and after."""
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

DEG = 0.0174532925199432954743716805978692718781530857086181640625
PASSES = ((1.0, .6), (1.5, .6), (2.0, .5), (2.5, .4), (3.0, .3), (4.0, .2), (5.0, .1), (6.0, .1))


def centers(poses):
    """ProjectionCenter of every image: the normalised quaternion conjugated, applied to -tvec"""
    q = poses[:, :4] / np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    return synth._quat_rotate(q * np.array([1.0, -1, -1, -1]), -poses[:, 4:])


def find_local_bundle(scene, poses, points, image, num_images=6, min_deg=6.0):
    """FindLocalBundle on the host, vectorised; ties in the shared count go to the lower image index"""
    oi, op = scene["obs_image"], scene["obs_point"]
    mine = oi == image
    n = int(mine.sum())
    mult = np.bincount(op[mine], minlength=len(points))
    shared = np.bincount(oi, weights=mult[op], minlength=len(poses)).astype(np.int64)
    shared[image] = 0
    cand = [int(j) for j in np.argsort(-shared, kind="stable") if shared[j] > 0]
    eff = min(num_images - 1, len(cand))
    if len(cand) == eff:
        return cand
    c = centers(poses)
    X = points[op[mine]]
    k = min(n - 1, int(np.floor(0.75 * (n - 1) + 0.5)))
    tri = {}

    def angle(j):
        if j not in tri:
            base2 = ((c[image] - c[j]) ** 2).sum()
            r1, r2 = ((X - c[image]) ** 2).sum(axis=1), ((X - c[j]) ** 2).sum(axis=1)
            den = 2.0 * np.sqrt(r1 * r2)
            with np.errstate(invalid="ignore", divide="ignore"):
                a = np.abs(np.arccos((r1 + r2 - base2) / den))
            a = np.where(den == 0.0, 0.0, np.minimum(a, np.pi - a))
            tri[j] = float(np.partition(a, k)[k])
        return tri[j]

    out, used = [], set()
    m = min_deg * DEG
    for d, f in PASSES:
        for j in cand:
            if float(shared[j]) < f * n:
                break
            if j not in used and angle(j) >= m / d:
                out.append(j); used.add(j)
                if len(out) >= eff:
                    return out
    for j in cand:
        if j not in used:
            out.append(j)
            if len(out) >= eff:
                break
    return out


def select(scene, poses, points, image, bundle):
    """the description of the local sub-problem, selected on the host"""
    I, P = len(poses), len(points)
    oi, op = scene["obs_image"], scene["obs_point"]
    inn = np.zeros(I, bool)
    inn[[image] + list(bundle)] = True
    length = np.bincount(op, minlength=P)
    V = np.zeros(P, bool)
    V[op[oi == image]] = True
    V &= length <= 1000
    keep = inn[oi] | V[op]
    kept = np.bincount(op[keep], minlength=P)
    pc = scene.get("point_const")
    pconst = ((kept > 0) & (kept < length)) | (False if pc is None else (np.asarray(pc) != 0))
    lkeep = V[scene["lidar_point"]]
    cp = scene.get("image_const_pose")
    cpose = ~inn if cp is None else (~inn | (np.asarray(cp) != 0))
    return dict(scene, poses=poses, points=points, image_const_pose=cpose.astype(np.uint8), point_const=pconst.astype(np.uint8),
                obs_image=oi[keep], obs_point=op[keep], obs_xy=scene["obs_xy"][keep],
                lidar_point=scene["lidar_point"][lkeep], lidar_abcd=scene["lidar_abcd"][lkeep],
                lidar_weight=scene["lidar_weight"][lkeep])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cams", type=int, default=1000)
    ap.add_argument("--points", type=int, default=1_000_000)
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

    log("# tools/ba_local_probe.py on %s, torch %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                   os.path.relpath(pcdhip.LIB_PATH, ROOT)))
    scene = synth.ba_scene(a.cams, a.points, seed=11, order="image")
    scene["obs_xy"] = np.asarray(scene["obs_xy"]).reshape(-1, 2)
    I, P, O = len(scene["poses"]), len(scene["points"]), len(scene["obs_image"])
    log("scene: %d images, %d points, %d observations, %d LiDAR terms" % (I, P, O, len(scene["lidar_point"])))
    rows = np.bincount(scene["obs_image"], minlength=I)
    order = np.argsort(rows, kind="stable")
    ba = pcdhip.BA(**scene)
    ba.schur_build()
    solve = dict(max_num_iterations=1, linear_solver="pcg")
    for image in (int(order[0]), int(order[I // 2]), int(order[-1])):
        h = dict(download=[], bundle=[], select=[], create=[], structure=[], upload=[], total=[])
        d = dict(bundle=[], build=[], wall=[], structure=[], commit=[], total=[])
        it_win = []
        info = bundle_h = bundle_d = None
        for rep in range(a.reps + 1):
            (poses, points), t_down = wall(ba.get_parameters)
            bundle_h, t_bundle = wall(lambda: find_local_bundle(scene, poses, points, image))
            sub, t_sel = wall(lambda: select(scene, poses, points, image, bundle_h))
            fresh, t_create = wall(lambda: pcdhip.BA(**sub))
            _, t_struct = wall(fresh.schur_build)
            _, t_up = wall(lambda: ba.set_parameters(*fresh.get_parameters()))
            st_host = fresh.schur_structure()
            fresh.close()
            if rep:
                for key, v in (("download", t_down), ("bundle", t_bundle), ("select", t_sel), ("create", t_create),
                               ("structure", t_struct), ("upload", t_up),
                               ("total", t_down + t_bundle + t_sel + t_create + t_struct + t_up)):
                    h[key].append(v)
            (bundle_d, binfo), t_b = wall(lambda: ba.local_bundle(image))
            bundle_d = [int(j) for j in bundle_d]
            (win, info), t_wall = wall(lambda: ba.local_window(binfo["image_set"], image=image))
            _, t_struct = wall(win.schur_build)
            _, t_commit = wall(lambda: ba.commit_window(win))
            st_dev = win.schur_structure()
            same = list(bundle_d) == list(bundle_h)
            if same:
                assert (win.O, win.L) == (len(sub["obs_image"]), len(sub["lidar_point"]))
                assert np.array_equal(st_dev["pairs"], st_host["pairs"])
            pcdhip.ba_solve(win, **solve)               # the first solve allocates the handle's state: warm up
            win.set_parameters(*ba.get_parameters())
            _, t_it = wall(lambda: pcdhip.ba_solve(win, **solve))
            win.close()
            if rep:
                d["bundle"].append(t_b); d["build"].append(info["build_ms"]); d["wall"].append(t_wall)
                d["structure"].append(t_struct); d["commit"].append(t_commit)
                d["total"].append(t_b + t_wall + t_struct + t_commit)
                it_win.append(t_it)
        log("image %d (%d rows): bundle %s%s; %d points variable, %d fixed, %d of %d observations, %d terms, %d pose rows"
            % (image, rows[image], bundle_d, "" if list(bundle_d) == list(bundle_h) else " (host: %s)" % bundle_h,
               info["num_points_variable"], info["num_points_fixed"], info["num_obs"], O, info["num_lidar"],
               info["num_pose_rows"]))
        log("  host route:   get_parameters %s ms | numpy FindLocalBundle %s ms | numpy selection %s ms | pcd_ba_create %s ms | "
            "Schur structure build %s ms | set_parameters %s ms | total %s ms"
            % (med(h["download"]), med(h["bundle"]), med(h["select"]), med(h["create"]), med(h["structure"]),
               med(h["upload"]), med(h["total"])))
        log("  device route: local_bundle %s ms | local_window %s ms (build_ms %s) | Schur structure build %s ms | "
            "commit_window %s ms | total %s ms" % (med(d["bundle"]), med(d["wall"]), med(d["build"]), med(d["structure"]),
                                                   med(d["commit"]), med(d["total"])))
        log("  one LM iteration on the window (pcd_ba_solve, PCG): %s ms" % med(it_win))
        # the bundle's launches alone (k_lb_mult .. k_lb_select with the sort), by the library's event scope
        pcdhip.profile_enable(True)
        pcdhip.profile_only("ba_local_bundle")
        scope = []
        for rep in range(a.reps + 1):
            pcdhip.profile_reset()
            ba.local_bundle(image)
            torch.cuda.synchronize()
            if rep:
                scope.append(pcdhip.profile_get()["ba_local_bundle"][1])
        pcdhip.profile_only(None)
        pcdhip.profile_enable(False)
        log("  device time of the bundle's launches (scope ba_local_bundle): %s ms" % med(scope))
    it_all = []
    for rep in range(a.reps + 1):
        ba.set_parameters(scene["poses"], scene["points"])
        _, t_it = wall(lambda: pcdhip.ba_solve(ba, **solve))
        if rep:
            it_all.append(t_it)
    log("one LM iteration on the whole handle (pcd_ba_solve, PCG): %s ms" % med(it_all))
    ba.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The sphere window of a global round at workload M (the bench's BA scene: synth.ba_scene(1000, 1_000_000, seed=11,
order="image")), two ways.

  python tools/ba_window_probe.py [--out profiles/ba_window_probe.txt] [--reps 3] [--cams N --points N]

Both routes start from a live BA handle that holds the whole map and end with a handle that holds the sphere sub-problem
of IncrementalMapper::AdjustGlobalBundleByLidar, its co-visibility structure built, and with the (here unchanged)
parameters back in the whole-map handle.  The sphere is centred on the last image and holds about 1 %, 10 % and 100 % of
the images (the radius sits between two neighbouring distances).

  host route     what the library offered before pcd_ba_window_create_device: pcd_ba_get_parameters, the selection in
                 numpy (centres, in-flags, active points, compaction of the rows and terms), pcd_ba_create on the
                 sub-problem, the structure build of its first Schur call, pcd_ba_set_parameters with its parameters.
  device route   BA.sphere_window on the live handle (build_ms as the call reports it, and its wall time), the same
                 structure build on the window, BA.commit_window.

Beside them: one LM iteration (pcd_ba_solve, PCG, max_num_iterations = 1) on the window and on the whole handle, each
after one warm-up solve on the same handle (the first solve allocates the handle's Schur, PCG and LM state) and from the
same parameters.
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


def distances(poses, center):
    """distance of every projection centre from image `center`'s, c = -R(q)^T t on the stored quaternion"""
    w, x, y, z, t0, t1, t2 = (poses[:, k] for k in range(7))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    c = np.stack([-(((1.0 - (tyy + tzz)) * t0 + (txy + twz) * t1) + (txz - twy) * t2),
                  -(((txy - twz) * t0 + (1.0 - (txx + tzz)) * t1) + (tyz + twx) * t2),
                  -(((txz + twy) * t0 + (tyz - twx) * t1) + (1.0 - (txx + tyy)) * t2)], axis=1)
    d = c[center] - c
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def select(scene, poses, points, center, radius):
    """the description of the sphere sub-problem, selected on the host"""
    inn = distances(poses, center) <= radius
    act = np.zeros(len(points), bool)
    act[scene["obs_point"][inn[scene["obs_image"]]]] = True
    keep = act[scene["obs_point"]]
    lkeep = act[scene["lidar_point"]]
    cp = scene.get("image_const_pose")
    cpose = ~inn if cp is None else (~inn | (np.asarray(cp) != 0))
    return dict(scene, poses=poses, points=points, image_const_pose=cpose.astype(np.uint8),
                obs_image=scene["obs_image"][keep], obs_point=scene["obs_point"][keep], obs_xy=scene["obs_xy"][keep],
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

    log("# tools/ba_window_probe.py on %s, torch %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                    os.path.relpath(pcdhip.LIB_PATH, ROOT)))
    scene = synth.ba_scene(a.cams, a.points, seed=11, order="image")
    scene["obs_xy"] = np.asarray(scene["obs_xy"]).reshape(-1, 2)
    I, P, O = len(scene["poses"]), len(scene["points"]), len(scene["obs_image"])
    log("scene: %d images, %d points, %d observations, %d LiDAR terms" % (I, P, O, len(scene["lidar_point"])))
    center = I - 1
    dist = np.sort(distances(np.asarray(scene["poses"], np.float64).reshape(-1, 7), center))
    ba = pcdhip.BA(**scene)
    ba.schur_build()
    solve = dict(max_num_iterations=1, linear_solver="pcg")
    for frac in (0.01, 0.1, 1.0):
        k = max(1, min(I, int(round(frac * I))))
        radius = float("inf") if k == I else float(0.5 * (dist[k - 1] + dist[k]))
        h = dict(download_select=[], create=[], structure=[], upload=[], total=[])
        d = dict(build=[], wall=[], structure=[], commit=[], total=[])
        it_win = []
        info = None
        for rep in range(a.reps + 1):
            def host_select():
                poses, points = ba.get_parameters()
                return select(scene, poses, points, center, radius)
            sub, t_sel = wall(host_select)
            fresh, t_create = wall(lambda: pcdhip.BA(**sub))
            _, t_struct = wall(fresh.schur_build)
            _, t_up = wall(lambda: ba.set_parameters(*fresh.get_parameters()))
            st_host = fresh.schur_structure()
            fresh.close()
            if rep:
                for key, v in (("download_select", t_sel), ("create", t_create), ("structure", t_struct), ("upload", t_up),
                               ("total", t_sel + t_create + t_struct + t_up)):
                    h[key].append(v)
            (win, info), t_wall = wall(lambda: ba.sphere_window(center, radius))
            _, t_struct = wall(win.schur_build)
            _, t_commit = wall(lambda: ba.commit_window(win))
            st_dev = win.schur_structure()
            assert (win.O, win.L) == (len(sub["obs_image"]), len(sub["lidar_point"]))
            assert np.array_equal(st_dev["pairs"], st_host["pairs"])
            # the first solve on a handle allocates its Schur, PCG and LM state: warm up, put the parameters back, time
            pcdhip.ba_solve(win, **solve)
            win.set_parameters(*ba.get_parameters())
            _, t_it = wall(lambda: pcdhip.ba_solve(win, **solve))
            win.close()
            if rep:
                d["build"].append(info["build_ms"]); d["wall"].append(t_wall); d["structure"].append(t_struct)
                d["commit"].append(t_commit); d["total"].append(t_wall + t_struct + t_commit)
                it_win.append(t_it)
        log("sphere of %d of %d images (radius %.3f): %d points active, %d of %d observations, %d terms, %d pose rows"
            % (info["num_images_in"], I, radius, info["num_points_active"], info["num_obs"], O, info["num_lidar"],
               info["num_pose_rows"]))
        log("  host route:   get_parameters + numpy selection %s ms | pcd_ba_create %s ms | Schur structure build %s ms | "
            "set_parameters %s ms | total %s ms" % (med(h["download_select"]), med(h["create"]), med(h["structure"]),
                                                    med(h["upload"]), med(h["total"])))
        log("  device route: build_ms %s | wall time of sphere_window %s ms | Schur structure build %s ms | commit_window "
            "%s ms | total %s ms" % (med(d["build"]), med(d["wall"]), med(d["structure"]), med(d["commit"]), med(d["total"])))
        log("  one LM iteration on the window (pcd_ba_solve, PCG): %s ms" % med(it_win))
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

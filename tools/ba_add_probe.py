"""Observations and points added between two bundle adjustments at workload M (the bench's BA scene: synth.ba_scene(1000,
1_000_000, seed=11, order="image")), two ways.

  python tools/ba_add_probe.py [--out profiles/ba_add_probe.txt] [--reps 3] [--cams N --points N]

Both routes start from a live BA handle that has a co-visibility structure and lacks some rows of the scene, and from
those rows in host memory (numpy), where CompleteAndMergeTracks and the retriangulation produce them.  Held out: roughly
0.1 %, 1 % and 10 % of the observations at random (one seed per fraction), and the last 0.1 % of the points with all
their rows.  What differs is how the handle gains them:

  host route     what the library offered before pcd_ba_add_observations_device: pcd_ba_get_parameters, the arrays
                 concatenated on the host (numpy), the handle destroyed, pcd_ba_create on the grown problem (every
                 observation uploaded, track CSR / sliced ELL / image-major order / pose rows rebuilt by host counting
                 sorts), then the structure build of the first Schur call (pcd_ba_schur_build_device).
  device route   BA.add_observations on the live handle with the numpy rows (their upload is inside the call's wall
                 time; rebuild_ms as pcd_ba_add_observations_device reports it), then the same structure build, which
                 both routes need: the structure depends on the observations.

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


def hold_out(scene, out, n_points):
    """(base, additions): the scene without the rows flagged in `out` and without its last n_points points, whose rows
    and LiDAR terms go with them"""
    Pb = len(scene["points"]) - n_points
    out = out | (scene["obs_point"] >= Pb)
    lkeep = scene["lidar_point"] < Pb
    base = dict(scene, points=scene["points"][:Pb], obs_image=scene["obs_image"][~out], obs_point=scene["obs_point"][~out],
                obs_xy=scene["obs_xy"][~out], lidar_point=scene["lidar_point"][lkeep], lidar_abcd=scene["lidar_abcd"][lkeep],
                lidar_weight=scene["lidar_weight"][lkeep])
    add = dict(obs_image=np.ascontiguousarray(scene["obs_image"][out]), obs_point=np.ascontiguousarray(scene["obs_point"][out]),
               obs_xy=np.ascontiguousarray(scene["obs_xy"][out]), new_points=np.ascontiguousarray(scene["points"][Pb:]))
    return base, add


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

    log("# tools/ba_add_probe.py on %s, torch %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                 os.path.relpath(pcdhip.LIB_PATH, ROOT)))
    scene = synth.ba_scene(a.cams, a.points, seed=11, order="image")
    scene["obs_xy"] = np.asarray(scene["obs_xy"]).reshape(-1, 2)
    P, O = len(scene["points"]), len(scene["obs_image"])
    log("scene: %d images, %d points, %d observations, %d LiDAR terms" % (len(scene["poses"]), P, O, len(scene["lidar_point"])))

    cases = [("%.1f %% of the observations" % (100 * f), f, 0) for f in (0.001, 0.01, 0.1)]
    cases.append(("0.1 % of the points with all their rows", 0.0, max(1, P // 1000)))
    for name, frac, n_points in cases:
        rng = np.random.default_rng(int(frac * 1e4) + n_points)
        base, add = hold_out(scene, rng.random(O) < frac, n_points)
        A, Pn = len(add["obs_image"]), len(add["new_points"])
        h = dict(download_concat=[], create=[], structure=[], total=[])
        d = dict(rebuild=[], wall=[], structure=[], total=[])
        for rep in range(a.reps + 1):
            ba = pcdhip.BA(**base)
            ba.schur_structure()

            def concat():
                poses, points = ba.get_parameters()
                pc = base.get("point_const")
                grown = dict(base, poses=poses, points=np.concatenate([points, add["new_points"]]),
                             obs_image=np.concatenate([base["obs_image"], add["obs_image"]]),
                             obs_point=np.concatenate([base["obs_point"], add["obs_point"]]),
                             obs_xy=np.concatenate([base["obs_xy"], add["obs_xy"]]))
                if pc is not None:
                    grown["point_const"] = np.concatenate([pc, np.zeros(Pn, np.uint8)])
                return grown
            new, t_host = wall(concat)

            def recreate():
                ba.close()
                return pcdhip.BA(**new)
            fresh, t_create = wall(recreate)
            _, t_struct = wall(fresh.schur_build)
            st_host = fresh.schur_structure()
            fresh.close()
            if rep:
                for k, v in (("download_concat", t_host), ("create", t_create), ("structure", t_struct),
                             ("total", t_host + t_create + t_struct)):
                    h[k].append(v)
            ba = pcdhip.BA(**base)
            ba.schur_structure()
            info, t_wall = wall(lambda: ba.add_observations(add["obs_image"], add["obs_point"], add["obs_xy"],
                                                            add["new_points"] if Pn else None))
            _, t_struct = wall(ba.schur_build)
            st_dev = ba.schur_structure()
            assert (ba.O, ba.P) == (O, P) and np.array_equal(st_dev["pairs"], st_host["pairs"])
            ba.close()
            if rep:
                d["rebuild"].append(info["rebuild_ms"]); d["wall"].append(t_wall); d["structure"].append(t_struct)
                d["total"].append(t_wall + t_struct)
        log("%s held out (%d rows and %d points added to %d rows and %d points)" % (name, A, Pn, O - A, P - Pn))
        log("  host route:   get_parameters + numpy concatenation %s ms | destroy + pcd_ba_create %s ms | Schur structure "
            "build %s ms | total %s ms" % (med(h["download_concat"]), med(h["create"]), med(h["structure"]), med(h["total"])))
        log("  device route: rebuild_ms %s | wall time of the call, upload of the rows included %s ms | Schur structure "
            "build %s ms | total %s ms" % (med(d["rebuild"]), med(d["wall"]), med(d["structure"]), med(d["total"])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

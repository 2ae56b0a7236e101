"""The filter step between two bundle adjustments at workload M (the bench's BA scene: synth.ba_scene(1000, 1_000_000,
seed=11, order="image")), two ways.

  python tools/ba_filter_probe.py [--out profiles/ba_filter_probe.txt] [--reps 3] [--cams N --points N]

Both routes start from a live BA handle that has a co-visibility structure and from filter flags on the device; roughly
0.1 %, 1 % and 10 % of the observations are flagged at random (one seed per fraction).  What differs is how the handle
loses them:

  host route     what the library offered before pcd_ba_remove_observations_device: the flags copied to the host, the
                 observation arrays compacted there (numpy), the handle destroyed, pcd_ba_create on the compacted problem
                 (every observation uploaded, track CSR / sliced ELL / image-major order / pose rows rebuilt by host
                 counting sorts), then the structure build of the first Schur call (pcd_ba_schur_build_device).
  device route   pcd_ba_remove_observations_device on the live handle (rebuild_ms as the call reports it, and the call's
                 wall time), then the same structure build, which both routes need: the structure depends on the
                 observations.  The build runs on the device; its stream synchronisations are reported.

The probe also times pcd_ba_filter_points_device beside pcd_ba_filter_tracks_device on the full handle.
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

    log("# tools/ba_filter_probe.py on %s, torch %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                    os.path.relpath(pcdhip.LIB_PATH, ROOT)))
    scene = synth.ba_scene(a.cams, a.points, seed=11, order="image")
    P, O = len(scene["points"]), len(scene["obs_image"])
    log("scene: %d images, %d points, %d observations, %d LiDAR terms" % (len(scene["poses"]), P, O, len(scene["lidar_point"])))
    dev = torch.device("cuda", 0)

    # ---- the two filters on the full handle ----
    ba = pcdhip.BA(**scene)
    out = ba.filter_points_device(8.0, 1.5)
    d_out = {k: (v.data_ptr() if v is not None else None) for k, v in out.items()}
    fo = pcdhip.BAFilterOut(*[d_out[k] for k, _ in pcdhip.BAFilterOut._fields_])
    import ctypes as C
    L = pcdhip.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    t_tracks, t_points = [], []
    opts = ba._filter_opts(8.0, 1.5)
    for rep in range(a.reps + 1):
        _, t1 = wall(lambda: L.pcd_ba_filter_tracks_device(ba._h, C.c_double(8.0), C.byref(fo), C.c_void_p(stream)))
        _, t2 = wall(lambda: L.pcd_ba_filter_points_device(ba._h, C.byref(opts), C.byref(fo), C.c_void_p(stream)))
        if rep:
            t_tracks.append(t1); t_points.append(t2)
    sm = out["summary"].cpu().numpy()
    L.pcd_ba_filter_tracks_device(ba._h, C.c_double(8.0), C.byref(fo), C.c_void_p(stream))
    sm1 = out["summary"].cpu().numpy()
    log("filter_tracks_device %s ms | filter_points_device (8 px, 1.5 deg) %s ms" % (med(t_tracks), med(t_points)))
    log("  the first filters %d elements and leaves %d points; the second filters %d (one per point of the angle stage) and "
        "leaves %d points" % (int(sm1[0]), int(sm1[2]), int(sm[0]), int(sm[2])))
    # the angle stage on EVERY track: a reprojection bound nothing exceeds, so stage 1 deletes only tracks shorter than 2
    wide = ba._filter_opts(1e9, 1.5)
    t_wide = []
    for rep in range(a.reps + 1):
        _, t3 = wall(lambda: L.pcd_ba_filter_points_device(ba._h, C.byref(wide), C.byref(fo), C.c_void_p(stream)))
        if rep:
            t_wide.append(t3)
    smw = out["summary"].cpu().numpy()
    L.pcd_ba_filter_tracks_device(ba._h, C.c_double(1e9), C.byref(fo), C.c_void_p(stream))
    smw1 = out["summary"].cpu().numpy()
    log("filter_points_device (1e9 px, 1.5 deg) %s ms: the angle stage runs on %d points and deletes %d"
        % (med(t_wide), int(smw1[2]), int(smw[0]) - int(smw1[0])))
    ba.close()

    # ---- the two routes of dropping observations ----
    for frac in (0.001, 0.01, 0.1):
        rng = np.random.default_rng(int(frac * 1e4))
        erase = (rng.random(O) < frac).astype(np.uint8)
        d_erase = torch.from_numpy(erase).to(dev)
        h = dict(d2h_compact=[], create=[], structure=[], total=[])
        d = dict(rebuild=[], wall=[], structure=[], total=[])
        kept = syncs = 0
        for rep in range(a.reps + 1):
            ba = pcdhip.BA(**scene)
            ba.schur_structure()

            def compact():
                e = d_erase.cpu().numpy() != 0
                return dict(scene, obs_image=scene["obs_image"][~e], obs_point=scene["obs_point"][~e],
                            obs_xy=np.asarray(scene["obs_xy"]).reshape(-1, 2)[~e])
            new, t_host = wall(compact)
            poses, points = ba.get_parameters()

            def recreate():
                ba.close()
                return pcdhip.BA(**dict(new, poses=poses, points=points))
            fresh, t_create = wall(recreate)
            b_host, t_struct = wall(fresh.schur_build)
            st_host = fresh.schur_structure()
            syncs = max(syncs, b_host["num_syncs"])
            kept = fresh.O
            fresh.close()
            if rep:
                for k, v in (("d2h_compact", t_host), ("create", t_create), ("structure", t_struct),
                             ("total", t_host + t_create + t_struct)):
                    h[k].append(v)
            ba = pcdhip.BA(**scene)
            ba.schur_structure()
            info, t_wall = wall(lambda: ba.remove_observations(d_erase))
            b_dev, t_struct = wall(ba.schur_build)
            st_dev = ba.schur_structure()
            syncs = max(syncs, b_dev["num_syncs"])
            assert ba.O == kept and np.array_equal(st_dev["pairs"], st_host["pairs"])
            ba.close()
            if rep:
                d["rebuild"].append(info["rebuild_ms"]); d["wall"].append(t_wall); d["structure"].append(t_struct)
                d["total"].append(t_wall + t_struct)
        log("%.1f %% flagged (%d of %d observations dropped)" % (100 * frac, O - kept, O))
        log("  host route:   flags to host + numpy compaction %s ms | destroy + pcd_ba_create %s ms | Schur structure build %s ms"
            " | total %s ms" % (med(h["d2h_compact"]), med(h["create"]), med(h["structure"]), med(h["total"])))
        log("  device route: rebuild_ms %s | wall time of the call %s ms | Schur structure build %s ms | total %s ms"
            % (med(d["rebuild"]), med(d["wall"]), med(d["structure"]), med(d["total"])))
        log("  structure builds: at most %d stream synchronisations each (num_syncs)" % syncs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

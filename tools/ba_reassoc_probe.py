"""One round's hand-over between association and bundle adjustment at workload M (the bench's BA scene and cloud:
synth.ba_scene(1000, 1_000_000, seed=11, order="image") against synth.cloud_planes(10_000_000)), two ways.

  python tools/ba_reassoc_probe.py [--out profiles/ba_reassoc_probe.txt] [--reps 3] [--cams N --points N --cloud N]

Both routes start from a live BA handle whose points are the next round's queries, and both run the same association
search (pcd_associate_device on all P points, MAPPER_GLOBAL, one radius).  What differs is what follows it:

  host route     the association rows (type, abcd, lidar_xyz: 57 B per point) copied to the host, the term rule applied
                 there (numpy), the handle destroyed, pcd_ba_create on the whole problem again (every observation
                 uploaded, track CSR / sliced ELL / image-major order / pose rows rebuilt), then the structure build of
                 the first Schur call (pcd_ba_schur_structure).  Only entry points that existed before the device route
                 are used, so the same script measures this route on an older library (PCDHIP_LIB=...).
  device route   pcd_ba_associate_lidar_device on the live handle: assoc_ms (the search and the epilogue) and rebuild_ms
                 (flag, scan, the one synchronisation, compaction, CSR bounds, thread-order fill) as the call reports
                 them, and the call's wall time.  The co-visibility structure is kept, so there is nothing else.

Medians of --reps after one warm-up round; wall times with the device idle before and after."""
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
    ap.add_argument("--cloud", type=int, default=10_000_000)
    ap.add_argument("--range", type=float, default=1.5)
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

    have_device_route = hasattr(pcdhip.lib(), "pcd_ba_associate_lidar_device") and hasattr(pcdhip.BA, "associate_lidar")
    log("# tools/ba_reassoc_probe.py on %s, torch %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                     os.path.relpath(pcdhip.LIB_PATH, ROOT)))
    xyz, nrm = synth.cloud_planes(a.cloud)
    cloud = pcdhip.Cloud(xyz, nrm, raw_lidar_frame=False)
    scene = synth.ba_scene(a.cams, a.points, seed=11, order="image")
    P, O = len(scene["points"]), len(scene["obs_image"])
    log("scene: %d images, %d points, %d observations, %d LiDAR terms at creation; cloud of %d points; radius %.2f m"
        % (len(scene["poses"]), P, O, len(scene["lidar_point"]), len(cloud), a.range))
    base = {k: v for k, v in scene.items() if k not in ("lidar_point", "lidar_abcd", "lidar_weight")}
    dev = torch.device("cuda", 0)
    d_out = dict(type=torch.empty(P, dtype=torch.uint8, device=dev), abcd=torch.empty((P, 4), dtype=torch.float64, device=dev),
                 lidar_xyz=torch.empty((P, 3), dtype=torch.float64, device=dev))
    d_range = torch.full((1,), a.range, dtype=torch.float64, device=dev)
    weight = np.array([0.0, 100.0, 1000.0, 0.0])

    # ---- host route ----
    ba = pcdhip.BA(**scene)
    ba.schur_structure()
    t = dict(assoc=[], d2h_filter=[], create=[], structure=[], handover=[])
    terms = 0
    for rep in range(a.reps + 1):
        points_ptr = ba.device_parameters()[1]
        _, t_assoc = wall(lambda: cloud.associate_device(points_ptr, P, d_range, 1, pcdhip.GATE_MAPPER_GLOBAL, d_out))

        def to_host():
            typ, abcd = d_out["type"].cpu().numpy(), d_out["abcd"].cpu().numpy()
            lxyz = d_out["lidar_xyz"].cpu().numpy()
            keep = (typ != 0) & ~np.isnan(abcd).any(axis=1)
            return dict(lidar_point=np.flatnonzero(keep).astype(np.int32), lidar_abcd=abcd[keep],
                        lidar_weight=weight[typ[keep]]), lxyz[keep]
        (new, _), t_host = wall(to_host)
        poses, points = ba.get_parameters()

        def recreate():
            ba.close()
            return pcdhip.BA(**dict(base, poses=poses, points=points), **new)
        ba, t_create = wall(recreate)
        _, t_struct = wall(ba.schur_structure)
        terms = len(new["lidar_point"])
        if rep:
            for k, v in (("assoc", t_assoc), ("d2h_filter", t_host), ("create", t_create), ("structure", t_struct),
                         ("handover", t_host + t_create + t_struct)):
                t[k].append(v)
    log("host route, %d terms: association %s ms | rows to host + filter %s ms | destroy + pcd_ba_create %s ms | "
        "Schur structure build %s ms" % (terms, med(t["assoc"]), med(t["d2h_filter"]), med(t["create"]), med(t["structure"])))
    log("host route hand-over (everything behind the association): %s ms" % med(t["handover"]))

    # ---- device route ----
    if have_device_route:
        r = dict(assoc=[], rebuild=[], wall=[])
        info = None
        for rep in range(a.reps + 1):
            info, t_wall = wall(lambda: ba.associate_lidar(cloud, max_range=d_range, gate_mode=pcdhip.GATE_MAPPER_GLOBAL))
            if rep:
                r["assoc"].append(info["assoc_ms"]); r["rebuild"].append(info["rebuild_ms"]); r["wall"].append(t_wall)
        assert info["num_terms"] == terms, (info, terms)
        log("device route, %d terms (%d icp, %d ground): assoc_ms %s | rebuild_ms %s | wall time of the call %s ms"
            % (info["num_terms"], info["num_icp"], info["num_icp_ground"], med(r["assoc"]), med(r["rebuild"]), med(r["wall"])))
        log("device route hand-over (rebuild_ms): %s ms" % med(r["rebuild"]))
    else:
        log("device route: this library has no pcd_ba_associate_lidar_device")
    ba.close()
    cloud.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

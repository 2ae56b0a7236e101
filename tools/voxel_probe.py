"""Time of the voxel-grid downsampling (pcd_cloud_voxel_downsample_device) on the bench cloud
(synth.cloud_planes(10_000_000)) at leaves 0.05 and 1.0 m, pass by pass, and the reduce kernels against their traffic
floor.

  python tools/voxel_probe.py [--out profiles/voxel_probe.txt] [--reps 10] [--points 10000000]

Per leaf: the median (min / max) of --reps runs after a warm-up, timed with the library's event scopes: `k_voxel_keys`,
`voxel_sort` (rocprim radix sort of 64-bit keys over the bits the key range needs), `voxel_heads` (head flags, the two
scans, segment starts, the min_points filter), `k_voxel_reduce` (the list of long voxels and both reduce kernels with
their epilogue), `k_voxel_map` (row_voxel) and `voxel_build` (the new handle's index build, host synchronisations
included).  The floor of the reduce: 36 B per row read (the 4-byte row index and the 32-byte pn8 record) plus 32 B per
voxel written, at the 6.29 TB/s a float4 copy reaches on this part (MI355X: 8 TB/s peak); the kernels also write the new
handle's pts4 (16 B per voxel more), which the floor leaves out."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pcdhip  # noqa: E402
from pcdhip import synth  # noqa: E402

COPY_TBS = 6.29
SCOPES = ("k_voxel_keys", "voxel_sort", "voxel_heads", "k_voxel_reduce", "k_voxel_map", "voxel_build")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--leaves", type=float, nargs="*", default=[0.05, 1.0])
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log("# tools/voxel_probe.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    xyz, nrm = synth.cloud_planes(a.points)
    cloud = pcdhip.Cloud(xyz, nrm, raw_lidar_frame=False)
    info = cloud.info()
    log("cloud_planes(%d): cell_size %.4f m, %d occupied cells, build %.1f ms"
        % (a.points, info["cell_size"], info["occupied_cells"], info["build_ms"]))
    d_map = torch.empty(len(cloud), dtype=torch.int32, device="cuda")
    for leaf in a.leaves:
        def run():
            out, vi = cloud.voxel_downsample_device(d_map, leaf)
            out.close()
            return vi
        vi = run()                                             # warm-up, and the counters
        t = {k: [] for k in SCOPES}
        total = []
        for _ in range(a.reps):
            pcdhip.profile_reset()
            pcdhip.profile_enable(True)
            v = run()
            torch.cuda.synchronize()
            got = pcdhip.profile_get()
            pcdhip.profile_enable(False)
            for k in SCOPES:
                t[k].append(got[k][1] if k in got else 0.0)
            total.append(v["ms"])
        med = {k: float(np.median(v)) for k, v in t.items()}
        log("== leaf %.2f m: %d rows -> %d voxels (at most %d rows per voxel, mean %.1f); dims %s"
            % (leaf, vi["num_input"], vi["num_voxels"], vi["max_points_per_voxel"],
               vi["num_input"] / max(vi["num_voxels"], 1), vi["dims"]))
        for k in SCOPES:
            log("   %-15s median %8.3f ms (min %.3f, max %.3f, n=%d)" % (k, med[k], min(t[k]), max(t[k]), len(t[k])))
        log("   info.ms (all passes before the build, host synchronisation included) median %.3f ms"
            % float(np.median(total)))
        floor_ms = (36.0 * vi["num_input"] + 32.0 * vi["num_voxels"]) / (COPY_TBS * 1e12) * 1e3
        log("   k_voxel_reduce: traffic floor (36 B per row + 32 B per voxel at %.2f TB/s) %.3f ms: measured / floor = "
            "%.2f, floor / measured = %.1f %%" % (COPY_TBS, floor_ms, med["k_voxel_reduce"] / floor_ms,
                                                 100.0 * floor_ms / max(med["k_voxel_reduce"], 1e-9)))
        log("   reduce / sort = %.2f" % (med["k_voxel_reduce"] / max(med["voxel_sort"], 1e-9)))
    cloud.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

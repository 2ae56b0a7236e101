"""Time of the normal estimation (pcd_cloud_estimate_normals_device) on the bench cloud
(synth.cloud_planes(10_000_000)) at r = 0.10, 0.15 and 0.20 m, against the VALU floor of its pair loop.

  python tools/normals_probe.py [--out profiles/normals_probe.txt] [--reps 10] [--points 10000000]

Per radius: the median (min / max) of --reps runs after a warm-up, timed with the library's event scopes
(`k_normals_brick`: the pair kernel, `normals_items`: the work-item list in front of it, which ends in one host
synchronisation); pair_tests and mean / max neighbours from the info struct; the floor
pair_tests x VALU_PER_PAIR / 64 lanes / 1024 SIMDs at the shader clock sampled (rocm-smi, read-only) while the pass runs
back to back, and measured time / floor.  The floor counts one wave instruction per SIMD per cycle; the second figure
weights the instructions with the issue intervals measured on this part (profiles/r02_ubench_valu_rate.txt)."""
import argparse
import os
import re
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pcdhip  # noqa: E402
from pcdhip import synth  # noqa: E402

# VALU instructions of one staged point in k_normals_brick's pair loop (gfx950 ISA of csrc/normals.hip): 1 v_mov,
# v_sub_f32 + v_pk_add_f32 (the three differences), v_mul_f32 + v_pk_mul_f32, 2 v_add_f32, v_cmp_le_f32, 3 v_cndmask_b32,
# 3 v_cvt_f64_f32, v_addc_co_u32 (the count), 3 v_add_f64, 6 v_fmac_f64
VALU_PER_PAIR = 24
F64_PER_PAIR = 12          # the widenings, sums and fused second moments
SIMDS = 256 * 4
# issue interval per wave64 instruction at 4-8 wavefronts per SIMD (profiles/r02_ubench_valu_rate.txt): fp32 ~2.4,
# fp64 / packed ~4.4 cycles
CYCLES_F32, CYCLES_F64 = 2.4, 4.4


def sample_clock(fn, seconds):
    """median sclk (MHz) reported while fn runs back to back for `seconds`; None when rocm-smi gives none"""
    stop, mhz = [False], []

    def sample():
        while not stop[0]:
            try:
                out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True,
                                     timeout=10).stdout
                mhz.extend(int(m) for m in re.findall(r"sclk clock level: \d+: \((\d+)Mhz\)", out))
            except Exception:
                pass
            time.sleep(0.05)
    th = threading.Thread(target=sample)
    th.start()
    t0 = time.time()
    while time.time() - t0 < seconds:
        fn()
        torch.cuda.synchronize()
    stop[0] = True
    th.join()
    return float(np.median(mhz)) if mhz else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--radii", type=float, nargs="*", default=[0.10, 0.15, 0.20])
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log("# tools/normals_probe.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    xyz, _ = synth.cloud_planes(a.points)
    cloud = pcdhip.Cloud(xyz, np.zeros_like(xyz), raw_lidar_frame=False)
    info = cloud.info()
    log("cloud_planes(%d): cell_size %.4f m, dims %s, %d occupied cells, build %.1f ms"
        % (a.points, info["cell_size"], info["dims"], info["occupied_cells"], info["build_ms"]))
    d_count = torch.empty(len(cloud), dtype=torch.int32, device="cuda")
    d_curv = torch.empty(len(cloud), dtype=torch.float64, device="cuda")
    for r in a.radii:
        host = cloud.estimate_normals(radius=r)["info"]            # counters (and the warm-up)
        run = lambda: cloud.estimate_normals_device(d_count, d_curv, radius=r)
        run()
        torch.cuda.synchronize()
        t = {"k_normals_brick": [], "normals_items": []}
        for _ in range(a.reps):
            pcdhip.profile_reset()
            pcdhip.profile_enable(True)
            run()
            torch.cuda.synchronize()
            got = pcdhip.profile_get()
            pcdhip.profile_enable(False)
            for k in t:
                t[k].append(got[k][1])
        mhz = sample_clock(run, 2.0)
        brick = np.asarray(t["k_normals_brick"])
        items = np.asarray(t["normals_items"])
        log("== r = %.2f m (%.2f cells): pair kernel median %.3f ms (min %.3f, max %.3f, n=%d); item list %.3f ms"
            % (r, r / info["cell_size"], np.median(brick), brick.min(), brick.max(), brick.size, np.median(items)))
        log("   pair_tests %.4g, neighbours mean %.1f / max %d; estimated %d, too few %d, degenerate %d"
            % (host["pair_tests"], host["mean_neighbors"], host["max_neighbors"], host["num_estimated"],
               host["num_too_few"], host["num_degenerate"]))
        if mhz is None:
            log("   shader clock: not measured (rocm-smi gave no sclk); no floor")
            continue
        wave_instr = host["pair_tests"] / 64.0 * VALU_PER_PAIR
        floor_ms = wave_instr / SIMDS / (mhz * 1e6) * 1e3
        cyc = (VALU_PER_PAIR - F64_PER_PAIR) * CYCLES_F32 + F64_PER_PAIR * CYCLES_F64
        issue_ms = host["pair_tests"] / 64.0 * cyc / SIMDS / (mhz * 1e6) * 1e3
        log("   sclk %.0f MHz while running; VALU floor (%d instructions per pair, 1 per SIMD per cycle) %.3f ms: "
            "measured / floor = %.2f" % (mhz, VALU_PER_PAIR, floor_ms, np.median(brick) / floor_ms))
        log("   with the measured issue intervals (%.1f cycles fp32, %.1f fp64: %.0f cycles per pair and wavefront) "
            "%.3f ms: measured / that = %.2f" % (CYCLES_F32, CYCLES_F64, cyc, issue_ms, np.median(brick) / issue_ms))
    cloud.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

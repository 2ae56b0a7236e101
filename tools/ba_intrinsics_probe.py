"""What a refining iteration of pcd_ba_solve costs (refined intrinsics in the reduced system), at bench.py's
BA workload M: 1000 images, 1 M points, 4.72 M observations, one shared OPENCV camera, the direct solver.

  python tools/ba_intrinsics_probe.py [--out profiles/ba_intrinsics_probe.txt] [--iters 10] [--warmup 2]
                                      [--parent-lib PATH/libpcdhip.so]

Legs: constant intrinsics (twice more at the end, to show the spread), focal length refined, all 8 parameters refined.
Each leg runs in a child process of its own (one handle, one HIP context): a warm-up solve of --warmup iterations, the
parameters put back, then one solve of --iters iterations with the library's profiling scopes on (hipEvents around each
scope's launches).  Reported per iteration: the sum of all scopes (device time), every scope, and the wall time of the
call.  The new scopes: ba_cameras + ba_cam_w (the camera blocks H_cam, g_cam, E_cam, W_cam), ba_schur_cam_eliminate (Wc,
Z, the partials of Z Wc^T and Z g, S_cam / rhs_cam) and ba_schur_cam_border (B).  The bytes the three new passes must move
are computed from the shapes.
--parent-lib: the constant-intrinsics leg on another build of the library (the parent commit's, built in a directory of its
own), alternated with this build's in the same call; no kernel on that path differs, so the two should agree within the
spread."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))

CAMS, POINTS = 1000, 1_000_000
LEGS = {"constant": None, "focal": (0, 1), "all8": tuple(range(8))}
NEW_SCOPES = ("ba_cameras", "ba_cam_w", "ba_schur_cam_eliminate", "ba_schur_cam_border")


def run_leg(leg, iters, warmup):
    """child: one leg, one JSON line"""
    import time

    import numpy as np

    import pcdhip
    from pcdhip import synth
    scene = synth.ba_scene(CAMS, POINTS, seed=11, order="image")
    refine = None
    if LEGS[leg] is not None:
        refine = np.zeros(len(scene["cam_params_list"][0]), np.uint8)
        refine[list(LEGS[leg])] = 1
    ba = pcdhip.BA(**scene, camera_refine=refine)
    kw = dict(linear_solver="cholesky")
    if refine is not None:
        kw["refine_intrinsics"] = True
    cams0 = np.concatenate([np.asarray(c, np.float64) for c in scene["cam_params_list"]])

    def reset():
        ba.set_parameters(scene["poses"], scene["points"])
        ba.set_camera_parameters(cams0)
    pcdhip.ba_solve(ba, max_num_iterations=warmup, **kw)
    reset()
    pcdhip.profile_reset()
    pcdhip.profile_enable(True)
    t0 = time.perf_counter()
    summary, hist = pcdhip.ba_solve(ba, max_num_iterations=iters, **kw)
    wall = (time.perf_counter() - t0) * 1e3
    scopes = pcdhip.profile_get()
    pcdhip.profile_enable(False)
    n = max(summary["num_iterations"], 1)
    out = dict(leg=leg, lib=pcdhip.LIB_PATH, iterations=summary["num_iterations"], accepted=summary["num_accepted"],
               I=ba.I, P=ba.P, O=ba.O, L=ba.L, wall_ms_per_iter=wall / n, total_ms_per_iter=summary["total_ms"] / n,
               initial_cost=summary["initial_cost"], final_cost=summary["final_cost"],
               scopes={k: [launches, ms / n] for k, (launches, ms) in scopes.items()})
    out["device_ms_per_iter"] = sum(v[1] for v in out["scopes"].values())
    if refine is not None:
        out["camera_parameters"] = ba.get_camera_parameters().tolist()
    print("PROBE " + json.dumps(out))


def child(leg, iters, warmup, lib=None):
    env = dict(os.environ)
    if lib:
        env["PCDHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--iters", str(iters), "--warmup", str(warmup)],
                       capture_output=True, text=True, env=env, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("PROBE "):
            return json.loads(line[6:])
    raise RuntimeError("leg %s failed (exit %d): %s %s" % (leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))


def new_pass_bytes(P, O, ncs):
    """bytes the three new passes must move per iteration, from the shapes (fp64; index arrays are int32 / uint32)"""
    npair = ncs * (ncs + 1) // 2
    # camera blocks: ba_cameras and ba_cam_w each read an observation (xy 16 B, point index 4 B, point 24 B) once;
    # W_cam [O][12][3] is written (H_cam, g_cam, E_cam are per camera / image: negligible)
    blocks = O * (2 * (16 + 4 + 24) + 288)
    # elimination: W_cam and the track list read per observation, V^-1 per point, Wc and Z [P][ncs][12][3] written; the
    # partials read 3 rows of Z (72 B) and Wc (288 B) per point, quarter and slot pair
    elim = O * (288 + 4) + P * 72 + 2 * 288 * P * ncs + 4 * (72 + 288) * P * npair
    # border: per observation, camera slot and half, 6 rows of Z (144 B, gathered), W (144 B) and the point index
    border = O * ncs * 2 * (144 + 144 + 4)
    return dict(camera_blocks=blocks, camera_elimination=elim, border=border)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_intrinsics_probe.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--parent-lib")
    a = ap.parse_args()
    if a.leg:
        return run_leg(a.leg, a.iters, a.warmup)
    assert a.iters >= 10, "time at least 10 iterations per leg"
    lines = []

    def log(s=""):
        print(s, flush=True)
        lines.append(s)
    runs = [("constant", None), ("focal", None), ("all8", None), ("constant", None), ("constant", None)]
    if a.parent_lib:
        runs += [("constant", a.parent_lib), ("constant", None), ("constant", a.parent_lib), ("constant", None)]
    res = []
    for leg, lib in runs:
        r = child(leg, a.iters, a.warmup, lib)
        r["parent"] = bool(lib)
        res.append(r)
        if len(res) == 1:
            log("BA workload M: %d images, %d points, %d observations, %d LiDAR terms, one shared OPENCV camera; pcd_ba_solve, "
                "direct solver, %d warm-up + %d timed iterations per leg, each leg in a process of its own"
                % (r["I"], r["P"], r["O"], r["L"], a.warmup, a.iters))
            log()
        log("%-9s %-7s device %9.3f ms / iteration   wall %9.3f   (%d iterations, %d accepted, cost %.6g -> %.6g)"
            % (leg, "parent" if lib else "this", r["device_ms_per_iter"], r["wall_ms_per_iter"], r["iterations"], r["accepted"],
               r["initial_cost"], r["final_cost"]))
    log()
    first = {leg: next(r for r in res if r["leg"] == leg and not r["parent"]) for leg in LEGS}
    names = sorted({k for r in first.values() for k in r["scopes"]})
    log("per-iteration device time by profiling scope (ms; launches of the whole solve in brackets)")
    log("%-26s %18s %18s %18s" % ("scope", "constant", "focal refined", "all 8 refined"))
    for k in names:
        cells = []
        for leg in ("constant", "focal", "all8"):
            v = first[leg]["scopes"].get(k)
            cells.append("%10.3f [%4d]" % (v[1], v[0]) if v else "%17s" % "-")
        log("%-26s %18s %18s %18s%s" % (k, cells[0], cells[1], cells[2], "   <- new" if k in NEW_SCOPES else ""))
    log("%-26s %18.3f %18.3f %18.3f" % ("sum", *[first[leg]["device_ms_per_iter"] for leg in ("constant", "focal", "all8")]))
    log()
    r = first["focal"]
    b = new_pass_bytes(r["P"], r["O"], 1)
    log("bytes the new passes must move per iteration (from the shapes, one camera slot): camera blocks %.2f GB, camera "
        "elimination %.2f GB, border %.2f GB" % (b["camera_blocks"] / 1e9, b["camera_elimination"] / 1e9, b["border"] / 1e9))
    for leg in ("focal", "all8"):
        sc = first[leg]["scopes"]
        t = dict(camera_blocks=sc.get("ba_cameras", [0, 0])[1] + sc.get("ba_cam_w", [0, 0])[1],
                 camera_elimination=sc.get("ba_schur_cam_eliminate", [0, 0])[1], border=sc.get("ba_schur_cam_border", [0, 0])[1])
        log("  %-6s " % leg + "   ".join("%s %.3f ms = %.0f GB/s" % (k, t[k], b[k] / 1e6 / max(t[k], 1e-9)) for k in t))
    log()
    mine = [x["device_ms_per_iter"] for x in res if x["leg"] == "constant" and not x["parent"]]
    log("constant-intrinsics leg, this build:   " + "  ".join("%.3f" % v for v in mine) +
        "   spread %.3f ms (%.2f %%)" % (max(mine) - min(mine), 100 * (max(mine) - min(mine)) / min(mine)))
    if a.parent_lib:
        par = [x["device_ms_per_iter"] for x in res if x["parent"]]
        log("constant-intrinsics leg, parent build: " + "  ".join("%.3f" % v for v in par) +
            "   spread %.3f ms" % (max(par) - min(par)))
        import statistics
        d = statistics.median(mine) - statistics.median(par)
        log("median this - median parent: %+.3f ms (%+.2f %%); the spread of the repeats is the yardstick: no kernel on the "
            "constant-intrinsics path differs between the two builds" % (d, 100 * d / statistics.median(par)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

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
spread.
The pcg_cam column: the same two refining legs with linear_solver="pcg_cam" (the bordered PCG, pcd_ba_schur_cam_solve_pcg*)
beside the Cholesky figures, by scope; ba_schur_pcg is the bordered PCG's scope.  Then one leg at config C's BA size (5000
images, 2 M points, all 8 parameters refined): the bordered PCG's time per LM iteration and per PCG iteration, the bytes a
PCG iteration must move (the row lists' S blocks, B once, the slot partials of the camera rows, the vectors) with the
bandwidth that time amounts to, and the dense route on the same scene: its time, or the status it failed with."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))

CAMS, POINTS = 1000, 1_000_000
SIZE_C = (5000, 2_000_000)      # config C's BA size
LEGS = {"constant": None, "focal": (0, 1), "all8": tuple(range(8)), "C_all8": tuple(range(8))}
NEW_SCOPES = ("ba_cameras", "ba_cam_w", "ba_schur_cam_eliminate", "ba_schur_cam_border")


def pcg_iteration_bytes(ns, npairs, ncs):
    """bytes one iteration of the bordered PCG must move (fp64): every block of the row lists once (a pair block sits in
    two rows), its partner's z and p (96 B), B once, the slot partials of the camera rows written and read, S_cam, and the
    vectors of the update (x, p, r, z, w, rhs: 9 streams of 6 ns + 12 ncs doubles) with the 6 x 6 and 12 x 12 inverses"""
    nrow, n = ns + 2 * npairs, 6 * ns + 12 * ncs
    return dict(S_blocks=nrow * (288 + 96 + 8), B=ns * ncs * 576, camera_partials=2 * ns * 12 * ncs * 8,
                S_cam=(12 * ncs) ** 2 * 8, vectors=9 * n * 8 + ns * 288 + ncs * 1152)


def fixed_iteration_times(ba, counts=(8, 40), reps=5):
    """the bordered PCG alone on the handle's current parameters, tolerances off: for each iteration limit the iterations
    it ran and the smallest wall time of `reps` calls (each ends with its read of the record), ms.  Marquardt at mu = 1
    (H + diag H): the bench scene's start is so far off (cost 1e33 and more) that at small mu its reduced system is not
    numerically positive definite -- the direct solve fails on it and the PCG breaks down in its first iteration -- and
    the time of an iteration does not depend on the values."""
    import time
    ba.schur_cam(1.0, want=("cost", "num_skipped"))
    out = []
    for c in counts:
        best, its = float("inf"), 0
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            _, info = ba.schur_cam_solve_pcg(max_iterations=c, q_tolerance=-1.0, r_tolerance=-1.0)
            best, its = min(best, (time.perf_counter() - t0) * 1e3), info["iterations"]
        out.append([its, best, info["termination"]])
    return out


def run_leg(leg, iters, warmup, solver):
    """child: one leg, one JSON line"""
    import time

    import numpy as np

    import pcdhip
    from pcdhip import synth
    scene = synth.ba_scene(*(SIZE_C if leg.startswith("C_") else (CAMS, POINTS)), seed=11, order="image")
    refine = None
    npairs = -1
    if solver == "pcg_cam":     # the structure queries are refused on a refined handle: ask the same problem unrefined
        plain = pcdhip.BA(**scene)
        npairs = int(plain.schur_structure()["pairs"].shape[0])
        plain.close()
    if LEGS[leg] is not None:
        refine = np.zeros(len(scene["cam_params_list"][0]), np.uint8)
        refine[list(LEGS[leg])] = 1
    ba = pcdhip.BA(**scene, camera_refine=refine)
    kw = dict(linear_solver=solver)
    if refine is not None:
        kw["refine_intrinsics"] = True
    cams0 = np.concatenate([np.asarray(c, np.float64) for c in scene["cam_params_list"]])

    def reset():
        ba.set_parameters(scene["poses"], scene["points"])
        ba.set_camera_parameters(cams0)
    try:
        pcdhip.ba_solve(ba, max_num_iterations=warmup, **kw)
    except pcdhip.PcdError as e:       # reported, not worked round (the dense scratch of the direct route may not fit)
        print("PROBE " + json.dumps(dict(leg=leg, solver=solver, lib=pcdhip.LIB_PATH, I=ba.I, P=ba.P, O=ba.O, L=ba.L,
                                         failed=dict(status=int(e.status), message=str(e)))))
        return
    reset()
    pcdhip.profile_reset()
    pcdhip.profile_enable(True)
    t0 = time.perf_counter()
    summary, hist = pcdhip.ba_solve(ba, max_num_iterations=iters, **kw)
    wall = (time.perf_counter() - t0) * 1e3
    scopes = pcdhip.profile_get()
    pcdhip.profile_enable(False)
    n = max(summary["num_iterations"], 1)
    out = dict(leg=leg, solver=solver, npairs=npairs, ns=ba._cam_dims()[0], lib=pcdhip.LIB_PATH,
               linear_iterations=sum(h["linear_iterations"] for h in hist), linear_ms=summary["linear_solver_ms"], iterations=summary["num_iterations"], accepted=summary["num_accepted"],
               I=ba.I, P=ba.P, O=ba.O, L=ba.L, wall_ms_per_iter=wall / n, total_ms_per_iter=summary["total_ms"] / n,
               initial_cost=summary["initial_cost"], final_cost=summary["final_cost"],
               scopes={k: [launches, ms / n] for k, (launches, ms) in scopes.items()})
    if solver == "pcg_cam":      # the LM loop times its PCG with an event pair of its own, not with a scope
        out["scopes"]["linear solve (event pair)"] = [n, summary["linear_solver_ms"] / n]
        out["fixed"] = fixed_iteration_times(ba)
    out["device_ms_per_iter"] = sum(v[1] for v in out["scopes"].values())
    if refine is not None:
        out["camera_parameters"] = ba.get_camera_parameters().tolist()
    print("PROBE " + json.dumps(out))


def child(leg, iters, warmup, lib=None, solver="cholesky"):
    env = dict(os.environ)
    if lib:
        env["PCDHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--iters", str(iters), "--warmup", str(warmup),
                        "--solver", solver], capture_output=True, text=True, env=env, timeout=900)
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
    ap.add_argument("--solver", default="cholesky", choices=("cholesky", "pcg_cam"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--iters-c", type=int, default=3, help="timed iterations of the 5000-image legs")
    a = ap.parse_args()
    if a.leg:
        return run_leg(a.leg, a.iters, a.warmup, a.solver)
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
    first = {leg: next(r for r in res if r["leg"] == leg and not r["parent"]) for leg in ("constant", "focal", "all8")}
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
    log()
    pcg = {leg: child(leg, a.iters, a.warmup, solver="pcg_cam") for leg in ("focal", "all8")}
    names = sorted({k for leg in pcg for r in (first[leg], pcg[leg]) for k in r["scopes"]})
    log("one refining LM iteration at workload M, bordered Cholesky against the bordered PCG (pcg_cam, default PCG options), "
        "per-iteration device time by scope (ms)")
    log("%-26s %14s %14s %14s %14s" % ("scope", "focal chol", "focal pcg_cam", "all8 chol", "all8 pcg_cam"))
    for k in names:
        cells = ["%14.3f" % r["scopes"][k][1] if k in r["scopes"] else "%14s" % "-"
                 for r in (first["focal"], pcg["focal"], first["all8"], pcg["all8"])]
        log("%-26s %s" % (k, " ".join(cells)))
    log("%-26s %14.3f %14.3f %14.3f %14.3f" % ("sum", first["focal"]["device_ms_per_iter"], pcg["focal"]["device_ms_per_iter"],
                                             first["all8"]["device_ms_per_iter"], pcg["all8"]["device_ms_per_iter"]))
    for leg in ("focal", "all8"):
        r = pcg[leg]
        log("  %-5s pcg_cam: %d LM iterations (%d accepted, cost %.6g -> %.6g), %d PCG iterations in all, linear solve %.3f ms "
            "per LM iteration, wall %.3f ms per LM iteration" % (leg, r["iterations"], r["accepted"], r["initial_cost"],
                                                                 r["final_cost"], r["linear_iterations"],
                                                                 r["linear_ms"] / max(r["iterations"], 1), r["wall_ms_per_iter"]))
    log()
    log("config C's BA size, all 8 parameters refined, one camera slot, 1 warm-up + %d timed iterations" % a.iters_c)
    for solver in ("pcg_cam", "cholesky"):
        r = child("C_all8", a.iters_c, 1, solver=solver)
        if "failed" in r:
            log("  %-8s %d images, %d points, %d observations: failed with status %d (%s)"
                % (solver, r["I"], r["P"], r["O"], r["failed"]["status"], r["failed"]["message"]))
            continue
        n = max(r["iterations"], 1)
        log("  %-8s %d images, %d points, %d observations: device %.3f ms / LM iteration, wall %.3f, linear solve %.3f ms / LM "
            "iteration (%d iterations, %d accepted, cost %.6g -> %.6g)"
            % (solver, r["I"], r["P"], r["O"], r["device_ms_per_iter"], r["wall_ms_per_iter"], r["linear_ms"] / n,
               r["iterations"], r["accepted"], r["initial_cost"], r["final_cost"]))
        log("           by scope: " + "  ".join("%s %.3f" % (k, v[1]) for k, v in sorted(r["scopes"].items())))
        if solver == "pcg_cam":
            b = pcg_iteration_bytes(r["ns"], r["npairs"], 1)
            tot = sum(b.values())
            (ia, ta, _), (ib, tb, term) = r["fixed"]
            per = (tb - ta) / max(ib - ia, 1)
            log("           %d pose slots, %d pairs; the LM loop ran %d PCG iterations in all (%.3f ms of linear solve per LM "
                "iteration with set-up and the flag read)" % (r["ns"], r["npairs"], r["linear_iterations"], r["linear_ms"] / n))
            log("           the PCG alone, tolerances off: %d iterations %.3f ms, %d iterations %.3f ms (termination %d): %.1f us "
                "per PCG iteration" % (ia, ta, ib, tb, term, 1e3 * per))
            log("           bytes a PCG iteration must move: " + ", ".join("%s %.2f MB" % (k, v / 1e6) for k, v in b.items()) +
                "; total %.2f MB = %.0f GB/s at that time (bytes actually moved: not measured, no counter run)"
                % (tot / 1e6, tot / 1e6 / max(per, 1e-9)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

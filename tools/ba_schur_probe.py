"""Timing of the device point elimination (pcd_ba_schur*) part by part, at workload M (bench.py's BA scene,
1000 images / 1 M points / 4.72 M observations) and at config B's size (450 images / 400 k points / 1.87 M observations).

  python tools/ba_schur_probe.py [--out profiles/ba_solve_probe.txt] [--reps 15] [--only M|B]

Parts: structure build (on the device, once per handle and after every edit of the observations), normal-equation pass, elimination, dense fill,
torch.linalg.cholesky + solve, back-substitution + plus, cost pass, a whole LM iteration of pcdhip.ba_solve_lm; then
the block-sparse PCG beside the Cholesky (at the defaults and to r_tolerance 1e-10, each call with its one read of the
record), the time per CG iteration, and a whole LM iteration through pcd_ba_solve; then the library's own blocked
Cholesky (fill + factor + solve, from the handle's blocks and from the same dense S torch factors) beside torch's in
the same run, and a whole LM iteration through pcd_ba_solve with that solver.
Device parts are timed with the library's per-scope hipEvents (pcdhip.profile_*), host-driven parts with
torch.cuda.Event pairs; warm-up first, then the median (and min / max) of --reps runs."""
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

SCENES = {"M": (1000, 1_000_000), "B": (450, 400_000)}


def stats(v):
    v = np.asarray(v)
    return "median %8.3f ms   min %8.3f   max %8.3f   (n=%d)" % (np.median(v), v.min(), v.max(), v.size)


def scoped(ba, fn, scope, reps):
    """library scope timings (hipEvents around the scope's launches) of `reps` calls of fn after one warm-up"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        pcdhip.profile_reset()
        pcdhip.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        t = pcdhip.profile_get()
        pcdhip.profile_enable(False)
        out.append(sum(ms for name, (_, ms) in t.items() if name == scope))
    return out


def evented(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def probe(tag, reps, log):
    cams, pts = SCENES[tag]
    scene = synth.ba_scene(cams, pts, seed=11, order="image")
    ba = pcdhip.BA(**scene)
    log("== %s: %d images, %d points, %d observations, %d LiDAR terms" % (tag, ba.I, ba.P, ba.O, ba.L))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    built = ba.schur_build()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    st = ba.schur_structure()
    info = ba.schur_stats()
    ns, npair = st["num_slots"], len(st["pairs"])
    log("structure build (device, once per handle): %.1f ms (library) / %.1f ms (call, device idle before and after); "
        "%d stream synchronisations; %d slots, %d pairs, %d entries"
        % (built["build_ms"], wall, built["num_syncs"], ns, npair, info["num_entries"]))
    rebuilds = []
    for _ in range(5):              # again, as after an edit: a no-op removal drops the structure, the scratch stays
        ba.remove_observations(torch.zeros(ba.O, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = ba.schur_build()
        torch.cuda.synchronize()
        rebuilds.append((time.perf_counter() - t0) * 1e3)
        assert again["num_syncs"] <= 2 and again["num_entries"] == built["num_entries"]
    log("structure rebuild on the live handle (scratch kept):  %s" % stats(rebuilds))
    mu = 1e-4
    ba.schur(mu, dense=True)     # allocates the scratch
    torch.cuda.synchronize()
    log("device memory held by the elimination: %.1f MB (dense S %.1f MB, caller-owned)"
        % (ba.schur_stats()["scratch_bytes"] / 1e6, 36.0 * ns * ns * 8 / 1e6))
    r = {}
    r["normal-equation pass"] = scoped(ba, lambda: ba.schur(mu), "ba_schur_normal", reps)
    r["elimination"] = scoped(ba, lambda: ba.schur(mu), "ba_schur_eliminate", reps)
    r["dense fill"] = scoped(ba, lambda: ba.schur(mu, dense=True), "ba_schur_dense", reps)
    out = ba.schur(mu, dense=True)
    S, rhs = out["S"], out["rhs"].reshape(-1, 1)

    torch_info = {}

    def chol():
        L, info_ = torch.linalg.cholesky_ex(S)
        torch_info["S"] = info_          # read after the timing: 0 = factored, k > 0 = the leading minor k is not PD
        return torch.cholesky_solve(rhs, L)
    r["cholesky + solve (torch)"] = evented(chol, reps)
    dpose = chol().reshape(-1, 6)
    dpoint = torch.empty((ba.P, 3), dtype=torch.float64, device="cuda")
    md = torch.empty(1, dtype=torch.float64, device="cuda")
    cp = torch.empty((ba.I, 7), dtype=torch.float64, device="cuda")
    cx = torch.empty((ba.P, 3), dtype=torch.float64, device="cuda")

    def back_plus():
        ba.back_substitute(dpose, dpoint)
        ba.plus(dpose, dpoint, cp, cx)
    r["back-substitution + plus"] = evented(back_plus, reps)
    cost = torch.empty(1, dtype=torch.float64, device="cuda")
    r["cost pass"] = evented(lambda: ba.cost_device(cost), reps)
    keep = scene["poses"].copy(), scene["points"].copy()

    def lm_iter():
        ba.set_parameters(*keep)          # every run starts from the same parameters (a host upload, not timed below)
        torch.cuda.synchronize()
        t = time.perf_counter()
        pcdhip.ba_solve_lm(ba, max_iterations=1)
        return (time.perf_counter() - t) * 1e3
    lm_iter()
    r["whole LM iteration (wall, incl. host syncs)"] = [lm_iter() for _ in range(reps)]
    # the reduced solve on the block-sparse system, same S (mu 1e-4, blocks left in the handle)
    ba.set_parameters(*keep)
    ba.schur(mu, want=("cost", "num_skipped"))
    xbuf = torch.empty((ns, 6), dtype=torch.float64, device="cuda")
    its = {}

    def pcg_default():
        its["default"] = ba.schur_solve_pcg(dpose=xbuf)[1]

    def pcg_tight():
        its["tight"] = ba.schur_solve_pcg(dpose=xbuf, r_tolerance=1e-10, q_tolerance=-1.0, max_iterations=2000)[1]
    r["PCG at the defaults"] = evented(pcg_default, reps)
    r["PCG to r_tolerance 1e-10"] = evented(pcg_tight, reps)

    def solve_iter():
        ba.set_parameters(*keep)
        torch.cuda.synchronize()
        t = time.perf_counter()
        pcdhip.ba_solve(ba, max_num_iterations=1)
        return (time.perf_counter() - t) * 1e3
    solve_iter()
    r["whole LM iteration, pcd_ba_solve (wall)"] = [solve_iter() for _ in range(reps)]
    # the library's direct solve: the same S as torch's leg above, then the handle's own blocks
    ba.set_parameters(*keep)
    ba.schur(mu, want=("cost", "num_skipped"))
    chol_info = {}

    def chol_hip_dense():
        chol_info["dense"] = ba.schur_solve_cholesky(S, rhs, dpose=xbuf)[1]

    def chol_hip_blocks():
        chol_info["blocks"] = ba.schur_solve_cholesky(dpose=xbuf)[1]
    r["cholesky + solve (library, caller's dense S)"] = evented(chol_hip_dense, reps)
    r["cholesky + solve (library, handle's blocks)"] = evented(chol_hip_blocks, reps)
    r["  of which on the device (scope)"] = scoped(ba, chol_hip_blocks, "ba_schur_cholesky", reps)
    r["cholesky + solve (torch), again"] = evented(chol, reps)
    x_hip = xbuf.reshape(-1, 1).clone()
    res = lambda x: float((S @ x - rhs).abs().max() / (S.abs().sum(1).max() * x.abs().max() + rhs.abs().max()))
    eta_hip, eta_torch = res(x_hip), res(chol())

    def solve_iter_chol():
        ba.set_parameters(*keep)
        torch.cuda.synchronize()
        t = time.perf_counter()
        pcdhip.ba_solve(ba, max_num_iterations=1, linear_solver="cholesky")
        return (time.perf_counter() - t) * 1e3
    solve_iter_chol()
    r["whole LM iteration, pcd_ba_solve cholesky"] = [solve_iter_chol() for _ in range(reps)]
    for k, v in r.items():
        log("  %-44s %s" % (k, stats(v)))
    nd, nt = its["default"]["iterations"], its["tight"]["iterations"]
    td, tt = np.median(r["PCG at the defaults"]), np.median(r["PCG to r_tolerance 1e-10"])
    log("  PCG iterations: %d at the defaults (relative residual %.3f), %d to 1e-10; %.1f us per CG iteration "
        "((tight - default) / (iterations apart)), %.1f us with the set-up shared out (tight / iterations); "
        "three launch boundaries are ~5 us"
        % (nd, its["default"]["residual_norm"] / its["default"]["rhs_norm"], nt,
           1e3 * (tt - td) / max(nt - nd, 1), 1e3 * tt / max(nt, 1)))
    lo, hi = np.min(r["whole LM iteration (wall, incl. host syncs)"]), np.max(r["whole LM iteration (wall, incl. host syncs)"])
    log("  whole LM iteration: dense Cholesky route %.3f ms (spread %.3f), pcd_ba_solve %.3f ms"
        % (np.median(r["whole LM iteration (wall, incl. host syncs)"]), hi - lo,
           np.median(r["whole LM iteration, pcd_ba_solve (wall)"])))
    tl, tb = np.median(r["cholesky + solve (library, caller's dense S)"]), np.median(r["cholesky + solve (library, handle's blocks)"])
    tt2 = min(np.median(r["cholesky + solve (torch)"]), np.median(r["cholesky + solve (torch), again"]))
    ci = chol_info["dense"]
    t_info = int(torch_info["S"].item())
    both_ok = ci["status"] == pcdhip.CHOL_OK and chol_info["blocks"]["status"] == pcdhip.CHOL_OK and t_info == 0
    log("  direct solve of the scene's S at mu %g, n = %d (%d panels of 96): library status %d failed_column %d pivots "
        "%.6g .. %.6g; torch cholesky_ex info %d" % (mu, ci["n"], ci["panels"], ci["status"], ci["failed_column"],
                                                    ci["min_pivot"], ci["max_pivot"], t_info))
    if both_ok:
        log("  library %.3f ms from the dense S, %.3f ms from the blocks; torch %.3f ms (the faster of its two legs): "
            "library / torch = %.2f (%s); backward error eta library %.2e, torch %.2e"
            % (tl, tb, tt2, tl / tt2, "the library wins" if tl < tt2 else "the library LOSES", eta_hip, eta_torch))
    else:
        log("  NO VERDICT on this system: a factorisation failed (S is not numerically positive definite for it), so the "
            "times above are times to the failure (library) or of a factor that was not completed (torch), not of a solve")
    lc = np.median(r["whole LM iteration, pcd_ba_solve cholesky"])
    ld = np.median(r["whole LM iteration (wall, incl. host syncs)"])
    _, it_hip = pcdhip.ba_solve(ba, max_num_iterations=1, linear_solver="cholesky")
    ba.set_parameters(*keep)
    it_lm = pcdhip.ba_solve_lm(ba, max_iterations=1)
    ba.set_parameters(*keep)
    step_ok = it_hip[0]["linear_termination"] == pcdhip.CHOL_OK and np.isfinite(it_lm[0]["candidate_cost"])
    log("  whole LM iteration: pcd_ba_solve cholesky %.3f ms (linear_termination %d), ba_solve_lm (torch) %.3f ms "
        "(step %s); pcd_ba_solve PCG %.3f ms"
        % (lc, it_hip[0]["linear_termination"], ld, "taken" if np.isfinite(it_lm[0]["candidate_cost"]) else
           "not taken: its factorisation failed", np.median(r["whole LM iteration, pcd_ba_solve (wall)"])))
    if step_ok:
        log("  ratio %.2f (%s)" % (lc / ld, "under ba_solve_lm" if lc < ld else "NOT under ba_solve_lm"))
    else:
        log("  NO VERDICT on the LM iteration: a factorisation failed, the iterations timed are rejected steps")
    # a system of the same size that both solvers factor: G G^T + n I from a seeded G (what tests/test_ba_chol_gpu.py
    # solves at n = 2700), the caller's-dense-S form
    n = 6 * ns
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7000 + ns)
    G = torch.randn((n, n), dtype=torch.float64, device="cuda", generator=gen)
    Sp = G @ G.T + n * torch.eye(n, dtype=torch.float64, device="cuda")
    Sp = 0.5 * (Sp + Sp.T)
    bp = Sp @ torch.randn((n, 1), dtype=torch.float64, device="cuda", generator=gen)
    del G
    spd = {}

    def chol_spd_torch():
        L, info_ = torch.linalg.cholesky_ex(Sp)
        spd["torch"] = info_
        return torch.cholesky_solve(bp, L)

    def chol_spd_hip():
        spd["hip"] = ba.schur_solve_cholesky(Sp, bp, dpose=xbuf)[1]
    ts = evented(chol_spd_torch, reps)
    th = evented(chol_spd_hip, reps)
    ts2 = evented(chol_spd_torch, reps)
    resp = lambda x: float((Sp @ x - bp).abs().max() / (Sp.abs().sum(1).max() * x.abs().max() + bp.abs().max()))
    e_h, e_t = resp(xbuf.reshape(-1, 1)), resp(chol_spd_torch())
    log("  SPD system G G^T + n I, n = %d:" % n)
    log("  %-44s %s" % ("cholesky + solve (torch)", stats(ts)))
    log("  %-44s %s" % ("cholesky + solve (library, caller's dense S)", stats(th)))
    log("  %-44s %s" % ("cholesky + solve (torch), again", stats(ts2)))
    hi_ = spd["hip"]
    log("  library status %d failed_column %d pivots %.6g .. %.6g; torch cholesky_ex info %d"
        % (hi_["status"], hi_["failed_column"], hi_["min_pivot"], hi_["max_pivot"], int(spd["torch"].item())))
    if hi_["status"] == pcdhip.CHOL_OK and int(spd["torch"].item()) == 0:
        tt3 = min(np.median(ts), np.median(ts2))
        log("  library %.3f ms, torch %.3f ms (the faster of its two legs): library / torch = %.2f (%s); backward error "
            "eta library %.2e, torch %.2e" % (np.median(th), tt3, np.median(th) / tt3,
                                              "the library wins" if np.median(th) < tt3 else "the library LOSES", e_h, e_t))
    else:
        log("  NO VERDICT: a factorisation failed")
    ba.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=sorted(SCENES), default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log("# tools/ba_schur_probe.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for tag in ([a.only] if a.only else ["M", "B"]):
        probe(tag, a.reps, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

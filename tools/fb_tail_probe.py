"""How many walks k_nn_fallback keeps in flight: the wavefronts' lives over the kernel's span.

    python tools/fb_tail_probe.py [--dump FILE.npz]     on the GPU: workload M, its N = 8 share and config A
    python tools/fb_tail_probe.py --load FILE.npz         no GPU: the figures from a dump

A pass with set_nn_tuning(collect_stats=16) makes every wavefront of k_nn_fallback write {start, end, walk
steps} (wall-clock ticks of 10 ns) into a buffer reserved for such passes only.  For workload M (bench.py: 10 M points,
1 M queries) and the queries [0, Q / 8) of it (tools/scaling_probe.py's split) the probe prints

  live wavefronts per CU     sum of the wavefronts' durations / (span * 256 CUs): the mean number of walks a CU has in
                             flight between the first start and the last end (the registers allow 32), and the same
                             over the middle half of the span, where neither the fill nor the tail counts
  finished share             per workgroup, the part of (wavefronts x workgroup's life) during which a wavefront of it
                             has ended while the workgroup -- and with it its LDS -- is still there; mean over workgroups
  (last end - mean end) / span   the share of the kernel during which, on average, a wavefront slot has nothing left
  duration against steps     least-squares line and correlation over the wavefronts, and the ticks per step in the
                             first and the last quarter of the starts (does a step cost the same early and late?)

and beside them a hash of the call's keys (the same for every build of the library) and the nn_fallback profile scope with statistics off (mean of 30 calls after 5, twice) for M, M_8 and
config A's one-launch call (2 M points, 20 k queries, PCD_NN_AUTO).  A library without the records (an older tree
loaded through PCDHIP_LIB) gives the timings alone.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))

TICK_US = 0.01   # wall_clock64: 100 MHz
CUS = 256


def report(name, rec, wpb, out=sys.stdout):
    rec = rec.astype(np.int64)
    rec = rec[: len(rec) // wpb * wpb]
    t0 = rec[:, 0].min()
    start, end, steps = (rec[:, 0] - t0) * TICK_US, (rec[:, 1] - t0) * TICK_US, rec[:, 2]
    dur = end - start
    span = end.max()
    work = steps > 0
    live = dur.sum() / (span * CUS)
    # live wavefronts over the middle half of the span: the overlap of every wavefront's life with [span/4, 3 span/4]
    a, b = 0.25 * span, 0.75 * span
    mid = np.clip(np.minimum(end, b) - np.maximum(start, a), 0, None).sum() / ((b - a) * CUS)
    print("%s: %d wavefronts in workgroups of %d, %d with a walk, %d steps" % (name, len(rec), wpb, work.sum(), steps.sum()), file=out)
    print("  span %.2f us; live wavefronts per CU %.1f over the span, %.1f over its middle half (32 fit the registers)" % (
        span, live, mid), file=out)
    if wpb > 1:
        s, e = start.reshape(-1, wpb), end.reshape(-1, wpb)
        life = e.max(1) - s.min(1)
        ok = life > 0
        fin = ((e.max(1)[:, None] - e).sum(1)[ok] / (wpb * life[ok]))
        print("  finished share of a workgroup's life: mean %.1f %%, weighted by life %.1f %%" % (
            100 * fin.mean(), 100 * (fin * life[ok]).sum() / life[ok].sum()), file=out)
    else:
        print("  finished share of a workgroup's life: 0 (one wavefront per workgroup)", file=out)
    print("  mean end %.2f us, last end %.2f us: (last - mean) / span %.1f %%" % (end[work].mean(), span, 100 * (span - end[work].mean()) / span), file=out)
    x, y = steps[work].astype(np.float64), dur[work]
    k, c = np.polyfit(x, y, 1)
    print("  duration = %.3f us * steps + %.2f us, correlation %.2f; mean %.2f us, max %.2f us (%d steps)" % (
        k, c, np.corrcoef(x, y)[0, 1], y.mean(), y.max(), x[y.argmax()]), file=out)
    order = np.argsort(start[work])
    q = len(order) // 4
    early, late = order[:q], order[-q:]
    print("  us per step: first quarter of the starts %.3f, last quarter %.3f" % (
        y[early].sum() / x[early].sum(), y[late].sum() / x[late].sum()), file=out)
    out.flush()
    return dict(span=span, live=live, live_mid=mid)


def timed(fn, scope="nn_fallback"):
    import torch
    import pcdhip
    res = []
    for _ in range(5):
        fn()
    for _ in range(2):
        pcdhip.profile_enable(True); pcdhip.profile_only(scope); pcdhip.profile_reset()
        for _ in range(30):
            fn()
        torch.cuda.synchronize()
        n, ms = pcdhip.profile_get()[scope]
        pcdhip.profile_enable(False); pcdhip.profile_only(None)
        res.append(ms / n)
    return np.array(res)


def measure(dump):
    import torch
    import pcdhip
    from pcdhip import synth, dist as pd
    has_rec = hasattr(pcdhip.lib(), "pcd_nn_last_fb_wave_records")
    dump["has_rec"] = np.array([int(has_rec)])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    xyz, nrm = synth.cloud_planes(10_000_000)
    q_all = synth.queries(xyz, 1_000_000, seed=99)
    cloud = pcdhip.Cloud(xyz, nrm, raw_lidar_frame=False)
    for name, N in (("M", 1), ("M_8", 8)):
        lo, hi = pd.shard_range(1_000_000, 0, N)
        Q = hi - lo
        dq = torch.from_numpy(np.ascontiguousarray(q_all[lo:hi])).to(dev)
        keys = torch.empty(Q, dtype=torch.int64, device=dev)
        pcdhip.set_nn_tuning(collect_stats=0)
        dump["%s_ms" % name] = timed(lambda: cloud.nn_device(dq, Q, keys, pcdhip.NN_AUTO, stream))
        # the records alone (bit 16 without bit 1): the counters' atomics of a statistics pass would keep every
        # workgroup alive for microseconds after its walks
        pcdhip.set_nn_tuning(collect_stats=16)
        for rep in range(3 if has_rec else 0):   # three passes: the figure's own spread
            cloud.nn_device(dq, Q, keys, pcdhip.NN_AUTO, stream)
            rec, wpb = cloud.last_fb_wave_records()
            dump["%s_rep%d" % (name, rep)] = rec
            dump["wpb"] = np.array([wpb])
        pcdhip.set_nn_tuning(collect_stats=1)
        cloud.nn_device(dq, Q, keys, pcdhip.NN_AUTO, stream)
        dump["%s_fallback_queries" % name] = np.array([cloud.last_stats()["fallback_queries"]])
        dump["%s_keys" % name] = np.array([hashlib.sha256(keys.cpu().numpy().tobytes()).hexdigest()[:16]])
        pcdhip.set_nn_tuning(collect_stats=0)
    cloud.close()
    xa, na = synth.cloud_planes(2_000_000)
    ca = pcdhip.Cloud(xa, na, raw_lidar_frame=False)
    qa = torch.from_numpy(synth.queries(xa, 20_000, seed=3)).to(dev)
    ka = torch.empty(20_000, dtype=torch.int64, device=dev)
    dump["A_ms"] = timed(lambda: ca.nn_device(qa, 20_000, ka, pcdhip.NN_AUTO, stream))
    ca.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dump", help="write the records to this .npz")
    ap.add_argument("--load", help="read the records from this .npz instead of measuring")
    a = ap.parse_args()
    if a.load:
        d = dict(np.load(a.load))
    else:
        d = {}
        measure(d)
        if a.dump:
            np.savez_compressed(a.dump, **d)
    for name in ("M", "M_8", "A"):
        extra = "" if name == "A" else "; fallback_queries of a statistics pass %d, sha256 of the keys %s" % (
            d["%s_fallback_queries" % name][0], d["%s_keys" % name][0])
        print("workload %s: nn_fallback %s ms (profile scope, statistics off, mean of 30, twice)%s" % (
            name, " ".join("%.4f" % v for v in d["%s_ms" % name]), extra))
        if name != "A" and d["has_rec"][0]:
            for rep in range(3):
                report("workload %s, records pass %d" % (name, rep), d["%s_rep%d" % (name, rep)], int(d["wpb"][0]))


if __name__ == "__main__":
    main()

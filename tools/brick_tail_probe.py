"""How long the wavefronts of k_nn_brick_clip run: the tail of the kernel under the static and the hybrid schedule.

    python tools/brick_tail_probe.py [--dump FILE.npz] [--no-fit]     on the GPU: workload M and its N = 8 share
    python tools/brick_tail_probe.py --load FILE.npz                    no GPU: the figures and the fit from a dump

A statistics pass with set_nn_tuning(collect_stats=5) makes every wavefront of the brick kernel write {start, end,
items} (wall-clock ticks of 10 ns) into a buffer reserved for such passes only.  For workload M (bench.py: 10 M points,
1 M queries) and the queries [0, Q / 8) of it (tools/scaling_probe.py's split), under both schedules
(pcdhip.set_nn_schedule), it prints per block class and overall: the span of the kernel (first start to last end), the
mean and the last wavefront end, and (last end - mean end) / span -- the share of the kernel during which, on average,
a wavefront slot has nothing left to do.

The static schedule tells which items a wavefront had (brick_clip_kernel.h: class c walks its eighth of the item list,
wavefront w of the class takes items w, w + S, ...), so the probe also fits
    duration of a wavefront ~ a * items + b * tiles + c * compare slots
by least squares over the wavefronts of the static pass, with the tiles and slots of every item from the model of
tools/brick_clip_sim.py (rule `class`).  The model orders the queries of a brick by query id, the library in atomic
order: the items are the same bricks with the same counts, their tiles may differ by a query's ball here and there.
tools/brick_schedule_sim.py prices schedules on the fitted cost.

What the first run showed (profiles/brick_schedule_probe.txt): under the static schedule the wavefronts' durations fall
into four plateaus by the quarter of the grid their workgroup belongs to -- the order in which a CU received its four
workgroups -- and the item costs explain little of them (the fit's residual is a fifth of the mean).  The report
therefore also prints the mean duration per quarter.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TICK_US = 0.01   # wall_clock64: 100 MHz


def classes_of(nwaves):
    """block class of every wavefront (0 for all when the grid is no multiple of 8: the one-class path)"""
    blocks = nwaves // 4
    b = np.arange(nwaves) // 4
    return (b & 7) if blocks % 8 == 0 else np.zeros(nwaves, np.int64)


def static_items(nwaves, nitems):
    """item lists of the static schedule: one index array per wavefront"""
    blocks = nwaves // 4
    w = np.arange(nwaves)
    out = []
    if blocks % 8 == 0:
        per, stride = (nitems + 7) // 8, (blocks // 8) * 4
        for i in w:
            cls, slot = (i // 4) & 7, ((i // 4) >> 3) * 4 + (i & 3)
            out.append(np.arange(min(nitems, cls * per) + slot, min(nitems, (cls + 1) * per), stride))
    else:
        for i in w:
            out.append(np.arange(i, nitems, nwaves))
    return out


def tail_report(name, rec, out=sys.stdout):
    rec = rec.astype(np.int64)
    t0 = rec[:, 0].min()
    start, end, items = (rec[:, 0] - t0) * TICK_US, (rec[:, 1] - t0) * TICK_US, rec[:, 2]
    cls = classes_of(len(rec))
    print("%s: %d wavefronts, %d items" % (name, len(rec), items.sum()), file=out)
    res = None
    for c in list(range(cls.max() + 1)) + [-1]:
        m = (cls == c) if c >= 0 else np.ones(len(rec), bool)
        work = m & (items > 0)
        if not work.any():
            continue
        span = end[m].max() - start[m].min()
        mean_end, last = end[work].mean() - start[m].min(), end[m].max() - start[m].min()
        tail = (last - mean_end) / span
        print("  %-8s waves %4d  items/wave %5.1f [%d, %d]  first start %7.2f us  span %7.2f us  mean end %7.2f  last end %7.2f  "
              "(last - mean) / span %5.2f %%" % ("class %d" % c if c >= 0 else "overall", work.sum(), items[work].mean(),
                                                  items[work].min(), items[work].max(), start[m].min(), span, mean_end, last,
                                                  100 * tail), file=out)
        res = dict(span=span, tail=tail)
    # the k-th workgroup a CU received (launch order: the grid's quarters when it fills the chip's 4 slots per CU once)
    if len(rec) % 16 == 0 and (items > 0).all():
        dur = (end - start).reshape(4, -1)
        print("  wavefront duration by quarter of the grid (launch order): mean %s us, items/wave %s" % (
            " / ".join("%.1f" % v for v in dur.mean(1)), " / ".join("%.1f" % v for v in items.reshape(4, -1).mean(1))), file=out)
    out.flush()
    return res


def item_costs(points, queries, lo=0, hi=None):
    """(count, tiles, slots) of every item of the model (rule `class`), in item order"""
    import brick_clip_sim as sim
    from pcdhip import synth
    xyz, _ = synth.cloud_planes(points)
    q = synth.queries(xyz, queries, seed=99)[lo:hi]
    m = sim.Model(xyz)
    ib3, ifirst, icnt, qs, _ = m.items(q)
    n = len(ib3)
    tiles, slots = np.zeros(n), np.zeros(n)
    for s in range(0, n, 8192):
        tab = m.tables(ib3[s:s + 8192])
        for j in range(len(tab)):
            i = s + j
            _, tslots, aslots = sim.simulate_item(m, "class", ib3[i], tab[j], qs[ifirst[i]:ifirst[i] + icnt[i]])
            tiles[i] = tslots / (sim.TILE * icnt[i])
            slots[i] = tslots + aslots
    return icnt.astype(np.float64), tiles, slots


def fit(rec, costs, out=sys.stdout):
    cnt, tiles, slots = costs
    nitems = int(rec[:, 2].sum())
    if nitems != len(cnt):
        print("  fit: the model has %d items, the library %d: no fit" % (len(cnt), nitems), file=out)
        return None
    lists = static_items(len(rec), nitems)
    dur = (rec[:, 1].astype(np.int64) - rec[:, 0].astype(np.int64)) * TICK_US
    ok = np.array([len(l) > 0 for l in lists])
    assert all(len(l) == int(k) for l, k in zip(lists, rec[:, 2])), "the records do not follow the static schedule"
    A = np.array([[len(l), tiles[l].sum(), slots[l].sum()] for l in lists], np.float64)[ok]
    x, *_ = np.linalg.lstsq(A, dur[ok], rcond=None)
    r = dur[ok] - A @ x
    tot = A.sum(0) * x
    print("  fit over %d wavefronts: duration = %.4f us * items + %.4f us * tiles + %.4f ns * slots;  rms residual %.2f us of mean %.1f us;"
          "  shares of the summed durations: items %.0f %%, tiles %.0f %%, slots %.0f %%" % (
              ok.sum(), x[0], x[1], 1e3 * x[2], np.sqrt((r * r).mean()), dur[ok].mean(),
              100 * tot[0] / tot.sum(), 100 * tot[1] / tot.sum(), 100 * tot[2] / tot.sum()), file=out)
    out.flush()
    return x


def measure(dump):
    import torch
    import pcdhip
    from pcdhip import synth, dist as pd
    xyz, nrm = synth.cloud_planes(10_000_000)
    q_all = synth.queries(xyz, 1_000_000, seed=99)
    cloud = pcdhip.Cloud(xyz, nrm, raw_lidar_frame=False)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for name, N in (("M", 1), ("M_8", 8)):
        lo, hi = pd.shard_range(1_000_000, 0, N)
        Q = hi - lo
        dq = torch.from_numpy(np.ascontiguousarray(q_all[lo:hi])).to(dev)
        keys = torch.empty(Q, dtype=torch.int64, device=dev)
        for sched in (1, 0):
            pcdhip.set_nn_schedule(sched)
            pcdhip.set_nn_tuning(collect_stats=0)
            for _ in range(5):
                cloud.nn_device(dq, Q, keys, pcdhip.NN_AUTO, stream)
            pcdhip.profile_enable(True); pcdhip.profile_only("nn_brick"); pcdhip.profile_reset()
            for _ in range(20):
                cloud.nn_device(dq, Q, keys, pcdhip.NN_AUTO, stream)
            torch.cuda.synchronize()
            n, ms = pcdhip.profile_get()["nn_brick"]
            pcdhip.profile_enable(False); pcdhip.profile_only(None)
            pcdhip.set_nn_tuning(collect_stats=5)
            for rep in range(3):   # three statistics passes: the figure's own spread
                cloud.nn_device(dq, Q, keys, pcdhip.NN_AUTO, stream)
                rec, nitems = cloud.last_wave_records()
                dump["%s_sched%d_rep%d" % (name, sched, rep)] = rec
            pcdhip.set_nn_tuning(collect_stats=0)
            dump["%s_sched%d_ms" % (name, sched)] = np.array([ms / n])
            dump["%s_nitems" % name] = np.array([nitems])
    pcdhip.set_nn_schedule(0)
    cloud.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dump", help="write the records to this .npz")
    ap.add_argument("--load", help="read the records from this .npz instead of measuring")
    ap.add_argument("--no-fit", action="store_true", help="skip the model and the fit (minutes of CPU time)")
    a = ap.parse_args()
    if a.load:
        d = dict(np.load(a.load))
    else:
        d = {}
        measure(d)
        if a.dump:
            np.savez_compressed(a.dump, **d)
    for name, N in (("M", 1), ("M_8", 8)):
        for sched in (1, 0):
            label = "workload %s, %s schedule" % (name, "static" if sched else "hybrid")
            print("%s: nn_brick %.4f ms (profile scope, statistics off, mean of 20)" % (label, d["%s_sched%d_ms" % (name, sched)][0]))
            for rep in range(3):
                tail_report("%s, statistics pass %d" % (label, rep), d["%s_sched%d_rep%d" % (name, sched, rep)])
        if not a.no_fit:
            costs = item_costs(10_000_000, 1_000_000, 0, 1_000_000 // N)
            for rep in range(3):
                fit(d["%s_sched1_rep%d" % (name, rep)], costs)


if __name__ == "__main__":
    main()

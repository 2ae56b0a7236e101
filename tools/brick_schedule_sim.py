"""Prices work schedules of k_nn_brick_clip (csrc/brick_clip_kernel.h) on a per-item cost model.

    python tools/brick_schedule_sim.py [--share 8] [--cache FILE.npz] [--fit A,B,C] [--waves-per-class 512]

The items of workload M (bench.py: 10 M points, 1 M queries; --share N: the queries [0, Q / N) of it) come from the model
of tools/brick_clip_sim.py (rule `class`): the count, the tiles and the compare slots of every item, in item order
(--cache keeps them: the model takes minutes).  An item costs
    a + b * tiles + c * slots                       --fit a,b,c: the fit tools/brick_tail_probe.py prints
or one of the two guessed models that stood in for the fit before anybody had measured the tail:
    g1   65 % fixed + 35 % compare slots            (shares of the summed cost)
    g2   33 % fixed + 67 % tiles * (6 + queries)

Schedules (as the kernel runs them: 8 block classes own contiguous eighths of the item list, S wavefronts a class):
    static          wavefront w takes items w, w + S, ...
    hybrid f, C     the first floor(f * rounds) rounds static, the rest in chunks of C consecutive items from a cursor per
                    class; a wavefront grabs its next chunk when it starts the last item it holds (the kernel's prefetch)
    dynamic         f = 0, C = 1
Two prices per schedule, both as the kernel's end over the balanced ideal (summed cost / wavefronts):
    alone    every wavefront runs at its own pace whatever its neighbours do (pessimistic: a late wavefront gets no help);
    shared   the 4 wavefronts of a SIMD share its issue slots: while all have work everything runs as priced; once the
             cursor is empty and wavefronts end, those left on a SIMD speed up by the occupancy scan of DESIGN.md 5
             (0.995 / 0.646 / 0.546 / 0.507 ms with 1 .. 4 wavefronts per SIMD).
It also prints the longest wavefront over the mean (static), the balance of the eighths, and per cursor the number of
grabs against what the dynamic phase could serve at 10 ns per same-address atomic.

numpy only; never touches the GPU.
"""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OCC_MS = (0.995, 0.646, 0.546, 0.507)             # kernel time with 1 .. 4 wavefronts per SIMD
RATE = [OCC_MS[3] / OCC_MS[k - 1] * 4.0 / k for k in (1, 2, 3, 4)]   # pace of ONE wavefront among k, 1 at k = 4
ATOMIC_US = 0.010


def drain(rem):
    """end of a SIMD whose wavefronts still have `rem` work each (priced at 4 per SIMD) when the others stop competing"""
    rem = sorted(r for r in rem if r > 0)
    t, done = 0.0, 0.0
    for i, r in enumerate(rem):
        k = len(rem) - i
        t += (r - done) / RATE[k - 1] if k < 4 else (r - done)
        done = r
    return t


def price_class(cost, S, f, C):
    """(end alone, end shared, grabs, length of the dynamic phase) of one class's items under static share f, chunk C"""
    n = len(cost)
    rounds = -(-n // S)
    r_s = rounds if f >= 1 else int(f * rounds)
    stat_end = min(r_s * S, n)
    free = np.zeros(S)
    for r in range(-(-stat_end // S)):
        seg = cost[r * S:min((r + 1) * S, stat_end)]
        free[:len(seg)] += seg
    if stat_end >= n:
        groups = free.reshape(-1, 4) if S % 4 == 0 else free.reshape(-1, 1)
        return free.max(), max(drain(g - g.min()) + g.min() for g in groups), 0, 0.0
    # dynamic phase: a wavefront grabs when it STARTS the last item it holds -> heap on that time
    csum = np.concatenate([[0.0], np.cumsum(cost)])
    last_start = np.empty(S)
    for w in range(S):      # the last static item of wavefront w (none: it grabs at time 0 and waits for nothing)
        k = (stat_end - 1 - w) // S if stat_end > w else -1
        last_start[w] = free[w] - (cost[k * S + w] if k >= 0 else 0.0)
    heap = [(last_start[w], w) for w in range(S)]
    heapq.heapify(heap)
    cursor, grabs, t_first, t_empty = stat_end, 0, None, None
    while heap:
        t, w = heapq.heappop(heap)
        grabs += 1
        t_first = t if t_first is None else t_first
        if cursor >= n:
            t_empty = t if t_empty is None else t_empty
            continue      # the wavefront ends with what it holds
        a, b = cursor, min(cursor + C, n)
        cursor = b
        start = free[w]                               # the chunk starts when the held items are done
        free[w] = start + csum[b] - csum[a]
        heapq.heappush(heap, (free[w] - cost[b - 1], w))
    alone = free.max()
    # shared: up to t_empty everything runs as priced; afterwards the SIMD's survivors speed up
    t0 = t_empty if t_empty is not None else 0.0
    groups = free.reshape(-1, 4) if S % 4 == 0 else free.reshape(-1, 1)
    shared = max(t0 + drain(np.maximum(g - t0, 0.0)) for g in groups)
    return alone, shared, grabs, alone - t_first


def price(cost, S, f, C, classes=8):
    n = len(cost)
    per = -(-n // classes)
    ends = [price_class(cost[c * per:min((c + 1) * per, n)], S, f, C) for c in range(classes)]
    ideal = cost.sum() / (classes * S)
    alone, shared = max(e[0] for e in ends) / ideal, max(e[1] for e in ends) / ideal
    return alone, shared, max(e[2] for e in ends), min((e[3] for e in ends if e[2]), default=0.0)


def models(cnt, tiles, slots, fit):
    out = {}
    if fit is not None:
        a, b, c = fit
        out["fit %.4g us + %.4g us * tiles + %.4g ns * slots" % (a, b, 1e3 * c)] = a + b * tiles + c * slots
    n = len(cnt)
    s = slots / slots.sum() * n
    out["g1: 65 % fixed + 35 % slots"] = 0.65 + 0.35 * s
    w = tiles * (6 + cnt)
    out["g2: 33 % fixed + 67 % tiles * (6 + queries)"] = 0.33 + 0.67 * w / w.sum() * n
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--share", type=int, default=1)
    ap.add_argument("--cache")
    ap.add_argument("--fit", help="a,b,c in us, us per tile, us per slot")
    ap.add_argument("--waves-per-class", type=int, default=512)
    ap.add_argument("--kernel-ms", type=float, default=0.426, help="the kernel's time: scales the guessed models to us")
    a = ap.parse_args()
    if a.cache and os.path.exists(a.cache):
        d = np.load(a.cache)
        cnt, tiles, slots = d["cnt"], d["tiles"], d["slots"]
    else:
        import brick_tail_probe as probe
        cnt, tiles, slots = probe.item_costs(10_000_000, 1_000_000, 0, 1_000_000 // a.share)
        if a.cache:
            np.savez_compressed(a.cache, cnt=cnt, tiles=tiles, slots=slots)
    S = a.waves_per_class
    print("items %d  queries/item: 1 -> %d, 8 -> %d  tiles: median %.0f, max %.0f  compare slots %.1f M  items per wavefront %.1f" % (
        len(cnt), (cnt == 1).sum(), (cnt == 8).sum(), np.median(tiles), tiles.max(), slots.sum() / 1e6, len(cnt) / (8.0 * S)))
    fit = [float(x) for x in a.fit.split(",")] if a.fit else None
    for name, cost in models(cnt, tiles, slots, fit).items():
        if not name.startswith("fit"):      # unit cost 1 per item on average -> microseconds of the measured kernel
            cost = cost * (a.kernel_ms * 1e3 * 8 * S / len(cnt))
        n, per = len(cost), -(-len(cost) // 8)
        cls = np.array([cost[c * per:min((c + 1) * per, n)].sum() for c in range(8)])
        longest = []
        for c in range(8):
            seg = cost[c * per:min((c + 1) * per, n)]
            w = np.bincount(np.arange(len(seg)) % S, weights=seg, minlength=S)
            longest.append(w.max() / w.mean())
        print("\n%s\n  eighths %+.1f .. %+.1f %% of their mean;  longest wavefront of a class %.2f .. %.2f x its mean" % (
            name, 100 * (cls.min() / cls.mean() - 1), 100 * (cls.max() / cls.mean() - 1), min(longest), max(longest)))
        rows = [("static", 1.0, 1)] + [("hybrid f %.2f C %d" % (f, C), f, C) for f in (0.5, 0.75, 0.8, 0.85, 0.9) for C in (1, 2, 4)]
        rows.append(("hybrid f 0.90 C 8", 0.9, 8))
        rows.append(("dynamic", 0.0, 1))
        for label, f, C in rows:
            alone, shared, grabs, phase = price(cost, S, f, C)
            served = phase / ATOMIC_US
            print("  %-20s end / ideal: alone %.3f  shared %.3f   grabs per cursor %5d, dynamic phase %6.1f us could serve %6.0f (%.1f x)" % (
                label, alone, shared, grabs, phase, served, served / grabs if grabs else 0.0))


if __name__ == "__main__":
    main()

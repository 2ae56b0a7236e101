"""What the order of k_nn_fallback's list and the granularity at which a walk's slot is released are worth: a schedule
model over the walk lengths of tools/fb_walk_sim.py's model.

    python tools/fb_schedule_sim.py [--every K] [--dump FILE.npz]     walk every K-th query of workload M's fallback list
    python tools/fb_schedule_sim.py --load FILE.npz                     the tables from a dump

The walk model (fb_walk_sim.py, the kernel as built: seed bound of 8 x 8 x 8 cells) gives the steps of every walked
query of the two classes (empty-halo / outside by query id, then open -- the order of the list up to the atomics'
order inside a class).  The schedule model is greedy in-order dispatch with cost = steps: entry e of the list goes to
wavefront e mod W (W = 65536 / K wavefronts, the kernel's grid; a wavefront's entries run one after the other), the
wavefronts start in order on S = 8192 / K slots (256 CUs x 32 wavefronts), a slot is released
  per wavefront           when the wavefront ends, or
  per workgroup of four   when the last of four consecutive wavefronts ends (they start together),
and the makespan is compared with the ideal sum / slots.  Orders: the list as it is; the empty-halo class by the
distance to the query's seed point, descending (a bound known before the walk); longest walk first (the true cost: not
available to the kernel).
"""
import argparse
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def makespan(cost, slots, group):
    """in-order dispatch of `cost` (one entry per wavefront) in groups of `group` wavefronts on slots / group group slots"""
    n = len(cost) // group * group
    g = cost[:n].reshape(-1, group).max(1)
    if n < len(cost):
        g = np.append(g, cost[n:].max())
    free = [0.0] * (slots // group)
    heapq.heapify(free)
    end = 0.0
    for c in g:
        t = heapq.heappop(free) + c
        heapq.heappush(free, t)
        end = max(end, t)
    return end


def finished_share(cost, group):
    n = len(cost) // group * group
    c = cost[:n].reshape(-1, group).astype(np.float64)
    life = c.max(1)
    return float(((life[:, None] - c).sum(1) / (group * life)).mean())


def per_wave(steps, waves):
    """cost of every wavefront: the entries e, e + waves, ... of the list"""
    c = np.zeros(waves)
    for s in range(0, len(steps), waves):
        part = steps[s:s + waves]
        c[:len(part)] += part
    return c[:min(waves, len(steps))]


def measure(every):
    import fb_walk_sim as sim
    W = sim.workload(10_000_000, 1_000_000, [8])
    out = {}
    for name, sel in (("empty", W["empty"]), ("open", W["open_"])):
        ids = np.nonzero(sel)[0][::every]
        steps, dist = np.zeros(len(ids), np.int64), np.zeros(len(ids))
        for r, i in enumerate(ids):
            best = sim.start_key(W, i, name, 8)
            dist[r] = np.sqrt(float(sim.start_key(W, i, "empty", 8)[0]))
            steps[r] = W["ix"].walk(W["qf"][i], best, False)[0]
        out[name + "_steps"], out[name + "_seed_dist"] = steps, dist
        print("%s: %d walks" % (name, len(ids)), flush=True)
    out["every"] = np.array([every])
    out["class_sizes"] = np.array([W["empty"].sum(), W["open_"].sum()])
    return out


def report(d):
    every = int(d["every"][0])
    e, o = d["empty_steps"], d["open_steps"]
    ed = d["empty_seed_dist"]
    allsteps = np.concatenate([e, o])
    print("workload M's fallback list: %d empty-halo / outside and %d open queries; every %d%s walked by the model" % (
        d["class_sizes"][0], d["class_sizes"][1], every, {1: "st", 2: "nd", 3: "rd"}.get(every, "th")))
    print("| class | mean steps | max |\n|---|---|---|")
    print("| empty-halo | %.2f | %d |\n| open | %.2f | %d |" % (e.mean(), e.max(), o.mean(), o.max()))
    print("| whole list | %.2f (p50 %d, p90 %d, p99 %d, p99.9 %d) | %d |" % ((allsteps.mean(),) + tuple(
        int(np.percentile(allsteps, p)) for p in (50, 90, 99, 99.9)) + (allsteps.max(),)))
    top = e >= np.percentile(e, 99)
    print("seed distance against steps (empty-halo class): correlation %.2f; median seed distance %.1f m of the longest "
          "1 %% of the walks, %.1f m of all" % (np.corrcoef(ed, e)[0, 1], np.median(ed[top]), np.median(ed)))
    waves, slots = 65536 // every, 8192 // every
    orders = {
        "today (empty-halo by id, then open)": allsteps,
        "empty-halo by seed distance, descending": np.concatenate([e[np.argsort(-ed, kind="stable")], o]),
        "longest first, true cost (not available)": np.sort(allsteps)[::-1],
    }
    ideal = allsteps.sum() / slots
    print("\n%d entries on %d wavefronts, %d slots; makespan in steps" % (len(allsteps), waves, slots))
    print("| order of the list | slot released per wavefront | slot released per workgroup of 4 |\n|---|---|---|")
    print("| ideal (sum / slots) | %.1f | %.1f |" % (ideal, ideal))
    for name, st in orders.items():
        c = per_wave(st, waves)
        a, b = makespan(c, slots, 1), makespan(c, slots, 4)
        print("| %s | %.0f (%.2fx) | %.0f (%.2fx) |" % (name, a, a / ideal, b, b / ideal))
    fin = finished_share(per_wave(allsteps, waves), 4)
    print("\na workgroup of four: its wavefronts are finished for %.0f %% of its life on average; 9 workgroups x 4 x %.2f = "
          "%.0f live wavefronts per CU of 32" % (100 * fin, 1 - fin, 9 * 4 * (1 - fin)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--every", type=int, default=2, help="walk every K-th query of each class (the model walks in Python)")
    ap.add_argument("--dump")
    ap.add_argument("--load")
    a = ap.parse_args()
    if a.load:
        d = dict(np.load(a.load))
    else:
        d = measure(a.every)
        if a.dump:
            np.savez_compressed(a.dump, **d)
    report(d)


if __name__ == "__main__":
    main()

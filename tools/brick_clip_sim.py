"""CPU model of what k_nn_brick_clip (csrc/brick_clip_kernel.h) stages, to price rules for the item's stage-A range.

    python tools/brick_clip_sim.py [--points N] [--queries Q] [--sigma S] [--sample K] [--seed R] [--cell-size H]
                                   (defaults: workload M of bench.py = 10 M points, 1 M queries, sigma 0.25 m; 6 000 items)

The model builds the grid as cloud.hip does (the cell-size iteration, float32 binning), sorts the cloud in grid.h's
quad-row cell order, sends the queries that lie outside the grid or in a brick with an empty halo to the fallback up
front and cuts the others into items of at most 8 queries of one brick (k_bk_emit; in query order inside a brick, where
the library has them in atomic order).  For a seeded sample of items it then does what the kernel does: stage A on the
first <= 128 records of the item's stage-A range in FLANN's float arithmetic, the clip masks from brick_clip_kernel.h's
float expressions, the hull of every quad row's masked x cells from the item's boundary table, the row stage A read
split around what it read, every range padded to groups of 4 slots, tiles of 256.  It prints staged points
(`staged_points` of last_stats()), the compare slots of the tiles and the compare slots with stage A's steps of 64
(`pair_evals` of last_stats() less its `fallback_points`: the library adds the fallback walk's point-query pairs to
the figure), scaled from the sample to all items and split by whether the brick's own cells hold a point.

Rules for the stage-A range of an item whose own 2x2x2 cells are empty (an item with own points always takes those):
  noclip    the clip switched off (pcd_nn_set_search(1)): every mask all ones, the whole region staged;
  own       none: d_k stays at its incoming value and the whole region is staged (the kernel before the substitute);
  class     the neighbouring two-cell span (= brick) of the lowest class -- face, edge, corner -- that holds a point,
            within the class the fullest one, ties to the lowest index of the boundary table;
  first     the first span with a point in that fixed order (class, then table index);
  fullest   the fullest span of all 26, ties to the lowest class, then table index;
  near      the span with a point whose brick is nearest to the item's first query (squared distance to the brick's
            box, ties to the fuller span, then table index);
  floor     not a rule: d_k = the true distance to the nearest point of the region, the least any rule can stage.

numpy only; never touches the GPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
from pcdhip import synth  # noqa: E402

F = np.float32
NK, NROWS, ATILE, TILE = 7, 9, 128, 256
RULES = ("noclip", "own", "class", "first", "fullest", "near", "floor")


def grid_params(p, cell_size=0.0):
    """cloud.hip choose_cell_size / set_dims: cell size (given, or the iteration towards 24 points per occupied cell)"""
    lo, hi = p.min(0), p.max(0)
    m = len(p)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    maxext = ext.max()
    h = np.cbrt((ext[0] + 1e-3) * (ext[1] + 1e-3) * (ext[2] + 1e-3) / float(1 << 26))
    for _ in range(64):
        if np.prod(np.floor(ext / h) + 1) <= float(1 << 26):
            break
        h *= 1.05
    hmin = max(h, 1e-6 * max(maxext, 1e-3))

    def cells(h):
        inv = F(1.0) / F(h)
        dims = np.maximum(np.floor(ext / np.float64(h)).astype(np.int64) + 1, 1)
        c = np.floor((p - lo) * inv).astype(np.int64)
        return np.clip(c, 0, dims - 1), dims, inv

    if cell_size > 0:
        h = F(max(cell_size, hmin))
    else:
        hg = np.sqrt(24.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2] + 1e-6) / m)
        h = F(min(max(hg, hmin), max(maxext, hmin)))
        for _ in range(6):
            c, dims, _ = cells(h)
            flat = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
            occ = m / max(len(np.unique(flat)), 1)
            if 0.75 * 24 < occ < 1.5 * 24:
                break
            hn = min(max(h * (24.0 / occ) ** (1 / 2.5), hmin), max(maxext, hmin))
            if abs(hn - h) < 1e-3 * h:
                break
            h = F(hn)
    c, dims, inv = cells(h)
    return dict(lo=lo, h=F(h), inv=inv, dims=dims, cell=c)


class Model:
    def __init__(self, xyz, cell_size=0.0):
        p = np.ascontiguousarray(xyz, F)
        g = grid_params(p, cell_size)
        self.lo, self.h, self.inv, self.dims = g["lo"], g["h"], g["inv"], g["dims"]
        nx, ny, nz = (int(v) for v in self.dims)
        self.nyq, self.nzq = (ny + 1) // 2, (nz + 1) // 2
        c = g["cell"]
        # grid.h cell_index: ((zq * nyq + yq) * nx + x) * 4 + (z & 1) * 2 + (y & 1)
        ci = (((c[:, 2] >> 1) * self.nyq + (c[:, 1] >> 1)) * nx + c[:, 0]) * 4 + ((c[:, 2] & 1) << 1) + (c[:, 1] & 1)
        order = np.argsort(ci, kind="stable")
        self.sp = p[order]
        ncells = nx * self.nyq * self.nzq * 4
        self.cell_start = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncells))]).astype(np.int64)

    def tables(self, b):
        """the items' boundary tables (clip_load_meta): [n, 9, 7], entry [row, k] = cell_start at x boundary k of region
        row `row` = ry + 3 rz, 0 for rows outside the grid"""
        nx = int(self.dims[0])
        b = np.asarray(b, np.int64)
        k = np.arange(NK)
        r = np.arange(NROWS)
        yq = b[:, 1, None] - 1 + (r % 3)[None, :]
        zq = b[:, 2, None] - 1 + (r // 3)[None, :]
        ok = (yq >= 0) & (yq < self.nyq) & (zq >= 0) & (zq < self.nzq)
        x = np.clip(2 * b[:, 0, None] - 2 + k[None, :], 0, nx)
        base = (np.where(ok, zq, 0) * self.nyq + np.where(ok, yq, 0)) * nx * 4
        t = self.cell_start[base[:, :, None] + 4 * x[:, None, :]]
        return np.where(ok[:, :, None], t, 0)

    def items(self, queries):
        """(brick [n, 3], first, count) of the items in brick order, the brick-sorted float queries, and the number of
        queries that go to the fallback up front"""
        q = np.asarray(queries, np.float64).astype(F)
        t = np.floor((q - self.lo) * self.inv)
        c = np.clip(t, -1, self.dims.astype(F)).astype(np.int64)
        inside = ((c >= 0) & (c < self.dims)).all(1)
        b = c >> 1
        nb = (self.dims + 1) // 2
        bid = (b[:, 2] * nb[1] + b[:, 1]) * nb[0] + b[:, 0]
        ub, inv = np.unique(bid[inside], return_inverse=True)
        ub3 = np.stack([ub % nb[0], (ub // nb[0]) % nb[1], ub // (nb[0] * nb[1])], 1)
        tab = self.tables(ub3)
        occupied = ((tab[:, :, NK - 1] - tab[:, :, 0]) > 0).any(1)      # k_brick_occupied
        keep = np.zeros(len(q), bool)
        keep[np.nonzero(inside)[0]] = occupied[inv]
        qi = np.nonzero(keep)[0]
        order = np.argsort(bid[qi], kind="stable")
        qs, bs = q[qi[order]], bid[qi[order]]
        ubk, first, cnt = np.unique(bs, return_index=True, return_counts=True)
        nit = (cnt + 7) // 8
        ib = np.repeat(np.arange(len(ubk)), nit)
        j = np.arange(len(ib)) - np.repeat(np.cumsum(nit) - nit, nit)
        ifirst = first[ib] + 8 * j
        icnt = np.minimum(cnt[ib] - 8 * j, 8)
        ub = ubk[ib]
        ib3 = np.stack([ub % nb[0], (ub // nb[0]) % nb[1], ub // (nb[0] * nb[1])], 1)
        return ib3, ifirst, icnt, qs, int(len(q) - len(qi))


def span_class(r, j):
    return (j != 1) + (r % 3 != 1) + (r // 3 != 1) - 1     # 0 face, 1 edge, 2 corner (-1: the brick itself)


CAND = [(r, j) for r in range(NROWS) for j in range(3) if (r, j) != (4, 1)]     # in table order


def l2(q, p):
    """FLANN L2_Simple in float32: ((dx dx) + dy dy) + dz dz, [queries, points]"""
    d = q[:, None, :] - p[None, :, :]
    d = d * d
    return (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]


def choose(rule, tab, q0, b, m):
    """(row, first boundary) of the stage-A range of an item whose own cells are empty; None: no substitute"""
    size = {c: int(tab[c[0], 2 * c[1] + 2] - tab[c[0], 2 * c[1]]) for c in CAND}
    live = [c for c in CAND if size[c] > 0]
    if rule in ("own", "noclip") or not live:
        return None
    idx = lambda c: 7 * c[0] + 2 * c[1]
    if rule == "class":
        c = min(live, key=lambda c: (span_class(*c), -size[c], idx(c)))
    elif rule == "first":
        c = min(live, key=lambda c: (span_class(*c), idx(c)))
    elif rule == "fullest":
        c = min(live, key=lambda c: (-size[c], span_class(*c), idx(c)))
    elif rule == "near":
        def dist(c):
            off = np.array([c[1] - 1, c[0] % 3 - 1, c[0] // 3 - 1])
            lo = m.lo.astype(np.float64) + (2 * (np.asarray(b) + off)) * float(m.h)
            d = np.maximum(np.maximum(lo - q0, q0 - (lo + 2 * float(m.h))), 0)
            return float((d * d).sum())
        c = min(live, key=lambda c: (dist(c), -size[c], idx(c)))
    else:
        raise ValueError(rule)
    return c[0], 2 * c[1]


def simulate_item(m, rule, b, tab, q):
    """(staged points, tile slots, stage-A slots) of one item under `rule`"""
    cnt = len(q)
    row, k0 = 4, 2
    if rule != "floor" and tab[4, 2] == tab[4, 4]:
        sub = choose(rule, tab, q[0].astype(np.float64), b, m)
        if sub is not None:
            row, k0 = sub
    sA, eA = int(tab[row, k0]), int(tab[row, k0 + 2])
    nA = min(eA - sA, ATILE)
    if rule == "floor":
        pts = np.concatenate([m.sp[int(tab[r, 0]):int(tab[r, NK - 1])] for r in range(NROWS)])
        d = l2(q, pts).min(1)
    elif nA > 0:
        d = l2(q, m.sp[sA:sA + nA]).min(1)
    else:
        d = np.full(cnt, np.finfo(F).max, F)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.sqrt(d) * F(1.00001) + ((np.abs(q[:, 0]) + np.abs(q[:, 1])) + np.abs(q[:, 2])) * F(2.4e-7) + F(1e-18)
        half = F(0.5)
        f0 = np.array([2 * b[0] - 2, b[1] - 1, b[2] - 1], F)
        lim = np.array([NK - 2, 2, 2], F)
        hv = np.array([1, half, half], F)     # quad rows: (x * inv_h) * 0.5f
        t0 = np.floor((q - r[:, None] - m.lo) * m.inv * hv)
        t1 = np.floor((q + r[:, None] - m.lo) * m.inv * hv)
        c0 = np.clip(np.nan_to_num(t0 - f0, nan=0.0, posinf=3e38, neginf=-3e38), 0, lim).astype(np.int64)
        c1 = np.clip(np.nan_to_num(t1 - f0, nan=0.0, posinf=3e38, neginf=-3e38), 0, lim).astype(np.int64)
    mask = np.zeros(NROWS, np.int64)
    if rule == "noclip":
        mask[:] = 63
        cnt_masks = 0
    else:
        cnt_masks = cnt
    for k in range(cnt_masks):
        xm = (2 << c1[k, 0]) - (1 << c0[k, 0])
        for rz in range(c0[k, 2], c1[k, 2] + 1):
            for ry in range(c0[k, 1], c1[k, 1] + 1):
                mask[3 * rz + ry] |= xm
    T = 0
    for rr in range(NROWS):
        xm = int(mask[rr])
        if not xm:
            continue
        lo_k = (xm & -xm).bit_length() - 1
        s, e = int(tab[rr, lo_k]), int(tab[rr, xm.bit_length()])
        if rr == row:     # without what stage A compared: [s, sA) and [sA + nA, e)
            for a, z in ((s, min(e, sA)), (max(s, sA + nA), e)):
                if z > a:
                    T += (z - a + 3) & ~3
        else:
            T += (e - s + 3) & ~3
    tiles = (T + TILE - 1) // TILE
    return nA + T, tiles * TILE * cnt, (128 if nA > 64 else 64 if nA else 0) * cnt


def run(m, queries, sample, seed, rules=RULES, out=sys.stdout):
    ib3, ifirst, icnt, qs, nfb = m.items(queries)
    n = len(ib3)
    pick = np.sort(np.random.default_rng(seed).choice(n, min(sample, n), replace=False))
    tab = m.tables(ib3[pick])
    own_empty_all = None
    if n <= 2_000_000:
        ta = m.tables(ib3)
        own_empty_all = ta[:, 4, 4] == ta[:, 4, 2]
        print("items %d  up-front fallback queries %d  items with empty own cells %d (%.1f %%), their queries %d (%.1f %% of %d)" % (
            n, nfb, own_empty_all.sum(), 100.0 * own_empty_all.mean(), icnt[own_empty_all].sum(),
            100.0 * icnt[own_empty_all].sum() / icnt.sum(), icnt.sum()), file=out, flush=True)
    scale = n / len(pick)
    empty = tab[:, 4, 4] == tab[:, 4, 2]
    res = {}
    for rule in rules:
        t = time.time()
        r = np.array([simulate_item(m, rule, ib3[i], tab[j], qs[ifirst[i]:ifirst[i] + icnt[i]])
                      for j, i in enumerate(pick)], np.float64)
        tot = r.sum(0) * scale
        e, o = r[empty].sum(0) * scale, r[~empty].sum(0) * scale
        res[rule] = dict(staged_points=tot[0], tile_slots=tot[1], pair_evals=tot[1] + tot[2],
                         staged_empty=e[0], staged_own=o[0],
                         per_item_empty=r[empty, 0].mean() if empty.any() else 0.0,
                         per_item_own=r[~empty, 0].mean() if (~empty).any() else 0.0)
        print("%-8s staged %8.2f M (own cells empty %8.2f M, %6.1f per item; with own points %8.2f M, %6.1f per item)  "
              "tile slots %8.2f M  pair_evals %8.2f M   [%.0f s]" % (
                  rule, tot[0] / 1e6, e[0] / 1e6, res[rule]["per_item_empty"], o[0] / 1e6, res[rule]["per_item_own"],
                  tot[1] / 1e6, (tot[1] + tot[2]) / 1e6, time.time() - t), file=out, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--sigma", type=float, default=0.25)
    ap.add_argument("--sample", type=int, default=6000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cell-size", type=float, default=0.0)
    ap.add_argument("--rules", default=",".join(RULES))
    a = ap.parse_args()
    t = time.time()
    xyz, _ = synth.cloud_planes(a.points)
    q = synth.queries(xyz, a.queries, seed=99, sigma=a.sigma)
    m = Model(xyz, a.cell_size)
    print("cloud %d points, %d queries (sigma %.3f): h %.4f, grid %s  [%.0f s]" % (
        len(xyz), len(q), a.sigma, m.h, "x".join(str(int(d)) for d in m.dims), time.time() - t), flush=True)
    run(m, q, a.sample, a.seed, a.rules.split(","))


if __name__ == "__main__":
    main()

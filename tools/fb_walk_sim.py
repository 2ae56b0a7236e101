"""CPU model of k_nn_fallback's walk (csrc/nn.hip), to price seed and slab bounds before building them.

    python tools/fb_walk_sim.py [N] [Q] [per_class]      (defaults: workload M = 10 M points, 1 M queries, 5000)

The model builds the cloud index as cloud.hip does (float32 binning, the cell-size iteration, 2x2x2-cell leaves,
4x4x4 pyramid nodes up to the first level with <= 64 nodes, the virtual top), splits the bench's queries
(synth.queries(..., seed=99)) into the two fallback classes the grid path produces, and walks a seeded sample of each
exactly as the kernel does: virtual top, nearest child first (ties: lowest lane), the first leaf of a node scanned and
then every other leaf of the node that still passes the tightened bound in one batch, pops counted as steps (what
PCD_FB_STATS counts).  Classes:
  empty   the query lies outside the grid or its brick's 6x6x6-cell halo holds no point: starts from kKeyInit;
  open    the brick kernel's region-restricted key is not provably final: starts from that key.
Cases: (a) today; (b) a seed bound: best starts at min(best, key of the seed point of the query's seed cell); (c) slab
bounds on the leaves, lb = max(AABB bound, plane-slab bound); (d) both.  Bounds are evaluated in double here (the
model prices walk lengths; exactness is the kernel's and the tests' business).

Bytes: the walk also counts what it requests from memory (Index.tr, printed per class for case "b seed 8", the kernel
as built): per expansion of a level-k node the child records of the DENSE lattice (64 records of 32 B = 16 lines of
128 B, whatever they hold), how many of them are occupied, how many 4-child rows (one line each) hold an occupied child,
and the lines a COMPACT child list needs (occupied records, contiguous: ceil(32 * n / 128), + 1 at worst when the list
does not start on a line); per leaf scan the 128-B lines its 16-B point records span.  That is the pricing of the
compact pyramid (cloud.h: records of the occupied nodes only).
"""
import os
import sys
import time

import numpy as np
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
from pcdhip import synth  # noqa: E402

F = np.float32


def build_grid(p):
    """cloud.hip choose_cell_size: cell size iteration and set_dims, float32 binning."""
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
    hg = np.sqrt(24.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2] + 1e-6) / m)
    h = F(min(max(hg, hmin), max(maxext, hmin)))

    def cells(h):
        inv = F(1.0) / F(h)
        dims = np.maximum(np.floor(ext / np.float64(h)).astype(np.int64) + 1, 1)
        c = np.floor((p - lo) * inv).astype(np.int64)
        return np.clip(c, 0, dims - 1), dims, inv

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


class Index:
    def __init__(self, p):
        t = time.time()
        g = build_grid(p)
        self.g = g
        dims = g["dims"]
        self.ld = np.array([(dims[0] + 1) // 2, (dims[1] + 1) // 2, (dims[2] + 1) // 2])
        leaf3 = g["cell"] >> 1
        lid = (leaf3[:, 2] * self.ld[1] + leaf3[:, 1]) * self.ld[0] + leaf3[:, 0]
        order = np.argsort(lid, kind="stable")
        self.sp = p[order]
        self.sidx = order.astype(np.int64)
        nl = int(np.prod(self.ld))
        cnt = np.bincount(lid, minlength=nl)
        self.start = np.concatenate([[0], np.cumsum(cnt)])
        self.cnt = cnt
        occ = np.nonzero(cnt)[0]
        lo = np.full((nl, 3), np.inf, F)
        hi = np.full((nl, 3), -np.inf, F)
        lo[occ] = np.minimum.reduceat(self.sp, self.start[occ], axis=0)
        hi[occ] = np.maximum.reduceat(self.sp, self.start[occ], axis=0)
        # levels: 0 = leaves; k+1 = 4x4x4 nodes of k, up to the first level with <= 64 nodes
        self.dims = [self.ld.copy()]
        self.lo, self.hi = [lo], [hi]
        while np.prod(self.dims[-1]) > 64:
            cd = self.dims[-1]
            pd = (cd + 3) // 4
            clo = self.lo[-1].reshape(cd[2], cd[1], cd[0], 3)
            chi = self.hi[-1].reshape(cd[2], cd[1], cd[0], 3)
            pad = [(0, 4 * pd[2] - cd[2]), (0, 4 * pd[1] - cd[1]), (0, 4 * pd[0] - cd[0]), (0, 0)]
            clo = np.pad(clo, pad, constant_values=np.inf).reshape(pd[2], 4, pd[1], 4, pd[0], 4, 3)
            chi = np.pad(chi, pad, constant_values=-np.inf).reshape(pd[2], 4, pd[1], 4, pd[0], 4, 3)
            self.lo.append(clo.min(axis=(1, 3, 5)).reshape(-1, 3))
            self.hi.append(chi.max(axis=(1, 3, 5)).reshape(-1, 3))
            self.dims.append(pd)
        self.top = len(self.dims)   # virtual top level
        self.slab = self._slabs()
        self.reset_traffic()
        print("index: h %.4f dims %s leaves %d (%d occupied) levels %s  %.1fs" % (
            g["h"], dims.tolist(), nl, len(occ), [d.tolist() for d in self.dims], time.time() - t), flush=True)

    def _slabs(self):
        """per leaf: plane-fit normal (float32) and the interval of n.p over its points (double)."""
        nl = len(self.cnt)
        occ = np.nonzero(self.cnt)[0]
        s = self.start[occ]
        P = self.sp.astype(np.float64)
        c = np.add.reduceat(P, s, axis=0) / self.cnt[occ, None]
        cid = np.repeat(np.arange(len(occ)), self.cnt[occ])
        d = P - c[cid]
        C = np.add.reduceat(d[:, :, None] * d[:, None, :], s, axis=0)
        w, v = np.linalg.eigh(C)
        n = v[:, :, 0].astype(F).astype(np.float64)
        t = np.einsum("ij,ij->i", P, n[cid])
        t0 = np.minimum.reduceat(t, s)
        t1 = np.maximum.reduceat(t, s)
        N = np.zeros((nl, 3))
        T0 = np.zeros(nl)
        T1 = np.zeros(nl)
        N[occ], T0[occ], T1[occ] = n, t0, t1
        return N, T0, T1

    def reset_traffic(self):
        """per level of the expanded node: expansions, occupied children, occupied 4-child rows, compact lines; leaf lines"""
        self.tr = dict(exp=np.zeros(12, np.int64), occ=np.zeros(12, np.int64), rows=np.zeros(12, np.int64),
                       clines=np.zeros(12, np.int64), dlines=np.zeros(12, np.int64), leaf_lines=0, queries=0)

    def traffic_report(self, name):
        t = self.tr
        nq = max(t["queries"], 1)
        print("%s: requested per query (n %d)" % (name, t["queries"]))
        dense = compact = 0.0
        for lev in range(1, self.top + 1):
            if not t["exp"][lev]:
                continue
            e = t["exp"][lev]
            print("  level-%d expansions %.2f  occupied children %.1f of 64  occupied rows %.1f  lines dense %.1f / compact %.1f"
                  % (lev, e / nq, t["occ"][lev] / e, t["rows"][lev] / e, t["dlines"][lev] / e, t["clines"][lev] / e))
            dense += 128.0 * t["dlines"][lev] / nq
            compact += 128.0 * t["clines"][lev] / nq
        leaf = 128.0 * t["leaf_lines"] / nq
        print("  leaf scans %.1f lines = %.1f KB; child records dense %.1f KB, compact %.1f KB; total %.1f -> %.1f KB (%.0f %% less)"
              % (t["leaf_lines"] / nq, leaf / 1e3, dense / 1e3, compact / 1e3, (leaf + dense) / 1e3, (leaf + compact) / 1e3,
                 100.0 * (dense - compact) / (leaf + dense)), flush=True)

    def region_min(self, qf, cell):
        """the brick kernel's region-restricted minimum: leaves within one leaf of the query's leaf."""
        b = cell >> 1
        best = (np.inf, -1)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    l3 = b + np.array([dx, dy, dz])
                    if (l3 < 0).any() or (l3 >= self.ld).any():
                        continue
                    li = (l3[2] * self.ld[1] + l3[1]) * self.ld[0] + l3[0]
                    s, e = self.start[li], self.start[li + 1]
                    if s == e:
                        continue
                    dd = l2(qf, self.sp[s:e])
                    k = np.lexsort((self.sidx[s:e], dd))[0]
                    if (dd[k], self.sidx[s + k]) < best:
                        best = (dd[k], self.sidx[s + k])
        return best

    def walk(self, qf, best, slab):
        """one query, exactly as k_nn_fallback walks it; returns (steps, leaf scans, leaf points, best)."""
        lanes = np.arange(64)
        ci, cj, ck = lanes & 3, (lanes >> 2) & 3, lanes >> 4
        q64 = qf.astype(np.float64)
        N, T0, T1 = self.slab

        def expand(lev, node):
            d = self.dims[lev - 1]
            if lev == self.top:
                cx, cy, cz = lanes % d[0], (lanes // d[0]) % d[1], lanes // (d[0] * d[1])
            else:
                cx, cy, cz = 4 * node[0] + ci, 4 * node[1] + cj, 4 * node[2] + ck
            inn = (cx < d[0]) & (cy < d[1]) & (cz < d[2])
            ids = np.where(inn, (cz * d[1] + cy) * d[0] + cx, 0)
            lo, hi = self.lo[lev - 1][ids], self.hi[lev - 1][ids]
            pc = np.minimum(np.maximum(qf, lo), hi)
            lb = l2(qf, pc)
            ok = inn & (lo[:, 0] <= hi[:, 0])
            lb = np.where(ok, lb, np.inf)
            tr = self.tr
            tr["exp"][lev] += 1
            tr["occ"][lev] += int(ok.sum())
            tr["rows"][lev] += int(ok.sum()) if lev == self.top else int(ok.reshape(16, 4).any(1).sum())
            tr["dlines"][lev] += -(-int(np.prod(d)) // 4) if lev == self.top else 16
            tr["clines"][lev] += -(-int(ok.sum()) // 4)
            if slab and lev == 1:
                t = N[ids] @ q64
                g = np.maximum(np.maximum(T0[ids] - t, t - T1[ids]), 0.0)
                lb = np.where(ok, np.maximum(lb, g * g), np.inf)
            return lb, ok, (cx, cy, cz), ids

        steps = leaves = pts = 0
        self.tr["queries"] += 1
        lev, node = self.top, (0, 0, 0)
        lb, mask, cc, ids = expand(lev, node)
        stack = {}
        while True:
            steps += 1
            m = mask & (lb <= best[0])
            if not m.any():
                if lev == self.top:
                    break
                lev += 1
                lb, mask, cc, ids, node = stack[lev]
                continue
            sl = int(np.argmin(np.where(m, lb, np.inf)))
            m[sl] = False
            mask = m
            if lev == 1:
                scan = [ids[sl]]
                best = self._scan(qf, ids[sl], best)
                mb = m & (lb <= best[0])
                if mb.any():
                    mask = m & ~mb
                    for li in ids[mb]:
                        scan.append(li)
                        best = self._scan(qf, li, best)
                leaves += len(scan)
                pts += int(self.cnt[scan].sum())
            else:
                stack[lev] = (lb, mask.copy(), cc, ids, node)
                node = (cc[0][sl], cc[1][sl], cc[2][sl])
                lev -= 1
                lb, mask, cc, ids = expand(lev, node)
        return steps, leaves, pts, best

    def _scan(self, qf, li, best):
        s, e = self.start[li], self.start[li + 1]
        if s == e:
            return best
        self.tr["leaf_lines"] += int((16 * e - 1) // 128 - (16 * s) // 128 + 1)
        dd = l2(qf, self.sp[s:e])
        k = np.lexsort((self.sidx[s:e], dd))[0]
        return min(best, (dd[k], self.sidx[s + k]))


def l2(q, p):
    """FLANN's L2_Simple<float>: ((dx*dx) + dy*dy) + dz*dz in float32."""
    d = (q - p).astype(F)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def workload(N, Q, seed_cells):
    """cloud, index, exact neighbours, the two fallback classes and the seed lattices of the bench's workload"""
    t = time.time()
    xyz, _ = synth.cloud_planes(N)
    q = synth.queries(xyz, Q, seed=99)
    qf = q.astype(F)
    print("gen %.1fs" % (time.time() - t), flush=True)
    ix = Index(xyz)
    g = ix.g
    dims = g["dims"]
    tree = cKDTree(xyz.astype(np.float64))
    t = time.time()
    dnn, inn = tree.query(qf.astype(np.float64), workers=-1)
    print("exact nn %.1fs" % (time.time() - t), flush=True)
    # classes: the query's brick (2x2x2 cells = its leaf) and its 6x6x6-cell halo region (3x3x3 leaves)
    craw = np.floor((qf - g["lo"]) * g["inv"])
    inside = ((craw >= 0) & (craw < dims)).all(1)
    cell = np.clip(craw, 0, dims - 1).astype(np.int64)
    occ3 = (ix.cnt > 0).reshape(ix.ld[2], ix.ld[1], ix.ld[0])
    halo = np.zeros_like(occ3)
    P = np.pad(occ3, 1)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                halo |= P[dz:dz + occ3.shape[0], dy:dy + occ3.shape[1], dx:dx + occ3.shape[2]]
    b = cell >> 1
    hq = halo[b[:, 2], b[:, 1], b[:, 0]]
    empty = ~inside | ~hq
    # open: in a brick with points in its halo, and the region-restricted result not provably final
    lo64 = g["lo"].astype(np.float64)
    h64 = np.float64(g["h"])
    c0 = np.maximum(2 * b - 2, 0)
    c1 = np.minimum(2 * b + 4, dims)
    q64 = qf.astype(np.float64)
    fl = np.where(c0 > 0, q64 - (lo64 + c0 * h64), np.inf)
    fh = np.where(c1 < dims, (lo64 + c1 * h64) - q64, np.inf)
    margin = np.minimum(fl, fh).min(1)
    ext = max(float((xyz.max(0).astype(np.float64) - lo64).max()), float(np.abs(xyz).max()))
    slack = ext * 9.6e-7
    bound = np.where(np.isinf(margin), np.inf, np.maximum(margin - 2 * slack, 0) ** 2 * (1 - 1e-5))
    pnn = xyz[inn]
    dnn_f = l2(qf, pnn)
    leaf_nn = (ix.g["cell"][inn] >> 1)
    nn_in_region = (np.abs(leaf_nn - b) <= 1).all(1)
    open_ = ~empty & ~(nn_in_region & (dnn_f < bound))
    print("queries %d: empty-halo / outside %d, open %d -> fallback %d" % (Q, empty.sum(), open_.sum(),
                                                                          empty.sum() + open_.sum()), flush=True)
    # seeds: the exact nearest point to the centre of every cell of a lattice of s x s x s grid cells
    seeds = {}
    for s in seed_cells:
        sd = (dims + s - 1) // s
        gz, gy, gx = np.meshgrid(np.arange(sd[2]), np.arange(sd[1]), np.arange(sd[0]), indexing="ij")
        ctr = lo64 + (np.stack([gx, gy, gz], -1).reshape(-1, 3) + 0.5) * s * h64
        t = time.time()
        _, si = tree.query(ctr, workers=-1)
        seeds[s] = (sd, si)
        print("seed lattice %d cells: %s = %d seeds, %.1fs" % (s, sd.tolist(), len(si), time.time() - t), flush=True)
    return dict(xyz=xyz, qf=qf, ix=ix, dims=dims, craw=craw, cell=cell, empty=empty, open_=open_, dnn_f=dnn_f, seeds=seeds)


def start_key(W, i, name, seed_s):
    """the key a walk of query i starts from: kKeyInit (empty) or the region-restricted result (open), and the seed"""
    ix, qf = W["ix"], W["qf"]
    if name == "empty":
        best = (F(np.finfo(F).max), 0)
    else:
        rb = ix.region_min(qf[i], W["cell"][i])
        best = (F(rb[0]), rb[1]) if rb[1] >= 0 else (F(np.finfo(F).max), 0)
    if seed_s is not None:
        sd, si = W["seeds"][seed_s]
        sc = np.clip(W["craw"][i], 0, W["dims"] - 1).astype(np.int64) // seed_s
        k = si[(sc[2] * sd[1] + sc[1]) * sd[0] + sc[0]]
        best = min(best, (l2(qf[i], W["xyz"][k]), int(k)))
    return best


def main():
    N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    Q = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
    seed_cells = [int(s) for s in os.environ.get("FB_SIM_SEED_CELLS", "2,8").split(",")]
    W = workload(N, Q, seed_cells)
    ix, qf, empty, open_, dnn_f = W["ix"], W["qf"], W["empty"], W["open_"], W["dnn_f"]
    rng = np.random.default_rng(5)
    samples = {}
    for name, sel in (("empty", empty), ("open", open_)):
        ids = np.nonzero(sel)[0]
        samples[name] = np.sort(rng.choice(ids, min(per, len(ids)), replace=False))
    rows = []
    for name, ids in samples.items():
        for case, seed_s, slab in [("a today", None, False)] + \
                [("b seed %d" % s, s, False) for s in seed_cells] + [("c slab", None, True)] + \
                [("d seed %d + slab" % s, s, True) for s in seed_cells]:
            t = time.time()
            ix.reset_traffic()
            st = np.zeros((len(ids), 3), np.int64)
            for r, i in enumerate(ids):
                best = start_key(W, i, name, seed_s)
                steps, leaves, pts, res = ix.walk(qf[i], best, slab)
                if res[0] > dnn_f[i]:   # (below it: float ties / rounding against the double-precision tree)
                    raise SystemExit("model walk is not exact for query %d: %r vs %r" % (i, res, dnn_f[i]))
                st[r] = steps, leaves, pts
            rows.append((name, case, len(ids), st[:, 0].mean(), st[:, 0].max(), st[:, 1].mean(), st[:, 1].max(),
                         st[:, 2].mean(), st[:, 2].max()))
            print("%-6s %-18s n %5d  steps %5.2f (max %3d)  leaves %5.2f (max %3d)  leaf points %6.1f (max %5d)  %.0fs"
                  % (rows[-1] + (time.time() - t,)), flush=True)
            if case == "b seed 8":
                ix.traffic_report(name)
    # the fallback as a whole: the classes weighted by their share
    w = {"empty": empty.sum(), "open": open_.sum()}
    print("\nweighted over the fallback list (%d empty-halo / outside + %d open):" % (w["empty"], w["open"]))
    for case in dict.fromkeys(r[1] for r in rows):
        sel = {r[0]: r for r in rows if r[1] == case}
        tot = sum(w.values())
        print("  %-18s steps %5.2f  leaves %5.2f  leaf points %6.1f  max steps %3d" % (
            case, sum(w[k] * sel[k][3] for k in w) / tot, sum(w[k] * sel[k][5] for k in w) / tot,
            sum(w[k] * sel[k][7] for k in w) / tot, max(sel[k][4] for k in w)))


if __name__ == "__main__":
    main()

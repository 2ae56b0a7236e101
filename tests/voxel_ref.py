"""numpy reference of the voxel-grid downsampling (pcd_cloud_voxel_downsample, definition in include/pcdhip.h), written
from the definition alone:

  * inv = float32(1) / leaf and the product p * inv in float32, np.floor, voxel coordinates relative to the floor of
    the tight bounds of the finite rows; refusals (ValueError) for |bounds * inv| >= 2^31 and 2^63 voxels or more;
  * a stable lexsort by (z, y, x) voxel coordinate = ascending key with the rows of a voxel in ascending source row;
  * per voxel the sums of the float32 values widened to float64 with math.fsum, i.e. exact and rounded once:
    c_ref = fsum(p) / k, s_ref = fsum(n);
  * per voxel also max_j |p_j| per component and max_j ||n_j||, which the tolerances of the device test are computed
    from (never from device output).
"""
import functools
import math

import numpy as np

EPS = 2.0 ** -53
NONE = 0xFFFFFFFF
STRONG = 1e-3          # a voxel's normal is compared as a vector when |s_ref| >= STRONG k max_j ||n_j||


def voxelize(xyz, nrm, leaf, min_points=0):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    leaf3 = np.broadcast_to(np.asarray(leaf, np.float32), (3,)).astype(np.float32)
    assert np.all(np.isfinite(leaf3)) and np.all(leaf3 > 0) and min_points >= 0
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    out = dict(n=n, num_input=int(fin.size), min_points=min_points)
    if fin.size == 0:
        z3 = np.zeros((0, 3))
        out.update(min_b=[0, 0, 0], dims=[0, 0, 0], rows_sorted=np.zeros(0, np.int64), seg=np.zeros(1, np.int64),
                   counts=np.zeros(0, np.int64), keys=[], c_ref=z3, s_ref=z3, maxp=z3, maxn=np.zeros(0),
                   row_vid=np.full(n, -1, np.int64))
        return _finish(out)
    with np.errstate(over="ignore", invalid="ignore"):
        inv = (np.float32(1.0) / leaf3).astype(np.float32)
        p = xyz[fin]
        lo = (p.min(axis=0) * inv).astype(np.float32)
        hi = (p.max(axis=0) * inv).astype(np.float32)
    if not (np.all(np.abs(lo) < 2.0 ** 31) and np.all(np.abs(hi) < 2.0 ** 31)):
        raise ValueError("voxel coordinates of the bounds leave the int32 range")
    min_b = [int(v) for v in np.floor(lo)]
    max_b = [int(v) for v in np.floor(hi)]
    d = [b - a + 1 for a, b in zip(min_b, max_b)]
    if d[0] * d[1] * d[2] >= 2 ** 63:
        raise ValueError("2^63 voxels or more")
    prod = (p * inv[None, :]).astype(np.float32)               # ONE float32 multiply
    c = np.floor(prod).astype(np.int64) - np.asarray(min_b, np.int64)[None, :]
    assert c.min() >= 0 and np.all(c.max(axis=0) < np.asarray(d))
    perm = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))             # stable; last key is the primary one
    cs = c[perm]
    rows_sorted = fin[perm]
    head = np.ones(fin.size, bool)
    head[1:] = np.any(cs[1:] != cs[:-1], axis=1)
    seg = np.concatenate([np.flatnonzero(head), [fin.size]]).astype(np.int64)
    nv = seg.size - 1
    counts = np.diff(seg)
    keys = [int(a) + d[0] * (int(b) + d[1] * int(e)) for a, b, e in cs[seg[:-1]]]
    assert all(x < y for x, y in zip(keys, keys[1:]))
    p64 = xyz.astype(np.float64)
    n64 = nrm.astype(np.float64)
    c_ref = np.empty((nv, 3))
    s_ref = np.empty((nv, 3))
    maxp = np.empty((nv, 3))
    maxn = np.empty(nv)
    nlen = np.sqrt((n64 * n64).sum(axis=1))
    for v in range(nv):
        r = rows_sorted[seg[v]:seg[v + 1]]
        assert np.all(np.diff(r) > 0)                          # ascending source row inside a voxel
        k = r.size
        for a in range(3):
            c_ref[v, a] = math.fsum(p64[r, a]) / k
            s_ref[v, a] = math.fsum(n64[r, a])
        maxp[v] = np.abs(p64[r]).max(axis=0)
        maxn[v] = nlen[r].max()
    row_vid = np.full(n, -1, np.int64)
    row_vid[rows_sorted] = np.repeat(np.arange(nv), counts)
    out.update(min_b=min_b, dims=d, rows_sorted=rows_sorted, seg=seg, counts=counts, keys=keys, c_ref=c_ref, s_ref=s_ref,
               maxp=maxp, maxn=maxn, row_vid=row_vid)
    return _finish(out)


def _finish(out):
    """the min_points filter, the map and the expected float32 output rows"""
    counts, nv = out["counts"], out["counts"].size
    keep = counts >= out["min_points"]
    out_row = np.cumsum(keep) - 1
    out["keep"] = keep
    out["num_voxels"] = int(nv)
    out["num_output"] = int(keep.sum())
    out["num_dropped_rows"] = int(counts[~keep].sum())
    out["max_points"] = int(counts.max(initial=0))
    rv = np.full(out["n"], NONE, np.uint32)
    has = out["row_vid"] >= 0
    vid = out["row_vid"][has]
    rv[has] = np.where(keep[vid], out_row[vid], NONE).astype(np.uint32)
    out["row_voxel"] = rv
    s = out["s_ref"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        slen = np.sqrt((s * s).sum(axis=1))
        unit = np.where((np.isfinite(slen) & ~(slen < 1e-12))[:, None], s / slen[:, None], 0.0)
    out["slen"] = slen
    out["pos32"] = out["c_ref"].astype(np.float32)
    out["nrm32"] = unit.astype(np.float32)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------- tolerances and voxel classes ----
def pos_tol(ref):
    """per component: one float32 rounding boundary of the mean plus a reordered fp64 sum of k terms and the divide"""
    k = ref["counts"].astype(np.float64)[:, None]
    return 2.0 ** -23 * np.abs(ref["c_ref"]) + 2.0 * k * EPS * ref["maxp"]


def normal_classes(ref):
    """(strong, zero, rest): vectors compared under normal_tol; exactly zero; only finite and zero-or-unit"""
    k = ref["counts"]
    s = ref["s_ref"]
    zero = (ref["maxn"] == 0) | ((k == 2) & np.all(s == 0, axis=1))
    strong = ~zero & np.isfinite(ref["slen"]) & (ref["slen"] >= STRONG * k * ref["maxn"]) & (ref["slen"] >= 1e-9)
    return strong, zero, ~(strong | zero)


def normal_tol(ref):
    """one float32 rounding plus the reordered sums through the normalisation; valid on the strong voxels"""
    k = ref["counts"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 ** -23 + 8.0 * k * EPS * ref["maxn"] / np.maximum(ref["slen"], 1e-300)


def rest_share(ref):
    strong, zero, rest = normal_classes(ref)
    return rest.sum() / max(rest.size, 1)


# --------------------------------------------------------------------------------------------- shared scenes ----
def planes_cloud():
    """tests/normals_ref.planes_cloud() with the normals it was generated with"""
    from pcdhip import synth
    return synth.cloud_planes(20000, seed=1, patches=8)


def uniform_cloud():
    from pcdhip import synth
    return synth.cloud_uniform(4000, seed=3, box=2.0)


PARITY_LEAVES = (0.05, 1.0, (0.05, 0.1, 0.2))


@functools.lru_cache(maxsize=None)
def parity_ref(name, leaf):
    """reference result of a parity cloud at one leaf, computed once per session; shared, read-only"""
    xyz, nrm = planes_cloud() if name == "planes" else uniform_cloud()
    return xyz, nrm, voxelize(xyz, nrm, leaf)


def lattice(spacing, n=10, start=-3):
    """points at (start + i) * spacing computed in float32: on the voxel faces of a leaf equal to the spacing"""
    g = (np.arange(n, dtype=np.float32) + np.float32(start)) * np.float32(spacing)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def straddle_cloud(n=6000, seed=5):
    """uniform in [-0.3, 0.3]^3 with a cluster inside (-leaf, 0) and (0, leaf) on every axis"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.3, 0.3, (n, 3))
    b = rng.uniform(-0.049, 0.049, (n // 4, 3))
    xyz = np.concatenate([a, b, [[-0.01, -0.01, -0.01], [0.0, 0.0, 0.0], [-0.0, 0.01, -0.01]]]).astype(np.float32)
    return xyz, unit_normals(xyz.shape[0], seed + 1)


def unit_normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    v[:, 1] = np.abs(v[:, 1]) + 0.5            # one hemisphere: sums do not cancel
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# segment lengths around every size at which the kernels take another path: the 8-lane group (8) and its 16- and 32-row
# tiers, the short / long threshold (32), one row of the long kernel's lanes (64), the piece (512), a piece and one more
# row of lanes (576), two pieces (1024)
SEGMENT_LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 1023,
                   1024, 1025, 4095, 4096, 4097, 20000)


def segments_cloud(seed=7):
    """voxel v (leaf 1) holds exactly SEGMENT_LENGTHS[v] rows; rows shuffled"""
    rng = np.random.default_rng(seed)
    parts = []
    for v, k in enumerate(SEGMENT_LENGTHS):
        parts.append(np.stack([v + rng.uniform(0.05, 0.95, k), rng.uniform(0.05, 0.95, k),
                               rng.uniform(-0.95, -0.05, k)], axis=1))
    xyz = np.concatenate(parts).astype(np.float32)
    nrm = unit_normals(xyz.shape[0], seed + 1)
    perm = rng.permutation(xyz.shape[0])
    return xyz[perm], nrm[perm]


def sparse_cloud(n=5000, seed=9):
    """sparse points over 100 m: at a 1 cm leaf the keys exceed 2^32"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    xyz[1::2] = xyz[0::2] + np.float32(0.001)          # pairs that mostly share a voxel
    return xyz, unit_normals(n, seed + 1)


def mixed_normals_cloud(seed=13):
    """leaf 1 voxels along x: opposed pairs (exactly zero), zero normals, one-hemisphere sets and free random sets"""
    rng = np.random.default_rng(seed)
    xyz, nrm = [], []

    def voxel(v, k, normals):
        xyz.append(np.stack([v + rng.uniform(0.1, 0.9, k), rng.uniform(0.1, 0.9, k), rng.uniform(0.1, 0.9, k)], axis=1))
        nrm.append(np.asarray(normals, np.float64).reshape(k, 3))
    v = 0
    for _ in range(40):                                  # opposed pairs
        a = rng.normal(0, 1, 3)
        a /= np.linalg.norm(a)
        a = a.astype(np.float32).astype(np.float64)
        voxel(v, 2, [a, -a])
        v += 1
    for k in (1, 3, 70):                                 # zero normals
        voxel(v, k, np.zeros((k, 3)))
        v += 1
    for k in (1, 2, 5, 9, 40, 100, 700):                 # one hemisphere
        voxel(v, k, unit_normals(k, seed + v))
        v += 1
    for _ in range(250):                                 # free directions: |s| ~ sqrt(k)
        k = int(rng.integers(20, 80))
        a = rng.normal(0, 1, (k, 3))
        voxel(v, k, a / np.linalg.norm(a, axis=1, keepdims=True))
        v += 1
    for k in (3, 30):                                    # zero normals mixed with real ones: they add nothing
        a = unit_normals(k, seed + v).astype(np.float64)
        a[::2] = 0
        voxel(v, k, a)
        v += 1
    return np.concatenate(xyz).astype(np.float32), np.concatenate(nrm).astype(np.float32)


def reference_scenes():
    """every (name, xyz, nrm, leaf) whose vectors a device test compares: the clouds the 1 % cap is a condition on"""
    scenes = []
    for name in ("planes", "uniform"):
        xyz, nrm = planes_cloud() if name == "planes" else uniform_cloud()
        for leaf in PARITY_LEAVES:
            scenes.append(("%s@%s" % (name, leaf), xyz, nrm, leaf))
    scenes.append(("straddle", *straddle_cloud(), 0.05))
    scenes.append(("segments", *segments_cloud(), 1.0))
    scenes.append(("sparse", *sparse_cloud(), 0.01))
    scenes.append(("mixed", *mixed_normals_cloud(), 1.0))
    return scenes

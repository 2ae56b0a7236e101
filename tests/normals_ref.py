"""numpy reference of the radius-PCA normal estimation (pcd_cloud_estimate_normals, definition in include/pcdhip.h),
written from the definition alone:

  * neighbour predicate in float32, the operation order of csrc/grid.h l2_simple3: d = p_i - p_j, ((dx*dx) + dy*dy) +
    dz*dz <= float32(r) * float32(r); chunked brute force over the finite rows; i itself and duplicates count;
  * the float32 differences widened to float64, m = S1 / k, C = S2 / k - m m^T, np.linalg.eigh;
  * no normal for k < max(min_neighbors, 3), l2 == 0, l1 <= 1e-10 l2 and rows with a non-finite coordinate;
  * orientation towards the viewpoint, evaluated in float64; a dot product of exactly 0 or ORIENT_NONE: the component of
    largest magnitude is positive (ties: lowest axis);
  * per row also gap = (l1 - l0) / l2, which the tolerances of the device test are computed from.
"""
import functools

import numpy as np

ORIENT_NONE, ORIENT_VIEWPOINT = 0, 1
EPS = 2.0 ** -53


def _d2(a, b):
    """float32 l2_simple3 of every row of a [A,3] against every row of b [B,3]"""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    r = dx * dx
    r = r + dy * dy
    r = r + dz * dz
    return r


def pairs_bruteforce(xyz, radii, chunk=512):
    """for each radius the (i, j) pairs with j in N_i, i ascending and j ascending inside i: list of (I, J) arrays"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    p = xyz[fin]
    r2 = [np.float32(r) * np.float32(r) for r in radii]
    out = [([], []) for _ in radii]
    for s in range(0, p.shape[0], chunk):
        d2 = _d2(p[s:s + chunk], p)
        for k, t in enumerate(r2):
            ii, jj = np.nonzero(d2 <= t)
            out[k][0].append(fin[ii + s])
            out[k][1].append(fin[jj])
    return [(np.concatenate(a) if a else np.zeros(0, np.int64), np.concatenate(b) if b else np.zeros(0, np.int64))
            for a, b in out]


def pairs_kdtree(xyz, r):
    """the same pairs from scipy.spatial.cKDTree candidates (a slightly larger float64 ball) filtered by the float32
    predicate"""
    from scipy.spatial import cKDTree
    xyz = np.ascontiguousarray(xyz, np.float32)
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    p = xyz[fin]
    tree = cKDTree(p.astype(np.float64))
    cand = tree.query_ball_point(p.astype(np.float64), float(r) * (1 + 1e-5) + 1e-12, return_sorted=True)
    I = np.repeat(np.arange(p.shape[0]), [len(c) for c in cand])
    J = np.concatenate([np.asarray(c, np.int64) for c in cand]) if len(I) else np.zeros(0, np.int64)
    d = p[I] - p[J]
    d2 = d[:, 0] * d[:, 0]
    d2 = d2 + d[:, 1] * d[:, 1]
    d2 = d2 + d[:, 2] * d[:, 2]
    keep = d2 <= np.float32(r) * np.float32(r)
    return fin[I[keep]], fin[J[keep]]


def from_pairs(xyz, I, J, min_neighbors=3, orient=ORIENT_VIEWPOINT, viewpoint=(0.0, 0.0, 0.0), perm=None):
    """moments, eigen-decomposition, rules and orientation from the neighbour pairs.  perm: a permutation of the pair
    list, i.e. another summation order of every row's moments"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    if perm is not None:
        I, J = I[perm], J[perm]
    d = (xyz[I] - xyz[J]).astype(np.float64)            # the float32 differences, widened
    k = np.bincount(I, minlength=n).astype(np.int64)
    s1 = np.stack([np.bincount(I, d[:, a], minlength=n) for a in range(3)], axis=1)
    s2 = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            s2[:, a, b] = s2[:, b, a] = np.bincount(I, d[:, a] * d[:, b], minlength=n)
    kk = np.maximum(k, 1).astype(np.float64)
    m = s1 / kk[:, None]
    C = s2 / kk[:, None, None] - m[:, :, None] * m[:, None, :]
    lam, vec = np.linalg.eigh(C)
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    too_few = k < max(min_neighbors, 3)
    finite = np.isfinite(xyz).all(axis=1)
    too_few &= finite
    degenerate = finite & ~too_few & ((l2 == 0) | (l1 <= 1e-10 * l2))
    ok = finite & ~too_few & ~degenerate
    nrm = vec[:, :, 0].copy()
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    w = np.asarray(viewpoint, np.float32).astype(np.float64)[None, :] - xyz.astype(np.float64)
    w[~finite] = 0
    dot = (nrm[:, 0] * w[:, 0] + nrm[:, 1] * w[:, 1]) + nrm[:, 2] * w[:, 2]
    big = nrm[np.arange(n), np.argmax(np.abs(nrm), axis=1)]     # argmax: first of equal magnitudes
    by_view = (dot != 0) if orient == ORIENT_VIEWPOINT else np.zeros(n, bool)
    flip = np.where(by_view, dot < 0, big < 0)
    nrm[flip] = -nrm[flip]
    nrm[~ok] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where(ok, l0 / ((l0 + l1) + l2), 0.0)
        gap = np.where(ok, (l1 - l0) / l2, 0.0)
        rank = np.where(finite & ~too_few & (l2 > 0), l1 / l2, np.inf)
        wn = np.linalg.norm(w, axis=1)
        dot_rel = np.where(ok & (wn > 0), np.abs(dot) / np.maximum(wn, 1e-300), 0.0)
    return dict(count=np.where(finite, k, 0).astype(np.uint32), curvature=curv, normal=nrm, gap=gap, lam=lam, ok=ok,
                too_few=too_few, degenerate=degenerate, finite=finite, rank=rank, dot_rel=dot_rel)


def estimate(xyz, r, **kw):
    I, J = pairs_bruteforce(xyz, [r])[0]
    return from_pairs(xyz, I, J, **kw)


# ------------------------------------------------------------- tolerances (from the reference's own k and gap) ----
GAP_MIN = 1e-3


def curvature_tol(ref):
    """eigenvalue perturbation under a reordered fp64 sum of k terms, relative to the trace"""
    return 64.0 * ref["count"].astype(np.float64) * EPS


def normal_tol(ref):
    """one float rounding plus Davis-Kahan; valid on the rows with gap >= GAP_MIN"""
    with np.errstate(divide="ignore"):
        return 2.0 ** -23 + 128.0 * ref["count"].astype(np.float64) * EPS / np.maximum(ref["gap"], 1e-300)


# ------------------------------------------------------------------------------------------- shared scenes ----
def planes_cloud():
    from pcdhip import synth
    return synth.cloud_planes(20000, seed=1, patches=8)[0]


def uniform_cloud():
    from pcdhip import synth
    return synth.cloud_uniform(4000, seed=3, box=2.0)[0]


PLANES_RADII = (0.08, 0.2, 0.5)      # with cell_size 0.2: below one cell, exactly one cell, 2.5 cells
UNIFORM_RADII = (0.25,)              # with cell_size 0.1 (reach of 3 cells) and 0.3


@functools.lru_cache(maxsize=None)
def parity_pairs(name):
    """neighbour pairs of a parity cloud at each of its radii, computed once per session: {radius: (I, J)}"""
    xyz, radii = (planes_cloud(), PLANES_RADII) if name == "planes" else (uniform_cloud(), UNIFORM_RADII)
    return xyz, dict(zip(radii, pairs_bruteforce(xyz, radii)))


@functools.lru_cache(maxsize=None)
def parity_ref(name, r):
    """reference result of a parity cloud (viewpoint (0,0,0), min_neighbors 3); shared, read-only"""
    xyz, pairs = parity_pairs(name)
    ref = from_pairs(xyz, *pairs[r])
    for v in ref.values():
        v.setflags(write=False)
    return xyz, ref


def lattice(n=12, spacing=0.125, offset=0.5):
    g = np.arange(n, dtype=np.float64) * spacing + offset
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def plane_lattice(n=40, spacing=0.03125, z=0.375):
    g = np.arange(n, dtype=np.float64) * spacing
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    return np.concatenate([xy, np.full((n * n, 1), z)], axis=1).astype(np.float32)


def patch5(spacing=0.02, at=(1.0, 1.0, 1.0)):
    """a 5 x 5 planar patch (z constant)"""
    g = np.arange(5, dtype=np.float64) * spacing
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    return (np.concatenate([xy, np.zeros((25, 1))], axis=1) + np.asarray(at)).astype(np.float32)


def degenerate_scenes():
    """(name, xyz, radius, min_neighbors, expected (estimated, too_few, degenerate), rows that must have no normal)"""
    one = np.array([[1.0, 1.0, 1.0]], np.float32)
    line = np.arange(50, dtype=np.float64)[:, None] * 0.01
    along_x = (np.array([[1.0, 1.0, 1.0]]) + line * np.array([[1.0, 0.0, 0.0]])).astype(np.float32)
    t = (1.0 + 0.01 * np.arange(50)).astype(np.float32)
    diagonal = np.stack([t, t, t], axis=1)
    patch = patch5()
    every = lambda a: np.arange(a.shape[0])
    scenes = [
        ("one_point", one, 0.1, 3, (0, 1, 0), every(one)),
        ("two_points", np.array([[1, 1, 1], [1.05, 1, 1]], np.float32), 0.1, 3, (0, 2, 0), np.arange(2)),
        ("coincident", np.repeat(one, 5, axis=0), 0.1, 3, (0, 0, 5), np.arange(5)),
        ("collinear_x", along_x, 0.05, 3, (0, 0, 50), every(along_x)),
        ("collinear_diagonal", diagonal, 0.05, 3, (0, 0, 50), every(diagonal)),
        ("isolated", np.concatenate([patch, np.array([[3.0, 1.0, 1.0]], np.float32)]), 0.1, 3, (25, 1, 0),
         np.array([25])),
        ("inf_row", np.concatenate([patch, np.array([[np.inf, 1.0, 1.0]], np.float32)]), 0.1, 3, (25, 0, 0),
         np.array([25])),
        ("min_neighbors", patch, 0.025, 10, (0, 25, 0), every(patch)),
    ]
    return scenes

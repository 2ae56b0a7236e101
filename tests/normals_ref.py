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


# ------------------------------------------------------------------- the grid as the device lays it out ----
def kept_mask(nrm):
    """only_missing keeps a stored normal iff the float64 norm of its widened floats is >= 1e-6 (a NaN: no)"""
    w = np.ascontiguousarray(nrm, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        return norm >= 1e-6                                  # NaN compares false


def grid_info(xyz, cell_size):
    """what pcd_cloud_get_info reports for a handle that keeps the user's cell size (cloud.hip set_dims): the CPU
    tests' stand-in for c.info()"""
    p = np.ascontiguousarray(xyz, np.float32)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = p.min(axis=0), p.max(axis=0)
    h = np.float32(cell_size)
    e = hi.astype(np.float64) - lo.astype(np.float64)
    dims = np.maximum(np.floor(e / np.float64(h)).astype(np.int64) + 1, 1)
    return dict(cell_size=float(h), origin=[float(v) for v in lo], dims=[int(v) for v in dims],
                bbox_lo=[float(v) for v in lo], bbox_hi=[float(v) for v in hi], num_indexed=int(p.shape[0]))


def range_table_geometry(xyz, info, r):
    """The range tables k_normals_brick builds, from a handle's info (dims, origin, cell_size), the cloud and the
    radius: float32 binning as grid.h cell_coord, the slack of cloud.hip set_dims, the reach of normals.hip.  Per
    occupied leaf (x pair, y quad, z quad): nrows and the points of every quad row of its window in table order
    (row = iy + ny * iz, x clipped to [2 sx - R, 2 sx + 2 + R)).  For asserting that a scene reaches the branch it is
    about; never for predicting device output."""
    f32 = np.float32
    p = np.ascontiguousarray(xyz, f32)
    p = p[np.isfinite(p).all(axis=1)]
    o, h, dims = np.asarray(info["origin"], f32), f32(info["cell_size"]), np.asarray(info["dims"], np.int64)
    lo, hi = o, p.max(axis=0)
    ext = f32(0)
    for d in range(3):
        ext = max(ext, f32(np.float64(hi[d]) - np.float64(lo[d])), abs(lo[d]), abs(hi[d]))
    slack = f32(f32(ext) * f32(9.6e-7) + f32(1e-30))
    rf = float(f32(r))
    R = int(np.floor((rf * (1.0 + 1e-5) + 2.0 * float(slack)) / float(h))) + 1
    R_noslack = int(np.floor(rf * (1.0 + 1e-5) / float(h))) + 1
    Rq = (R + 1) // 2
    inv_h = f32(1) / h
    t = np.floor(((p - o).astype(f32) * inv_h).astype(f32))
    c = np.clip(t, 0, (dims - 1).astype(f32)).astype(np.int64)
    qd = (dims[1:] + 1) // 2
    hist = np.zeros((qd[1], qd[0], dims[0] + 1), np.int64)              # [zq, yq, 1 + cx]
    np.add.at(hist, (c[:, 2] // 2, c[:, 1] // 2, c[:, 0] + 1), 1)
    cum = np.cumsum(hist, axis=2)                                       # cum[.., x] = points with cx < x
    leaves = np.unique(np.stack([c[:, 0] // 2, c[:, 1] // 2, c[:, 2] // 2], axis=1), axis=0)
    nrows, rows = [], []
    for sx, sy, sz in leaves:
        cx0, cx1 = max(2 * sx - R, 0), min(2 * sx + 2 + R, dims[0])
        y0, y1 = max(sy - Rq, 0), min(sy + Rq, qd[0] - 1)
        z0, z1 = max(sz - Rq, 0), min(sz + Rq, qd[1] - 1)
        w = cum[z0:z1 + 1, y0:y1 + 1, cx1] - cum[z0:z1 + 1, y0:y1 + 1, cx0]
        rows.append(w.ravel())                                          # iz-major: row = iy + ny * iz
        nrows.append(w.size)
    return dict(R=R, Rq=Rq, R_noslack=R_noslack, slack=float(slack), leaves=leaves, nrows=np.asarray(nrows, np.int64),
                rows=rows)


# ------------------------------------------------------------------------------- the edge scenes ----
def _thin_sheet(n, seed):
    """n points of a thin sheet inside one cell of 0.5 (test_dense_brick's, smaller)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.05, 0.45, n), rng.uniform(0.05, 0.45, n), 0.25 + rng.normal(0, 0.002, n)],
                    axis=1).astype(np.float32)


def _near_line(jitter, seed):
    rng = np.random.default_rng(seed)
    x = 1.0 + 0.01 * np.arange(60)
    return np.stack([x, 1.0 + rng.normal(0, jitter, 60), 1.0 + rng.normal(0, jitter, 60)], axis=1).astype(np.float32)


TAIL_SIZES = (63, 64, 65, 255, 256, 257, 258, 513)
NEAR_LINE_JITTER = (1e-5, 1e-4)
FAR_VIEWPOINT = (4001.0, -2499.0, 300.5)


def _wide_dense():
    return (np.random.default_rng(31).random((3000, 3)) * np.array([0.3, 3.2, 2.9])).astype(np.float32)


def _wide_sparse():
    """two sheets in wide_dense's box, z in [0, 0.2] and [2.7, 2.9]; the upper one has no point with y in [0.75, 1.25),
    two y quads whose rows are empty in the tables of the leaves around them"""
    rng = np.random.default_rng(32)
    low = rng.random((600, 3)) * np.array([0.3, 3.2, 0.2])
    high = rng.random((600, 3)) * np.array([0.3, 2.7, 0.2]) + np.array([0.0, 0.0, 2.7])
    high[:, 1] += np.where(high[:, 1] >= 0.75, 0.5, 0.0)
    return np.concatenate([low, high]).astype(np.float32)


def _far():
    return (np.random.default_rng(0).random((3000, 3)) * np.array([2.0, 2.0, 1.0])
            + np.array([4000.0, -2500.0, 300.0])).astype(np.float32)


def _wide_extent():
    rng = np.random.default_rng(34)
    a = rng.random((1500, 3)) + np.array([-2000.0, 0.0, 0.0])
    b = rng.random((1500, 3)) + np.array([2000.0, 0.0, 0.0])
    return np.concatenate([a, b]).astype(np.float32)


def reach_refusal_cloud():
    """a 2 m cube at 1e5 on every axis (the slack is a whole cell of 0.1) and one Inf row, the last"""
    p = np.random.default_rng(35).random((2000, 3)) * 2.0 + 1e5
    return np.concatenate([p, np.array([[np.inf, 1e5, 1e5]])]).astype(np.float32)


def only_missing_scene():
    """(xyz, stored normals): patch5 with the seven stored normals of the ||n|| >= 1e-6 rule in turn, then two rows
    with an Inf coordinate, one with a unit normal and one with none"""
    tiny = np.float32(1e-6)                               # widens to 9.99999997e-7: below the threshold
    above = np.nextafter(tiny, np.float32(1))             # the next float: at least 1e-6
    assert float(tiny) < 1e-6 <= float(above)
    stored = np.array([[0, 0, 0], [9e-7, 0, 0], [tiny, 0, 0], [above, 0, 0], [1e-3, 0, 0], [1, np.nan, 0],
                       [np.inf, 0, 0]], np.float32)
    xyz = np.concatenate([patch5(), np.array([[np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0]], np.float32)])
    nrm = np.concatenate([stored[np.arange(25) % 7], np.array([[0, 0, 1], [0, 0, 0]], np.float32)])
    return xyz, nrm


# name -> (cloud, cell_size, radius, options of the estimate, compare vectors, expected (estimated, too few,
# degenerate, min k, max k) of the reference)
def _edge_table():
    t = {
        "wide_dense": (_wide_dense, 0.125, 1.0, {}, True, (3000, 0, 0, 262, 1058)),
        "wide_dense_r7": (_wide_dense, 0.125, 0.875, {}, True, (3000, 0, 0, 199, 823)),
        "wide_sparse": (_wide_sparse, 0.125, 1.0, {}, True, (1200, 0, 0, 170, 430)),
        "far": (_far, 0.1, 0.199, dict(viewpoint=FAR_VIEWPOINT), True, (3000, 0, 0, 4, 46)),
        "wide_extent": (_wide_extent, 0.1, 0.199, {}, True, (3000, 0, 0, 7, 76)),
        "reach_0.7": (reach_refusal_cloud, 0.1, 0.7, {}, True, (2000, 0, 0, 59, 394)),
        "tie_plane": (lambda: plane_lattice(n=9, spacing=0.125, z=0.0), 0.1, 0.3, {}, True, (81, 0, 0, 8, 21)),
        "only_missing": (lambda: only_missing_scene()[0], 0.1, 0.1, {}, True, (25, 0, 0, 22, 25)),
    }
    for j in NEAR_LINE_JITTER:      # the eigenvectors of l0 and l1 are free (no gap): counts, classes, curvature, norms
        t["near_line_%g" % j] = (functools.partial(_near_line, j, 41), 0.1, 0.055, {}, False, (60, 0, 0, 6, 11))
    for n in TAIL_SIZES:            # every point is a neighbour of some query: max k is not pinned, min k >= 10 is
        t["tail_%d" % n] = (functools.partial(_thin_sheet, n, 50 + n), 0.5, 0.3, {}, True, (n, 0, 0, None, None))
    return t


EDGE_SCENES = tuple(_edge_table())


@functools.lru_cache(maxsize=None)
def edge_scene(name):
    """(xyz, cell_size, radius, options, vectors, expected) of an edge scene; xyz is shared and read-only"""
    make, cell, r, opts, vectors, expect = _edge_table()[name]
    xyz = make()
    xyz.setflags(write=False)
    return xyz, cell, r, opts, vectors, expect


@functools.lru_cache(maxsize=None)
def edge_pairs(name):
    xyz, _, r = edge_scene(name)[:3]
    I, J = pairs_bruteforce(xyz, [r])[0]
    I.setflags(write=False)
    J.setflags(write=False)
    return I, J


@functools.lru_cache(maxsize=None)
def edge_ref(name):
    """reference result of an edge scene with its own options; computed once per session, read-only"""
    xyz, _, _, opts = edge_scene(name)[:4]
    ref = from_pairs(xyz, *edge_pairs(name), **opts)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def orient_none_ref():
    """the uniform parity cloud at r = 0.25 without a viewpoint: (xyz, reference), shared and read-only"""
    xyz, pairs = parity_pairs("uniform")
    ref = from_pairs(xyz, *pairs[0.25], orient=ORIENT_NONE)
    for v in ref.values():
        v.setflags(write=False)
    return xyz, ref


def orient_none_sure(ref):
    """rows where ORIENT_NONE's sign is decided: the reference's largest component exceeds the runner-up in magnitude by
    more than twice the row's normal tolerance, so no admissible device vector can have another largest component"""
    a = np.sort(np.abs(ref["normal"]), axis=1)
    return ref["ok"] & (a[:, 2] - a[:, 1] > 2.0 * normal_tol(ref))

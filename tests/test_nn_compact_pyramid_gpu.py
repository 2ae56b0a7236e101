"""k_nn_fallback on the compact pyramid (cloud.h: blk_aabb holds a 64-ary tree over the OCCUPIED nodes only).

The compaction keeps the children of a node contiguous and in the order of their lane in the dense 4x4x4 lattice, so
the walk visits the same nodes in the same order as on the dense lattice.  Two kinds of check:

  exactness   index, distance bits and found flag against brute force, through every form of the walk, on clouds
              built with an explicit cell size so that the shape of the tree is pinned (every cloud below asserts the
              child counts it is meant to produce, from a numpy restatement of the lattice);
  same walk   the number of walked queries and of scanned leaf points equals what the dense-lattice kernel of the
              parent commit counted on the same input (constants below).

Points sit at (cell + 0.5 + [0, 0.4)) * h with the cell's exact centre as its first point, and every axis has a point
in cell 0: the grid's origin is 0.5 h, binning is exact and dims = the largest cell index + 1.
"""
import numpy as np
import pytest

from tests.test_nn_fallback_bounds_gpu import _check, _tilted_planes, _queries

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- clouds ----
def _cells_cloud(cells, h, seed, per=3):
    """`per` points in every listed cell: the centre first, then jittered towards the cell's upper corner"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.float64)
    pts = [(cells + 0.5) * h]
    for _ in range(per - 1):
        pts.append((cells + 0.5 + rng.uniform(0, 0.4, cells.shape)) * h)
    xyz = np.stack(pts, 1).reshape(-1, 3).astype(np.float32)
    return xyz[rng.permutation(len(xyz))]


def _child_counts(xyz, h):
    """numpy restatement of the lattice (cloud.hip build_lattice with a user cell size): per real level above the
    leaves the sorted list of the number of occupied children of every occupied node, top level last; and the number
    of occupied nodes of the top real level (= the children of the virtual top)"""
    lo = xyz.min(0)
    ext = xyz.max(0).astype(np.float64) - lo.astype(np.float64)
    dims = np.floor(ext / h).astype(np.int64) + 1
    cell = np.clip(np.floor((xyz - lo) * (np.float32(1.0) / np.float32(h))).astype(np.int64), 0, dims - 1)
    node = np.unique(cell >> 1, axis=0)
    d = (dims + 1) // 2
    levels = []
    while np.prod(d) > 64:
        parent, cnt = np.unique(node >> 2, axis=0, return_counts=True)
        levels.append(sorted(cnt.tolist()))
        node, d = parent, (d + 3) // 4
    return levels, len(node)


def _cloud_single():
    return np.float32([[3.25, -1.5, 7.0]]), 1.0


def _cloud_twin():
    return np.float32([[3.25, -1.5, 7.0], [3.25, -1.5, 7.0]]), 1.0


def _cloud_block(cells_per_edge):
    g = np.stack(np.meshgrid(*[np.arange(cells_per_edge)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return _cells_cloud(g, 0.5, 3, per=2), 0.5


def _cloud_ragged():
    """leaf lattice 5 x 3 x 9 (cells 10 x 6 x 18), one real inner level of 2 x 1 x 3 parents; the parents at the
    ragged edges hold 12, 3, 2 and 1 occupied leaves, the two full ones a random half of their 48"""
    rng = np.random.default_rng(5)
    leaves = []
    for lz in range(9):
        for ly in range(3):
            for lx in range(5):
                px, pz = lx >> 2, lz >> 2
                if (px, pz) == (1, 0) or (px, pz) == (1, 2):      # 12 and 3 possible: all occupied
                    keep = True
                elif (px, pz) == (1, 1):                           # 12 possible: two
                    keep = (lx, ly, lz) in ((4, 0, 4), (4, 2, 7))
                elif (px, pz) == (0, 2):                           # 12 possible: one
                    keep = (lx, ly, lz) == (2, 1, 8)
                else:                                              # 48 possible each
                    keep = (lx, ly, lz) == (0, 0, 0) or rng.random() < 0.5
                if keep:
                    leaves.append((lx, ly, lz))
    leaves = np.array(leaves)
    cells = 2 * leaves + rng.integers(0, 2, leaves.shape)
    cells[(leaves == (0, 0, 0)).all(1)] = (0, 0, 0)
    cells[(leaves == (4, 2, 8)).all(1)] = (9, 5, 17)
    return _cells_cloud(cells, 0.5, 6), 0.5


def _cloud_corners():
    """cells 16 x 8 x 8 = leaves 8 x 4 x 4, two parents: one whose only child is lane 0 (leaf (0,0,0)), one whose only
    child is lane 63 (leaf (7,3,3) = (3,3,3) inside the second parent)"""
    return _cells_cloud([(0, 0, 0), (15, 7, 7)], 0.5, 7, per=1), 0.5


def _cloud_clusters():
    """two clusters of 200 points 60 m apart along the diagonal at h = 0.25: leaves ~70^3, four real levels, nearly all
    subtrees empty"""
    rng = np.random.default_rng(8)
    a = rng.uniform(0, 0.75, (200, 3))
    a[0] = 0.0
    b = 60.0 / np.sqrt(3.0) + rng.uniform(0, 0.75, (200, 3))
    return np.concatenate([a, b]).astype(np.float32), 0.25


def _cloud_lattice():
    """unit lattice 17 x 9 x 9 in shuffled index order (cells = points, leaves 9 x 5 x 5, parents 3 x 2 x 2)"""
    rng = np.random.default_rng(9)
    g = np.stack(np.meshgrid(np.arange(17), np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 3)
    return g[rng.permutation(len(g))].astype(np.float32), 1.0


def _q(xyz, n, seed):
    """near the points, in the (mostly empty) box, outside the grid on every side near and far"""
    rng = np.random.default_rng(seed)
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1.0)
    k = n // 4
    near = xyz[rng.integers(0, len(xyz), k)].astype(np.float64) + rng.normal(0, 0.3, (k, 3))
    box = lo + rng.random((k, 3)) * ext
    out = lo - ext + rng.random((k, 3)) * 3 * ext
    far = lo - 10 * ext + rng.random((n - 3 * k, 3)) * 21 * ext
    return np.concatenate([near, box, out, far])


def _lattice_queries():
    """midpoints of the lattice's edges and faces (exact ties between 2 and 4 points, across leaf and parent
    boundaries: x = 7.5 separates two level-1 parents) and the same one lattice step outside the grid"""
    rng = np.random.default_rng(10)
    base = rng.integers(-1, 18, (2000, 3)).astype(np.float64)
    base[:, 1:] = rng.integers(-1, 10, (2000, 2))
    off = np.array([[.5, 0, 0], [0, .5, 0], [0, 0, .5], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])[rng.integers(0, 6, 2000)]
    q = base + off
    q[:200, 0] = 7.5     # the parents' boundary
    return q


# name -> (builder, expected child counts per level above the leaves, children of the virtual top)
CASES = {
    "single": (_cloud_single, [], 1),
    "twin": (_cloud_twin, [], 1),
    "block8": (lambda: _cloud_block(8), [], 64),                 # the virtual top over 4x4x4 leaves, every lane live
    "block16": (lambda: _cloud_block(16), [[64] * 8], 8),        # inner nodes with count == 64
    "ragged": (_cloud_ragged, None, 6),
    "corners": (_cloud_corners, [[1, 1]], 2),
    "clusters": (_cloud_clusters, None, 2),
    "lattice": (_cloud_lattice, None, 12),
}

_memo = {}


def _case(name, oracle):
    """cloud, normals, cell size, queries and the brute-force result: computed once per session, never modified"""
    if name not in _memo:
        xyz, h = CASES[name][0]()
        q = _lattice_queries() if name == "lattice" else _q(xyz, 2000, 40 + len(name))
        nrm = np.tile(np.float32([0, 1, 0]), (len(xyz), 1))
        _memo[name] = (xyz, nrm, h, q, oracle.nn_bruteforce(xyz, q))
        for a in _memo[name][:2] + (q,) + _memo[name][4]:
            a.setflags(write=False)
    return _memo[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_shape_is_pinned(oracle, name):
    """the cloud produces the tree the case is about (numpy restatement, no device work)"""
    xyz, _, h, _, _ = _case(name, oracle)
    levels, ntop = _child_counts(xyz, h)
    want, want_top = CASES[name][1:]
    assert ntop == want_top, (levels, ntop)
    if want is not None:
        assert levels == want, levels
    if name == "ragged":
        assert len(levels) == 1 and {1, 2, 3, 12} <= set(levels[0]) and len(levels[0]) == 6, levels
    if name == "clusters":
        assert levels == [[8, 8], [1, 1], [1, 1]], levels      # four real levels, two chains of single children
    if name == "lattice":
        assert len(levels) == 1 and max(levels[0]) == 64, levels


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_every_form(gpu, oracle, name):
    """one-launch form <1>, the grid path's second stage <0> and the automatic choice"""
    xyz, nrm, h, q, exp = _case(name, oracle)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=h)
    try:
        for algo in ("FALLBACK_ONLY", "GRID", "AUTO"):
            _check(c.nn(q, getattr(gpu, "NN_" + algo)), exp, f"{name}/{algo}")
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_gate_bounded_one_launch(gpu, oracle, name):
    """the gate-bounded one-launch form <2>: association = unbounded search + the gate"""
    xyz, nrm, h, q, (idx, sq, found) = _case(name, oracle)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=h)
    try:
        out = c.associate(q, 1.5, gpu.GATE_MAPPER_LOCAL)
    finally:
        c.close()
    out6, ok = oracle.search_nearest_neibor(xyz, nrm, idx, found)
    _, typ, _, _, _ = oracle.associate(q, out6, ok, 1.5, 0)
    assert np.array_equal(out["type"], typ)
    hit = typ != 0
    assert hit.any()
    assert np.array_equal(out["nn_idx"][hit], idx[hit])
    assert np.array_equal(out["nn_sqdist"][hit].view(np.uint32), sq[hit].view(np.uint32))


def test_empty_cloud_not_found(gpu):
    z3 = np.zeros((0, 3), np.float32)
    q = _q(np.float32([[0, 0, 0], [1, 1, 1]]), 2000, 50)
    c = gpu.Cloud(z3, z3, raw_lidar_frame=False, cell_size=0.5)
    try:
        for algo in ("FALLBACK_ONLY", "GRID", "AUTO"):
            idx, _, found = c.nn(q, getattr(gpu, "NN_" + algo))
            assert not found.any() and (idx == 0xFFFFFFFF).all(), algo
    finally:
        c.close()


# ------------------------------------------------------- the same walk ----
# fallback_queries / fallback_points of a NN_FALLBACK_ONLY call with the statistics on, measured on the dense-lattice
# kernel of the parent commit af34c7d ("Add a blocked fp64 Cholesky solve of the reduced camera system") with
#     python tools/fb_walk_counts.py
# run on a checkout of that commit with this file and the script added (the script imports the inputs below from this
# file).  Equality is exact: same nodes, same order.
PARENT_WALK = {
    "ragged": (2000, 7071),
    "clusters": (2000, 80190),
    "tilted_planes": (3000, 1266224),
}


def walk_input(name, oracle=None):
    """(xyz, cell size or 0, queries) of a same-walk case"""
    if name == "tilted_planes":
        xyz = _tilted_planes(30000, 11)
        return xyz, 0.0, _queries(xyz, 3000, 12)
    xyz, h = CASES[name][0]()
    return xyz, h, _q(xyz, 2000, 40 + len(name))


def walk_counts(gpu, name):
    xyz, h, q = walk_input(name)
    c = gpu.Cloud(xyz, np.zeros_like(xyz), raw_lidar_frame=False, cell_size=h)
    try:
        gpu.set_nn_tuning(0, -1, 1)
        c.nn(q, gpu.NN_FALLBACK_ONLY)
        st = c.last_stats()
    finally:
        gpu.set_nn_tuning(0, -1, 0)
        c.close()
    return st["fallback_queries"], st["fallback_points"]


@pytest.mark.parametrize("name", sorted(PARENT_WALK))
def test_walk_is_the_parents_walk(gpu, name):
    got = walk_counts(gpu, name)
    print(name, "fallback_queries, fallback_points =", got)
    assert got == PARENT_WALK[name], (got, PARENT_WALK[name])

"""The cloud build of csrc/cloud.hip against the plain restatement of tests/cloud_ref.py: everything
pcd_cloud_get_info reports, on clouds that stress the bounding box, the cell-size rule and its cell budget, the
layouts and the row filter -- and the exactness of every search algorithm on top of those builds, at the launch-shape
boundaries of the build and search kernels.  Bit-exact throughout; the one tolerance is the relative 1e-6 between the
reported cell size and the host rule restated in numpy (double arithmetic rounded to float: a last-ulp difference of
cbrt between the two maths libraries and nothing more)."""
import functools

import numpy as np
import pytest

from pcdhip import synth
from tests import cloud_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
CELL_SIZES = (0.0, 0.05, 0.3, 2.0, 50.0)
MAX_CELLS = 1 << 26
SMALL_BATCH = 65536      # nn.hip kSmallBatch


def _algos(gpu):
    return (("auto", gpu.NN_AUTO), ("bruteforce", gpu.NN_BRUTEFORCE), ("fallback", gpu.NN_FALLBACK_ONLY),
            ("grid", gpu.NN_GRID))


def _exact(got, exp, what):
    for x, y, n in zip(got, exp, ("idx", "sqdist", "found")):
        xv = x.view(np.uint32) if x.dtype == np.float32 else x
        yv = y.view(np.uint32) if y.dtype == np.float32 else y
        bad = np.nonzero(xv != yv)[0]
        assert bad.size == 0, f"{what}: {n} differs at {bad[:5]}: {x[bad[:5]]} vs {y[bad[:5]]}"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _normals(n, seed=1):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _raw_transform(xyz, nrm):
    """ply.cc:38-54 in numpy: rows with a NaN in any of the six values dropped, (x,y,z) -> (-y,-z,x)"""
    keep = ~(np.isnan(xyz).any(axis=1) | np.isnan(nrm).any(axis=1))
    f = lambda a: np.stack([-a[:, 1], -a[:, 2], a[:, 0]], axis=1).astype(F)
    return f(xyz[keep]), f(nrm[keep])


def outlier_cloud():
    """a body of 50 k points in 20 m and two stray returns 100 km away on different axes"""
    rng = np.random.default_rng(31)
    xyz = (rng.random((50002, 3)) * [20, 6, 20]).astype(F)
    xyz[20000] = [1e5 + 3, 2, 7]
    xyz[40000] = [5, -1e5, 11]
    return xyz


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """name -> (input xyz, input nrm, raw_lidar_frame, cloud in the handle's frame, its normals)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    raw = False
    if name == "uniform":
        xyz = (rng.random((20000, 3)) * [12, 4, 12]).astype(F)
    elif name == "planes":
        xyz = synth.cloud_planes(30000, seed=4, patches=16)[0]
    elif name == "line":
        xyz = np.stack([np.linspace(-3, 40, 5000), np.full(5000, 0.5), np.full(5000, -1.0)], axis=1).astype(F)
    elif name == "one point":
        xyz = np.array([[1.5, -2.25, 3.0]], F)
    elif name == "two points":
        xyz = np.array([[1.5, -2.25, 3.0], [1.5, 4.0, 3.5]], F)
    elif name == "identical":
        xyz = np.repeat(np.array([[7.1, 0.3, -2.2]], F), 1000, axis=0)
    elif name == "lattice":       # rows ON the cell faces of h = 0.3 (in float: 0.3f * k)
        g = np.stack(np.meshgrid(np.arange(12), np.arange(11), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3)
        xyz = (g.astype(F) * F(0.3)).astype(F)
    elif name == "negative":
        xyz = (rng.random((20000, 3)) * [15, 5, 9] - [60, 55, 50]).astype(F)
    elif name == "offset 3e6":    # a float ulp is 0.25 m there
        xyz = (rng.random((20000, 3)) * [20, 5, 20] + 3e6).astype(F)
    elif name == "outliers":
        xyz = outlier_cloud()
    elif name == "inf rows":
        xyz = (rng.random((20000, 3)) * [12, 4, 12]).astype(F)
        rows = rng.choice(20000, 300, replace=False)
        xyz[rows, rng.integers(0, 3, 300)] = np.where(rng.random(300) < 0.5, np.inf, -np.inf)
        xyz[0] = np.inf
    elif name == "raw frame":
        raw = True
        xyz = (rng.random((20000, 3)) * [12, 12, 4] - [0, 6, 2]).astype(F)
        nrm = _normals(20000)
        xyz[rng.choice(20000, 150, replace=False), rng.integers(0, 3, 150)] = np.nan
        nrm[rng.choice(20000, 150, replace=False), rng.integers(0, 3, 150)] = np.nan
        xyz[rng.choice(20000, 20, replace=False), rng.integers(0, 3, 20)] = np.inf       # kept: only NaN drops a row
        xyz[0], nrm[19999, 2] = np.nan, np.nan                                            # first and last row
        hx, hn = _raw_transform(xyz, nrm)
        assert 19650 <= hx.shape[0] < 19720
        return xyz, nrm, raw, hx, hn
    else:
        raise KeyError(name)
    nrm = _normals(xyz.shape[0])
    return xyz, nrm, raw, xyz, nrm


CLOUDS = ("uniform", "planes", "line", "one point", "two points", "identical", "lattice", "negative", "offset 3e6",
          "outliers", "inf rows", "raw frame")


def _check_info(info, n_rows, hx, user_h, what):
    """pcd_cloud_get_info against the reference evaluated at the reported cell size; returns the reported size"""
    h = F(info["cell_size"])
    m, lo, hi = ref.tight_box(hx)
    assert n_rows == hx.shape[0], what
    assert info["num_indexed"] == m, what
    assert _bits(info["bbox_lo"]).tolist() == _bits(lo).tolist(), (what, info["bbox_lo"], lo)
    assert _bits(info["bbox_hi"]).tolist() == _bits(hi).tolist(), (what, info["bbox_hi"], hi)
    assert _bits(info["origin"]).tolist() == _bits(info["bbox_lo"]).tolist(), what
    assert h > 0 and np.isfinite(h), what
    g = ref.grid_info(hx, h)
    assert info["dims"] == g["dims"], (what, h)
    assert info["block_dims"] == g["block_dims"], (what, h)
    assert info["occupied_cells"] == g["occupied_cells"], (what, h)
    assert np.prod(np.array(info["dims"], np.float64)) <= MAX_CELLS, what
    if user_h > 0:
        exp = ref.effective_cell_size(lo, hi, m, user_h)
        assert abs(float(h) - float(exp)) <= 1e-6 * float(exp), (what, h, exp)
    else:
        occ = m / max(info["occupied_cells"], 1)
        print(f"{what}: chosen cell {float(h):.5g} m, dims {info['dims']}, {occ:.2f} rows per occupied cell")
    return h


@pytest.mark.parametrize("cell_size", CELL_SIZES)
@pytest.mark.parametrize("name", CLOUDS)
def test_info_parity(gpu, name, cell_size):
    xyz, nrm, raw, hx, hn = _cloud(name)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=raw, cell_size=cell_size)
    _check_info(c.info(), len(c), hx, cell_size, f"{name} @ {cell_size}")
    dx, dn = c.download()
    assert np.array_equal(_bits(dx), _bits(hx)) and np.array_equal(_bits(dn), _bits(hn)), name
    c.close()


def _slab(thickness):
    rng = np.random.default_rng(8)
    xyz = (rng.random((20000, 3)) * [2000, 2000, thickness]).astype(F)
    q = xyz[rng.integers(0, 20000, 2000)].astype(np.float64) + rng.normal(0, 3.0, (2000, 3))
    q[:50] = xyz[:50]                                            # on a point: distance 0
    q[50:100] += [0, 0, 40]                                      # off the slab
    q[100:120] = rng.random((20, 3)) * [2000, 2000, thickness] + [2500, -700, 0]     # outside the box
    return xyz, q


@pytest.mark.parametrize("thickness", [2.0, 0.2], ids=["slab 2 m", "thin 0.2 m"])
def test_budget_clamp(gpu, oracle, thickness):
    """20 k rows in 2000 x 2000 m with cell_size 0.05 ask for 6.4e10 (8e9 in the thin case) cells: the build must
    raise the size to the budget's, and every search stays exact on the grid it gets.  The largest case of this file:
    a table of 2^26 cells (2^27 entries in the thin case, where dims[2] == 1 pads every quad row with an empty z)."""
    xyz, q = _slab(thickness)
    c = gpu.Cloud(xyz, _normals(20000), raw_lidar_frame=False, cell_size=0.05)
    info = c.info()
    h = _check_info(info, len(c), xyz, 0.05, f"slab {thickness}")
    assert h > F(0.05) * 4
    if thickness < 1:
        assert info["dims"][2] == 1
    exp = oracle.nn_bruteforce(xyz, q)
    for an, algo in _algos(gpu)[1:]:
        _exact(c.nn(q, algo), exp, f"slab {thickness} {an}")
    c.close()


_stray_cache = {}


@functools.lru_cache(maxsize=None)
def _stray_case():
    xyz = outlier_cloud()
    rng = np.random.default_rng(2)
    a, b = xyz[20000].astype(np.float64), xyz[40000].astype(np.float64)
    q = [synth.queries(np.delete(xyz, [20000, 40000], axis=0), 600, seed=3, box=np.array([20.0, 6, 20])),
         a + rng.normal(0, 2.0, (20, 3)), b + rng.normal(0, 2.0, (20, 3)), a[None], b[None],
         (a + b)[None] / 2, (a + b)[None] / 2 + rng.normal(0, 50.0, (10, 3)),
         a + (a - b) * rng.random((10, 1)),                                  # outside the box, beyond one stray
         np.array([[10, 3, 10]]) + rng.normal(0, 1.0, (10, 3)) * [3e5, 3e5, 3e3],
         # between the body and a stray at the distance where the winner changes: |q - body| ~ |q - stray|
         np.array([[5e4, 2, 7], [5.0001e4, 2, 7], [4.9999e4, 2, 7], [5, -5e4, 11], [5, -5.0001e4, 11]])]
    return xyz, np.concatenate(q, axis=0)


@pytest.mark.parametrize("cell_size", CELL_SIZES[1:])
def test_stray_rows(gpu, oracle, cell_size):
    """two returns 100 km from a 20 m body set the box, the budget size (18 m and more: the whole body in a few cells)
    and the binning slack; all four algorithms on every user cell size, association bounded = unbounded + gate"""
    xyz, q = _stray_case()
    nrm = _normals(xyz.shape[0])
    if "exp" not in _stray_cache:
        _stray_cache["exp"] = oracle.nn_bruteforce(xyz, q)
    exp = _stray_cache["exp"]
    assert {20000, 40000} <= set(exp[0].tolist()) and (exp[2] == 1).all()
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=cell_size)
    _check_info(c.info(), len(c), xyz, cell_size, f"outliers @ {cell_size}")
    for an, algo in _algos(gpu):
        _exact(c.nn(q, algo), exp, f"outliers @ {cell_size} {an}")
    Q = q.shape[0]
    mr = np.resize(np.array([1.5, 0.2, 3.0, np.nan, 1e5]), Q)
    for mode in (gpu.GATE_MAPPER_LOCAL, gpu.GATE_MAPPER_GLOBAL, gpu.GATE_CONTROLLER):
        full = c.associate(q, mr, mode)
        assert np.array_equal(full["nn_idx"], exp[0]) and np.array_equal(_bits(full["nn_sqdist"]), _bits(exp[1]))
        bnd = c.associate(q, mr, mode | gpu.GATE_BOUNDED_SEARCH)
        assert np.array_equal(bnd["type"], full["type"]), (mode, np.nonzero(bnd["type"] != full["type"])[0][:10])
        acc = full["type"] != 0
        assert 0 < acc.sum() < Q
        for k in full:
            assert np.array_equal(np.ascontiguousarray(bnd[k][acc]).view(np.uint8),
                                  np.ascontiguousarray(full[k][acc]).view(np.uint8)), (mode, k)
    c.close()


def test_layouts(gpu, oracle):
    """AOS32 rows (x y z pad nx ny nz pad) without the raw frame, garbage in the pad floats: the handle equals the
    two-array one; in the raw frame a NaN in a pad float alone does not drop the row"""
    rng = np.random.default_rng(6)
    n = 5000
    xyz = (rng.random((n, 3)) * [12, 4, 12]).astype(F)
    nrm = _normals(n)
    aos = np.empty((n, 8), F)
    aos[:, :3], aos[:, 4:7] = xyz, nrm
    junk = np.array([np.nan, np.inf, -np.inf, 1e30, -7.5, 0.0], F)
    aos[:, 3], aos[:, 7] = junk[rng.integers(0, 6, n)], junk[rng.integers(0, 6, n)]
    q = synth.queries(xyz, 1000, seed=1, box=np.array([12.0, 4, 12]))
    two = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=0.3)
    one = gpu.Cloud(aos, None, raw_lidar_frame=False, cell_size=0.3, layout=gpu.LAYOUT_AOS32)
    ia, ib = two.info(), one.info()
    assert {k: v for k, v in ia.items() if k != "build_ms"} == {k: v for k, v in ib.items() if k != "build_ms"}
    _check_info(ib, len(one), xyz, 0.3, "aos32")
    for a, b in zip(two.download(), one.download()):
        assert np.array_equal(_bits(a), _bits(b))
    exp = oracle.nn_bruteforce(xyz, q)
    for an, algo in _algos(gpu):
        _exact(one.nn(q, algo), exp, f"aos32 {an}")
        _exact(two.nn(q, algo), exp, f"two arrays {an}")
    a, b = two.associate(q, 1.5, gpu.GATE_MAPPER_LOCAL), one.associate(q, 1.5, gpu.GATE_MAPPER_LOCAL)
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    two.close(); one.close()
    # raw frame: NaN in a pad float only -> kept; NaN in the position or the normal -> dropped
    raw = aos.copy()
    raw[:, 3], raw[:, 7] = 0, 0
    raw[10, 3], raw[11, 7], raw[4999, 3] = np.nan, np.nan, np.nan
    raw[20, 1], raw[21, 6] = np.nan, np.nan
    hx, hn = _raw_transform(raw[:, :3], raw[:, 4:7])
    assert hx.shape[0] == n - 2
    c = gpu.Cloud(raw, None, raw_lidar_frame=True, layout=gpu.LAYOUT_AOS32)
    assert len(c) == n - 2
    dx, dn = c.download()
    assert np.array_equal(_bits(dx), _bits(hx)) and np.array_equal(_bits(dn), _bits(hn))
    _check_info(c.info(), len(c), hx, 0.0, "aos32 raw frame")
    qh = synth.queries(hx, 500, seed=2, box=np.array([4.0, 12, 12]))
    _exact(c.nn(qh), oracle.nn_bruteforce(hx, qh), "aos32 raw frame")
    c.close()


ROWS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
QUERIES = (1, 3, 4, 5, 255, 256, 257)


@pytest.mark.parametrize("n", ROWS)
def test_launch_shape_boundaries(gpu, oracle, n):
    """row counts around the 64-lane leaf reduction, the 1024-row brute-force tile and its 4096-row chunks; query counts
    around the 4-query blocks of the pyramid walk and the 256-thread blocks: every algorithm against the oracle"""
    rng = np.random.default_rng(n)
    xyz = (rng.random((n, 3)) * [3, 1, 3]).astype(F)
    if n > 3:
        xyz[n - 1] = xyz[0]                     # the last row ties with the first: index 0 must win
    qa = np.concatenate([xyz[rng.integers(0, n, 129)].astype(np.float64) + rng.normal(0, 0.3, (129, 3)),
                         xyz[rng.integers(0, n, 64)].astype(np.float64), xyz[-1:].astype(np.float64),
                         rng.random((63, 3)) * 40 - 20], axis=0)
    for cell in (0.0, 0.3):                     # one cell for the small clouds at 0, several at 0.3
        c = gpu.Cloud(xyz, _normals(n), raw_lidar_frame=False, cell_size=cell)
        _check_info(c.info(), len(c), xyz, cell, f"{n} rows @ {cell}")
        for Q in QUERIES:
            q = qa[rng.permutation(257)[:Q]]
            if Q >= 3:
                q[Q - 1] = xyz[-1]              # the last query sits on the tied pair
            exp = oracle.nn_bruteforce(xyz, q)
            for an, algo in _algos(gpu):
                _exact(c.nn(q, algo), exp, f"{n} rows, {Q} queries, cell {cell}, {an}")
        c.close()


def test_small_batch_switch(gpu, oracle):
    """PCD_NN_AUTO on one 5 k-row cloud: Q = 65536 is the last batch of the one-launch path, 65537 the first of the
    grid path; both against the oracle's KD-tree"""
    xyz = synth.cloud_planes(5000, seed=12, patches=6)[0]
    q = synth.queries(xyz, SMALL_BATCH + 1, seed=7)
    q[5] = np.nan
    q[SMALL_BATCH] = xyz[77]
    c = gpu.Cloud(xyz, _normals(5000), raw_lidar_frame=False)
    exp = oracle.KDTree(xyz).query(q)
    _exact(oracle.nn_bruteforce(xyz, q[:3000]), tuple(e[:3000] for e in exp), "kd-tree vs brute force")
    _exact(c.nn(q[:SMALL_BATCH]), tuple(e[:SMALL_BATCH] for e in exp), "Q = 65536")
    _exact(c.nn(q), exp, "Q = 65537")
    c.close()

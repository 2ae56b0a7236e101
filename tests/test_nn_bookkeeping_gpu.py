"""The query bookkeeping in front of the brick kernel (csrc/nn.hip: k_bk_slots with the fused prepare, k_bk_colscan,
k_bk_scatter, k_bk_count, k_bk_emit, the self-cleaning counters) at its edges.

Bar: bit-exact, as tests/test_nn_gpu.py -- same index, same float32 distance bits, same found flag.  Expected values come
from the CPU oracle, or from the device brute force (itself oracle-checked in test_nn_gpu.py) where the oracle would take
seconds; every case is also compared with the radix-sort bookkeeping, which shares none of these kernels.
"""
import numpy as np
import pytest

from pcdhip import synth

pytestmark = pytest.mark.gpu


def _check_exact(got, exp, what=""):
    gi, gd, gf = got
    ei, ed, ef = exp
    assert np.array_equal(gf, ef), f"{what}: found flags differ at {np.nonzero(gf != ef)[0][:10]}"
    bad = np.nonzero((gi != ei) | (gd.view(np.uint32) != ed.view(np.uint32)))[0]
    assert bad.size == 0, (f"{what}: {bad.size} mismatches, first {bad[:5]}: idx {gi[bad[:5]]} vs {ei[bad[:5]]}, "
                           f"d {gd[bad[:5]]} vs {ed[bad[:5]]}")


def _radix(gpu, fn):
    """fn() under the radix-sort bookkeeping"""
    try:
        gpu.set_nn_bookkeeping(1)
        return fn()
    finally:
        gpu.set_nn_bookkeeping(0)


def _grid_exact(gpu, c, q, exp, what, algo=None):
    """the grid path on q: equal to exp, and to the same call under the radix-sort bookkeeping"""
    algo = gpu.NN_GRID if algo is None else algo
    got = c.nn(q, algo)
    _check_exact(got, exp, what)
    _check_exact(got, _radix(gpu, lambda: c.nn(q, algo)), what + " vs radix-sort bookkeeping")
    return got


@pytest.fixture(scope="module")
def planes():
    """one 40 k-point cloud and its queries' oracle answers, shared by the cases below (never modified)"""
    xyz, nrm = synth.cloud_planes(40000, seed=41, patches=10)
    return xyz, nrm


@pytest.mark.parametrize("Q", [1, 7, 8, 9, 4095, 4096, 4097, 12289])
def test_item_and_range_edges(gpu, oracle, planes, Q):
    """one query, one item short of / exactly / one past G = 8, one round of 4096 short of / exactly / one past, three
    rounds and one query"""
    xyz, nrm = planes
    q = synth.queries(xyz, Q, seed=100 + Q, sigma=0.05)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    _grid_exact(gpu, c, q, oracle.nn_bruteforce(xyz, q), f"Q={Q}")
    c.close()


def test_more_than_256_ranges_of_queries(gpu):
    """Q = 256 x 4096 + 5: every range of k_bk_slots / k_bk_scatter runs two rounds and the last one is ragged"""
    xyz, nrm = synth.cloud_planes(20000, seed=42, patches=6)
    Q = 256 * 4096 + 5
    q = synth.queries(xyz, Q, seed=43, sigma=0.1)
    q[::4099] = np.nan
    q[5::8191] += 300.0
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    _grid_exact(gpu, c, q, c.nn(q, gpu.NN_BRUTEFORCE), "Q = 256 * 4096 + 5")
    c.close()


def _brick_box(info, brick):
    """corners of a brick of 2 x 2 x 2 cells, clipped to the grid and shrunk by a thousandth of a cell"""
    h = info["cell_size"]
    o = np.array(info["origin"], np.float64)
    d = np.array(info["dims"], np.int64)
    lo = o + 2.0 * np.array(brick) * h + 1e-3 * h
    hi = o + np.minimum(2 * np.array(brick) + 2, d) * h - 1e-3 * h
    return lo, hi


@pytest.mark.parametrize("which", ["a brick inside", "the brick of highest id"])
def test_all_queries_in_one_brick(gpu, oracle, which):
    """10 000 queries in one brick: one bucket, one fine key, 1250 items, every rank atomic on one cursor; in the brick
    of highest id the bucket is the last, partial one"""
    xyz, nrm = synth.cloud_uniform(30000, seed=44, box=np.array([12.0, 4.0, 9.0]))
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    info = c.info()
    d = np.array(info["dims"], np.int64)
    if which == "a brick inside":
        cell = np.floor((xyz[123].astype(np.float64) - np.array(info["origin"])) / info["cell_size"]).astype(np.int64)
        brick = np.minimum(cell, d - 1) // 2
    else:
        brick = (d - 1) // 2          # the grid's far corner: the bounding box ends there, so points lie next to it
    lo, hi = _brick_box(info, brick)
    q = lo + np.random.default_rng(45).random((10000, 3)) * (hi - lo)
    _grid_exact(gpu, c, q, oracle.nn_bruteforce(xyz, q), which)
    c.close()


@pytest.mark.parametrize("case", ["not finite", "far outside", "mixed"])
def test_nothing_or_little_in_the_grid(gpu, oracle, planes, case):
    xyz, nrm = planes
    Q = 9001
    rng = np.random.default_rng(46)
    q = synth.queries(xyz, Q, seed=47, sigma=0.1)
    if case == "not finite":
        q[:] = np.nan
        q[::3, 1] = np.inf
        q[1::3, 2] = -np.inf
    elif case == "far outside":       # n_in_grid = 0, no items: the whole batch goes through the fallback list
        q += np.array([400.0, -700.0, 300.0]) * rng.choice([-1.0, 1.0], (Q, 1))
    else:
        q[::7] = np.nan
        q[3::13, 0] = np.inf
        q[5::11] += 500.0
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    got = _grid_exact(gpu, c, q, oracle.nn_bruteforce(xyz, q), case)
    if case == "not finite":
        assert not got[2].any()
    c.close()


# ------------------------------------------------------------------ the three prepare flavours on the grid path
QF = 70000        # above the small-batch limit: PCD_NN_AUTO takes the grid path


@pytest.fixture(scope="module")
def flavour_scene():
    xyz, nrm = synth.cloud_planes(30000, seed=48, patches=8)
    order = np.argsort(xyz[:, 0], kind="stable")      # two spatially compact halves along x
    xyz, nrm = np.ascontiguousarray(xyz[order]), np.ascontiguousarray(nrm[order])
    q = synth.queries(xyz, QF, seed=49, sigma=0.15)
    q[::101] = np.nan
    q[7::257] += 250.0
    return xyz, nrm, q


def test_flavour_plain(gpu, flavour_scene):
    xyz, nrm, q = flavour_scene
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    _grid_exact(gpu, c, q, c.nn(q, gpu.NN_BRUTEFORCE), "plain, Q = 70 000", algo=gpu.NN_AUTO)
    c.close()


def test_flavour_gate_bounded(gpu, flavour_scene):
    """associate with the gate as the search bound accepts exactly what the unbounded search + gate accept"""
    xyz, nrm, q = flavour_scene
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    mr = np.full(QF, 0.2)
    mr[::5] = 0.05
    mr[3::97] = np.nan
    a = c.associate(q, mr, gpu.GATE_MAPPER_LOCAL)
    b = c.associate(q, mr, gpu.GATE_MAPPER_LOCAL | gpu.GATE_BOUNDED_SEARCH)
    br = _radix(gpu, lambda: c.associate(q, mr, gpu.GATE_MAPPER_LOCAL | gpu.GATE_BOUNDED_SEARCH))
    bi, bd, bf = c.nn(q, gpu.NN_BRUTEFORCE)
    assert np.array_equal(a["nn_idx"][bf != 0], bi[bf != 0])     # the unbounded search is the exact one
    assert np.array_equal(a["type"], b["type"])
    acc = a["type"] != 0
    assert acc.any() and (~acc).any()
    for k in ("nn_idx", "nn_sqdist", "lidar_xyz", "abcd", "dist", "angle"):
        assert np.array_equal(a[k][acc], b[k][acc]), k
        assert np.array_equal(b[k][acc], br[k][acc]), k + " (radix-sort bookkeeping)"
    assert np.array_equal(b["type"], br["type"])
    c.close()


def test_flavour_refine(gpu, flavour_scene):
    """keys arrive from the other shard, some queries are skipped: the searched ones leave with the unsharded key, the
    skipped ones with the key they came with"""
    import torch
    xyz, nrm, q = flavour_scene
    n = xyz.shape[0]
    cut = n // 2
    single = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    dq = torch.from_numpy(q).cuda()
    want = torch.empty(QF, dtype=torch.int64, device="cuda")
    single.nn_device(dq, QF, want, gpu.NN_BRUTEFORCE)
    sh = [gpu.Cloud(xyz[a:b], nrm[a:b], raw_lidar_frame=False, index_base=a) for a, b in ((0, cut), (cut, n))]
    inc = torch.empty(QF, dtype=torch.int64, device="cuda")
    sh[0].nn_device(dq, QF, inc, gpu.NN_BRUTEFORCE)               # the other shard's results
    skip = np.zeros(QF, np.uint8)
    skip[::9] = 1
    dskip = torch.from_numpy(skip).cuda()
    keys = inc.clone()
    sh[1].nn_refine_device(dq, QF, keys, dskip)
    torch.cuda.synchronize()
    kr = inc.clone()
    _radix(gpu, lambda: (sh[1].nn_refine_device(dq, QF, kr, dskip), torch.cuda.synchronize()))
    got, w, i0 = keys.cpu().numpy(), want.cpu().numpy(), inc.cpu().numpy()
    s = skip != 0
    assert np.array_equal(got[~s], w[~s]), np.nonzero(got[~s] != w[~s])[0][:5]
    assert np.array_equal(got[s], i0[s])
    assert (got[~s] != i0[~s]).any(), "the second shard improved nothing: the case does not exercise the search"
    assert np.array_equal(got, kr.cpu().numpy())
    for c in sh + [single]:
        c.close()


# ------------------------------------------------------------------ the counters clean themselves
def test_self_cleaning_state(gpu, oracle, planes):
    xyz, nrm = planes
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    qa = synth.queries(xyz, 70000, seed=50, sigma=0.1)
    qb = synth.queries(xyz, 1000, seed=51, sigma=0.1)
    qc = synth.queries(xyz, 9000, seed=52, sigma=0.1)
    qd = synth.queries(xyz, 70000, seed=53, sigma=0.3)
    qd[::77] = np.nan
    _check_exact(c.nn(qa), c.nn(qa, gpu.NN_BRUTEFORCE), "1: grid call, Q = 70 000")
    _check_exact(c.nn(qb), oracle.nn_bruteforce(xyz, qb), "2: one-launch call, Q = 1 000")
    _check_exact(c.nn(qc, gpu.NN_GRID), oracle.nn_bruteforce(xyz, qc), "3: grid call, Q = 9 000")
    _check_exact(c.nn(qd), c.nn(qd, gpu.NN_BRUTEFORCE), "4: grid call, other queries")
    exp_a = c.nn(qa, gpu.NN_BRUTEFORCE)
    try:
        gpu.set_nn_tuning(0, -1, 1)
        _check_exact(c.nn(qa), exp_a, "statistics call 1")
        s1 = c.last_stats()
        _check_exact(c.nn(qa), exp_a, "statistics call 2")
        s2 = c.last_stats()
        gpu.set_nn_tuning(0, -1, 0)
        _check_exact(c.nn(qd), c.nn(qd, gpu.NN_BRUTEFORCE), "a call without statistics")
        gpu.set_nn_tuning(0, -1, 1)
        _check_exact(c.nn(qa), exp_a, "statistics call 3")
        s3 = c.last_stats()
    finally:
        gpu.set_nn_tuning(0, -1, 0)
    print("stats:", s1, s2, s3)
    # The same batch three times: the items per brick are ceil(queries / 8) whatever the order, WHICH queries share an
    # item (and with it the clip and the pairs evaluated) varies with the order the atomics hand out.  5 % is far above
    # that variation and far below the factor 2 a sum over two calls would show.
    for k in ("brick_groups", "pair_evals"):
        assert s1[k] > 0 and s2[k] > 0 and s3[k] > 0, (k, s1, s2, s3)
        assert abs(s2[k] - s1[k]) <= 0.05 * s1[k], (k, s1, s2)
        assert abs(s3[k] - s1[k]) <= 0.05 * s1[k], (k, s1, s3)
    c.close()


def test_wide_grid_dynamic_lds_maximum(gpu):
    """the 40 M-cell cloud of test_large_sparse_grid_counting_sort: shift = 12, 4096 fine keys per bucket -- the most LDS
    k_bk_emit asks for"""
    rng = np.random.default_rng(31)
    n, Q = 200000, 20000
    xyz = (rng.random((n, 3)) * np.array([60.0, 60.0, 12.0])).astype(np.float32)
    nrm = np.zeros_like(xyz)
    nrm[:, 2] = 1.0
    q = (xyz[rng.integers(0, n, Q)] + rng.normal(0, 0.08, (Q, 3))).astype(np.float32)
    q[::97] = np.nan
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=0.1)
    assert int(np.prod(c.info()["dims"])) > 38_000_000, c.info()
    _grid_exact(gpu, c, q, c.nn(q, gpu.NN_BRUTEFORCE), "40 M-cell grid")
    c.close()

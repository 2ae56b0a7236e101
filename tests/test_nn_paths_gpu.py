"""Every path the NN host driver (csrc/nn.hip nn_device) can take, on one cloud: brute force, the one-launch walk, prepare +
walk, the grid path with either bookkeeping, for the plain, the refine and the gate-bounded flavour, on both sides of the
small-batch limit; the empty cloud; an unknown algo; the statistics of a grid and of a one-launch call.

Bar: keys equal bit for bit to PCD_NN_BRUTEFORCE on the same cloud (itself oracle-checked in tests/test_nn_gpu.py).  The
refine predicate is the one of tests/cloud_ref.py, the gate decision the exact one of tests/assoc_edge_ref.py.
"""
import numpy as np
import pytest
import torch

from pcdhip import synth
from tests import assoc_edge_ref, cloud_ref

pytestmark = pytest.mark.gpu

SMALL_BATCH = 65536      # nn.hip kSmallBatch: PCD_NN_AUTO walks up to it and takes the grid path above
QMAX = SMALL_BATCH + 1
KEY_NONE = np.int64(0x7FFFFFFFFFFFFFFF)


def _keys(call, Q, init=None):
    """the int64 keys a device entry point leaves (call(d_keys)); init: the keys it finds"""
    k = torch.empty(Q, dtype=torch.int64, device="cuda") if init is None else torch.from_numpy(init.copy()).cuda()
    call(k)
    torch.cuda.synchronize()
    return k.cpu().numpy()


def _same(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} keys differ, first {bad[:5]}: {got[bad[:5]]} vs {exp[bad[:5]]}"


def _bookkeepings(gpu, Q):
    """the bookkeeping switch settings that matter at this batch size: the radix sort only exists on the grid path"""
    return (0, 1) if Q > SMALL_BATCH else (0,)


class _Bookkeeping:
    def __init__(self, gpu, radix):
        self.gpu, self.radix = gpu, radix

    def __enter__(self):
        self.gpu.set_nn_bookkeeping(self.radix)

    def __exit__(self, *a):
        self.gpu.set_nn_bookkeeping(0)


@pytest.fixture(scope="module")
def scene(gpu):
    """30 000 points on planes, sorted along x (two compact shards); 65 537 queries near the surface with a few that are
    not finite, a few just outside the grid and a few far away; the brute-force keys of the whole cloud and of either
    shard.  Shared by every test below and never modified."""
    xyz, nrm = synth.cloud_planes(30000, seed=61, patches=8)
    order = np.argsort(xyz[:, 0], kind="stable")
    xyz, nrm = np.ascontiguousarray(xyz[order]), np.ascontiguousarray(nrm[order])
    q = synth.queries(xyz, QMAX, seed=62, sigma=0.15)
    ext = (xyz.max(axis=0) - xyz.min(axis=0)).astype(np.float64)
    q[3::1013] = np.nan
    q[5::2027, 1] = np.inf
    q[7::509] += 1.5 * ext                     # outside the grid, next to it
    q[11::4099] -= np.array([9.0e3, 2.0e4, -7.0e3])   # far outliers
    q[256] = q[7]                              # the ragged last workgroup of Q = 257 holds one of them
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    cut = xyz.shape[0] // 2
    sh = [gpu.Cloud(xyz[a:b], nrm[a:b], raw_lidar_frame=False, index_base=a) for a, b in ((0, cut), (cut, xyz.shape[0]))]
    dq = torch.from_numpy(q).cuda()
    want = _keys(lambda k: c.nn_device(dq, QMAX, k, gpu.NN_BRUTEFORCE), QMAX)
    own = [_keys(lambda k, s=s: s.nn_device(dq, QMAX, k, gpu.NN_BRUTEFORCE), QMAX) for s in sh]
    _same(np.minimum(own[0], own[1]), want, "brute force: shards vs whole cloud")
    finite = np.isfinite(q.astype(np.float32)).all(axis=1)
    assert np.array_equal(want != KEY_NONE, finite) and 0 < (~finite).sum() < 200
    yield dict(xyz=xyz, nrm=nrm, q=q, dq=dq, c=c, sh=sh, want=want, own=own, finite=finite)
    for h in sh + [c]:
        h.close()


# ------------------------------------------------------------------ the algos, a ragged last workgroup
@pytest.mark.parametrize("algo", ["NN_BRUTEFORCE", "NN_FALLBACK_ONLY", "NN_GRID"])
def test_algos_at_257(gpu, scene, algo):
    """Q = 257: one workgroup of 256 and one query; NN_GRID at a batch size NN_AUTO never sends there"""
    c, dq, Q = scene["c"], scene["dq"], 257
    for radix in ((0, 1) if algo == "NN_GRID" else (0,)):
        with _Bookkeeping(gpu, radix):
            _same(_keys(lambda k: c.nn_device(dq, Q, k, getattr(gpu, algo)), Q), scene["want"][:Q], (algo, radix))


# ------------------------------------------------------------------ NN_AUTO on both sides of the small-batch limit
@pytest.mark.parametrize("Q", [SMALL_BATCH, SMALL_BATCH + 1])
def test_auto_plain(gpu, scene, Q):
    c, dq = scene["c"], scene["dq"]
    for radix in _bookkeepings(gpu, Q):
        with _Bookkeeping(gpu, radix):
            _same(_keys(lambda k: c.nn_device(dq, Q, k), Q), scene["want"][:Q], (Q, radix))
    # the host entry point: the same keys, unpacked
    idx, sq, found = c.nn(scene["q"][:Q])
    w = scene["want"][:Q]
    f = w != KEY_NONE
    assert np.array_equal(found != 0, f)
    assert np.array_equal(idx[f], (w[f] & 0xFFFFFFFF).astype(np.uint32))
    assert np.array_equal(sq[f].view(np.uint32), (w[f] >> 32).astype(np.uint32))


@pytest.mark.parametrize("Q", [SMALL_BATCH, SMALL_BATCH + 1])
def test_auto_refine(gpu, scene, Q):
    """pcd_nn_refine_device of the second shard: keys arrive from the first shard (some as KEY_NONE), some queries are
    skipped.  A query is searched iff it is not skipped and the reference predicate holds; then it leaves with the minimum
    of the two keys, otherwise with the key it came with."""
    sh, dq, q = scene["sh"][1], scene["dq"], scene["q"][:Q]
    own = scene["own"][1][:Q]
    inc = scene["own"][0][:Q].copy()
    inc[2::7] = KEY_NONE
    skip = np.zeros(Q, np.uint8)
    skip[::9] = 1
    info = sh.info()
    sqbits = np.where(inc == KEY_NONE, cloud_ref.FLT_MAX_BITS, inc >> 32).astype(np.uint32)
    active = cloud_ref.refine_active(q, info["bbox_lo"], info["bbox_hi"], sqbits) & (skip == 0)
    exp = np.where(active, np.minimum(inc, own), inc)
    assert (exp != inc).any() and (~active & (skip == 0) & scene["finite"][:Q]).any()
    # the predicate drops nothing the shard would have improved: the searched queries end at the whole cloud's key
    s = (skip == 0) & (inc != KEY_NONE)
    _same(exp[s], scene["want"][:Q][s], "reference")
    dskip = torch.from_numpy(skip).cuda()
    for radix in _bookkeepings(gpu, Q):
        with _Bookkeeping(gpu, radix):
            _same(_keys(lambda k: sh.nn_refine_device(dq, Q, k, dskip), Q, inc), exp, (Q, radix, "skip mask"))
            noskip = cloud_ref.refine_active(q, info["bbox_lo"], info["bbox_hi"], sqbits)
            _same(_keys(lambda k: sh.nn_refine_device(dq, Q, k), Q, inc), np.where(noskip, np.minimum(inc, own), inc),
                  (Q, radix, "no skip mask"))


def _dev_out(Q):
    return dict(type=torch.empty(Q, dtype=torch.uint8, device="cuda"), nn_idx=torch.empty(Q, dtype=torch.int32, device="cuda"),
                nn_sqdist=torch.empty(Q, dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("Q", [SMALL_BATCH, SMALL_BATCH + 1])
def test_auto_bounded(gpu, scene, Q):
    """pcd_associate_device with the gate as the search bound, per-query and scalar ranges: the gate's decision is the
    exact one, and every accepted row carries the brute-force key"""
    c, dq, q = scene["c"], scene["dq"], scene["q"][:Q]
    want = scene["want"][:Q]
    found = want != KEY_NONE
    widx = np.where(found, want & 0xFFFFFFFF, 0).astype(np.int64)
    wsq = (want >> 32).astype(np.uint32)
    rng = np.random.default_rng(63)
    per_query = rng.choice([0.05, 0.2, 0.4, 1.5], Q)
    per_query[3::97] = np.nan                  # `dist > NaN` rejects nothing: unbounded
    per_query[4::211] = 0.0
    rows = np.arange(0, Q, 211)                # the exact reference, row by row in rational arithmetic, on a sample
    for mr, count in ((per_query, Q), (np.array([0.2]), 1)):
        dmr = torch.from_numpy(np.ascontiguousarray(mr)).cuda()
        ref = assoc_edge_ref.associate_ref(q[rows], scene["xyz"][widx[rows]], scene["nrm"][widx[rows]], found[rows],
                                           mr[rows] if count == Q else float(mr[0]), 0)
        # the whole batch: the epilogue on the brute-force keys (no search at all)
        full = _dev_out(Q)
        c.associate_device(dq, Q, dmr, count, gpu.GATE_MAPPER_LOCAL, full, torch.from_numpy(want).cuda())
        torch.cuda.synchronize()
        ftype = full["type"].cpu().numpy()
        assert np.array_equal(ftype[rows], ref["type"]), (Q, count)
        acc = ftype != 0
        assert 0 < acc.sum() < found.sum()
        for radix in _bookkeepings(gpu, Q):
            with _Bookkeeping(gpu, radix):
                d = _dev_out(Q)
                c.associate_device(dq, Q, dmr, count, gpu.GATE_MAPPER_LOCAL | gpu.GATE_BOUNDED_SEARCH, d)
                torch.cuda.synchronize()
            what = (Q, count, radix)
            assert np.array_equal(d["type"].cpu().numpy(), ftype), what
            assert np.array_equal(d["nn_idx"].cpu().numpy().view(np.uint32)[acc], widx[acc].astype(np.uint32)), what
            assert np.array_equal(d["nn_sqdist"].cpu().numpy().view(np.uint32)[acc], wsq[acc]), what


# ------------------------------------------------------------------ the corners of the path choice
def test_unknown_algo_is_refused(gpu, scene):
    c, dq, Q = scene["c"], scene["dq"], 257
    for algo in (4, -1, 99):
        with pytest.raises(gpu.PcdError) as e:
            c.nn_device(dq, Q, torch.empty(Q, dtype=torch.int64, device="cuda"), algo)
        assert e.value.status == gpu.PCD_ERR_INVALID, e.value
        assert f"unknown nn algo {algo}" in str(e.value)
        for valid in (gpu.NN_AUTO, gpu.NN_GRID):
            _same(_keys(lambda k: c.nn_device(dq, Q, k, valid), Q), scene["want"][:Q], ("after algo", algo, valid))


def test_empty_cloud_and_empty_batch(gpu, scene):
    """an empty cloud answers PCD_OK with every key KEY_NONE, whatever the algo and the flavour; Q = 0 is PCD_OK"""
    z3 = np.zeros((0, 3), np.float32)
    e = gpu.Cloud(z3, z3, raw_lidar_frame=False)
    dq, Q = scene["dq"], 257
    for algo in (gpu.NN_AUTO, gpu.NN_BRUTEFORCE, gpu.NN_FALLBACK_ONLY, gpu.NN_GRID, 99):
        assert (_keys(lambda k: e.nn_device(dq, Q, k, algo), Q) == KEY_NONE).all(), algo
    inc = scene["want"][:Q]
    _same(_keys(lambda k: e.nn_refine_device(dq, Q, k), Q, inc), inc, "refine on an empty cloud")
    e.nn_device(dq, 0, None)
    scene["c"].nn_device(dq, 0, None, 99)
    e.close()


def _grid_path_walks(q, want, info):
    """(queries the grid path hands to the exact walk, those of them outside the grid).  A finite query walks iff it lies
    outside the grid or its nearest distance is not below the bound that proves it inside its brick's region -- the
    brick's cells grown by two (brick_clip_kernel.h proven_bound_f, restated in float32 one operation at a time; a brick
    whose region holds no point never proves anything, so the bitmap of empty regions changes nothing)."""
    f32 = np.float32
    qf = q.astype(f32)
    fin = np.isfinite(qf).all(axis=1)
    qf, d = qf[fin], (want[fin] >> 32).astype(np.uint32).view(f32)
    o, h, n = np.asarray(info["origin"], f32), f32(info["cell_size"]), np.asarray(info["dims"], np.int64)
    t = np.floor(((qf - o).astype(f32) * (f32(1) / h)).astype(f32))
    c = np.clip(t, -1.0, n.astype(f32)).astype(np.int64)
    inside = ((c >= 0) & (c < n)).all(axis=1)
    c0, c1 = np.maximum(2 * (c // 2) - 2, 0), np.minimum(2 * (c // 2) + 4, n)
    big = f32(3e38)
    mlo = np.where(c0 > 0, (qf - (o + (c0.astype(f32) * h).astype(f32)).astype(f32)).astype(f32), big)
    mhi = np.where(c1 < n, ((o + (c1.astype(f32) * h).astype(f32)).astype(f32) - qf).astype(f32), big)
    margin = np.minimum(mlo, mhi).min(axis=1).astype(f32)
    lo, hi = np.asarray(info["bbox_lo"], f32), np.asarray(info["bbox_hi"], f32)
    ext = max(f32((hi.astype(np.float64) - lo.astype(np.float64)).max()), np.abs(lo).max(), np.abs(hi).max())
    slack = f32(f32(ext) * f32(9.6e-7) + f32(1e-30))                     # cloud.hip set_dims
    m = (margin - f32(f32(2) * slack)).astype(f32)
    sq = ((m * m).astype(f32) * f32(f32(1) - f32(1e-5))).astype(f32)
    bound = np.where(margin >= big, big, np.where(m > 0, sq, f32(-1)))
    return int((~inside).sum() + (inside & ~(d < bound)).sum()), int((~inside).sum())


def test_stats_of_a_grid_and_a_one_launch_call(gpu, scene):
    c, dq = scene["c"], scene["dq"]
    finite = scene["finite"]
    walks, outside = _grid_path_walks(scene["q"], scene["want"], c.info())
    assert 100 < outside < walks < 0.2 * QMAX, (outside, walks)
    try:
        gpu.set_nn_tuning(0, -1, 1)
        _same(_keys(lambda k: c.nn_device(dq, QMAX, k), QMAX), scene["want"], "grid call with statistics")
        g1 = c.last_stats()
        Q = 20000
        _same(_keys(lambda k: c.nn_device(dq, Q, k), Q), scene["want"][:Q], "one-launch call with statistics")
        o1 = c.last_stats()
        _same(_keys(lambda k: c.nn_device(dq, QMAX, k), QMAX), scene["want"], "grid call with statistics, again")
        g2 = c.last_stats()
    finally:
        gpu.set_nn_tuning(0, -1, 0)
    print("stats:", g1, o1, g2)
    # the one-launch call walks every finite query and nothing else
    assert o1["fallback_queries"] == int(finite[:Q].sum()), o1
    assert o1["brick_groups"] == 0 and o1["staged_points"] == 0 and o1["fallback_points"] == o1["pair_evals"] > 0, o1
    # the grid call: exactly the queries the brick kernel cannot prove walk; the counters are those of ONE call (the
    # bound of tests/test_nn_bookkeeping_gpu.py: which queries share a work item varies from run to run)
    for g in (g1, g2):
        assert g["fallback_queries"] == walks, (g, walks, outside)
        assert g["brick_groups"] > 0 and g["pair_evals"] > g["fallback_points"] > 0, g
    for k in ("brick_groups", "pair_evals"):
        assert abs(g2[k] - g1[k]) <= 0.05 * g1[k], (k, g1, g2)

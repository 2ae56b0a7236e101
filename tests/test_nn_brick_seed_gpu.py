"""k_nn_brick_clip on items whose brick holds no cloud point of its own (csrc/brick_clip_kernel.h, issue_a): stage A
then compares up to 128 records of a neighbouring two-cell span -- lowest class (face, edge, corner neighbour) with a
point, in it the fullest span, ties to the lowest entry of the boundary table -- and the stage-B split follows the row
those records came from.

Every case runs through NN_GRID on a cloud built with an explicit cell size (the brick kernel runs whatever the batch
size) and compares index, float bits and found flag with the CPU oracle's brute force, with the clip on and with the
clip-off switch set_nn_search(1).

Geometry.  h = 0.5 and a point at the origin: binning is exact, cell c covers [c / 2, c / 2 + 1 / 2) and BRICK b covers
[b, b + 1) on every axis; the region of a brick is the 3 x 3 x 3 bricks around it.  Scenes are placed at least 4 bricks
apart, so a scene's region holds the scene's points only; far filler points give the grid its extent.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 0.5
NEIGHBOURS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def _in_brick(rng, b, n, lo=0.1, hi=0.9):
    """n points in brick b, inside [lo, hi) of its edge on every axis"""
    return np.asarray(b, np.float64) + rng.uniform(lo, hi, (n, 3))


def _cloud(parts, extent):
    """the parts + the filler points: the origin and the far corner"""
    xyz = np.concatenate([np.zeros((1, 3))] + [np.asarray(p, np.float64).reshape(-1, 3) for p in parts]
                         + [np.full((1, 3), float(extent))]).astype(np.float32)
    assert (xyz.min(0) == 0).all()
    return xyz


def _check(got, exp, what):
    gi, gd, gf = got
    ei, ed, ef = exp
    assert np.array_equal(gf, ef), f"{what}: found flags differ at {np.nonzero(gf != ef)[0][:10]}"
    bad = np.nonzero((gi != ei) | (gd.view(np.uint32) != ed.view(np.uint32)))[0]
    assert bad.size == 0, (f"{what}: {bad.size} mismatches, first {bad[:5]}: idx {gi[bad[:5]]} vs {ei[bad[:5]]}, "
                           f"d {gd[bad[:5]]} vs {ed[bad[:5]]}")


def _both_ways(gpu, oracle, xyz, q, what, h=H, stats=False):
    """NN_GRID with the clip on and off against the oracle; the statistics of the clip-on call when asked for"""
    exp = oracle.nn_bruteforce(xyz, q)
    c = gpu.Cloud(xyz, np.zeros_like(xyz), raw_lidar_frame=False, cell_size=h)
    st = None
    try:
        assert abs(c.info()["cell_size"] - h) < 1e-6, c.info()
        if stats:
            gpu.set_nn_tuning(0, -1, 1)
        _check(c.nn(q, gpu.NN_GRID), exp, what + " (clip on)")
        if stats:
            st = c.last_stats()
        gpu.set_nn_search(1)
        _check(c.nn(q, gpu.NN_GRID), exp, what + " (clip off)")
    finally:
        gpu.set_nn_search(0)
        gpu.set_nn_tuning(0, -1, 0)
        c.close()
    return st


def _centres():
    """27 scene centres 4 bricks apart"""
    return [(2 + 4 * i, 2 + 4 * j, 2 + 4 * k) for k in range(3) for j in range(3) for i in range(3)]


def _positions_scene(nq, seed):
    """scene s: a cluster of 40 points in neighbour s of an empty brick, nq queries in the brick"""
    rng = np.random.default_rng(seed)
    pts, qs = [], []
    for c, d in zip(_centres(), NEIGHBOURS):
        pts.append(_in_brick(rng, np.add(c, d), 40))
        qs.append(_in_brick(rng, c, nq, 0.02, 0.98))
    return _cloud(pts, 13.25), np.concatenate(qs)


@pytest.mark.parametrize("nq", [1, 5, 8, 9])
def test_all_26_positions(gpu, oracle, nq):
    """the only occupied span of the region at each of the 26 places in turn; 1, 5 and 8 queries are one item, 9 two"""
    xyz, q = _positions_scene(nq, 60 + nq)
    st = _both_ways(gpu, oracle, xyz, q, f"26 positions, {nq} queries", stats=(nq == 9))
    if nq == 9:
        assert st["brick_groups"] == 2 * 26, st      # every query went through the brick kernel, 8 + 1 per brick
        # a region holds its cluster alone: nothing is staged twice (<= 3 padding slots a range)
        assert st["staged_points"] <= 2 * 26 * (40 + 3 * 10), st


@pytest.mark.parametrize("d", [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (-1, 1, -1)])
def test_span_of_more_than_128_points(gpu, oracle, d):
    """300 points in the chosen span; the 200 of its first x cell -- the first records in sorted order, all that stage A
    reads -- lie far from the queries, the true neighbours are among the 100 of the second x cell, which only the
    right-hand remainder of the row (range 9) brings into stage B"""
    rng = np.random.default_rng(70)
    c = np.array((6, 6, 6))
    b = c + d
    first = b + np.concatenate([rng.uniform(0.02, 0.48, (200, 1)), rng.uniform(0.02, 0.98, (200, 2))], 1)
    second = b + np.concatenate([rng.uniform(0.52, 0.98, (100, 1)), rng.uniform(0.02, 0.98, (100, 2))], 1)
    # pull the far cell's points away from the brick and the near cell's towards it along y / z where the span lies there
    for ax in (1, 2):
        if d[ax]:
            far = (0.6, 0.98) if d[ax] > 0 else (0.02, 0.4)
            near = (0.02, 0.3) if d[ax] > 0 else (0.7, 0.98)
            first[:, ax] = b[ax] + rng.uniform(*far, 200)
            second[:, ax] = b[ax] + rng.uniform(*near, 100)
    q = _in_brick(rng, c, 8, 0.02, 0.98)
    q[:, 0] = c[0] + (rng.uniform(0.55, 0.98, 8) if d[0] >= 0 else rng.uniform(0.02, 0.2, 8))
    xyz = _cloud([first, second], 13.25)
    if d[0] <= 0:      # the case is about this: the nearest point is not one stage A can see (at +x the near cell comes first)
        idx = oracle.nn_bruteforce(xyz, q)[0]
        assert (idx > 200).all(), idx
    st = _both_ways(gpu, oracle, xyz, q, f"300 points in span {d}", stats=True)
    assert st["brick_groups"] == 1, st
    assert st["staged_points"] <= 300 + 3 * 10, st     # nothing staged twice: 128 + the remainders, <= 3 padding slots a range


def test_grid_corner_and_face(gpu, oracle):
    """empty query bricks at the grid's lowest corner, on a low face, and at the highest corner of a grid of odd
    dimensions (the last brick is one cell wide): rows outside the grid have zero table entries"""
    rng = np.random.default_rng(71)
    pts = [[0.0, 3.3, 3.3], [3.3, 0.0, 3.3], [3.3, 3.3, 0.0]]                    # the low faces' extent, outside every region below
    pts.append(_in_brick(rng, (1, 1, 0), 40))                                     # corner brick (0, 0, 0): an edge neighbour
    q = [_in_brick(rng, (0, 0, 0), 5, 0.02, 0.98)]
    pts.append(_in_brick(rng, (0, 6, 5), 40))                                     # face brick (0, 5, 5): a face neighbour
    pts.append(_in_brick(rng, (1, 4, 4), 25))                                     # ... and a corner neighbour
    q.append(_in_brick(rng, (0, 5, 5), 8, 0.02, 0.98))
    hi = 9.25                                                                     # 19 cells: brick 9 is cell 18 alone
    pts += [[hi, 5.7, 5.7], [5.7, hi, 5.7], [5.7, 5.7, hi]]                       # the high faces' extent
    pts.append(np.array([8.0, 9.0, 9.0]) + rng.uniform(0.02, 0.98, (40, 3)) * np.array([1.0, 0.25, 0.25]))
    q.append(9.0 + rng.uniform(0.01, 0.24, (5, 3)))
    xyz = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p in pts]).astype(np.float32)
    assert (xyz.min(0) == 0).all() and (xyz.max(0) == np.float32(hi)).all()
    q = np.concatenate(q)
    st = _both_ways(gpu, oracle, xyz, q, "grid corner and face", stats=True)
    assert st["brick_groups"] == 3, st


@pytest.mark.parametrize("sizes", [(30, 50), (50, 30), (40, 40)])
def test_two_candidates_of_one_class(gpu, oracle, sizes):
    """two face neighbours (the fuller one is taken; equal sizes: the lower table entry) beside a fuller edge and a
    fuller corner neighbour, which the class order passes over"""
    rng = np.random.default_rng(72 + sizes[0])
    c = np.array((6, 6, 6))
    pts = [_in_brick(rng, c + (0, -1, 0), sizes[0]), _in_brick(rng, c + (1, 0, 0), sizes[1]),
           _in_brick(rng, c + (1, 1, 0), 90), _in_brick(rng, c + (-1, -1, 1), 120)]
    q = _in_brick(rng, c, 8, 0.02, 0.98)
    _both_ways(gpu, oracle, _cloud(pts, 13.25), q, f"two face neighbours {sizes}")


@pytest.mark.parametrize("d", [(1, 0, 0), (-1, 1, 0), (1, -1, -1)])
def test_single_point_in_the_halo(gpu, oracle, d):
    rng = np.random.default_rng(75)
    c = np.array((6, 6, 6))
    q = np.concatenate([_in_brick(rng, c, 8, 0.02, 0.98), _in_brick(rng, c, 3, 0.02, 0.98)])
    _both_ways(gpu, oracle, _cloud([_in_brick(rng, c + d, 1)], 13.25), q, f"one point at {d}")


@pytest.mark.parametrize("n", [40, 128, 129, 200])
def test_duplicates_fill_the_span(gpu, oracle, n):
    """n copies of one point: every copy is at the same distance, the lowest index has to win -- also when the copies
    straddle stage A's 128 records"""
    rng = np.random.default_rng(76)
    c = np.array((6, 6, 6))
    p = np.repeat(_in_brick(rng, c + (0, 0, -1), 1), n, 0)
    q = _in_brick(rng, c, 8, 0.02, 0.98)
    _both_ways(gpu, oracle, _cloud([p], 13.25), q, f"{n} duplicates")


# ------------------------------------------------------------------------------------------- incoming bounds ----
QB = 70000        # above the small-batch limit: associate and refine take the grid path


def _bounds_scene():
    """the 26 positions again, 70 000 queries spread over the 26 empty bricks"""
    rng = np.random.default_rng(80)
    pts = [_in_brick(rng, np.add(c, d), 40) for c, d in zip(_centres(), NEIGHBOURS)]
    cs = np.array(_centres()[:26], np.float64)
    q = cs[rng.integers(0, 26, QB)] + rng.uniform(0.02, 0.98, (QB, 3))
    # the filler points twice: either half of the cloud (every second point) spans the same grid
    xyz = np.concatenate([np.zeros((2, 3))] + pts + [np.full((2, 3), 13.25)]).astype(np.float32)
    return xyz, q


def test_gate_bounded_association(gpu, oracle):
    """pcd_associate_device with GATE_BOUNDED_SEARCH: d_k = min(gate bound, substitute); gates smaller (0.25 m) and
    larger (1.5 m) than the distance to the substitute's points, which lie 0.1 .. 2.9 m away"""
    import torch
    xyz, q = _bounds_scene()
    nrm = np.tile(np.float32([0, 1, 0]), (len(xyz), 1))
    mr = np.where(np.arange(QB) % 2 == 0, 0.25, 1.5)
    idx, sq, found = oracle.nn_bruteforce(xyz, q)
    out6, ok = oracle.search_nearest_neibor(xyz, nrm, idx, found)
    _, typ, _, _, _ = oracle.associate(q, out6, ok, mr, 0)
    hit = typ != 0
    assert hit[0::2].any() and (~hit[0::2]).any() and hit[1::2].any(), "the gates do not straddle the distances"
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=H)
    try:
        dq, dmr = torch.from_numpy(q).cuda(), torch.from_numpy(mr).cuda()
        for search in (0, 1):
            gpu.set_nn_search(search)
            gpu.set_nn_tuning(0, -1, 1)
            d = dict(type=torch.zeros(QB, dtype=torch.uint8, device="cuda"),
                     nn_idx=torch.zeros(QB, dtype=torch.int32, device="cuda"),
                     nn_sqdist=torch.zeros(QB, dtype=torch.float32, device="cuda"))
            c.associate_device(dq, QB, dmr, QB, gpu.GATE_MAPPER_LOCAL | gpu.GATE_BOUNDED_SEARCH, d)
            torch.cuda.synchronize()
            assert c.last_stats()["brick_groups"] > 0
            assert np.array_equal(d["type"].cpu().numpy(), typ), search
            assert np.array_equal(d["nn_idx"].cpu().numpy().view(np.uint32)[hit], idx[hit]), search
            assert np.array_equal(d["nn_sqdist"].cpu().numpy().view(np.uint32)[hit], sq.view(np.uint32)[hit]), search
    finally:
        gpu.set_nn_search(0)
        gpu.set_nn_tuning(0, -1, 0)
        c.close()


def test_refine_with_incoming_keys(gpu, oracle):
    """pcd_nn_refine_device: the keys come in holding the result on the other half of the cloud (every second cluster
    point and a filler), so a query arrives with a bound that is sometimes nearer than the substitute's points"""
    import torch
    xyz, q = _bounds_scene()
    idx, sq, found = oracle.nn_bruteforce(xyz, q)
    assert found.all()
    shards = [gpu.Cloud(xyz[s::2], np.zeros_like(xyz[s::2]), raw_lidar_frame=False, cell_size=H, index_base=s,
                        index_stride=2) for s in range(2)]
    try:
        dq = torch.from_numpy(q).cuda()
        for search in (0, 1):
            gpu.set_nn_search(search)
            keys = torch.empty(QB, dtype=torch.int64, device="cuda")
            shards[0].nn_device(dq, QB, keys, gpu.NN_GRID)
            shards[1].nn_refine_device(dq, QB, keys)
            torch.cuda.synchronize()
            k = keys.cpu().numpy().astype(np.uint64)
            assert np.array_equal((k & 0xFFFFFFFF).astype(np.uint32), idx), search
            assert np.array_equal((k >> 32).astype(np.uint32), sq.view(np.uint32)), search
    finally:
        gpu.set_nn_search(0)
        for s in shards:
            s.close()


# ------------------------------------------------------------------------------------------------- a sheet ----
SHEET_H = 0.6
# staged_points of the clip-on NN_GRID call below with the statistics on, measured on the parent commit 909c1f5
# ("Compact the NN fallback pyramid to its occupied nodes"), whose kernel leaves an empty brick's d_k at its incoming
# value, with
#     python tools/brick_seed_counts.py
# run on a checkout of that commit with this file and the script added (the script imports sheet_input from this
# file).  tools/brick_clip_sim.py's model (the script prints it too) gives 418 002 for that kernel and 330 678 for the
# substitute rule on this input: a ratio of 0.79, so the 0.95 below is not marginal (measured with the substitute:
# 330 766).  Which queries share an item varies from run to run (tests/test_nn_bookkeeping_gpu.py allows 5 % for that).
PARENT_SHEET_STAGED = 419526


def sheet_input():
    """20 000 points on a tilted plane (6 and 8.5 degrees about two axes, 16 m x 16 m: 28 points per occupied cell of
    0.6 m), 4 000 queries pushed 0.3 .. 0.6 m off it to either side"""
    rng = np.random.default_rng(90)
    n = np.array([0.1, 1.0, 0.15])
    n /= np.linalg.norm(n)
    e1 = np.cross(n, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    uv = rng.uniform(-8.0, 8.0, (20000, 2))
    xyz = (np.array([12.0, 12.0, 12.0]) + uv[:, :1] * e1 + uv[:, 1:] * e2).astype(np.float32)
    pick = rng.integers(0, len(xyz), 4000)
    off = rng.uniform(0.3, 0.6, 4000) * rng.choice([-1.0, 1.0], 4000)
    q = xyz[pick].astype(np.float64) + off[:, None] * n + rng.normal(0, 0.02, (4000, 3))
    return xyz, q


def sheet_staged(gpu, oracle=None):
    xyz, q = sheet_input()
    if oracle is not None:
        return _both_ways(gpu, oracle, xyz, q, "sheet", h=SHEET_H, stats=True)["staged_points"]
    c = gpu.Cloud(xyz, np.zeros_like(xyz), raw_lidar_frame=False, cell_size=SHEET_H)
    try:
        gpu.set_nn_tuning(0, -1, 1)
        c.nn(q, gpu.NN_GRID)
        return c.last_stats()["staged_points"]
    finally:
        gpu.set_nn_tuning(0, -1, 0)
        c.close()


def test_sheet_stages_less_than_the_parent(gpu, oracle):
    got = sheet_staged(gpu, oracle)
    print("sheet: staged_points", got, "parent", PARENT_SHEET_STAGED, "ratio %.3f" % (got / PARENT_SHEET_STAGED))
    assert got <= 0.95 * PARENT_SHEET_STAGED, (got, PARENT_SHEET_STAGED)

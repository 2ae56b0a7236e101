"""tests/cloud_ref.py on hand-computed cases, its shard split against pcdhip.dist, and the rounding property that makes
the refine bound of the sharded search safe.  No device."""
import numpy as np

from pcdhip import dist
from tests import cloud_ref as ref

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_tight_box_by_hand():
    m, lo, hi = ref.tight_box([[1, 2, 3], [-1, 5, 0], [np.inf, -9, 9], [0, 0, np.nan]])
    assert m == 2 and lo.tolist() == [-1, 2, 0] and hi.tolist() == [1, 5, 3]
    m, lo, hi = ref.tight_box(np.zeros((0, 3)))
    assert m == 0 and not lo.any() and not hi.any()
    m, lo, hi = ref.tight_box([[np.inf, 0, 0]])
    assert m == 0 and _bits(lo).tolist() == [0, 0, 0] and _bits(hi).tolist() == [0, 0, 0]
    # signed zeros: the minimum is -0.0 and the maximum +0.0 whatever the row order
    for rows in ([[0.0, -0.0, 1], [-0.0, 0.0, 1]], [[-0.0, 0.0, 1], [0.0, -0.0, 1]]):
        m, lo, hi = ref.tight_box(rows)
        assert _bits(lo).tolist() == [0x80000000, 0x80000000, 0x3F800000]
        assert _bits(hi).tolist() == [0, 0, 0x3F800000]


def test_grid_info_by_hand():
    x = np.array([[0, 0, 0], [0.5, 0, 0], [1, 0, 0], [0.26, 0, 0], [np.inf, 0, 0]], F)
    g = ref.grid_info(x, 0.5)
    # extent 1: floor(1 / 0.5) + 1 = 3 cells; x = 1 bins to floor(2) = 2, 0.26 to 0: cells {0, 1, 2}
    assert g["len"] == 5 and g["num_indexed"] == 4
    assert g["dims"] == [3, 1, 1] and g["block_dims"] == [1, 1, 1] and g["occupied_cells"] == 3
    assert g["bbox_lo"].tolist() == [0, 0, 0] and g["bbox_hi"].tolist() == [1, 0, 0] and g["origin"].tolist() == [0, 0, 0]
    g = ref.grid_info(x, 0.25)
    # floor(1 / 0.25) + 1 = 5 cells -> 2 blocks of 4; cells {0, 2, 4, 1}
    assert g["dims"] == [5, 1, 1] and g["block_dims"] == [2, 1, 1] and g["occupied_cells"] == 4
    g = ref.grid_info(x, 50.0)
    assert g["dims"] == [1, 1, 1] and g["occupied_cells"] == 1
    # floor(extent / h) + 1 per axis: floor(2) + 1, floor(1.8) + 1, floor(0.8) + 1
    assert ref.grid_dims([0, 0, 0], [1.0, 0.9, 0.4], 0.5).tolist() == [3, 2, 1]
    # a row on the upper face bins past the last cell in float and is clamped into it
    y = np.array([[0, 0, 0], [3, 3, 3]], F)
    assert ref.cell_coords(y, [0, 0, 0], 1.5, [3, 3, 3]).tolist() == [[0, 0, 0], [2, 2, 2]]
    assert ref.cell_coords(y, [0, 0, 0], 1.0, [3, 3, 3]).tolist() == [[0, 0, 0], [2, 2, 2]]   # floor(3) = 3 -> 2
    g = ref.grid_info(np.zeros((0, 3), F), 1.0)
    assert g["num_indexed"] == 0 and g["dims"] == [1, 1, 1] and g["occupied_cells"] == 0 and g["len"] == 0
    # binning is float32: (p - o) * inv_h with inv_h = fl(1 / 0.1) = 10 exactly, (0.3f - 0) * 10 = 3.0000001 -> 3,
    # where the double quotient 0.3f / 0.1f = 2.99999996 would give 2
    z = np.array([[0, 0, 0], [F(0.3), 0, 0], [0.35, 0, 0]], F)
    assert ref.cell_coords(z, [0, 0, 0], F(0.1), [4, 1, 1])[:, 0].tolist() == [0, 3, 3]
    assert ref.grid_info(z, F(0.1))["occupied_cells"] == 2


def test_effective_cell_size_by_hand():
    lo, hi = np.zeros(3, F), np.array([2000, 2000, 2], F)
    # start cbrt(2000.001^2 * 2.001 / 2^26) = 0.49230: 4063^2 * 5 cells = 82.5 M > 2^26; one step of 1.05 -> 0.51692:
    # 3870^2 * 4 = 59.9 M fits
    h0 = np.cbrt(2000.001 * 2000.001 * 2.001 / 2 ** 26)
    assert abs(h0 - 0.49230) < 1e-4
    assert (np.floor(2000 / h0) + 1) ** 2 * (np.floor(2 / h0) + 1) > 2 ** 26
    h = ref.effective_cell_size(lo, hi, 20000, 0.05)
    assert h.dtype == np.float32 and h == F(h0 * 1.05) and abs(float(h) - 0.51692) < 1e-4
    assert np.prod(ref.grid_dims(lo, hi, h)) <= 2 ** 26
    assert ref.effective_cell_size(lo, hi, 20000, 2.0) == F(2.0)            # above the budget size: kept
    assert ref.effective_cell_size(lo, hi, 0, 0.05) == F(0.05)              # no finite row
    assert ref.effective_cell_size(lo, lo, 7, 0.05) == F(0.05)              # every row identical: extent 0
    # a line of 1000 km: the relative floor 1e-6 * extent = 1 m is above the budget size (1e6 / 2^26 = 0.0149 m)
    far = np.array([1e6, 0, 0], F)
    assert ref.effective_cell_size(lo, far, 10, 0.1) == F(1.0)
    assert 0.0149 < ref.budget_min_cell([1e6, 0.0, 0.0]) < 0.0149 * 1.05 ** 2
    # a 20 m body with strays at +-1e5 m on two axes: 2e5 x 1e5 x 20 m
    ext = [2e5, 1e5, 20.0]
    hb = ref.budget_min_cell(ext)
    cells = lambda v: np.prod([np.floor(e / v) + 1 for e in ext])
    assert cells(hb) <= 2 ** 26 < cells(hb / 1.05)
    assert ref.effective_cell_size(lo, np.array(ext, F), 50002, 0.3) == F(hb)


def test_shard_split_by_hand():
    x = np.array([[0.5, 0, 0], [0.2, 0, 1.5], [np.inf, 0, 0], [1.5, 0, 0], [0.1, 0, 0]], F)
    # finite minimum (0.1, 0, 0): cells (0,0,0) (0,0,1) - (1,0,0) (0,0,0); the Inf row has key 0
    assert ref.shard_keys(x).tolist() == [0, 1 << 42, 0, 1, 0]
    order, cuts, boxes = ref.shard_split(x, 2)
    assert order.tolist() == [0, 2, 4, 3, 1] and cuts == [0, 2, 5]
    assert boxes[0].tolist() == [0.5, 0, 0, 0.5, 0, 0]
    assert np.array_equal(boxes[1], np.array([0.1, 0, 0, 1.5, 0, 1.5], F))
    order, cuts, boxes = ref.shard_split(x, 4)
    assert cuts == [0, 1, 2, 3, 5]
    assert boxes[1].tolist() == [np.inf] * 3 + [-np.inf] * 3          # shard 1 = the Inf row alone: inverted box
    order, cuts, boxes = ref.shard_split(x[:3], 4)                    # more shards than rows
    assert cuts == [0, 0, 1, 2, 3] and boxes[0].tolist() == [np.inf] * 3 + [-np.inf] * 3
    order, cuts, boxes = ref.shard_split(np.zeros((0, 3), F), 3)
    assert order.size == 0 and cuts == [0, 0, 0, 0] and np.isinf(boxes).all()
    # y outranks x, z outranks y
    y = np.array([[5, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], F)
    assert ref.shard_split(y, 1)[0].tolist() == [3, 0, 1, 2]
    # the cap: every cell past 2 097 151 shares the last key of its axis
    z = np.array([[0, 0, 0], [5e6, 0, 0], [4e6, 0, 0], [2097151, 0, 0], [2097150.5, 0, 0]], F)
    assert ref.shard_keys(z).tolist() == [0, 2097151, 2097151, 2097151, 2097150]
    assert ref.shard_split(z, 1)[0].tolist() == [0, 4, 1, 2, 3]


def test_shard_split_equals_dist():
    rng = np.random.default_rng(11)
    clouds = [(rng.random((5000, 3)) * [40, 6, 25] - [20, 3, 0]).astype(F),
              (rng.random((777, 3)) * 0.9 + 3e6).astype(F),                 # one cell far from the origin
              np.repeat(np.array([[1.25, -3, 7]], F), 50, axis=0),
              np.zeros((0, 3), F), np.array([[np.inf, 0, 0]], F)]
    bad = clouds[0].copy()
    bad[rng.integers(0, 5000, 60), rng.integers(0, 3, 60)] = np.inf
    bad[rng.integers(0, 5000, 60), rng.integers(0, 3, 60)] = -np.inf
    bad[17] = np.nan                                                        # (a handle built without the filter)
    clouds.append(bad)
    for x in clouds:
        for ndev in (1, 2, 3, 4, 7, 64):
            order, cuts, _ = ref.shard_split(x, ndev)
            if x.shape[0]:
                assert np.array_equal(order, dist.compact_order(x)), (x.shape, ndev)
            assert cuts == dist.shard_cuts(x.shape[0], ndev)
            assert np.array_equal(np.sort(order), np.arange(x.shape[0]))


def test_refine_active_by_hand():
    lo, hi = [0, 0, 0], [1, 1, 1]
    one = _bits([1.0])
    below = _bits([np.nextafter(F(1), F(0))])
    q = np.array([[2, 0.5, 0.5]])
    assert ref.box_distance(q, lo, hi).tolist() == [1.0]
    assert ref.refine_active(q, lo, hi, one).tolist() == [True]             # equality is kept
    assert ref.refine_active(q, lo, hi, below).tolist() == [False]
    assert ref.refine_active([[0.3, 0.9, 0.1]], lo, hi, _bits([0.0])).tolist() == [True]     # inside: distance 0
    assert ref.box_distance([[3, -2, 0.5]], lo, hi).tolist() == [8.0]
    q = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, 0, 1e39]])            # 1e39 is Inf as a float
    assert ref.refine_active(q, lo, hi, [ref.FLT_MAX_BITS] * 3).tolist() == [False] * 3
    # a shard without a finite row never refines, even for a query that has no result yet
    assert ref.refine_active([[0.5, 0.5, 0.5]], [np.inf] * 3, [-np.inf] * 3, [ref.FLT_MAX_BITS]).tolist() == [False]
    # the query is rounded to float first: 2 + 1e-9 is 2
    assert ref.refine_active([[2 + 1e-9, 0.5, 0.5]], lo, hi, one).tolist() == [True]


def test_refine_bound_is_monotone():
    """fl_dist(q, clamp(q, box)) <= fl_dist(q, p) for every p in the box, with no slack at all: per axis the clamp lies
    between q and p, float subtraction, squaring and addition are monotone.  1.2 M triples, near the origin and at
    offsets where a float ulp is 8 mm and 25 cm."""
    rng = np.random.default_rng(5)
    n = 400000
    for off in (0.0, 1e5, 3e6):
        lo = (off + rng.normal(0, 30, (n, 3))).astype(F)
        size = rng.random((n, 3)) * np.array([20, 20, 2]) * (rng.random((n, 1)) < 0.8)     # 20 % degenerate boxes
        hi = np.maximum(lo, (lo.astype(np.float64) + size).astype(F))
        p = np.clip((lo + rng.random((n, 3)) * (hi.astype(np.float64) - lo)).astype(F), lo, hi)
        face = rng.random((n, 3)) < 0.2
        p = np.where(face, np.where(rng.random((n, 3)) < 0.5, lo, hi), p)                   # points on the faces
        q = off + rng.normal(0, 40, (n, 3))
        q = np.where(rng.random((n, 3)) < 0.15, p.astype(np.float64), q)                    # shared coordinates
        q = np.where(rng.random((n, 3)) < 0.05, np.nextafter(hi, F(np.inf)).astype(np.float64), q)
        qf = q.astype(F)
        clamp = np.fmin(np.fmax(qf, lo), hi)
        db = ref._l2_simple3(qf, clamp)
        dp = ref.point_distance(q, p)
        assert (db <= dp).all(), (off, np.nonzero(db > dp)[0][:5])
        assert (db == dp).any() and (db < dp).any()
        # the scalar-box form the tests use agrees with the vectorised one
        for i in range(0, 50):
            assert ref.box_distance(q[i], lo[i], hi[i])[0] == db[i]

"""The sharded search (csrc/shards.hip and the refine form of csrc/nn.hip) at its degenerate splits, all shards on
device 0.  The expected result is always the single handle's, which is compared with the oracle in the same test; the
split itself (permutation, cuts, boxes) and the refine predicate are compared with tests/cloud_ref.py.  Everything is
bit-exact: index, float bits, flags, every association field."""
import ctypes as C

import numpy as np
import pytest
import torch

from pcdhip import dist, synth
from tests import cloud_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
FIELDS = ("type", "nn_idx", "nn_sqdist", "lidar_xyz", "abcd", "dist", "angle", "dist2plane")


def _exact(a, b, what):
    for x, y, n in zip(a, b, ("idx", "sqdist", "found")):
        xv = x.view(np.uint32) if x.dtype == np.float32 else x
        yv = y.view(np.uint32) if y.dtype == np.float32 else y
        bad = np.nonzero(xv != yv)[0]
        assert bad.size == 0, f"{what}: {n} differs at {bad[:5]}: {x[bad[:5]]} vs {y[bad[:5]]}"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bytes_equal(a, b, what):
    for k in FIELDS:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


def _normals(n, seed=1):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F).reshape(n, 3)


def _around(xyz, n, seed, sigma=0.4):
    """queries around the finite rows, a few far away and a few non-finite"""
    rng = np.random.default_rng(seed)
    fin = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    if fin.shape[0] == 0:
        fin = np.zeros((1, 3))
    q = fin[rng.integers(0, fin.shape[0], n)] + rng.normal(0, sigma, (n, 3))
    q[: n // 8] = fin[rng.integers(0, fin.shape[0], n // 8)]          # on a row
    q[n // 8: n // 8 + 5] += 500.0
    q[n // 8 + 5] = np.nan
    q[n // 8 + 6, 1] = np.inf
    return q


def _check_split(sh, hx, hn, ndev):
    """every borrowed shard handle against the reference split: rows, order, box"""
    order, cuts, boxes = ref.shard_split(hx, ndev)
    assert sh.count() == ndev and len(sh) == hx.shape[0]
    for s in range(ndev):
        rows = order[cuts[s]:cuts[s + 1]]
        c = sh.shard(s)
        assert len(c) == rows.size, s
        dx, dn = c.download()
        assert np.array_equal(_bits(dx), _bits(hx[rows])), f"shard {s}: rows or their order differ"
        assert np.array_equal(_bits(dn), _bits(hn[rows])), s
        info = c.info()
        m = int(np.isfinite(hx[rows]).all(axis=1).sum())
        assert info["num_indexed"] == m, s
        if m:
            assert _bits(info["bbox_lo"]).tolist() == _bits(boxes[s, :3]).tolist(), s
            assert _bits(info["bbox_hi"]).tolist() == _bits(boxes[s, 3:]).tolist(), s
        else:
            assert np.isinf(boxes[s]).all()
        c.close()
    return order, cuts, boxes


def _shard_alone(sh, oracle, hx, order, cuts, s, q):
    """a shard handle queried on its own answers with GLOBAL indices: the oracle over its rows taken in the order of
    their original indices (a tie goes to the lowest ORIGINAL index, whatever the row order inside the shard)"""
    rows = np.sort(order[cuts[s]:cuts[s + 1]])
    idx, sq, found = oracle.nn_bruteforce(hx[rows], q)
    gidx = np.where(found.astype(bool), rows[np.minimum(idx, max(rows.size - 1, 0))] if rows.size else 0, 0xFFFFFFFF)
    c = sh.shard(s)
    got = c.nn(q)
    _exact(got, (gidx.astype(np.uint32), sq, found), f"shard {s} alone")
    c.close()
    return dist.pack_keys(*got)


def _check_refine(sh, q, boxes, own_keys):
    """pcd_nn_refine_device of every shard on the keys of the PREVIOUS shard: a query is searched iff the reference
    predicate holds -- then the key is the minimum of the two -- and otherwise leaves with the key it came with; and
    the predicate never drops a query the shard would have improved"""
    ndev = len(own_keys)
    dq = torch.from_numpy(np.ascontiguousarray(q, np.float64)).cuda()
    hit = 0
    for s in range(ndev):
        inc = own_keys[(s - 1) % ndev]
        own = own_keys[s]
        sqbits = np.where(inc == dist.KEY_NONE, ref.FLT_MAX_BITS, inc >> 32).astype(np.uint32)
        active = ref.refine_active(q, boxes[s, :3], boxes[s, 3:], sqbits)
        exp = np.where(active, np.minimum(inc, own), inc)
        keys = torch.from_numpy(inc.copy()).cuda()
        c = sh.shard(s)
        c.nn_refine_device(dq, q.shape[0], keys)
        torch.cuda.synchronize()
        got = keys.cpu().numpy()
        c.close()
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (s, bad[:5], got[bad[:5]], exp[bad[:5]], active[bad[:5]])
        assert np.array_equal(exp, np.minimum(inc, own)), f"shard {s}: the bound dropped a query it would have improved"
        edge = ref.box_distance(q, boxes[s, :3], boxes[s, 3:]).view(np.uint32) == sqbits
        hit += int((edge & (own < inc)).sum())
    return hit


def _check_all(gpu, oracle, xyz, nrm, ndev, q, what, split=True, assoc=True, **kw):
    """single handle vs oracle, sharded vs single (search and association), the split against the reference"""
    hx = kw.pop("hx", xyz)
    hn = kw.pop("hn", nrm)
    single = gpu.Cloud(xyz, nrm, **kw)
    want = single.nn(q)
    _exact(want, oracle.nn_bruteforce(hx, q), f"{what}: single cloud vs oracle")
    sh = gpu.ShardedCloud(xyz, nrm, [0] * ndev, **kw)
    assert len(sh) == len(single) == hx.shape[0]
    _exact(sh.nn(q), want, f"{what}: {ndev} shards")
    split_out = _check_split(sh, hx, hn, ndev) if split else None
    if assoc:
        for mode in (gpu.GATE_MAPPER_LOCAL, gpu.GATE_MAPPER_GLOBAL, gpu.GATE_CONTROLLER):
            _bytes_equal(sh.associate(q, 1.5, mode), single.associate(q, 1.5, mode), (what, mode))
    single.close()
    return sh, want, split_out


# ------------------------------------------------------------------ split parity
@pytest.mark.parametrize("ndev", [1, 3, 4])
def test_split_parity(gpu, oracle, ndev):
    rng = np.random.default_rng(40)
    n = 9000
    xyz = (rng.random((n, 3)) * [9, 5, 14] - [3, 2, 30]).astype(F)
    src, dst = rng.integers(0, n // 2, 200), rng.integers(n // 2, n, 200)
    xyz[dst] = xyz[src]                                                  # duplicates far apart in the file
    xyz[rng.choice(n, 40, replace=False), rng.integers(0, 3, 40)] = np.inf
    nrm = _normals(n)
    q = _around(xyz, 1500, seed=1)
    q[:200] = xyz[src]
    q[~np.isfinite(q).all(axis=1)] = np.nan
    sh, want, (order, cuts, boxes) = _check_all(gpu, oracle, xyz, nrm, ndev, q, "split parity", raw_lidar_frame=False)
    own = [_shard_alone(sh, oracle, xyz, order, cuts, s, q) for s in range(ndev)]
    _check_refine(sh, q, boxes, own)
    sh.close()


# ------------------------------------------------------------------ degenerate splits
def _degenerate(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "0 rows / 4":
        return np.zeros((0, 3), F), 4
    if name == "1 row / 4":
        return np.array([[0.5, -1, 2]], F), 4
    if name == "3 rows / 4":
        return np.array([[0.5, -1, 2], [0.5, -1, 7.5], [3, 0, 2]], F), 4
    if name == "inf half / 2":        # shard 0 = the four Inf rows: no finite row, inverted box
        return np.array([[np.inf, 0, 0], [0, -np.inf, 0], [np.inf, np.inf, np.inf], [1, 1, np.inf],
                         [1, 1, 1], [3, 1, 1], [1, 3, 1], [1, 1, 3]], F), 2
    if name == "one sort cell / 3":
        return (rng.random((300, 3)) * 0.9 + [10, -4, 2]).astype(F), 3
    if name == "identical / 4":
        return np.repeat(np.array([[2.5, 1.25, -3]], F), 100, axis=0), 4
    if name == "1 k rows / 64":
        return (rng.random((1000, 3)) * [6, 3, 20]).astype(F), 64
    raise KeyError(name)


@pytest.mark.parametrize("name", ["0 rows / 4", "1 row / 4", "3 rows / 4", "inf half / 2", "one sort cell / 3",
                                  "identical / 4", "1 k rows / 64"])
def test_degenerate_splits(gpu, oracle, name):
    xyz, ndev = _degenerate(name)
    n = xyz.shape[0]
    nrm = _normals(n)
    q = _around(xyz, 400, seed=3)
    sh, want, (order, cuts, boxes) = _check_all(gpu, oracle, xyz, nrm, ndev, q, name, raw_lidar_frame=False)
    fin = np.isfinite(q).all(axis=1)
    if n == 0:
        assert not want[2].any()
    if name == "identical / 4":
        assert (want[0][fin] == 0).all() and (want[2][fin] == 1).all()       # index 0 wins every tie
    if name == "inf half / 2":
        assert order.tolist() == list(range(8)) and np.isinf(boxes[0]).all() and (want[0][fin] >= 4).all()
    own = [_shard_alone(sh, oracle, xyz, order, cuts, s, q) for s in range(ndev)]
    _check_refine(sh, q, boxes, own)
    sh.close()


# ------------------------------------------------------------------ ties across cuts
@pytest.mark.parametrize("ndev", [2, 3, 4, 7])
def test_lattice_ties_across_cuts(gpu, oracle, ndev):
    """integer lattice, 1 m spacing, file order reversed: the sort cells hold one row each, with 4 shards the cuts fall
    on cell borders (two z layers per shard) and the boxes touch nowhere but leave exactly 1 m between them; of two rows
    at the same distance the LOWER original index sits in the LATER shard.  Queries at half-integer positions are 2-, 4-
    and 8-way ties, those between two layers of different shards are ties across the cut, at the box distance exactly."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    lat = g[np.lexsort((g[:, 0], g[:, 1], g[:, 2]))].astype(F)          # z-major
    xyz = np.ascontiguousarray(lat[::-1])
    n = xyz.shape[0]
    nrm = _normals(n)
    h = np.stack(np.meshgrid(np.arange(-1, 12), np.arange(-1, 10), np.arange(-1, 16), indexing="ij"), axis=-1).reshape(-1, 3)
    q = h.astype(np.float64) * 0.5                                        # every lattice point and every half position
    sh, want, (order, cuts, boxes) = _check_all(gpu, oracle, xyz, nrm, ndev, q, "lattice", raw_lidar_frame=False)
    assert np.array_equal(order, np.arange(n - 1, -1, -1))
    own = [_shard_alone(sh, oracle, xyz, order, cuts, s, q) for s in range(ndev)]
    hit = _check_refine(sh, q, boxes, own)
    assert hit > 0, "no query tied across a cut at exactly the box distance"
    # of the tied rows the lowest index won although its shard comes later
    between = (q[:, 2] % 1 == 0.5) & (q[:, 2] > 0) & (q[:, 2] < 7)
    s_of = np.searchsorted(np.array(cuts[1:]), order.argsort()[want[0][between]], side="right")
    home = dist.home_shards(q[between], boxes[:, :3], boxes[:, 3:])
    if ndev > 1:
        assert (s_of > home).any()
    sh.close()


def test_duplicates_in_three_shards(gpu, oracle):
    """500 copies of one point in the middle of 900 rows over 3 shards: the run of equal keys spans both cuts, every
    shard holds copies, and the lowest original index among them wins"""
    rng = np.random.default_rng(9)
    P = np.array([1.25, 0.5, 10.5], F)
    xyz = np.concatenate([(rng.random((200, 3)) * [3, 2, 9]).astype(F), np.repeat(P[None], 500, axis=0),
                          (rng.random((200, 3)) * [3, 2, 9] + [0, 0, 12]).astype(F)])
    perm = rng.permutation(900)
    xyz = np.ascontiguousarray(xyz[perm])
    nrm = _normals(900)
    first = int(np.nonzero((xyz == P).all(axis=1))[0][0])
    q = _around(xyz, 600, seed=4, sigma=1.0)
    q[:50] = P.astype(np.float64)
    sh, want, (order, cuts, boxes) = _check_all(gpu, oracle, xyz, nrm, 3, q, "duplicates", raw_lidar_frame=False)
    assert (want[0][:50] == first).all()
    for s in range(3):
        assert (xyz[order[cuts[s]:cuts[s + 1]]] == P).all(axis=1).any(), s
    own = [_shard_alone(sh, oracle, xyz, order, cuts, s, q) for s in range(3)]
    _check_refine(sh, q, boxes, own)
    sh.close()


# ------------------------------------------------------------------ box faces
def test_box_faces(gpu, oracle):
    """queries exactly on the planes of every shard's box, one float ulp to either side, and half way between the
    facing planes of neighbouring boxes"""
    rng = np.random.default_rng(17)
    xyz = (rng.random((6000, 3)) * [4, 4, 12]).astype(F)
    nrm = _normals(6000)
    order, cuts, boxes = ref.shard_split(xyz, 3)
    qs = []
    for s in range(3):
        for d in range(3):
            for plane in (boxes[s, d], boxes[s, 3 + d]):
                for v in (plane, np.nextafter(plane, F(np.inf)), np.nextafter(plane, F(-np.inf))):
                    p = rng.random((40, 3)) * [4, 4, 12]
                    p[:, d] = np.float64(v)
                    qs.append(p)
                    p = p.copy()
                    p[:, 2] = np.float64(v) if d == 2 else boxes[s, 2] + (boxes[s, 5] - boxes[s, 2]) * rng.random(40)
                    qs.append(p)
        t = (s + 1) % 3
        mid = (np.float64(boxes[s, 5]) + np.float64(boxes[t, 2])) / 2        # equidistant from two boxes in z
        p = rng.random((40, 3)) * [4, 4, 12]
        p[:, 2] = mid
        qs.append(p)
    corners = np.array([[boxes[s, 3 * i], boxes[s, 1 + 3 * j], boxes[s, 2 + 3 * k]] for s in range(3) for i in (0, 1)
                        for j in (0, 1) for k in (0, 1)], np.float64)
    q = np.concatenate(qs + [corners, corners + 0.75, corners - 0.75], axis=0)
    sh, want, (o2, c2, b2) = _check_all(gpu, oracle, xyz, nrm, 3, q, "box faces", raw_lidar_frame=False)
    assert np.array_equal(_bits(b2), _bits(boxes))
    own = [_shard_alone(sh, oracle, xyz, order, cuts, s, q) for s in range(3)]
    _check_refine(sh, q, boxes, own)
    sh.close()


# ------------------------------------------------------------------ key cap
def test_key_cap(gpu, oracle):
    """two clusters 5e6 m apart: the far one lies past the 2 097 151-cell cap of the sort key, where every row shares
    one key per axis (and a float ulp is 0.5 m: many exact ties)"""
    rng = np.random.default_rng(23)
    a = (rng.random((300, 3)) * [3, 3, 3]).astype(F)
    b = (rng.random((300, 3)) * [30, 3, 3] + [5e6, 0, 0]).astype(F)
    xyz = np.ascontiguousarray(np.concatenate([a, b])[rng.permutation(600)])
    assert int(ref.shard_keys(xyz).max()) & 0x1FFFFF == ref.KEY_CAP
    nrm = _normals(600)
    q = _around(xyz, 600, seed=6, sigma=1.0)
    q[100:120] = [2.5e6, 1, 1] + rng.normal(0, 10, (20, 3))               # midway
    sh, want, (order, cuts, boxes) = _check_all(gpu, oracle, xyz, nrm, 3, q, "key cap", raw_lidar_frame=False)
    own = [_shard_alone(sh, oracle, xyz, order, cuts, s, q) for s in range(3)]
    _check_refine(sh, q, boxes, own)
    sh.close()


# ------------------------------------------------------------------ large batch
def test_large_batch(gpu, oracle):
    """Q = 70 000 > 65536: both refine phases of every shard go through the grid path"""
    xyz, nrm = synth.cloud_planes(20000, seed=14, patches=12)
    q = synth.queries(xyz, 70000, seed=8)
    q[7] = np.nan
    exp = oracle.KDTree(xyz).query(q)
    single = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    _exact(single.nn(q), exp, "single cloud vs kd-tree")
    sh = gpu.ShardedCloud(xyz, nrm, [0, 0, 0], raw_lidar_frame=False)
    _exact(sh.nn(q), exp, "3 shards, 70 000 queries")
    mr = synth.max_range_schedule(70000, seed=2)
    _bytes_equal(sh.associate(q, mr, gpu.GATE_MAPPER_LOCAL), single.associate(q, mr, gpu.GATE_MAPPER_LOCAL), "70 000")
    single.close(); sh.close()


# ------------------------------------------------------------------ layouts and filter
def test_layouts_and_filter(gpu, oracle):
    """raw frame + NaN rows (position, normal) + Inf rows + the AOS32 layout with junk in its pad floats through
    pcd_cloud_create_sharded: indices are post-filter, a NaN pad does not drop a row"""
    rng = np.random.default_rng(12)
    n = 8000
    raw = np.zeros((n, 8), F)
    raw[:, :3] = rng.random((n, 3)) * [14, 6, 4] - [0, 3, 2]
    raw[:, 4:7] = _normals(n)
    raw[:, 3] = np.array([np.nan, np.inf, 3.5, 0], F)[rng.integers(0, 4, n)]
    raw[:, 7] = np.array([np.nan, -np.inf, -1e30, 0], F)[rng.integers(0, 4, n)]
    raw[rng.choice(n, 100, replace=False), rng.integers(0, 3, 100)] = np.nan
    raw[rng.choice(n, 100, replace=False), 4 + rng.integers(0, 3, 100)] = np.nan
    raw[rng.choice(n, 30, replace=False), rng.integers(0, 3, 30)] = np.inf
    raw[0, 0], raw[n - 1, 6] = np.nan, np.nan
    keep = ~np.isnan(raw[:, [0, 1, 2, 4, 5, 6]]).any(axis=1)
    f = lambda a: np.stack([-a[:, 1], -a[:, 2], a[:, 0]], axis=1).astype(F)
    hx, hn = f(raw[keep, :3]), f(raw[keep, 4:7])
    ox, on = oracle.direction_trans(np.ascontiguousarray(raw[:, :3]), np.ascontiguousarray(raw[:, 4:7]))
    assert np.array_equal(_bits(ox), _bits(hx)) and np.array_equal(_bits(on), _bits(hn))
    assert n - 202 <= hx.shape[0] < n - 150
    q = _around(hx, 2000, seed=2)
    sh, want, _ = _check_all(gpu, oracle, raw, None, 3, q, "aos32 raw frame", raw_lidar_frame=True,
                             layout=gpu.LAYOUT_AOS32, hx=hx, hn=hn)
    sh.close()
    # the same rows as two arrays
    sh, _, _ = _check_all(gpu, oracle, np.ascontiguousarray(raw[:, :3]), np.ascontiguousarray(raw[:, 4:7]), 4, q,
                          "two arrays raw frame", raw_lidar_frame=True, hx=hx, hn=hn)
    _exact(sh.nn(q), want, "layouts agree")
    sh.close()


# ------------------------------------------------------------------ association
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_association_modes(gpu, oracle, mode):
    xyz, nrm = synth.cloud_planes(12000, seed=15, patches=8)
    Q = 3000
    q = synth.queries(xyz, Q, seed=9)
    q[11] = np.nan
    rng = np.random.default_rng(1)
    mrq = synth.max_range_schedule(Q, seed=3)
    mrq[rng.choice(Q, 150, replace=False)] = np.nan
    mrq[rng.choice(Q, 150, replace=False)] = -1.0
    mrq[rng.choice(Q, 50, replace=False)] = 0.0
    single = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    sh = gpu.ShardedCloud(xyz, nrm, [0] * 3, raw_lidar_frame=False)
    idx, sq, found = oracle.nn_bruteforce(xyz, q)
    for mr in (mrq, 1.2, np.nan, -1.0):
        a = single.associate(q, mr, mode)
        assert np.array_equal(a["nn_idx"], idx) and np.array_equal(_bits(a["nn_sqdist"]), _bits(sq))
        b = sh.associate(q, mr, mode)
        _bytes_equal(b, a, (mode, "per query" if mr is mrq else mr))
        _bytes_equal(sh.associate(q, mr, mode | gpu.GATE_BOUNDED_SEARCH), a, (mode, "bounded flag"))
    assert 0 < (single.associate(q, mrq, mode)["type"] != 0).sum() < Q
    single.close(); sh.close()


# ------------------------------------------------------------------ callbacks
def _view(ptr, count, dtype):
    class _A:   # noqa: N801
        pass
    a = _A()
    a.__cuda_array_interface__ = {"shape": (count,), "typestr": dtype, "data": (ptr, False), "version": 2}
    return torch.as_tensor(a, device="cuda:0")


def _reducer(op, dtype, calls, name, fail=None):
    def fn(user, bufs, devices, n, count):
        calls[name] += 1
        if fail is not None and fail["on"]:
            return 1
        ts = [_view(bufs[s], count, dtype) for s in range(n)]
        m = ts[0].clone()
        for t in ts[1:]:
            m = op(m, t)
        for t in ts:
            t.copy_(m)
        torch.cuda.synchronize()
        return 0
    return fn


def test_callbacks(gpu, oracle):
    """one member of pcd_shard_reduce given, the other NULL (that step runs the library's own reduction); a callback that
    fails: PCD_ERR_INVALID with its message, and the same handle answers correctly on the next call"""
    xyz, nrm = synth.cloud_uniform(6000, seed=5, box=np.array([6.0, 3.0, 15.0]))
    q = _around(xyz, 1500, seed=5)
    single = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    want = single.nn(q)
    _exact(want, oracle.nn_bruteforce(xyz, q), "single cloud vs oracle")
    wa = single.associate(q, 1.2, gpu.GATE_MAPPER_LOCAL)
    sh = gpu.ShardedCloud(xyz, nrm, [0, 0, 0], raw_lidar_frame=False)
    calls = {"min": 0, "sum": 0}
    fail = {"on": False}
    mn = gpu.ShardReduce.MINFN(_reducer(torch.minimum, "<i8", calls, "min", fail))   # keys < 2^63: signed = unsigned order
    sm = gpu.ShardReduce.SUMFN(_reducer(torch.add, "<i4", calls, "sum", fail))
    only_min = gpu.ShardReduce(mn, gpu.ShardReduce.SUMFN(), None)
    only_sum = gpu.ShardReduce(gpu.ShardReduce.MINFN(), sm, None)
    _exact(sh.nn(q, only_min), want, "min_u64 only")
    assert calls == {"min": 2, "sum": 0}
    _bytes_equal(sh.associate(q, 1.2, gpu.GATE_MAPPER_LOCAL, only_min), wa, "min_u64 only")
    assert calls == {"min": 4, "sum": 0}
    _exact(sh.nn(q, only_sum), want, "sum_i32 only")
    _bytes_equal(sh.associate(q, 1.2, gpu.GATE_MAPPER_LOCAL, only_sum), wa, "sum_i32 only")
    assert calls == {"min": 4, "sum": 1}
    fail["on"] = True
    with pytest.raises(gpu.PcdError) as e:
        sh.nn(q, only_min)
    assert e.value.status == gpu.PCD_ERR_INVALID and "pcd_shard_reduce.min_u64 failed" in str(e.value)
    with pytest.raises(gpu.PcdError) as e:
        sh.associate(q, 1.2, gpu.GATE_MAPPER_LOCAL, only_sum)
    assert e.value.status == gpu.PCD_ERR_INVALID and "pcd_shard_reduce.sum_i32 failed" in str(e.value)
    assert calls == {"min": 5, "sum": 2}
    fail["on"] = False
    _exact(sh.nn(q, only_min), want, "after a failed callback")
    _exact(sh.nn(q), want, "after a failed callback, library reduction")
    _bytes_equal(sh.associate(q, 1.2, gpu.GATE_MAPPER_LOCAL, only_sum), wa, "after a failed callback")
    single.close(); sh.close()


# ------------------------------------------------------------------ guards
def test_guards(gpu):
    """refused with PCD_ERR_INVALID before anything runs, *out left NULL; Q = 0 is OK with null arrays"""
    L = gpu.lib()
    xyz, nrm = synth.cloud_uniform(100, seed=1, box=np.array([2.0, 2.0, 2.0]))
    sh0 = gpu.ShardedCloud(xyz, nrm, [0, 0], raw_lidar_frame=False)      # (sets the argtypes)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(ndev=2, **fields):
        o = gpu.CloudOptions()
        L.pcd_cloud_options_default(C.byref(o))
        o.raw_lidar_frame = 0
        for k, v in fields.items():
            setattr(o, k, v)
        dv = (C.c_int * 65)(*([0] * 65))
        h = C.c_void_p(0xDEAD0)
        st = L.pcd_cloud_create_sharded(ptr(xyz), ptr(nrm), 100, C.byref(o), dv, ndev, C.byref(h))
        return st, h.value

    for kw in (dict(ndev=0), dict(ndev=65), dict(ndev=-1), dict(index_base=1), dict(index_stride=2), dict(layout=2),
               dict(layout=-1)):
        st, h = create(**kw)
        assert st == gpu.PCD_ERR_INVALID and h is None, (kw, st, h)
        assert L.pcd_last_error(), kw
    st, h = create(index_stride=0)                                        # 0 is read as 1
    assert st == gpu.PCD_OK and h
    L.pcd_cloud_shards_destroy(C.c_void_p(h))
    st, h = create(ndev=64)
    assert st == gpu.PCD_OK and L.pcd_cloud_shards_count(C.c_void_p(h)) == 64
    L.pcd_cloud_shards_destroy(C.c_void_p(h))
    assert L.pcd_cloud_create_sharded(ptr(xyz), ptr(nrm), 100, None, (C.c_int * 1)(0), 1, None) == gpu.PCD_ERR_INVALID

    q = np.ascontiguousarray(xyz[:10], np.float64)
    for mode in (3, -1, 3 | gpu.GATE_BOUNDED_SEARCH, 0x200):
        with pytest.raises(gpu.PcdError) as e:
            sh0.associate(q, 1.0, mode)
        assert e.value.status == gpu.PCD_ERR_INVALID, mode
    for count in (0, 2, 9, 11):
        with pytest.raises(gpu.PcdError) as e:
            sh0.associate(q, np.ones(count), gpu.GATE_MAPPER_LOCAL)
        assert e.value.status == gpu.PCD_ERR_INVALID, count
    sh0.associate(q, np.ones(0), gpu.GATE_CONTROLLER)                     # the controller gate reads no range
    # Q = 0: OK, nothing is touched
    L.pcd_nn_query_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.pcd_nn_query_sharded(sh0._h, None, 0, None, None, None, None) == gpu.PCD_OK
    ao = gpu.AssocOut()
    one = np.ones(1)
    assert L.pcd_associate_sharded(sh0._h, None, 0, ptr(one), 1, 0, None, C.byref(ao)) == gpu.PCD_OK
    assert L.pcd_associate_sharded(sh0._h, None, 0, None, 0, 2, None, C.byref(ao)) == gpu.PCD_OK
    idx, sq, found = sh0.nn(np.zeros((0, 3)))
    assert idx.size == 0 and sq.size == 0 and found.size == 0
    sh0.close()

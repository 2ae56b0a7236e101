"""k_nn_fallback with its seed bound (nn.hip fb_seed_table): bit-exact against brute force for every query.

The walk starts from min(incoming key, key of the seed point of the query's 8x8x8-cell cube).  These tests force
queries through every form of the walk -- the one-launch forms <1> (plain) and <2> (gate-bounded), the grid path's
second stage <0>, refining another shard's keys -- on clouds whose seeds are poor (tilted planes, a thin sheet, a
sphere), far from the origin, with queries outside the grid, and with exact distance ties (lowest index must win).
"""
import numpy as np
import pytest

from pcdhip import synth

pytestmark = pytest.mark.gpu


def _check(got, exp, what):
    gi, gd, gf = got
    ei, ed, ef = exp
    assert np.array_equal(gf, ef), f"{what}: found flags differ at {np.nonzero(gf != ef)[0][:10]}"
    bad = np.nonzero((gi != ei) | (gd.view(np.uint32) != ed.view(np.uint32)))[0]
    assert bad.size == 0, (f"{what}: {bad.size} mismatches, first {bad[:5]}: idx {gi[bad[:5]]} vs {ei[bad[:5]]}, "
                           f"d {gd[bad[:5]]} vs {ed[bad[:5]]}")


def _tilted_planes(n, seed):
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(6):
        nv = rng.normal(size=3)
        nv /= np.linalg.norm(nv)
        e1 = np.cross(nv, [0.3, 1.0, 0.2]); e1 /= np.linalg.norm(e1)
        e2 = np.cross(nv, e1)
        uv = rng.uniform(-4, 4, (n // 6, 2))
        parts.append(rng.uniform(0, 20, 3) + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0, 0.005, (n // 6, 1)) * nv)
    return np.concatenate(parts).astype(np.float32)


def _thin_sheet(n, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 3))
    p[:, 0] = rng.uniform(0, 30, n)
    p[:, 2] = rng.uniform(0, 30, n)
    p[:, 1] = 0.3 * p[:, 0] + rng.normal(0, 1e-4, n)     # a tilted sheet of (almost) zero thickness
    return p.astype(np.float32)


def _sphere(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return (10.0 * v / np.linalg.norm(v, axis=1, keepdims=True) + 12.0).astype(np.float32)


def _queries(xyz, n, seed):
    """near-surface, far inside the box, and outside the grid on every side"""
    rng = np.random.default_rng(seed)
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    ext = hi - lo
    near = xyz[rng.integers(0, len(xyz), n // 3)].astype(np.float64) + rng.normal(0, 0.3, (n // 3, 3))
    far = lo + rng.random((n // 3, 3)) * ext
    out = lo - ext + rng.random((n - 2 * (n // 3), 3)) * 3 * ext
    return np.concatenate([near, far, out])


CLOUDS = {"tilted_planes": _tilted_planes, "thin_sheet": _thin_sheet, "sphere": _sphere}


@pytest.mark.parametrize("offset", [0.0, 8000.0])
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_fallback_only_exact(gpu, oracle, name, offset):
    """every query walks the pyramid from its seed: one-launch form <1> and the grid path (<0> after the brick
    kernel), on a cloud at the origin and 8 km from it"""
    xyz = CLOUDS[name](30000, 11) + np.float32(offset)
    q = _queries(xyz, 3000, 12)
    exp = oracle.nn_bruteforce(xyz, q)
    c = gpu.Cloud(xyz, np.zeros_like(xyz), raw_lidar_frame=False)
    _check(c.nn(q, gpu.NN_FALLBACK_ONLY), exp, f"{name}+{offset}/fallback")
    _check(c.nn(q, gpu.NN_GRID), exp, f"{name}+{offset}/grid")
    _check(c.nn(q, gpu.NN_AUTO), exp, f"{name}+{offset}/auto")
    c.close()


def test_fallback_ties_lowest_index(gpu, oracle):
    """an integer lattice in shuffled index order with duplicates, queries at half-integer positions (exact float
    ties between up to eight points) inside and far outside the grid: the lowest index must win even where the
    seed is a tied point with a higher index"""
    rng = np.random.default_rng(21)
    g = np.stack(np.meshgrid(np.arange(24), np.arange(6), np.arange(24), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.random(len(g)) < 0.6]
    xyz = np.concatenate([g, g[::-1]]).astype(np.float32)[rng.permutation(2 * len(g))]
    q = np.concatenate([rng.integers(-30, 54, (3000, 3)) + 0.5, rng.integers(-30, 54, (1000, 3)).astype(np.float64)])
    exp = oracle.nn_bruteforce(xyz, q)
    c = gpu.Cloud(xyz, np.zeros_like(xyz), raw_lidar_frame=False, cell_size=1.0)
    for algo in ("FALLBACK_ONLY", "GRID"):
        _check(c.nn(q, getattr(gpu, "NN_" + algo)), exp, f"ties/{algo}")
    c.close()


def test_fallback_bounded_one_launch(gpu, oracle):
    """the gate-bounded one-launch form <2>: the seed only ever replaces the gate's bound by a real point inside
    it, so association = unbounded search + the gate"""
    xyz = _tilted_planes(24000, 31)
    nrm = np.tile(np.float32([0, 1, 0]), (len(xyz), 1))
    q = _queries(xyz, 3000, 32)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    out = c.associate(q, 1.5, gpu.GATE_MAPPER_LOCAL)
    idx, sq, found = oracle.nn_bruteforce(xyz, q)
    out6, ok = oracle.search_nearest_neibor(xyz, nrm, idx, found)
    _, typ, _, _, _ = oracle.associate(q, out6, ok, 1.5, 0)
    assert np.array_equal(out["type"], typ)
    hit = typ != 0
    assert np.array_equal(out["nn_idx"][hit], idx[hit])
    assert np.array_equal(out["nn_sqdist"][hit].view(np.uint32), sq[hit].view(np.uint32))
    c.close()


@pytest.mark.parametrize("Q", [3000, 70000])
def test_refine_with_incoming_keys(gpu, oracle, Q):
    """pcd_nn_refine_device: the keys come in holding the other shard's result and the seed is a point of THIS
    shard; small batches walk every query (<0> over the whole batch), large ones go through the grid path"""
    import torch
    xyz = _sphere(40000, 41)
    rng = np.random.default_rng(42)
    q = np.concatenate([_queries(xyz, Q // 2, 43), xyz[rng.integers(0, len(xyz), Q - Q // 2)] + rng.normal(0, 0.4, (Q - Q // 2, 3))])
    S = 2
    shards = [gpu.Cloud(xyz[s::S], np.zeros_like(xyz[s::S]), raw_lidar_frame=False, index_base=s, index_stride=S)
              for s in range(S)]
    dq = torch.from_numpy(q).cuda()
    keys = torch.empty(Q, dtype=torch.int64, device="cuda")
    shards[0].nn_device(dq, Q, keys, gpu.NN_GRID)
    shards[1].nn_refine_device(dq, Q, keys)
    torch.cuda.synchronize()
    idx, sq, found = oracle.nn_bruteforce(xyz, q)
    k = keys.cpu().numpy().astype(np.uint64)
    assert found.all()
    assert np.array_equal((k & 0xFFFFFFFF).astype(np.uint32), idx)
    assert np.array_equal((k >> 32).astype(np.uint32), sq.view(np.uint32))
    for s in shards:
        s.close()

"""k_nn_fallback's stack is dynamic LDS of (pyramid levels - 2) entries and a workgroup is one wavefront (nn.hip).

Every key is compared bit for bit with the brute-force algo of the library on the same cloud, through every form of
the walk, on pyramids of three depths -- two levels (the walk never pushes: a launch with zero bytes of LDS), three, and
six -- with walks that push and pop through every level (queries between two far clusters and outside the grid on every
side), queries on the points themselves and non-finite ones; at 3, 4099 and 65 537 queries: fewer than one workgroup
of any size, no multiple of one, and more list entries than the grid has wavefronts (a wavefront then takes a second
query).  The depth a cloud reaches is computed from the handle's grid, the way cloud.hip's build_lattice does.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (3, 4099, 65537)


# ---------------------------------------------------------------- clouds ----
def _box_cloud(ext, n, seed):
    """n points uniform in [0, ext), the two corners of the box among them (they pin the grid's dims)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 1, (n, 3)) * np.asarray(ext, np.float64)
    xyz[0], xyz[1] = 0.0, ext
    return xyz.astype(np.float32)


def _cloud_flat():
    """8 x 8 x 8 cells of 1 m: 4 x 4 x 4 leaves under the virtual top -- two levels, no stack"""
    return _box_cloud((7.9, 7.9, 7.9), 5000, 1), 1.0, 2


def _cloud_one_more():
    """16 x 8 x 8 cells: 128 leaves under two inner nodes -- three levels, one stack entry"""
    return _box_cloud((15.9, 7.9, 7.9), 6000, 2), 1.0, 3


def _cloud_deep():
    """two clusters of 1 m, 4 km apart along x, cells of 0.25 m: 16004 x 4 x 4 cells, leaves 8002 x 2 x 2, then 2001,
    501, 126 and 32 nodes along x -- five real levels and the virtual top, four stack entries, nearly all subtrees
    empty"""
    a = _box_cloud((0.9, 0.9, 0.9), 4000, 3)
    b = _box_cloud((0.9, 0.9, 0.9), 4000, 4) + np.float32([4000.0, 0, 0])
    return np.concatenate([a, b]), 0.25, 6


CLOUDS = {"flat": _cloud_flat, "one_more": _cloud_one_more, "deep": _cloud_deep}


def _nlev(dims):
    """pyramid levels of a grid of `dims` cells (cloud.hip build_lattice): leaves of 2 x 2 x 2 cells, levels of 4 x 4 x 4
    nodes up to the first with at most 64, plus the virtual top"""
    d = [(int(v) + 1) // 2 for v in dims]
    n = 1
    while d[0] * d[1] * d[2] > 64:
        d = [(v + 3) // 4 for v in d]
        n += 1
    return n + 1


def _queries(xyz, n, seed):
    """a fifth each, interleaved so that any prefix holds every kind: inside the box (between the clusters of the
    deep cloud), outside the grid beyond one of its six sides, far outside past a corner, on a point itself, and
    near a point; every 11th of them non-finite"""
    rng = np.random.default_rng(seed)
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    ext = hi - lo
    q = np.empty((n, 3))
    for i in range(0, n, 5):
        k = (i // 5) % 6
        side = lo + rng.random(3) * ext
        side[k % 3] = (lo[k % 3] - (0.1 + rng.random()) * ext[k % 3]) if k < 3 else (hi[k % 3] + (0.1 + rng.random()) * ext[k % 3])
        corner = np.where(rng.random(3) < 0.5, lo - (1 + rng.random(3)) * ext, hi + (1 + rng.random(3)) * ext)
        p = xyz[rng.integers(0, len(xyz))].astype(np.float64)
        block = [lo + rng.random(3) * ext, p, side, corner, p + rng.normal(0, 0.3, 3)]
        q[i:i + 5] = block[:n - i]
    bad = np.arange(2, n, 11)
    q[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf])[bad % 3]
    return q


_memo = {}


def _case(gpu, name, Q):
    """the cloud (one handle per session and cloud, its depth checked once), Q queries on the device and the
    brute-force keys of the library: computed once, never modified"""
    import torch
    if name not in _memo:
        xyz, h, want = CLOUDS[name]()
        assert len(xyz) <= 20000
        nrm = np.tile(np.float32([0, 1, 0]), (len(xyz), 1))
        c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=h)
        assert _nlev(c.info()["dims"]) == want, c.info()["dims"]
        # a second handle over the first 50 rows (same global indices): the incoming keys of the refine form
        _memo[name] = (xyz, c, gpu.Cloud(xyz[:50], nrm[:50], raw_lidar_frame=False, cell_size=h))
    xyz, c, part = _memo[name]
    if (name, Q) not in _memo:
        dq = torch.from_numpy(_queries(xyz, Q, 100 + Q % 97)).cuda()
        want = torch.empty(Q, dtype=torch.int64, device="cuda")
        c.nn_device(dq, Q, want, gpu.NN_BRUTEFORCE)
        torch.cuda.synchronize()
        _memo[(name, Q)] = (dq, want)
    return (c, part) + _memo[(name, Q)]


def _same(got, want, what):
    import torch
    torch.cuda.synchronize()
    bad = torch.nonzero(got != want).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} keys differ, first at {bad[:5].tolist()}"


@pytest.mark.parametrize("Q", COUNTS)
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_every_form_matches_bruteforce(gpu, name, Q):
    import torch
    c, part, dq, want = _case(gpu, name, Q)
    found = (want != 0x7FFFFFFFFFFFFFFF)      # PCD_KEY_NONE
    assert 0 < int(found.sum()) < Q or Q == 3      # finite and non-finite queries both present
    keys = torch.empty(Q, dtype=torch.int64, device="cuda")
    # <0> behind the brick kernel
    keys.fill_(0x5A5A5A5A)
    c.nn_device(dq, Q, keys, gpu.NN_GRID)
    _same(keys, want, f"{name}/{Q}/grid")
    # <1>: the walk as the only launch (65 537 queries reach it only through the fallback-only algo)
    keys.fill_(0x5A5A5A5A)
    c.nn_device(dq, Q, keys, gpu.NN_FALLBACK_ONLY)
    _same(keys, want, f"{name}/{Q}/one launch")
    # refine: prepare + <0> over keys that come in holding the result of the first 50 rows
    part.nn_device(dq, Q, keys, gpu.NN_BRUTEFORCE)
    c.nn_refine_device(dq, Q, keys)
    _same(keys, want, f"{name}/{Q}/refine")
    # <2>: the gate-bounded search of associate_device (one launch up to 65 536 queries, the grid path above) against
    # the epilogue alone on the brute-force keys
    mr = torch.tensor([1.5], dtype=torch.float64, device="cuda")

    def out():
        return {"type": torch.full((Q,), 77, dtype=torch.uint8, device="cuda"),
                "nn_idx": torch.zeros(Q, dtype=torch.int32, device="cuda"),
                "nn_sqdist": torch.zeros(Q, dtype=torch.float32, device="cuda")}
    ref, got = out(), out()
    c.associate_device(dq, Q, mr, 1, gpu.GATE_MAPPER_LOCAL, ref, want)
    c.associate_device(dq, Q, mr, 1, gpu.GATE_MAPPER_LOCAL | gpu.GATE_BOUNDED_SEARCH, got)
    torch.cuda.synchronize()
    assert torch.equal(got["type"], ref["type"]), f"{name}/{Q}/bounded: types differ"
    hit = ref["type"] != 0
    assert Q == 3 or bool(hit.any())
    assert torch.equal(got["nn_idx"][hit], ref["nn_idx"][hit])
    assert torch.equal(got["nn_sqdist"][hit].view(torch.int32), ref["nn_sqdist"][hit].view(torch.int32))


def test_alternating_depths_on_one_stream(gpu):
    """two clouds of different depth used alternately without a synchronise in between: every launch runs with the
    stack size of its own cloud"""
    import torch
    Q = 4099
    flat, _, dq_f, want_f = _case(gpu, "flat", Q)
    deep, _, dq_d, want_d = _case(gpu, "deep", Q)
    runs = []
    for r in range(3):
        for c, dq, want in ((deep, dq_d, want_d), (flat, dq_f, want_f)):
            keys = torch.full((Q,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
            c.nn_device(dq, Q, keys, gpu.NN_FALLBACK_ONLY if r != 1 else gpu.NN_GRID)
            runs.append((keys, want))
    for i, (keys, want) in enumerate(runs):
        _same(keys, want, f"run {i}")

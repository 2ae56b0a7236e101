"""The work schedule of k_nn_brick_clip (csrc/brick_clip_kernel.h): inside a block class a wavefront takes its first
R_s strided rounds statically and then chunks of consecutive items from the class's cursor in NnCounters; the switch
set_nn_schedule(1) leaves the static schedule alone.  Which wavefront handles an item must not show anywhere: keys are
compared bit for bit with the brute-force kernel (NN_BRUTEFORCE) under both schedules, at the grid sizes, item counts
and call sequences where the schedule takes another path.  Nothing here depends on timing.

Cloud: 50 000 points on three planes in a 4 m cube; the queries lie around the planes, so that a brick holds many of
them: 70 000 queries (the grid capped at 1024 workgroups) give every wavefront a handful of items, a static and a dynamic
part.  Every 50th query lies outside the grid and every 50th is NaN.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QMAX = 70000
SIZES = [1, 7, 200, 1000, 4097, 20000, 70000]
COUNTERS = ("staged_points", "pair_evals", "brick_groups", "fallback_queries", "fallback_points")


def _planes(rng, n):
    """n points on z = 1.1, x = 2.6 and the tilted plane y = 0.5 + 0.3 x + 0.2 z, 2 cm of noise, inside [0, 4]^3"""
    uv = rng.uniform(0.0, 4.0, (n, 2))
    which = rng.integers(0, 3, n)
    p = np.empty((n, 3))
    p[which == 0] = np.c_[uv[which == 0], np.full((which == 0).sum(), 1.1)]
    p[which == 1] = np.c_[np.full((which == 1).sum(), 2.6), uv[which == 1]]
    t = uv[which == 2]
    p[which == 2] = np.c_[t[:, 0], 0.5 + 0.3 * t[:, 0] + 0.2 * t[:, 1], t[:, 1]]
    return np.clip(p + rng.normal(0, 0.02, (n, 3)), 0.0, 4.0)


def _normals(xyz):
    n = np.zeros_like(xyz)
    n[:, 2] = 1
    return n


@pytest.fixture(scope="module")
def scene(gpu):
    """the cloud handle, the queries and their brute-force result (computed once, shared, never changed)"""
    rng = np.random.default_rng(4242)
    xyz = _planes(rng, 50000).astype(np.float32)
    xyz[0], xyz[1] = 0.0, 4.0                      # the grid's extent
    q = _planes(rng, QMAX) + rng.normal(0, 0.04, (QMAX, 3))
    i = np.arange(QMAX)
    q[i % 50 == 3] += 9.0                          # outside the grid
    q[i % 50 == 5, 1] = np.nan
    c = gpu.Cloud(xyz, _normals(xyz), raw_lidar_frame=False)
    ref = c.nn(q, gpu.NN_BRUTEFORCE)
    assert ref[2][i % 50 == 3].all() and not ref[2][i % 50 == 5].any()
    for a in ref:
        a.setflags(write=False)
    yield dict(c=c, xyz=xyz, q=q, ref=ref)
    gpu.set_nn_schedule(0)
    gpu.set_nn_bookkeeping(0)
    gpu.set_nn_tuning(0, -1, 0)
    c.close()


def _check(got, ref, Q, what):
    gi, gd, gf = got
    ei, ed, ef = (a[:Q] for a in ref)
    assert np.array_equal(gf, ef), f"{what}: found flags differ at {np.nonzero(gf != ef)[0][:10]}"
    ok = ef != 0
    bad = np.nonzero(ok & ((gi != ei) | (gd.view(np.uint32) != ed.view(np.uint32))))[0]
    assert bad.size == 0, (f"{what}: {bad.size} mismatches, first {bad[:5]}: idx {gi[bad[:5]]} vs {ei[bad[:5]]}, "
                           f"d {gd[bad[:5]]} vs {ed[bad[:5]]}")
    assert np.array_equal(gi[~ok], ei[~ok]) and np.array_equal(gd[~ok].view(np.uint32), ed[~ok].view(np.uint32)), what


def _run(gpu, scene, Q, schedule, what):
    gpu.set_nn_schedule(schedule)
    try:
        _check(scene["c"].nn(scene["q"][:Q], gpu.NN_GRID), scene["ref"], Q, f"{what}, Q {Q}, schedule {schedule}")
    finally:
        gpu.set_nn_schedule(0)


def _blocks(Q):
    """workgroups of the brick kernel for Q queries (nn.hip run_grid)"""
    return min(-(-(-(-Q // 8)) // 4) + 1, 1024)


def _classes(gpu, Q, nitems):
    """[(items of the class, its static items R_s * stride capped by nothing, stride)] as the kernel splits them"""
    pct, _ = gpu.nn_schedule_params()
    blocks = _blocks(Q)
    if blocks % 8:
        full, stride, counts = nitems, blocks * 4, [nitems]
    else:
        per, stride = -(-nitems // 8), blocks // 8 * 4
        full, counts = per, [min(nitems, (c + 1) * per) - min(nitems, c * per) for c in range(8)]
    r_s = -(-full // stride) * pct // 100
    return [(n, r_s * stride, stride) for n in counts]


@pytest.mark.parametrize("Q", SIZES)
def test_sizes(gpu, scene, Q):
    """1: two workgroups, the one-class path, fewer items than wavefronts; 200: 8 workgroups; 70 000: the capped grid"""
    assert _blocks(1) == 2 and _blocks(200) == 8 and _blocks(70000) == 1024
    for schedule in (0, 1):
        _run(gpu, scene, Q, schedule, "sizes")
    if Q == QMAX:      # both parts of the schedule are there
        nitems = scene["c"].last_wave_records()[1]
        for n, static, stride in _classes(gpu, Q, nitems):
            assert 0 < static < n, (n, static, stride)
        print("Q %d: %d items, classes %s" % (Q, nitems, _classes(gpu, Q, nitems)))


def _clustered(n=2000):
    """queries around the plane z = 1.1, the first half inside a square of 0.9 m, the second of 1.6 m: one or three
    dozen bricks, so that a few hundred queries make a few dozen items and a class holds about as many items as the
    class has wavefronts"""
    rng = np.random.default_rng(99)
    side = np.where(np.arange(n) < n // 2, 0.9, 1.6)[:, None]
    return np.c_[1.0 + side * rng.uniform(0.0, 1.0, (n, 2)), 1.1 + rng.normal(0, 0.04, n)]


def test_item_counts_around_the_static_part(gpu, scene):
    """Q (and the slice of a clustered query set) chosen by a search on the host so that some class holds exactly its
    static items (an empty dynamic range), one fewer (a wavefront without its last static item), one more (one grab)
    and a short last chunk"""
    pct, chunk = gpu.nn_schedule_params()
    want = {"exact": lambda d: d == 0, "minus 1": lambda d: d == -1, "plus 1": lambda d: d == 1}
    if chunk > 1:
        want["short last chunk"] = lambda d: d > chunk and d % chunk != 0
    found = {}
    c = scene["c"]
    qc = _clustered()
    ref = c.nn(qc, gpu.NN_BRUTEFORCE)
    for Q in [Q for Q in range(9, 800) if _blocks(Q) % 8 == 0]:
        for s in range(0, 1500, 250):
            if len(found) == len(want):
                break
            c.nn(qc[s:s + Q], gpu.NN_GRID)
            nitems = c.last_wave_records()[1]
            for n, static, stride in _classes(gpu, Q, nitems):
                for name, hit in want.items():
                    if name not in found and static > 0 and n > 0 and hit(n - static):
                        found[name] = (Q, s, nitems, n, static, stride)
    print("static share %d %%, chunk %d: cases (Q, slice, items, items of the class, its static items, stride)" % (pct, chunk), found)
    assert set(found) == set(want), (found, "the search found no Q for some case")
    for name, (Q, s, *_) in found.items():
        for schedule in (0, 1):
            gpu.set_nn_schedule(schedule)
            try:
                _check(c.nn(qc[s:s + Q], gpu.NN_GRID), tuple(a[s:] for a in ref), Q, f"{name}, Q {Q}, schedule {schedule}")
            finally:
                gpu.set_nn_schedule(0)


def test_repeated_calls_alternate_the_counter_blocks(gpu, scene):
    """three calls in a row on one handle (the cursors of the next call's block are cleared by this call's bookkeeping),
    then the radix-sort bookkeeping (the memset path) and back"""
    for Q in (70000, 4097, 20000):
        _run(gpu, scene, Q, 0, "in a row")
    gpu.set_nn_bookkeeping(1)
    try:
        _run(gpu, scene, 20000, 0, "radix-sort bookkeeping")
        _run(gpu, scene, 70000, 0, "radix-sort bookkeeping")
    finally:
        gpu.set_nn_bookkeeping(0)
    for Q in (70000, 1000, 70000):
        _run(gpu, scene, Q, 0, "back on the counting sort")


def test_gate_bounded_search(gpu, scene, oracle):
    """the same kernel with keys carried in: pcd_associate_device with GATE_BOUNDED_SEARCH under both schedules"""
    import torch
    xyz, q, (idx, sq, found) = scene["xyz"], scene["q"], scene["ref"]
    mr = np.where(np.arange(QMAX) % 2 == 0, 0.03, 1.5)
    out6, ok = oracle.search_nearest_neibor(xyz, _normals(xyz), idx, found)
    _, typ, _, _, _ = oracle.associate(q, out6, ok, mr, 0)
    hit = typ != 0
    assert hit[0::2].any() and (~hit[0::2]).any() and hit[1::2].any(), "the gates do not straddle the distances"
    dq, dmr = torch.from_numpy(q).cuda(), torch.from_numpy(mr).cuda()
    try:
        for schedule in (0, 1):
            gpu.set_nn_schedule(schedule)
            gpu.set_nn_tuning(0, -1, 1)
            d = dict(type=torch.zeros(QMAX, dtype=torch.uint8, device="cuda"),
                     nn_idx=torch.zeros(QMAX, dtype=torch.int32, device="cuda"),
                     nn_sqdist=torch.zeros(QMAX, dtype=torch.float32, device="cuda"))
            scene["c"].associate_device(dq, QMAX, dmr, QMAX, gpu.GATE_MAPPER_LOCAL | gpu.GATE_BOUNDED_SEARCH, d)
            torch.cuda.synchronize()
            assert scene["c"].last_stats()["brick_groups"] > 0
            assert np.array_equal(d["type"].cpu().numpy(), typ), schedule
            assert np.array_equal(d["nn_idx"].cpu().numpy().view(np.uint32)[hit], idx[hit]), schedule
            assert np.array_equal(d["nn_sqdist"].cpu().numpy().view(np.uint32)[hit], sq.view(np.uint32)[hit]), schedule
    finally:
        gpu.set_nn_schedule(0)
        gpu.set_nn_tuning(0, -1, 0)


def test_counters_do_not_depend_on_the_schedule(gpu, scene):
    """the statistics depend on the items only.  Which queries of a brick share an item varies from run to run (the
    bookkeeping places them in atomic order), so here a brick holds either at most 8 different queries (one item,
    whatever the order) or 1 .. 20 copies of one query (whichever copies meet in an item, the items are the same).
    Bricks are binned on the host (the grid starts at the cloud's minimum, 0; a brick is 2 cells wide); queries within
    a millimetre of a cell boundary stay out, so that float rounding cannot put one into the neighbouring brick"""
    rng = np.random.default_rng(7)
    h = float(scene["c"].info()["cell_size"])
    base = scene["q"][:20000]
    t = base / h
    base = base[np.isfinite(t).all(1) & (t > 0).all(1) & (t < 4.0 / h - 1).all(1) & (np.abs(t - np.round(t)) > 1e-3 / h).all(1)]
    b = np.floor(base / h).astype(np.int64) >> 1
    bid = (b[:, 2] * 64 + b[:, 1]) * 64 + b[:, 0]
    order = np.argsort(bid, kind="stable")
    ub, first, cnt = np.unique(bid[order], return_index=True, return_counts=True)
    parts = []
    for u, f, n in zip(ub, first, cnt):
        rows = base[order[f:f + n]]
        parts.append(rows[:min(n, 8)] if u % 2 else np.repeat(rows[:1], rng.integers(1, 21), 0))
    q = np.concatenate(parts)
    q = q[rng.permutation(len(q))]
    assert len(ub) > 300 and 2000 < len(q) < QMAX, (len(ub), len(q))
    ref = scene["c"].nn(q, gpu.NN_BRUTEFORCE)
    st = {}
    try:
        for schedule in (0, 1, 0):
            gpu.set_nn_schedule(schedule)
            gpu.set_nn_tuning(0, -1, 1)
            _check(scene["c"].nn(q, gpu.NN_GRID), ref, len(q), f"repeated positions, schedule {schedule}")
            s = scene["c"].last_stats()
            assert s["brick_groups"] > 0 and s["staged_points"] > 0, s
            st.setdefault(schedule, []).append({k: s[k] for k in COUNTERS})
    finally:
        gpu.set_nn_schedule(0)
        gpu.set_nn_tuning(0, -1, 0)
    print("counters", st)
    assert st[0][0] == st[0][1], "the counters vary from run to run: the comparison would prove nothing"
    assert st[0][0] == st[1][0], st


@pytest.mark.parametrize("Q", [200, 70000])
def test_statistics_pass_records_every_wavefront(gpu, scene, Q):
    """collect_stats bit 4: one record {start, end, items} per launched wavefront, also of those without an item"""
    c = scene["c"]
    try:
        for schedule in (0, 1):
            gpu.set_nn_schedule(schedule)
            gpu.set_nn_tuning(0, -1, 5)
            _check(c.nn(scene["q"][:Q], gpu.NN_GRID), scene["ref"], Q, f"statistics pass, schedule {schedule}")
            rec, nitems = c.last_wave_records()
            assert rec.shape == (4 * _blocks(Q), 3), rec.shape
            assert (rec[:, 0] > 0).all() and (rec[:, 1] >= rec[:, 0]).all()
            assert int(rec[:, 2].sum()) == nitems == c.last_stats()["brick_groups"], (rec[:, 2].sum(), nitems)
            gpu.set_nn_tuning(0, -1, 1)      # without the bit: no records kept
            c.nn(scene["q"][:Q], gpu.NN_GRID)
            assert c.last_wave_records()[0].shape == (0, 3)
    finally:
        gpu.set_nn_schedule(0)
        gpu.set_nn_tuning(0, -1, 0)

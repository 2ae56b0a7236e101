"""The association epilogue, the gate-bounded search in front of it, the staged path and the outlier filter on the
boundary scenes of tests/assoc_edge_ref.py: rows whose decisive quantity sits exactly on its threshold.

Expected = the oracle (nn_bruteforce -> search_nearest_neibor -> associate): the same operation order as the kernel.
type / nn_idx / nn_sqdist bits equal; doubles equal on the rows the census calls exact, within RTOL elsewhere (NaN
where the oracle has NaN: the Inf normal, the angle of a query on its point).  tests/test_assoc_edge_cpu.py pins the
oracle itself against exact arithmetic on the same rows."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import assoc_edge_ref as ref

pytestmark = pytest.mark.gpu
RTOL = 1e-12            # tests/test_assoc_gpu.py
SMALL_BATCH = 65536     # nn.hip kSmallBatch: PCD_NN_AUTO takes the one-launch path up to it, the grid path above
STAGE_CUT = 200000      # assoc.hip pcd_associate_staged: two chunks from here on
DOUBLES = ("lidar_xyz", "abcd", "dist", "angle", "dist2plane")
SENTINEL = {torch.float64: -777.25, torch.uint8: 0xAB, torch.float32: -777.25, torch.int32: -7}


@functools.lru_cache(maxsize=None)
def _scene(translated):
    sc = ref.build_scene(translated)
    rows = ref.census(sc["q"], sc["xyz"][sc["point"]], sc["nrm"][sc["point"]], sc["mr"])
    sc["exact"] = np.array([any(s[0] == "exact" for s in row.values()) for row in rows])
    return sc


def _tiled(a, Q):
    return np.ascontiguousarray(np.resize(a, (Q,) + a.shape[1:]))     # np.resize repeats the rows in order


_expected_cache = {}


def _expected(oracle, translated, Q, mr_name, mode):
    """oracle outputs for the scene tiled to Q rows; mr_name: "q" = the scene's per-query ranges, else a scalar"""
    key = (translated, Q, mr_name if mode != 2 else None, mode)
    if key not in _expected_cache:
        sc = _scene(translated)
        q = _tiled(sc["q"], Q)
        nk = (translated, Q)
        if nk not in _expected_cache:
            idx, sq, found = oracle.nn_bruteforce(sc["xyz"], q)
            out6, ok = oracle.search_nearest_neibor(sc["xyz"], sc["nrm"], idx, found)
            _expected_cache[nk] = (idx, sq, out6, ok)
        idx, sq, out6, ok = _expected_cache[nk]
        mr = None if mode == 2 else _tiled(sc["mr"], Q) if mr_name == "q" else mr_name
        abcd, typ, dist, ang, d2p = oracle.associate(q, out6, ok, mr, mode)
        _expected_cache[key] = dict(nn_idx=idx, nn_sqdist=sq, ok=ok.astype(bool), lidar_xyz=out6[:, :3], abcd=abcd,
                                    type=typ, dist=dist, angle=ang, dist2plane=d2p)
    return _expected_cache[key]


def _check(out, exp, exact, what, rows=None, keys=True):
    """out against the oracle on `rows` (default: all)"""
    sel = np.ones(len(exp["type"]), bool) if rows is None else rows
    assert np.array_equal(out["type"][sel], exp["type"][sel]), (what, np.nonzero(out["type"] != exp["type"])[0][:10])
    if keys:
        assert np.array_equal(out["nn_idx"][sel], exp["nn_idx"][sel]), what
        assert np.array_equal(out["nn_sqdist"][sel].view(np.uint32), exp["nn_sqdist"][sel].view(np.uint32)), what
    for k in DOUBLES:
        if k not in out:
            continue
        m = sel & exp["ok"] if k == "lidar_xyz" else sel
        np.testing.assert_allclose(out[k][m], exp[k][m], rtol=RTOL, atol=1e-15 if k == "dist2plane" else 0,
                                   equal_nan=True, err_msg=f"{what} {k}")
        e = m & exact
        assert np.array_equal(out[k][e], exp[k][e], equal_nan=True), (what, k, "exact rows")


def _cloud(gpu, translated, **kw):
    sc = _scene(translated)
    return gpu.Cloud(sc["xyz"], sc["nrm"], raw_lidar_frame=False, **kw)


@pytest.mark.parametrize("translated", [False, True], ids=["origin", "translated"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_boundary_rows(gpu, oracle, mode, translated):
    """pcd_associate on the boundary rows, unbounded and gate-bounded, on the one-launch path (the scene's own size,
    SMALL_BATCH - 1, SMALL_BATCH) and on the grid path (SMALL_BATCH + 1); per-query and scalar ranges"""
    sc = _scene(translated)
    R = len(sc["q"])
    c = _cloud(gpu, translated)
    for Q in (R, SMALL_BATCH - 1, SMALL_BATCH, SMALL_BATCH + 1):
        q, exact = _tiled(sc["q"], Q), _tiled(sc["exact"], Q)
        for mr_name in ("q",) + (ref.SCALAR_RANGES if Q == R and mode != 2 else ()):
            mr = None if mode == 2 else _tiled(sc["mr"], Q) if mr_name == "q" else mr_name
            exp = _expected(oracle, translated, Q, mr_name, mode)
            full = c.associate(q, mr, mode)
            _check(full, exp, exact, (Q, mr_name, "unbounded"))
            bnd = c.associate(q, mr, mode | gpu.GATE_BOUNDED_SEARCH)
            assert np.array_equal(bnd["type"], full["type"]), (Q, mr_name, np.nonzero(bnd["type"] != full["type"])[0][:10])
            acc = full["type"] != 0
            assert 0 < acc.sum() < Q
            for k in DOUBLES + ("nn_idx", "nn_sqdist"):
                assert np.array_equal(bnd[k][acc], full[k][acc], equal_nan=True), (Q, mr_name, k)
            _check(bnd, exp, exact, (Q, mr_name, "bounded"), rows=acc)
    c.close()


def _dev_out(Q, names, pad=64):
    spec = dict(lidar_xyz=((Q + pad, 3), torch.float64), abcd=((Q + pad, 4), torch.float64), type=((Q + pad,), torch.uint8),
                dist=((Q + pad,), torch.float64), angle=((Q + pad,), torch.float64), dist2plane=((Q + pad,), torch.float64),
                nn_idx=((Q + pad,), torch.int32), nn_sqdist=((Q + pad,), torch.float32))
    return {n: torch.full(spec[n][0], SENTINEL[spec[n][1]], dtype=spec[n][1], device="cuda") for n in names}


def _host(d, Q):
    """rows 0..Q-1 of every output; the rows behind them must still hold the sentinel"""
    torch.cuda.synchronize()
    out = {}
    for n, t in d.items():
        a = t.cpu().numpy()
        assert (a[Q:] == SENTINEL[t.dtype]).all(), f"{n}: written past row {Q}"
        out[n] = a[:Q].view(np.uint32) if n == "nn_idx" else a[:Q]     # (torch fills no uint32 tensor)
    return out


ALL = DOUBLES + ("type", "nn_idx", "nn_sqdist")


@pytest.mark.parametrize("Q", [1, 255, 256, 257])
def test_device_shapes_and_null_members(gpu, oracle, Q):
    """pcd_associate_device: block-edge batch sizes with a sentinel tail, NULL members of pcd_assoc_out, one range
    (taken from entry 0 of a buffer whose other entries would reject everything) and Q ranges -- also at Q == 1"""
    translated = True
    sc = _scene(translated)
    c = _cloud(gpu, translated)
    q, exact = _tiled(sc["q"], Q), _tiled(sc["exact"], Q)
    dq = torch.from_numpy(q).cuda()
    for mode in (0, 2, 1 | gpu.GATE_BOUNDED_SEARCH):
        for count, mr_name in ((Q, "q"), (1, 0.625)):
            exp = _expected(oracle, translated, Q, mr_name, mode & 3)
            mr = _tiled(sc["mr"], Q) if mr_name == "q" else np.concatenate([[mr_name], np.full(Q, -1.0)])
            dmr = torch.from_numpy(mr).cuda()
            for names in (ALL, ("type",), ("nn_idx",), tuple(n for n in ALL if n != "dist2plane")):
                d = _dev_out(Q, names)
                c.associate_device(dq, Q, dmr, count, mode, d)
                out = _host(d, Q)
                bounded = bool(mode & gpu.GATE_BOUNDED_SEARCH)
                rows = exp["type"] != 0 if bounded else None
                if "type" in out:
                    assert np.array_equal(out["type"], exp["type"]), (mode, mr_name, names)
                    _check(out, exp, exact, (mode, mr_name, names), rows=rows, keys="nn_sqdist" in out)
                else:
                    sel = exp["type"] != 0 if bounded else np.ones(Q, bool)
                    assert np.array_equal(out["nn_idx"][sel], exp["nn_idx"][sel])
    c.close()


def _merge(outs, owner):
    return {n: np.where((owner == 0).reshape((-1,) + (1,) * (outs[0][n].ndim - 1)), outs[0][n], outs[1][n])
            for n in outs[0]}


@pytest.mark.parametrize("mode", [1, 2])
def test_payload_and_foreign_keys(gpu, oracle, mode):
    """two interleaved shards of the lattice: MIN of the keys + SUM of the winner payloads + the payload epilogue, and
    pcd_associate_device with the combined keys on either shard, reproduce the single cloud on the boundary rows"""
    translated = False
    sc = _scene(translated)
    Q = len(sc["q"])
    exp = _expected(oracle, translated, Q, "q", mode)
    shards = [gpu.Cloud(sc["xyz"][s::2], sc["nrm"][s::2], raw_lidar_frame=False, index_base=s, index_stride=2)
              for s in range(2)]
    dq = torch.from_numpy(sc["q"]).cuda()
    dmr = torch.from_numpy(sc["mr"]).cuda()
    keys = [torch.empty(Q, dtype=torch.int64, device="cuda") for _ in range(2)]
    for s in range(2):
        shards[s].nn_device(dq, Q, keys[s])
    kmin = torch.minimum(keys[0], keys[1])
    payload = torch.zeros(Q, 6, dtype=torch.int32, device="cuda")
    for s in range(2):
        p = torch.full((Q + 64, 6), SENTINEL[torch.int32], dtype=torch.int32, device="cuda")
        shards[s].winner_payload_device(kmin, Q, p)
        torch.cuda.synchronize()
        assert (p[Q:] == SENTINEL[torch.int32]).all()
        payload += p[:Q]
    d = _dev_out(Q, ALL)
    gpu.associate_from_payload_device(0, dq, Q, dmr, Q, mode, kmin, payload, d)
    _check(_host(d, Q), exp, sc["exact"], ("payload", mode))
    outs = []
    for s in range(2):
        d = _dev_out(Q, ALL)
        shards[s].associate_device(dq, Q, dmr, Q, mode, d, kmin)
        outs.append(_host(d, Q))
    owner = exp["nn_idx"] % 2
    for s in range(2):
        foreign = owner != s
        assert foreign.any() and (outs[s]["type"][foreign] == 0).all() and (outs[s]["abcd"][foreign] == 0).all()
    _check(_merge(outs, owner), exp, sc["exact"], ("foreign keys", mode))
    for s in shards:
        s.close()


@pytest.mark.parametrize("nshards", [2, 3])
def test_sharded_equals_single_cloud(gpu, oracle, nshards):
    for translated in (False, True):
        sc = _scene(translated)
        c = _cloud(gpu, translated)
        sh = gpu.ShardedCloud(sc["xyz"], sc["nrm"], [0] * nshards, raw_lidar_frame=False)
        for mode in (0, 1, 2):
            one = c.associate(sc["q"], None if mode == 2 else sc["mr"], mode)
            many = sh.associate(sc["q"], sc["mr"], mode)
            for k in ALL:
                assert np.array_equal(one[k].view(np.uint8), many[k].view(np.uint8)), (translated, mode, k)
            _check(many, _expected(oracle, translated, len(sc["q"]), "q", mode), sc["exact"], ("sharded", mode))
        sh.close()
        c.close()


def _staged_equals_full(c, gpu, q, mr, count, mode, what):
    Q = len(q)
    full = c.associate(q, None if mode == 2 else (mr if count == Q else mr[0]), mode)
    sq, smr = c.staging(Q)
    sq[:] = q
    if mode != 2:
        smr[:count] = mr[:count]
    hits = c.associate_staged(Q, count, mode)
    acc = np.nonzero(full["type"])[0]
    assert len(hits) == len(acc), (what, len(hits), len(acc))
    assert np.array_equal(hits["query"], acc), what
    assert np.array_equal(hits["type"], full["type"][acc]), what
    for k in ("lidar_xyz", "abcd", "dist", "angle"):
        assert np.array_equal(hits[k], full[k][acc], equal_nan=True), (what, k)
    return acc


@pytest.mark.parametrize("Q", [STAGE_CUT - 1, STAGE_CUT, STAGE_CUT + 1])
def test_staged_chunks(gpu, oracle, Q):
    """pcd_associate_staged around the two-chunk cut: chunks with and without hits, the deciding query at a chunk's
    end, per-query ranges that differ between the chunks; the records are the accepted rows of pcd_associate"""
    translated = True
    sc = _scene(translated)
    R = len(sc["q"])
    c = _cloud(gpu, translated)
    q, mr0 = _tiled(sc["q"], Q), _tiled(sc["mr"], Q)
    half = (Q + 1) // 2                       # first query of the second chunk when there are two
    assert half % R != 0                      # the second chunk's ranges are not a repeat of the first's
    r0 = float(sc["mr"][0])                   # row 0: "gate eq", accepted at exactly this range, rejected one ulp below
    assert sc["tag"][0] == "gate eq" and sc["exact"][0]
    exp_typ = _expected(oracle, translated, Q, "q", 0)["type"]
    acc = _staged_equals_full(c, gpu, q, mr0, Q, 0, "tiled scene")
    assert np.array_equal(acc, np.nonzero(exp_typ)[0]) and (acc < half).any() and (acc >= half).any()
    mr = mr0.copy(); mr[half:] = -1.0
    acc = _staged_equals_full(c, gpu, q, mr, Q, 0, "hits in the first chunk only")
    assert len(acc) and acc.max() < half
    mr = mr0.copy(); mr[:half] = -1.0
    acc = _staged_equals_full(c, gpu, q, mr, Q, 0, "hits in the second chunk only")
    assert len(acc) and acc.min() >= half
    q1 = q.copy(); q1[Q - 1] = sc["q"][0]
    mr = np.full(Q, -1.0); mr[Q - 1] = r0
    assert list(_staged_equals_full(c, gpu, q1, mr, Q, 0, "one hit, on the last query")) == [Q - 1]
    mr[Q - 1] = ref.pred(r0)
    assert len(_staged_equals_full(c, gpu, q1, mr, Q, 0, "no hit")) == 0
    for a, b, what in ((r0, ref.pred(r0), "chunk end hit, next miss"), (ref.pred(r0), r0, "chunk end miss, next hit")):
        q2 = q.copy(); q2[half - 1] = q2[half] = sc["q"][0]
        mr = mr0.copy(); mr[half - 1] = a; mr[half] = b
        acc = _staged_equals_full(c, gpu, q2, mr, Q, 0, what)
        assert (half - 1 in acc) == (a == r0) and (half in acc) == (b == r0)
    mr = np.full(Q, 0.625)
    _staged_equals_full(c, gpu, q, mr, 1, 0, "one range")
    acc = _staged_equals_full(c, gpu, q, mr0, Q, 2, "controller gate")
    assert np.array_equal(acc, np.nonzero(_expected(oracle, translated, Q, "q", 2)["type"])[0])
    # the handle after a larger call: the scene's own size, and one query (max_range_count == Q == 1)
    _staged_equals_full(c, gpu, sc["q"], sc["mr"], R, 0, "reuse")
    for mrv, n in ((r0, 1), (ref.pred(r0), 0)):
        assert len(_staged_equals_full(c, gpu, sc["q"][:1], np.array([mrv]), 1, 0, "Q == 1")) == n
    c.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_outlier_filter_boundaries(gpu, oracle, n):
    X, lx, typ, tags, bounds = ref.build_filter_scene()
    X, lx, typ = _tiled(X, n), _tiled(lx, n), _tiled(typ, n)
    d = [torch.from_numpy(a).cuda() for a in (X, lx, typ)]
    for mp, mi in bounds:
        exp = oracle.filter_lidar_outlier(X, lx, typ, mp, mi)
        assert np.array_equal(exp, ref.filter_ref(X, lx, typ, mp, mi))
        out = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        gpu.filter_lidar_outlier_device(d[0], d[1], d[2], n, mp, mi, out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[n:] == 0xAB).all(), "written past row n"
        assert np.array_equal(got[:n], exp), ((mp, mi), [tags[i % len(tags)] for i in np.nonzero(got[:n] != exp)[0][:5]])
    gpu.filter_lidar_outlier_device(None, None, None, 0, 1.0, 1.0, None)      # n == 0 with null pointers is OK

"""Edge pinning of the MFMA SIFT matcher (csrc/sift.hip) against the plain reference of tests/sift_edge_ref.py: equal
best scores in every placement the end-of-walk merges meet, second bests that decide, descriptors with bytes >= 128
(the re-centred product's row / column constants), sizes on the MFMA row tile, the wavefront's rows, the stripe and the
one-workgroup compaction limit, NaN / inf residuals of the guided filter.  Bar: m12, m21 and the match lists are
identical; tests/test_sift_edge_cpu.py shows that no row of these inputs decides within 1e-4 rad of a float threshold,
so nothing is left out.  Every case asserts that what it compares is not empty."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sift_edge_ref as er
from tests import sift_guided_ref as gref

pytestmark = pytest.mark.gpu
I3 = np.eye(3, dtype=np.float32)
P95 = dict(max_ratio=0.95, max_distance=3.2)


@pytest.fixture
def sift_tuning(gpu):
    def set_(nchunk=0, batch_partials=0):
        gpu.set_sift_tuning(nchunk, batch_partials)
    yield set_
    gpu.set_sift_tuning(0, 0)


@pytest.fixture(scope="module")
def expected():
    """reference results, computed once per (inputs, options) and shared: key -> (matches, m12, m21)"""
    cache = {}

    def get(key, S, cross_check=True, **opt):
        k = (key, cross_check, tuple(sorted(opt.items())))
        if k not in cache:
            cache[k] = er.match(S() if callable(S) else S, cross_check=cross_check, **opt)[:3]
        return cache[k]
    return get


def _device(gpu, d1, d2, cross_check=True, guide=None, **opt):
    """(matches, m12, m21) of the device entry; guide = (loc1, loc2, H, F, th, tf): the guided device entry"""
    n1, n2 = len(d1), len(d2)
    t1, t2 = torch.tensor(np.asarray(d1), device="cuda"), torch.tensor(np.asarray(d2), device="cuda")
    m12 = torch.full((n1,), -7, dtype=torch.int32, device="cuda")
    m21 = torch.full((n2,), -7, dtype=torch.int32, device="cuda")
    mm = torch.full((n1, 2), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    if guide is None:
        gpu.sift_match_device(t1, n1, t2, n2, m12, m21, mm, cnt, cross_check=cross_check, **opt)
    else:
        loc1, loc2, H, F, th, tf = guide
        l1, l2 = torch.from_numpy(np.ascontiguousarray(loc1, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(loc2, np.float32)).cuda()
        Hm, Fm = gpu._mat3(H), gpu._mat3(F)
        L = gpu.lib()
        L.pcd_sift_match_guided_device.argtypes = (
            [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            + [C.c_float] * 4 + [C.c_int] + [C.c_void_p] * 5)
        gpu._check(L.pcd_sift_match_guided_device(0, gpu._ptr(t1), gpu._ptr(l1), n1, gpu._ptr(t2), gpu._ptr(l2), n2,
                                                  gpu._vp(Hm), gpu._vp(Fm), th, tf, opt["max_ratio"], opt["max_distance"],
                                                  int(cross_check), gpu._ptr(m12), gpu._ptr(m21), gpu._ptr(mm),
                                                  gpu._ptr(cnt), None))
    torch.cuda.synchronize()
    k = int(cnt.item())
    assert 0 <= k <= n1
    return mm.cpu().numpy()[:k].astype(np.uint32), m12.cpu().numpy(), m21.cpu().numpy()


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("matches", "m12", "m21")):
        assert g.shape == e.shape and np.array_equal(g, e), (what, name, int((g != e).sum()) if g.shape == e.shape else (g.shape, e.shape))


# ---------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("nchunk", [0, 1, 2, 5])
def test_ties_first_index_wins(gpu, expected, nchunk, sift_tuning):
    """every row's best score is tied over many tiles, blocks, both lane halves and all chunks; the first column must
    win in both directions (ARG_PROBE), and a tied row must pass a ratio above 1 (RATIO_PROBE)"""
    sift_tuning(nchunk=nchunk)
    d1, d2 = er.tied_sets(*er.TIED_SHAPE)
    for name, a, b in (("tied", d1, d2), ("tied^T", d2, d1)):
        S = er.scores(a, b)
        for probe in (er.ARG_PROBE, er.RATIO_PROBE):
            for cross in (True, False):
                exp = expected(name, S, cross_check=cross, **probe)
                _same(_device(gpu, a, b, cross_check=cross, **probe), exp, (name, nchunk, probe, cross))
            small, large = sorted(((exp[1] != -1).sum(), (exp[2] != -1).sum()))
            assert small >= 600 and large >= 1800 and len(exp[0]) >= 600        # (cross off: one match per live row)
    assert len(expected("tied", None, cross_check=True, **er.RATIO_PROBE)[0]) == 6


@pytest.mark.parametrize("budget", [0, 3000])
@pytest.mark.parametrize("nchunk", [0, 2])
def test_ties_through_the_batch_entry(gpu, expected, nchunk, budget, sift_tuning):
    """the same two sets in both orders in one batch (budget: a bound on the partials that cuts the batch in two)"""
    sift_tuning(nchunk=nchunk, batch_partials=budget)
    d1, d2 = er.tied_sets(*er.TIED_SHAPE)
    for probe in (er.ARG_PROBE, er.RATIO_PROBE):
        for cross in (True, False):
            got = gpu.sift_match_batch([d1, d2], [[0, 1], [1, 0], [0, 1]], cross_check=cross, **probe)
            e01 = expected("tied", lambda: er.scores(d1, d2), cross_check=cross, **probe)[0]
            e10 = expected("tied^T", lambda: er.scores(d2, d1), cross_check=cross, **probe)[0]
            assert len(e01) >= 6 and len(e10) >= 6
            for g, e in zip(got, (e01, e10, e01)):
                assert np.array_equal(g, e), (nchunk, budget, probe, cross, len(g), len(e))


# ---------------------------------------------------------------------------------------------- placements
def _check_entries(m12, m21, entries, far, what):
    hit = 0
    for e in entries:
        want = er.placement_expected(e, far)
        assert (m12, m21)[e[0]][e[1]] == want, (what, e, (m12, m21)[e[0]][e[1]], want)
        hit += 1
    assert hit == len(entries) == 60


@pytest.mark.parametrize("nchunk", [1, 2, 5])
def test_placements(gpu, expected, nchunk, sift_tuning):
    """the table of equal-best pairs / best and runner-up (sift_edge_ref.placements): unguided, guided with a filter
    that passes everything (the guided walk's own scan order), guided with filters that reject the first of the pair"""
    sift_tuning(nchunk=nchunk)
    A, B, entries = er.placements()
    S = er.scores(A, B)
    exp = expected("place", S, cross_check=False, **er.ARG_PROBE)
    got = _device(gpu, A, B, cross_check=False, **er.ARG_PROBE)
    _check_entries(got[1], got[2], entries, "none", ("single", nchunk))
    _same(got, exp, ("place", nchunk))
    e95 = expected("place", S, cross_check=False, **P95)
    assert 3 <= (e95[1] != -1).sum() < 60                       # the single entries pass, ties and runner-ups do not
    _same(_device(gpu, A, B, cross_check=False, **P95), e95, ("place 0.95", nchunk))
    both = gpu.sift_match_batch([A, B], [[0, 1], [1, 0]], cross_check=False, **er.ARG_PROBE)
    assert np.array_equal(both[0], exp[0]) and len(exp[0]) > 1000
    assert np.array_equal(both[1], er.cross(exp[2], exp[1], False))
    for far in ("none", "a", "b"):
        loc = er.placement_locations(far)
        Sg = S.copy()
        Sg[gref.guided_reject(loc, loc, I3, None, 16.0, 16.0)] = 0
        eg = expected("place " + far, Sg, cross_check=False, **er.ARG_PROBE)
        gg = _device(gpu, A, B, cross_check=False, guide=(loc, loc, I3, None, 16.0, 16.0), **er.ARG_PROBE)
        _check_entries(gg[1], gg[2], entries, far, ("guided", far, nchunk))
        _same(gg, eg, ("place guided", far, nchunk))
        gb = gpu.sift_match_guided_batch([A, B], [loc, loc], [[0, 1], [1, 0]], [(I3, None), (I3, None)],
                                         h_max_residual=16.0, cross_check=False, **er.ARG_PROBE)
        assert np.array_equal(gb[0], eg[0]) and np.array_equal(gb[1], er.cross(eg[2], eg[1], False)), (far, nchunk)
        e95g = expected("place " + far, Sg, cross_check=False, **P95)
        _same(_device(gpu, A, B, cross_check=False, guide=(loc, loc, I3, None, 16.0, 16.0), **P95), e95g, ("guided 0.95", far))


# ---------------------------------------------------------------------------------------------- high bytes
@pytest.mark.parametrize("shape", er.HIGH_SHAPES)
def test_high_bytes(gpu, expected, shape):
    """L1-root descriptors (bytes up to 255 in most rows): the re-centred product with its row and column constants;
    rows whose winner is decided by ONE row byte >= 128 (the +1 / -1 neighbours of a true match)"""
    d1, d2, info = er.high_byte_sets(*shape)
    S = er.scores(d1, d2)
    for a, b, Sab, name in ((d1, d2, S, "high"), (d2, d1, S.T, "high^T")):
        for opt in (er.DEFAULTS, er.ARG_PROBE):
            for cross in (True, False):
                exp = expected((name, shape), Sab, cross_check=cross, **opt)
                assert len(exp[0]) > 10
                _same(_device(gpu, a, b, cross_check=cross, **opt), exp, (name, shape, opt, cross))
                assert np.array_equal(gpu.sift_match(a, b, cross_check=cross, **opt), exp[0])
    arg = expected(("high", shape), S, cross_check=False, **er.ARG_PROBE)[1]
    assert (arg[info["plus"][:, 0]] == info["plus"][:, 2]).sum() >= 1          # rows decided by a planted neighbour
    assert (arg[info["minus"][:, 0]] == info["minus"][:, 1]).sum() >= 1
    for opt in (er.DEFAULTS, er.ARG_PROBE):
        got = gpu.sift_match_batch([d1, d2], [[0, 1], [1, 0]], **opt)
        assert np.array_equal(got[0], expected(("high", shape), S, **opt)[0])
        assert np.array_equal(got[1], expected(("high^T", shape), S.T, **opt)[0])


@pytest.mark.parametrize("shape", er.UNIFORM_SHAPES)
def test_uniform_bytes_clamp_pattern(gpu, expected, shape):
    """uniform bytes 0..255: most rows' second best reaches 512^2 and clamps, the row reports -1; the pattern of -1
    under ARG_PROBE is the pattern of clamped second bests"""
    d1, d2 = er.uniform_sets(*shape)
    exp = expected(("uniform", shape), er.scores(d1, d2), cross_check=False, **er.ARG_PROBE)
    for m in exp[1:]:
        assert (m == -1).sum() > 10 and (m != -1).sum() > 10
    _same(_device(gpu, d1, d2, cross_check=False, **er.ARG_PROBE), exp, ("uniform", shape))
    got = gpu.sift_match_batch([d1, d2], [[0, 1], [1, 0]], cross_check=False, **er.ARG_PROBE)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], er.cross(exp[2], exp[1], False))


# --------------------------------------------------------------------------------------------- second best
@pytest.mark.parametrize("nchunk", [0, 1, 2, 5])
def test_second_best_decides(gpu, expected, nchunk, sift_tuning):
    """400 of 1000 rows are rejected only because of a planted runner-up in the other lane half / another block / tile /
    chunk, before or behind the best; with a lost or wrong second best they would be accepted (and the 400 rows without
    a runner-up would be rejected if the second best were too high)"""
    sift_tuning(nchunk=nchunk)
    d1, d2, plan = er.second_sensitive()
    S = er.scores(d1, d2)
    runner = plan[plan[:, 2] >= 0][:, 0]
    plain = plan[plan[:, 2] < 0][:, 0]
    for ratio in er.SECOND_RATIOS:
        opt = dict(max_ratio=ratio, max_distance=0.7)
        for a, b, Sab, name in ((d1, d2, S, "second"), (d2, d1, S.T, "second^T")):
            for cross in (True, False):
                exp = expected(name, Sab, cross_check=cross, **opt)
                assert len(exp[0]) > 100
                _same(_device(gpu, a, b, cross_check=cross, **opt), exp, (name, nchunk, ratio, cross))
        e12 = expected("second", S, cross_check=False, **opt)[1]
        assert (e12[runner] == -1).all() and len(runner) >= 200 and (e12[plain] != -1).mean() > 0.9
        got = gpu.sift_match_batch([d1, d2], [[0, 1], [1, 0]], **opt)
        assert np.array_equal(got[0], expected("second", S, **opt)[0])
        assert np.array_equal(got[1], expected("second^T", S.T, **opt)[0])


# --------------------------------------------------------------------------------------------- shape edges
@pytest.mark.parametrize("n", er.EDGE_NS)
def test_row_counts_on_the_tile_wave_and_stripe(gpu, expected, n):
    """n descriptors on either side, around the MFMA row tile (32), the wavefront's rows (64), the stripe (512) and two
    stripes (1024), against 130 and 257 on the other side: tied and high-byte data under ARG_PROBE"""
    for m in er.EDGE_MS:
        for a, b in ((n, m), (m, n)):
            for kind, (x, y) in (("tied", er.tied_sets(a, b)), ("high", er.high_byte_sets(a, b)[:2])):
                exp = expected((kind, a, b), er.scores(x, y), cross_check=False, **er.ARG_PROBE)
                assert (exp[1] != -1).sum() >= a - 1 and (exp[2] != -1).sum() >= b // 2
                _same(_device(gpu, x, y, cross_check=False, **er.ARG_PROBE), exp, (kind, a, b))


@pytest.mark.parametrize("cross", [True, False])
@pytest.mark.parametrize("n1", er.WIDE_NS)
def test_compaction_limit(gpu, expected, n1, cross):
    """16384 rows is the most the one-workgroup cross check + compaction takes; 16385 takes the three-kernel path"""
    d1, d2, _ = er.high_byte_sets(n1, er.WIDE_M)
    S = er.scores(d1, d2)
    for opt in (er.DEFAULTS, er.ARG_PROBE):
        exp = expected(("wide", n1), S, cross_check=cross, **opt)
        got = _device(gpu, d1, d2, cross_check=cross, **opt)
        assert len(got[0]) == len(exp[0]) > 10
        assert (np.diff(got[0][:, 0].astype(np.int64)) > 0).all()
        _same(got, exp, ("wide", n1, cross, opt))
    if not cross:
        assert len(exp[0]) > 16000                              # ARG_PROBE: a list as long as the set


def test_batches_at_the_compaction_limit(gpu, expected):
    """a batch that mixes a 16384-descriptor image with smaller ones (the batch kernels), and a batch that holds a
    16385-descriptor first image (the pair-by-pair route)"""
    w0, small, _ = er.high_byte_sets(er.WIDE_NS[1], er.WIDE_M)
    w1 = er.high_byte_sets(er.WIDE_NS[2], er.WIDE_M)[0]
    t1, _ = er.tied_sets(700, 130)
    imgs = [w0, small, t1, w1]
    for pairs in ([(0, 1), (1, 0), (2, 1), (1, 2), (0, 2)], [(3, 1), (1, 3), (0, 1), (2, 1)]):
        for cross, opt in ((True, er.DEFAULTS), (False, er.ARG_PROBE)):
            got = gpu.sift_match_batch(imgs, pairs, cross_check=cross, **opt)
            total = 0
            for (a, b), g in zip(pairs, got):
                exp = expected(("img", a, b), lambda: er.scores(imgs[a], imgs[b]), cross_check=cross, **opt)[0]
                assert np.array_equal(g, exp), (pairs, a, b, cross, len(g), len(exp))
                total += len(exp)
            assert total > 20


# ------------------------------------------------------------------------------------------ guided NaN / inf
def _nan_scene():
    """keypoints of set 1 at x = 6 (h2 = 1) except every 5th at x = 5, where the third row (1, 0, -5) of H gives
    h2 = 0; partners in set 2 sit where the regular rows are mapped to (1, y); the special rows' partners lie far away"""
    rng = np.random.default_rng(7)
    n1, n2 = 400, 500
    d1, d2 = er.l1_root(rng, n1), er.l1_root(rng, n2)
    cols = rng.permutation(n2)[:n1]
    d2[cols] = np.clip(d1.astype(np.int32) - rng.integers(0, 4, d1.shape), 0, 255).astype(np.uint8)
    y = 10.0 * np.arange(n1)
    loc1 = np.stack([np.full(n1, 6.0), y + 10.0], axis=1).astype(np.float32)
    special = np.arange(0, n1, 5)
    loc1[special, 0] = 5.0
    loc2 = rng.uniform(2000, 3000, (n2, 2)).astype(np.float32)
    loc2[cols] = np.stack([np.full(n1, 1.0), y + 10.0], axis=1)
    loc2[cols[special]] = (700.0, 3.0)
    return d1, loc1, d2, loc2, special, cols


def test_guided_nan_and_inf_residuals(gpu, oracle):
    """h2 == 0: 0 / 0 = NaN residuals pass (NaN > t is false), x / 0 = inf residuals are rejected unless the threshold
    is inf as well; F = 0: 0 / 0 for every pair, everything passes.  Both walk directions (m12 and m21)."""
    d1, l1, d2, l2, special, cols = _nan_scene()
    S = er.scores(d1, d2)
    H_nan = np.array([[1, 0, -5], [0, 1, 0], [1, 0, -5]], np.float32)      # x = 5: h0 = h2 = 0
    H_inf = np.array([[1, 0, 0], [0, 1, 0], [1, 0, -5]], np.float32)       # x = 5: h0 = 5, h2 = 0
    F0 = np.zeros((3, 3), np.float32)
    opt = dict(max_ratio=0.8, max_distance=0.7)
    plain = er.match(S, cross_check=False, **opt)
    assert (plain[1][special] == cols[special]).sum() >= 60
    runs = (("nan", H_nan, None, 64.0), ("inf", H_inf, None, 64.0), ("inf <= inf", H_inf, None, np.inf),
            ("F = 0", None, F0, 64.0), ("nan + F = 0", H_nan, F0, 64.0))
    for name, H, F, th in runs:
        Sg = S.copy()
        rej = gref.guided_reject(l1, l2, H, F, th, 4.0)
        Sg[rej] = 0
        for cross in (False, True):
            exp = er.match(Sg, cross_check=cross, **opt)
            assert exp[3] >= er.MARGIN
            got = _device(gpu, d1, d2, cross_check=cross, guide=(l1, l2, H, F, th, 4.0), **opt)
            _same(got, exp[:3], (name, cross))
            assert np.array_equal(gpu.sift_match_guided(d1, l1, d2, l2, H=H, F=F, h_max_residual=th, f_max_residual=4.0,
                                                        cross_check=cross, **opt), exp[0])
        e12, e21 = er.match(Sg, cross_check=False, **opt)[1:3]
        by_nan12 = (e12[special] == cols[special]).sum()
        by_nan21 = (e21[cols[special]] == special).sum()
        regular = np.setdiff1d(np.arange(len(d1)), special)
        if name in ("nan", "nan + F = 0"):
            # the special rows' partners lie 700 away: only the NaN rule lets them through, in both directions
            assert not rej[special].any() and by_nan12 >= 10 and by_nan21 >= 10
            assert (e12[regular] == cols[regular]).sum() >= 100 and rej[regular].mean() > 0.9
        elif name == "inf":
            assert rej[special].all() and by_nan12 == 0 and by_nan21 == 0 and (e12[regular] != -1).sum() >= 100
        else:
            assert not rej[special].any() and by_nan12 >= 10
            if F is not None:
                assert not rej.any() and np.array_equal(e12, plain[1])


def test_guided_f_denominator_order(gpu):
    """the F residual's denominator is ((a0^2 + a1^2) + b0^2) + b1^2 in THAT order in both walks: with a0^2 + a1^2 = 1,
    b0^2 = 2^-24 and b1^2 just above it, the other order of the last two terms rounds to the next float, the quotient
    9 / den drops by one ulp, and a threshold set to that lower quotient tells the two apart.  Keypoints of set 2 at
    the origin carry the critical pair (rejected: the true quotient is above the threshold), the others have e = 0."""
    b0, b1 = np.float32(2.0 ** -12), np.float32(2.0 ** -12 * 1.005)
    F = np.array([[0, 0, 1], [0, 0, 0], [b0, b1, 3]], np.float32)
    one = np.float32(1.0)
    den_ref, den_swapped = (one + b0 * b0) + b1 * b1, (one + b1 * b1) + b0 * b0
    tf = np.float32(9.0) / den_swapped
    assert den_ref < den_swapped and np.float32(9.0) / den_ref > tf
    rng = np.random.default_rng(12)
    n = 300
    d1 = er.l1_root(rng, n)
    d2 = np.clip(d1.astype(np.int32) - rng.integers(0, 4, d1.shape), 0, 255).astype(np.uint8)
    l1 = np.zeros((n, 2), np.float32)
    l2 = np.zeros((n, 2), np.float32)
    l2[1::2, 0] = -3.0                                          # e = x2 + 3 = 0: passes
    S = er.scores(d1, d2)
    rej = gref.guided_reject(l1, l2, None, F, 16.0, float(tf))
    assert rej[:, 0::2].all() and not rej[:, 1::2].any()
    S[rej] = 0
    opt = dict(max_ratio=0.8, max_distance=0.7)
    for cross in (False, True):
        exp = er.match(S, cross_check=cross, **opt)
        assert exp[3] >= er.MARGIN
        if not cross:
            assert (exp[1][1::2] != -1).sum() > 100 and (exp[1][0::2] == -1).all() and (exp[2][0::2] == -1).all()
        _same(_device(gpu, d1, d2, cross_check=cross, guide=(l1, l2, None, F, 16.0, float(tf)), **opt), exp[:3], ("F order", cross))

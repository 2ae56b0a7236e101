"""CPU checks of tests/sift_edge_ref.py: the plain reference equals the C oracle and tests/sift_guided_ref.py on every
generator and option set that tests/test_sift_edge_gpu.py uses, every generator has the properties it is built for,
and no row of any of them decides within MARGIN of a float threshold (so the GPU tests leave out nothing)."""
import numpy as np
import pytest

from tests import sift_edge_ref as er
from tests import sift_guided_ref as gref

P95 = dict(max_ratio=0.95, max_distance=3.2)


def _cases():
    """(name, d1, d2, option sets): everything the GPU file runs unguided"""
    t1, t2 = er.tied_sets(*er.TIED_SHAPE)
    yield "tied", t1, t2, (er.ARG_PROBE, er.RATIO_PROBE)
    yield "tied^T", t2, t1, (er.ARG_PROBE, er.RATIO_PROBE)
    A, B, _ = er.placements()
    yield "placements", A, B, (er.ARG_PROBE, P95)
    for shape in er.HIGH_SHAPES:
        d1, d2, _ = er.high_byte_sets(*shape)
        yield "high%s" % (shape,), d1, d2, (er.DEFAULTS, er.ARG_PROBE)
    for shape in er.UNIFORM_SHAPES:
        yield ("uniform%s" % (shape,),) + er.uniform_sets(*shape) + ((er.ARG_PROBE,),)
    s1, s2, _ = er.second_sensitive()
    yield "second", s1, s2, tuple(dict(max_ratio=r, max_distance=0.7) for r in er.SECOND_RATIOS)
    yield "second^T", s2, s1, tuple(dict(max_ratio=r, max_distance=0.7) for r in er.SECOND_RATIOS)
    for n in er.EDGE_NS:
        for m in er.EDGE_MS:
            for a, b in ((n, m), (m, n)):
                yield "edge tied %d x %d" % (a, b), *er.tied_sets(a, b), (er.ARG_PROBE,)
                yield "edge high %d x %d" % (a, b), *er.high_byte_sets(a, b)[:2], (er.ARG_PROBE,)
    for n in er.WIDE_NS:
        yield "wide %d" % n, *er.high_byte_sets(n, er.WIDE_M)[:2], (er.DEFAULTS, er.ARG_PROBE)


def test_reference_equals_oracle_and_margin_holds(oracle):
    worst = np.inf
    for name, d1, d2, optsets in _cases():
        S = er.scores(d1, d2)
        assert np.array_equal(S, oracle.sift_distance_matrix(d1, d2)), name
        for opt in optsets:
            for cross in (True, False):
                m, m12, m21, margin = er.match(S, cross_check=cross, **opt)
                o, o12, o21 = oracle.sift_match(d1, d2, cross_check=cross, **opt)
                assert np.array_equal(m, o) and np.array_equal(m12, o12) and np.array_equal(m21, o21), (name, opt, cross)
                assert np.array_equal(m, gref.match_from_dists(S, cross_check=cross, **opt)), (name, opt, cross)
            assert margin >= er.MARGIN, (name, opt, margin)
            worst = min(worst, margin)
    print("smallest margin of any row: %.3g rad" % worst)


def test_top2_rule_on_small_tables():
    S = np.array([[0, 0, 0], [5, 5, 3], [3, 5, 5], [1, 2, 3], [3, 2, 1], [0, 7, 0], [4, 9, 4]], np.int64)
    best, second, arg = er.top2(S)
    assert best.tolist() == [0, 5, 5, 3, 3, 7, 9]
    assert second.tolist() == [0, 5, 5, 2, 2, 0, 4]
    assert arg.tolist() == [-1, 0, 1, 2, 0, 1, 1]
    assert er.third(S).tolist() == [0, 3, 3, 1, 1, 0, 4]
    # the probes: a tie passes RATIO_PROBE and no ratio <= 1; ARG_PROBE reports arg unless the second place clamps
    b = np.array([1000, 1000, 300000, 300000, 0], np.int64)
    s = np.array([1000, 10, 10, 262144, 0], np.int64)
    a = np.array([4, 5, 6, 7, -1], np.int64)
    assert er.one_way(b, s, a, **er.RATIO_PROBE)[0].tolist() == [4, 5, 6, -1, -1]
    assert er.one_way(b, s, a, 1.0, 3.2)[0].tolist() == [-1, 5, 6, -1, -1]
    m, margin = er.one_way(b, s, a, **er.ARG_PROBE)
    assert m.tolist() == [4, 5, 6, -1, -1]
    assert margin[3] == 4.0 and np.isinf(margin[4]) and margin[:3].min() > 1.0   # two clamped places: distance only


def test_tied_sets_conditions(oracle):
    d1, d2 = er.tied_sets(*er.TIED_SHAPE)
    S = er.scores(d1, d2)
    assert S.max() < er.CLAMP
    spread, upper = er.tie_stats(S)
    spread_t, _ = er.tie_stats(S.T)
    high = np.mean(np.concatenate([d1.reshape(-1), d2.reshape(-1)]) >= 128)
    print("tied rows %.3f (transposed %.3f), first tied column in the upper half %.3f, bytes >= 128 %.4f"
          % (spread, spread_t, upper, high))
    assert spread >= 0.9 and spread_t >= 0.9 and upper >= 0.3 and high >= 0.02
    assert (d1 == 0).all(axis=1).sum() == 1
    _, m12, m21, _ = er.match(S, **er.RATIO_PROBE)
    assert (m12 != -1).sum() == er.TIED_SHAPE[0] - 1 and (m21 != -1).sum() == er.TIED_SHAPE[1]
    assert len(oracle.sift_match(d1, d2, max_ratio=1.0, max_distance=3.2, cross_check=False)[0]) == 0
    assert len(er.match(S, **er.RATIO_PROBE)[0]) == 6          # one row per base survives the cross check


@pytest.mark.parametrize("shape", er.HIGH_SHAPES + tuple((n, er.WIDE_M) for n in er.WIDE_NS))
def test_high_byte_sets_conditions(shape):
    d1, d2, info = er.high_byte_sets(*shape)
    S = er.scores(d1, d2)
    assert ((d1 >= 128).any(axis=1)).mean() >= 0.3 and ((d2 >= 128).any(axis=1)).mean() >= 0.3
    same = (d1[:, None, :8] == d2[None, :, :8]).all(axis=2)     # candidates, then the full comparison
    i, j = np.nonzero(same)
    ident = np.zeros(S.shape, bool)
    full = (d1[i] == d2[j]).all(axis=1)
    ident[i[full], j[full]] = True
    assert S[~ident].max() < er.CLAMP                        # scores of different descriptors stay below the clamp
    assert (S[ident] >= er.CLAMP).any()                      # ... some self-scores reach it
    best, second, arg = er.top2(S)
    plus, minus = info["plus"], info["minus"]
    won = (arg[plus[:, 0]] == plus[:, 2]).sum()              # the +1 neighbour beats the true match by one row byte
    held = ((arg[minus[:, 0]] == minus[:, 1]) & (second[minus[:, 0]] == S[minus[:, 0], minus[:, 2]])).sum()
    gap = best[plus[:, 0]] - second[plus[:, 0]]
    print(shape, "rows won by a +1 neighbour", won, "held against a -1 neighbour", held)
    assert won >= 1 and held >= 1 and won == len(plus) and held == len(minus)
    assert (gap >= 128).all() and (gap <= 255).all()
    assert len(er.match(S, **er.DEFAULTS)[0]) > 10


@pytest.mark.parametrize("shape", er.UNIFORM_SHAPES)
def test_uniform_sets_conditions(shape):
    d1, d2 = er.uniform_sets(*shape)
    _, m12, m21, _ = er.match(er.scores(d1, d2), **er.ARG_PROBE)
    for m in (m12, m21):
        assert 0.1 < (m == -1).mean() and (m == -1).mean() > (m != -1).mean() > 0.05, (m == -1).mean()


def test_second_sensitive_conditions():
    d1, d2, plan = er.second_sensitive()
    n2 = d2.shape[0]
    tiles = (n2 + 127) // 128
    cols_per_chunk = [128 * ((tiles + c - 1) // c) for c in (2, 5)]
    for S in (er.scores(d1, d2), er.scores(d2, d1)):
        best, second, arg = er.top2(S)
        u = er.second_place(S)
        for ratio in er.SECOND_RATIOS:
            true = er.one_way(best, second, arg, ratio, 0.7)[0]
            wrong = er.one_way(best, er.third(S), arg, ratio, 0.7)[0]
            differ = np.nonzero(true != wrong)[0]
            print("ratio %.2f: %d of %d rows decide by the second best" % (ratio, len(differ), len(S)))
            assert (true != -1).sum() > 100
            if S.shape[0] == d1.shape[0]:
                assert len(differ) >= 0.2 * len(S)
                seen = set()
                for i in differ:
                    seen |= er.second_relation(int(arg[i]), int(u[i]), cols_per_chunk)
                assert seen == set(er.SECOND_KINDS) | {"before"}, seen
    planned = plan[plan[:, 2] >= 0]
    best, second, arg = er.top2(er.scores(d1, d2))
    assert np.array_equal(arg[planned[:, 0]], planned[:, 1])
    assert np.array_equal(er.second_place(er.scores(d1, d2))[planned[:, 0]], planned[:, 2])


def test_placements_expect_what_the_oracle_returns(oracle):
    A, B, entries = er.placements()
    o, o12, o21 = oracle.sift_match(A, B, cross_check=False, **er.ARG_PROBE)
    S = er.scores(A, B)
    assert S.max() < er.CLAMP
    ties = 0
    for e in entries:
        direction, r, cols, w = e
        got = (o12, o21)[direction][r]
        assert got == er.placement_expected(e), e
        row = S[r] if direction == 0 else S[:, r]
        assert sorted(np.nonzero(row >= 39800)[0].tolist()) == sorted(cols)
        ties += w == -1 and (row[list(cols)] == 40000).all()
    assert ties == 2 * (len(er.PLACE_PAIRS) + 1)
    # the runner-up entries decide by their second best at ratio 0.95, the single ones pass
    _, p12, p21, _ = er.match(S, **P95)
    for direction, r, cols, w in entries:
        assert ((p12, p21)[direction][r] != -1) == (len(cols) == 1)
    # guided: the far columns are rejected for every row, the next of the row's columns must win
    for far in ("a", "b"):
        loc = er.placement_locations(far)
        Sg = S.copy()
        Sg[gref.guided_reject(loc, loc, np.eye(3, dtype=np.float32), None, 16.0, 16.0)] = 0
        _, g12, g21, _ = er.match(Sg, **er.ARG_PROBE)
        moved = 0
        for e in entries:
            want = er.placement_expected(e, far)
            assert want is not None and (g12, g21)[e[0]][e[1]] == want, (far, e)
            moved += want != er.placement_expected(e)
        assert moved >= 8, (far, moved)

"""The boundary scenes of tests/assoc_edge_ref.py on the CPU: the census (every row exact or margined, every
threshold met from both sides), the oracle against the exact-arithmetic reference in every decision and within a
counted rounding bound in every value, and the brute-force winners (the scenes mean what they say).

No exact row exists for the norm test: its threshold, the double 1e-6, is not a float, and the norm of a float
normal cannot come closer to it than ~1e-9 relative while evaluating exactly.  Its rows are margined, the nearest on
either side being 2.5e-9 below (the float 1e-6f itself, and a searched normal between double(1e-6f) and 1e-6) and one
float ulp above.  Likewise the ratio test has exact rows AT 10 and, above it, the nearest ratio floats allow
(succ32(10) / 1, one float ulp = 9.5e-8 relative: margined)."""
import math
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

from tests import assoc_edge_ref as ref

U = Decimal(2) ** -53
# roundings on the way to each output in assoc_oracle.c, every one at most 2^-53 relative to a term of the sum S:
#   a, b, c      3 squares + 2 additions + sqrt + the division                                      = 7
#   d            a (7) + its product with l + the three subtractions                                = 11
#   dist         X - l, the square, 2 additions, sqrt                                               = 5
#   dist2plane   a (7) + product + 2 additions + the final addition, or d (11) + the final addition = 12
#   angle        a (7) + X - l + product + 2 additions + the division + dist (5)                    = 17
N_ABC, N_D, N_DIST, N_D2P, N_ANGLE = 7, 11, 5, 12, 17


@pytest.fixture(scope="module", params=[False, True], ids=["origin", "translated"])
def scene(request, oracle):
    sc = ref.build_scene(request.param)
    idx, sq, found = oracle.nn_bruteforce(sc["xyz"], sc["q"])
    sc["idx"], sc["found"] = idx, found
    sc["out6"], sc["ok"] = oracle.search_nearest_neibor(sc["xyz"], sc["nrm"], idx, found)
    sc["translated"] = request.param
    return sc


def _ranges(sc):
    return [("per query", sc["mr"])] + [(repr(s), s) for s in ref.SCALAR_RANGES]


def test_winners(scene):
    assert scene["found"].all()
    assert np.array_equal(scene["idx"], scene["point"])
    off = np.abs(scene["q"] - scene["xyz"][scene["point"]].astype(np.float64)).max()
    assert off <= 2.5
    if scene["translated"]:
        q = scene["q"]
        # the row that needs bounded_init_key's `e`: float(q) lies farther from the winner than the gate allows
        i = next(r for r in range(len(q)) if scene["point"][r] == 50 and scene["tag"][r] == "gate eq")
        df = np.linalg.norm(q[i].astype(np.float32).astype(np.float64) - scene["xyz"][50].astype(np.float64))
        assert df * df > scene["mr"][i] ** 2 * (1 + 1e-5)
        assert (q.astype(np.float32).astype(np.float64) != q).any(axis=1).sum() > len(q) // 2


def test_census(scene):
    l, n = scene["xyz"][scene["point"]], scene["nrm"][scene["point"]]
    for name, mr in _ranges(scene):
        rows = ref.census(scene["q"], l, n, mr)
        bad = [(r, scene["tag"][r], d, s) for r, row in enumerate(rows) for d, s in row.items() if s[0] == "neither"]
        assert not bad, (name, bad[:5])
    rows = ref.census(scene["q"], l, n, scene["mr"])
    sides = {d: {s[1] for row in rows if d in row and row[d][0] == "exact" for s in [row[d]]} for d in ref.DECISIONS}
    assert sides["gate"] == {"eq", "above", "below"}
    for d in ("d2p", "p2p2"):
        assert {"eq", "above"} <= sides[d], (d, sides[d])
    cat = {name: ref.CATALOGUE_FIRST + k for k, (name, _, _) in enumerate(ref.normal_catalogue())}
    by_point = {int(scene["point"][r]): row for r, row in enumerate(rows)}
    for d in ("ratio_x", "ratio_z"):
        assert by_point[cat["ratio 10"]][d] == ("exact", "eq") and by_point[cat["ratio 10 scaled"]][d] == ("exact", "eq")
        assert by_point[cat["ratio succ32(10)"]][d] == ("margined", "above")
        assert by_point[cat["ratio 1/0.1f"]][d] == ("margined", "below")
    assert by_point[cat["only x passes"]]["ratio_x"][1] == "above" and by_point[cat["only x passes"]]["ratio_z"][1] == "below"
    assert by_point[cat["only z passes"]]["ratio_x"][1] == "above" and by_point[cat["only z passes"]]["ratio_z"][1] == "below"
    assert by_point[cat["x at 10, z passes"]]["ratio_x"] == ("exact", "eq") and by_point[cat["x at 10, z passes"]]["ratio_z"][1] == "above"
    assert by_point[cat["z at 10, x passes"]]["ratio_z"] == ("exact", "eq") and by_point[cat["z at 10, x passes"]]["ratio_x"][1] == "above"
    for name, side in (("norm 1e-6f", "below"), ("norm between constants", "below"), ("norm succ32(1e-6f)", "above"),
                       ("norm 6-8-10", "above"), ("denormal", "below"), ("zeros", "below"), ("Inf component", "above"),
                       ("NaN component", "unordered")):
        assert by_point[cat[name]]["norm"] == ("margined", side), name
    # the searched normal pins the DOUBLE constant: its norm is not below the float 1e-6f
    bx, by, _ = ref.normal_catalogue()[cat["norm between constants"] - ref.CATALOGUE_FIRST][1]
    n2 = Fraction(bx) ** 2 + Fraction(by) ** 2
    assert Fraction(ref.f32(1e-6)) ** 2 <= n2 < Fraction(1e-6) ** 2
    assert not math.sqrt(bx * bx + by * by) < ref.f32(1e-6) and math.sqrt(bx * bx + by * by) < 1e-6


def _within(got, want, n, s, what):
    if isinstance(want, float):            # NaN expected
        assert got != got, what
        return
    assert abs(Decimal(float(got)) - want) <= n * U * s, (what, got, want, n * U * s)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_against_exact_reference(scene, oracle, mode):
    l, n = scene["xyz"][scene["point"]], scene["nrm"][scene["point"]]
    accepted = rejected = 0
    for name, mr in _ranges(scene) if mode != 2 else [("none", None)]:
        abcd, typ, dist, ang, d2p = oracle.associate(scene["q"], scene["out6"], scene["ok"], mr, mode)
        r = ref.associate_ref(scene["q"], l, n, scene["found"], mr, mode)
        assert np.array_equal(scene["ok"], r["ok"]), name
        bad = np.nonzero(typ != r["type"])[0]
        assert bad.size == 0, (name, [(i, scene["tag"][i], typ[i], r["type"][i]) for i in bad[:5]])
        cen = ref.census(scene["q"], l, n, 0.0 if mr is None else mr)
        for i in range(len(typ)):
            what = (name, i, scene["tag"][i])
            for k in range(4):
                _within(abcd[i, k], r["abcd"][i][k], N_D if k == 3 else N_ABC, r["abcd_terms"][i][k], what + ("abcd", k))
            _within(dist[i], r["dist"][i], N_DIST, r["dist_terms"][i], what + ("dist",))
            _within(d2p[i], r["dist2plane"][i], N_D2P, r["dist2plane_terms"][i], what + ("dist2plane",))
            _within(ang[i], r["angle"][i], N_ANGLE, r["angle_terms"][i], what + ("angle",))
            # exact rows: the decisive value carries no rounding at all
            gate = cen[i].get("p2p2" if mode == 2 else "gate")
            if typ[i] and gate and gate[0] == "exact":
                assert float(dist[i]) == float(r["dist"][i]), what   # (50 digits round a double's tail)
            if cen[i].get("d2p", ("", ""))[0] == "exact":
                assert float(d2p[i]) == float(r["dist2plane"][i]), what
        accepted += int((typ != 0).sum())
        rejected += int((typ == 0).sum())
    assert accepted > 10 and rejected > 10
    # the catalogue's classes, on the rows every gate accepts
    if mode != 2:
        _, typ, _, _, _ = oracle.associate(scene["q"], scene["out6"], scene["ok"], scene["mr"], mode)
    else:
        _, typ, _, _, _ = oracle.associate(scene["q"], scene["out6"], scene["ok"], None, mode)
    for k, (name, _, cls) in enumerate(ref.normal_catalogue()):
        i = scene["tag"].index("normal " + name)
        assert typ[i] == cls, (name, typ[i], cls)


def test_filter_against_exact_reference(oracle):
    X, lx, typ, tags, bounds = ref.build_filter_scene()
    seen = set()
    for mp, mi in bounds:
        exp = oracle.filter_lidar_outlier(X, lx, typ, mp, mi)
        got = ref.filter_ref(X, lx, typ, mp, mi)
        assert np.array_equal(exp, got), ((mp, mi), [tags[i] for i in np.nonzero(exp != got)[0][:5]])
        cen = ref.filter_census(X, lx, typ, mp, mi)
        assert not [tags[i] for i, c in enumerate(cen) if c and c[0] == "neither"]
        seen |= {(c[1], int(t == ref.PROJ)) for c, t in zip(cen, typ) if c and c[0] == "exact"}
        assert exp[typ == 0].sum() == 0
        if mp == mp and 0 <= mp < math.inf:
            assert 0 < exp.sum() < (typ != 0).sum()
    assert seen == {(s, p) for s in ("eq", "above", "below") for p in (0, 1)}
    neg = oracle.filter_lidar_outlier(X, lx, typ, -1.0, -1.0)
    fin = ~np.isnan(X).any(axis=1) & ~np.isnan(lx).any(axis=1)
    assert (neg[(typ != 0) & fin] == 1).all() and (neg[~fin] == 0).all()          # erases even dist == 0; NaN kept
    assert oracle.filter_lidar_outlier(X, lx, typ, math.inf, math.inf).sum() == 0

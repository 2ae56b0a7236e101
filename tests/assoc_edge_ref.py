"""Boundary scenes and a second reference for the association epilogue (csrc/assoc.hip, oracle/assoc_oracle.c).

Scenes: a 5x5x5 lattice of LiDAR points at 8 m spacing (integer coordinates, negative ones included), a catalogue of
normals, and queries = lattice point + an offset of at most 2.5 m, so the nearest point is never in doubt.  The rows
are built so that the quantity each comparison of assoc_core tests is EXACT in double: it sits on its threshold, or
one representable step from it, and no rounding happens on the way.  A second copy of every scene is translated by
(4096, -8192, 2048), exact in float; there the axis offsets carry an extra 2^-30, so float(q) != q, and one of them an
extra 3 * 2^-12 that float(q) rounds away from the point: on that row the `e` term of bounded_init_key (nn.hip)
decides whether the gate-bounded search still finds a point at exactly the gate distance.
(The two-component offsets (0.375, 0.5, 0) and the offsets of exactly 1 m / 2 m of the controller gate stay as they
are in the translated copy: any change would take the decisive quantity off its threshold.)

associate_ref / filter_ref restate the decisions from the float inputs in exact rational arithmetic (fractions,
compared on squares: no square root) and the values in 50-digit decimal.  census() says for every row and decision
whether it is
    exact    -- within 1e-9 (relative) of the threshold, the exact quantity is a double, and evaluating it in float64
                in the reference's operation order reproduces that double: the decision is computed without any
                rounding, so every correct implementation of that operation order takes it alike;
    margined -- at least 1e-9 (relative) away from the threshold: ~1e7 ulp, no rounding can cross it;
anything else is "neither" and must not occur.  numpy and the standard library only.
"""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

TRANSLATION = np.array([4096.0, -8192.0, 2048.0])
ORIGIN_POINT = 62                       # lattice point (0, 0, 0)
NORMAL_X_POINT = 52                     # (0, -16, 0): carries the normal (1, 0, 0)
CATALOGUE_FIRST = 100                   # catalogue normals sit on lattice points 100, 101, ...
MARGIN = Fraction(1, 10 ** 9)
NORM_MIN = 1e-6                         # ply.cc:101, a double constant
NONE, ICP, GROUND, PROJ = 0, 1, 2, 3
DECISIONS = ("norm", "ratio_x", "ratio_z", "gate", "d2p", "p2p2")


def f32(x):
    return float(np.float32(x))


def succ32(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def succ(x):
    return math.nextafter(x, math.inf)


def pred(x):
    return math.nextafter(x, -math.inf)


def _search_norm_between_constants():
    """two-component float normal whose double norm lies in [double(1e-6f), 1e-6), at least 1e-9 (relative) below
    1e-6: rejected by the double constant, accepted if the constant were read as the float 1e-6f"""
    lo, hi = Fraction(f32(1e-6)) ** 2, (Fraction(NORM_MIN) * (1 - MARGIN)) ** 2
    rng = np.random.default_rng(20240917)
    for _ in range(100000):
        x = np.float32(rng.uniform(3e-7, 8e-7))
        y = np.float32(math.sqrt(float((lo + hi) / 2) - float(x) ** 2))
        if lo <= Fraction(float(x)) ** 2 + Fraction(float(y)) ** 2 <= hi:
            return float(x), float(y)
    raise AssertionError("no normal found between the two constants")


def normal_catalogue():
    """(name, normal, expected class); expected is the type of an accepted row, NONE = rejected by the norm test"""
    bx, by = _search_norm_between_constants()
    inf, nan = math.inf, math.nan
    return [
        ("ratio 10", (1.0, 10.0, 1.0), ICP),
        ("ratio 10 scaled", (2.0, 20.0, 2.0), ICP),
        ("ratio succ32(10)", (1.0, succ32(10.0), 1.0), GROUND),
        ("ratio 1/0.1f", (f32(0.1), 1.0, f32(0.1)), ICP),           # 9.99999985 in double
        ("signs", (-1.0, -10.5, 1.0), GROUND),
        ("nz = 0", (1.0, 10.5, 0.0), GROUND),
        ("only x passes", (0.0, 5.0, 1.0), ICP),                     # inf and 5
        ("only z passes", (1.0, 20.0, 5.0), ICP),                    # 20 and 4
        ("x at 10, z passes", (1.0, 10.0, 0.5), ICP),                # 10 and 20: `>=` on the x ratio alone shows
        ("z at 10, x passes", (0.5, 10.0, 1.0), ICP),                # 20 and 10
        ("axis y", (0.0, 1.0, 0.0), GROUND),                         # inf and inf
        ("axis z", (0.0, 0.0, 1.0), ICP),                            # 0/0 = NaN fails
        ("norm 1e-6f", (f32(1e-6), 0.0, 0.0), NONE),                 # 9.99999997e-7 < 1e-6
        ("norm succ32(1e-6f)", (succ32(1e-6), 0.0, 0.0), ICP),
        ("norm 6-8-10", (f32(6e-7), f32(8e-7), 0.0), ICP),           # 1.00000002e-6
        ("norm between constants", (bx, by, 0.0), NONE),
        ("denormal", (1e-45, 0.0, 0.0), NONE),
        ("zeros", (0.0, 0.0, 0.0), NONE),
        ("NaN component", (1.0, nan, 0.0), NONE),
        ("Inf component", (inf, 0.0, 0.0), ICP),                     # abcd = (NaN, 0, 0, NaN)
    ]


def lattice(translated):
    """125 points, index i = ix + 5 iy + 25 iz, coordinates 8 (ix - 2) etc.; normals (0, 0, 1) except the catalogue's"""
    i = np.arange(125)
    xyz = np.stack([8.0 * (i % 5 - 2), 8.0 * (i // 5 % 5 - 2), 8.0 * (i // 25 - 2)], axis=1)
    if translated:
        xyz = xyz + TRANSLATION
    nrm = np.zeros((125, 3), np.float32)
    nrm[:, 2] = 1.0
    nrm[NORMAL_X_POINT] = (1.0, 0.0, 0.0)
    for k, (_, n, _) in enumerate(normal_catalogue()):
        nrm[CATALOGUE_FIRST + k] = n
    xyz32 = xyz.astype(np.float32)
    assert np.array_equal(xyz32.astype(np.float64), xyz)
    return xyz32, nrm


def build_scene(translated):
    """-> dict(xyz, nrm, q [R][3], mr [R], point [R] intended winner, tag [R])"""
    xyz, nrm = lattice(translated)
    L = xyz.astype(np.float64)
    eps = 2.0 ** -30 if translated else 0.0
    rows = []

    def add(point, off, mr, tag):
        q = L[point] + np.asarray(off, np.float64)
        rows.append((point, q, mr, tag))
        return q

    # mapper gate: axis-aligned offsets d (sqrt(fl(d*d)) == d), ranges d, pred(d), succ(d) and the special values
    # translated, point 50 (y = -8208, float ulp 2^-10): the offset's extra 3 * 2^-12 rounds AWAY from the point in
    # float(q), so the float distance the search minimises exceeds the gate (1.2510 against 1.2507) by far more than
    # the bound's relative slack: only the `e` term of bounded_init_key keeps the point at exactly the gate distance
    for point, axis, d in ((ORIGIN_POINT, 0, 0.625), (50, 1, -(1.25 + 3 * 2.0 ** -12) if translated else -1.25),
                           (74, 2, 0.3125 if translated else 0.3), (56, 0, -2.375)):
        off = [0.0, 0.0, 0.0]
        off[axis] = d + math.copysign(eps, d)
        q = L[point] + np.asarray(off)
        r = abs(float(q[axis] - L[point][axis]))
        for mr, tag in ((r, "gate eq"), (pred(r), "gate above"), (succ(r), "gate below"), (-1.0, "gate -1"),
                        (math.inf, "gate inf"), (math.nan, "gate nan"), (5e-324, "gate denormal"), (0.0, "gate 0 far")):
            add(point, off, mr, tag)
    for point, off, r in ((51, (0.375, 0.5, 0.0), 0.625), (73, (0.75, -1.0, 0.0), 1.25), (63, (0.0, -0.75, 1.0), 1.25)):
        for mr, tag in ((r, "gate eq 2d"), (pred(r), "gate above 2d"), (succ(r), "gate below 2d")):
            add(point, off, mr, tag)
    # the query on its point: dist == 0, angle 0/0
    for point in (ORIGIN_POINT, 50, 74):
        for mr in (0.0, -0.0, 5e-324, -1.0, math.nan, math.inf, 1.0):
            add(point, (0.0, 0.0, 0.0), mr, "on point")
    # controller gate: unit axis normals, X.n + d exact; the mapper range 1.75 is clear of every distance here
    z1 = 1.0 + 2.0 ** -30 if translated else succ(1.0)
    z2 = 2.0 + 2.0 ** -30 if translated else succ(2.0)
    for point, off, tag in ((ORIGIN_POINT, (eps, 0.0, 1.0), "d2p eq"), (ORIGIN_POINT, (0.0, 0.0, z1), "d2p above"),
                            (68, (0.0, eps, -1.0), "d2p eq"), (NORMAL_X_POINT, (0.0, 0.0, 2.0), "p2p2 eq"),
                            (NORMAL_X_POINT, (0.0, 0.0, z2), "p2p2 above"), (NORMAL_X_POINT, (0.0, -2.0, 0.0), "p2p2 eq"),
                            (ORIGIN_POINT, (0.0, 0.0, 1.5), "d2p alone"), (NORMAL_X_POINT, (0.0, 0.0, 2.25), "p2p2 alone"),
                            (NORMAL_X_POINT, (1.0, 0.0, 0.0), "d2p eq"), (56, (0.25, 0.0, 0.5), "controller inside")):
        add(point, off, 1.75, tag)
    # ground and norm tests: one accepted row per catalogue normal (and one the mapper gate rejects)
    for k, (name, _, _) in enumerate(normal_catalogue()):
        add(CATALOGUE_FIRST + k, (0.25 + eps, 0.5, -0.25), 1.5, "normal " + name)
        add(CATALOGUE_FIRST + k, (0.25 + eps, 0.5, -0.25), 0.5, "normal far " + name)
    return dict(xyz=xyz, nrm=nrm, q=np.array([r[1] for r in rows]), mr=np.array([r[2] for r in rows]),
                point=np.array([r[0] for r in rows], np.uint32), tag=[r[3] for r in rows])


SCALAR_RANGES = (0.625, 1.25, 0.0, math.nan)      # passed as one range for the whole scene


# ------------------------------------------------------------------ reference ---
def _fr(v):
    return [Fraction(float(x)) for x in v]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _gt_threshold(q2, t):
    """`sqrt(q2) > t` for an exact square q2 >= 0 and a double threshold t, with IEEE semantics for t"""
    if t != t or t == math.inf:
        return False
    if t < 0:
        return True
    return q2 > Fraction(t) ** 2


def _ieee_div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _dec(fr, ctx):
    return ctx.divide(Decimal(fr.numerator), Decimal(fr.denominator))


def associate_ref(X, l32, n32, found, mr, mode):
    """rows: X [R][3] double, winner (l32, n32) [R][3] float32, found [R]; mr [R] or scalar or None (mode 2).
    -> dict: type [R] uint8, ok [R] (passed the norm test), and per output `abcd`, `dist`, `angle`, `dist2plane`
    a list of Decimal / math.nan per row plus, under the same name + "_terms", the sum of the magnitudes of the terms
    that are rounded on the way to it (the S of the error bound N 2^-53 S)."""
    R = len(X)
    mr = None if mr is None else np.broadcast_to(np.asarray(mr, np.float64), (R,))
    out = dict(type=np.zeros(R, np.uint8), ok=np.zeros(R, np.uint8), abcd=[], dist=[], angle=[], dist2plane=[],
               abcd_terms=[], dist_terms=[], angle_terms=[], dist2plane_terms=[])
    zero = Decimal(0)
    with localcontext() as ctx:
        ctx.prec = 50
        for r in range(R):
            lf, nf = [float(v) for v in l32[r]], [float(v) for v in n32[r]]
            vals = dict(abcd=[zero] * 4, dist=zero, angle=zero, dist2plane=zero, abcd_terms=[zero] * 4, dist_terms=zero,
                        angle_terms=zero, dist2plane_terms=zero)
            ok = bool(found[r]) and not any(v != v for v in lf + nf)
            nonfinite = ok and any(math.isinf(v) for v in nf)
            if ok and not nonfinite:
                ok = not _dot(_fr(nf), _fr(nf)) < Fraction(NORM_MIN) ** 2
            if ok:
                out["ok"][r] = 1
                v = [Fraction(float(X[r][k])) - Fraction(lf[k]) for k in range(3)]
                p2 = _dot(v, v)
                p2p = _dec(p2, ctx).sqrt()
                ground = abs(_ieee_div(nf[1], nf[0])) > 10 and abs(_ieee_div(nf[1], nf[2])) > 10 if nonfinite else \
                    (abs(Fraction(nf[1])) > 10 * abs(Fraction(nf[0])) and abs(Fraction(nf[1])) > 10 * abs(Fraction(nf[2])))
                if nonfinite:      # inf / inf = NaN, finite / inf = 0, NaN * l = NaN
                    vals["abcd"] = [math.nan if math.isinf(c) else zero for c in nf] + [math.nan]
                    vals["dist2plane"] = math.nan
                    ang = math.nan
                    reject_plane = False                       # NaN > 1 is false
                else:
                    n = _fr(nf)
                    n2, nv = _dot(n, n), _dot(n, v)
                    norm = _dec(n2, ctx).sqrt()
                    abc = [_dec(c, ctx) / norm for c in n]
                    al = [abc[k] * _dec(Fraction(lf[k]), ctx) for k in range(3)]
                    ax = [abc[k] * _dec(Fraction(float(X[r][k])), ctx) for k in range(3)]
                    vals["abcd"] = abc + [-(al[0] + al[1] + al[2])]
                    vals["abcd_terms"] = [abs(c) for c in abc] + [sum(abs(t) for t in al)]
                    vals["dist2plane"] = abs(_dec(nv, ctx)) / norm
                    vals["dist2plane_terms"] = sum(abs(t) for t in al) + sum(abs(t) for t in ax)
                    ang = abs(_dec(nv, ctx)) / norm / p2p if p2 else math.nan
                    vals["angle_terms"] = sum(abs(abc[k] * _dec(v[k], ctx)) for k in range(3)) / p2p if p2 else zero
                    reject_plane = nv * nv > n2                # d2p > 1
                if mode == 2:
                    reject = reject_plane or p2 > 4
                else:
                    reject = _gt_threshold(p2, float(mr[r]))
                if not reject:
                    out["type"][r] = GROUND if ground else ICP
                    vals["dist"], vals["dist_terms"], vals["angle"] = p2p, p2p, ang
            for k, val in vals.items():
                out[k].append(val)
    return out


def filter_ref(X, lidar_xyz, typ, max_proj, max_icp):
    """base/reconstruction.cc:771-805 in exact arithmetic: 1 = erased.  Any type byte other than 0 / 3 takes the Icp
    bound (the reference's switch has Proj, Icp, IcpGround; the oracle and the kernel test `== Proj` only)."""
    out = np.zeros(len(X), np.uint8)
    for i in range(len(X)):
        if typ[i] == NONE or any(c != c for c in list(X[i]) + list(lidar_xyz[i])):
            continue                                           # NaN distance: `dist > bound` is false
        v = [Fraction(float(lidar_xyz[i][k])) - Fraction(float(X[i][k])) for k in range(3)]
        out[i] = _gt_threshold(_dot(v, v), max_proj if typ[i] == PROJ else max_icp)
    return out


# --------------------------------------------------------------------- census ---
def _exact_sqrt(q2):
    x = math.sqrt(q2.numerator / q2.denominator) if q2.denominator.bit_length() < 1000 else None
    return x if x is not None and Fraction(x) ** 2 == q2 else None


def classify(q2, t, f64val):
    """q2: the exact square of the quantity, t: the threshold (double), f64val: the quantity as float64 arithmetic in
    the reference's order gives it.  -> (status, side): status exact / margined / neither; side above (the `>` holds),
    eq, below, unordered (NaN threshold)"""
    if t != t:
        return "margined", "unordered"
    if t == math.inf:
        return "margined", "below"
    if t < 0:
        return "margined", "above"
    T = Fraction(t)
    if T == 0:
        if q2 == 0:
            return ("exact" if f64val == 0.0 else "neither"), "eq"
        return "margined", "above"
    if q2 >= (T * (1 + MARGIN)) ** 2:
        return "margined", "above"
    if q2 <= (T * (1 - MARGIN)) ** 2:
        return "margined", "below"
    side = "eq" if q2 == T * T else "above" if q2 > T * T else "below"
    x = _exact_sqrt(q2)
    return ("exact" if x is not None and f64val == x else "neither"), side


def _f64_row(X, l, n):
    """assoc_oracle.c's operation order in Python floats (IEEE double, round to nearest, nothing contracted)"""
    nn = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    vx, vy, vz = X[0] - l[0], X[1] - l[1], X[2] - l[2]
    p2p = math.sqrt(vx * vx + vy * vy + vz * vz)
    d2p = math.nan
    if math.isfinite(nn) and nn > 0:
        a, b, c = n[0] / nn, n[1] / nn, n[2] / nn
        d = 0 - a * l[0] - b * l[1] - c * l[2]
        d2p = abs((X[0] * a + X[1] * b + X[2] * c) + d)
    return nn, p2p, d2p


def census(X, l32, n32, mr):
    """per row: dict decision -> (status, side) for the decisions the row reaches (a row the norm test rejects reaches
    no other).  `gate` is the mapper gate against mr[r]; d2p / p2p2 are the controller gate's two halves."""
    R = len(X)
    mr = np.broadcast_to(np.asarray(mr, np.float64), (R,))
    rows = []
    for r in range(R):
        lf, nf, Xf = [float(v) for v in l32[r]], [float(v) for v in n32[r]], [float(v) for v in X[r]]
        dec = {}
        rows.append(dec)
        if any(v != v for v in nf):
            dec["norm"] = ("margined", "unordered")            # ply.cc:100, the isnan branch
            continue
        finite = all(math.isfinite(v) for v in nf)
        nn, p2p, d2p = _f64_row(Xf, lf, nf)
        n, v = _fr(nf) if finite else None, [Fraction(Xf[k]) - Fraction(lf[k]) for k in range(3)]
        if finite:
            # `nn < 1e-6`: the quantity is below the threshold when rejected
            dec["norm"] = classify(_dot(n, n), NORM_MIN, nn)
            if dec["norm"][1] == "below":
                continue
            for name, k in (("ratio_x", 0), ("ratio_z", 2)):
                if n[k] == 0:
                    dec[name] = ("margined", "above" if n[1] != 0 else "unordered")    # inf, or 0/0
                else:
                    dec[name] = classify((n[1] / n[k]) ** 2, 10.0, abs(nf[1] / nf[k]))
            nv = _dot(n, v)
            dec["d2p"] = classify(nv * nv / _dot(n, n), 1.0, d2p)
        else:
            dec["norm"] = ("margined", "above")
            dec["ratio_x"] = dec["ratio_z"] = dec["d2p"] = ("margined", "unordered")
        dec["gate"] = classify(_dot(v, v), float(mr[r]), p2p)
        dec["p2p2"] = classify(_dot(v, v), 2.0, p2p)
    return rows


# --------------------------------------------------------------- outlier filter ---
def build_filter_scene():
    """-> X [n][3], lidar_xyz [n][3], type [n], tags, and the (max_proj, max_icp) pairs to run it with.
    Integer base coordinates (negative ones included) and axis-aligned differences: lidar - X is exact."""
    rows = []
    base = [(-16.0, 8.0, 0.0), (24.0, -8.0, 16.0), (0.0, 0.0, 0.0), (-8.0, -24.0, 8.0)]
    k = 0
    for d in (0.75, succ(0.75), pred(0.75), 1.5, succ(1.5), pred(1.5), 1.0, 0.0, 3.0):
        for t in (1, 2, 3, 4, 255, 0):
            for axis in (k % 3,):
                X = np.array(base[k % 4])
                k += 1
                lx = X.copy()
                lx[axis] += d if k % 2 else -d
                rows.append((X, lx, t, f"d={d!r} type {t}"))
    for t in (1, 3):
        X = np.array([1.0, math.nan, 2.0])
        rows.append((X, np.array([1.0, 2.0, 2.0]), t, "NaN point"))
        rows.append((np.array([1.0, 2.0, 2.0]), X.copy(), t, "NaN lidar"))
    bounds = [(1.5, 0.75), (0.75, 1.5), (-1.0, -1.0), (math.inf, math.inf), (0.0, 0.0), (math.nan, 1.0)]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], np.uint8),
            [r[3] for r in rows], bounds)


def filter_census(X, lidar_xyz, typ, max_proj, max_icp):
    out = []
    for i in range(len(X)):
        if typ[i] == NONE:
            out.append(None)
            continue
        if any(c != c for c in list(X[i]) + list(lidar_xyz[i])):
            out.append(("margined", "unordered"))
            continue
        vf = [float(lidar_xyz[i][k]) - float(X[i][k]) for k in range(3)]
        v = [Fraction(float(lidar_xyz[i][k])) - Fraction(float(X[i][k])) for k in range(3)]
        out.append(classify(_dot(v, v), max_proj if typ[i] == PROJ else max_icp,
                            math.sqrt(vf[0] * vf[0] + vf[1] * vf[1] + vf[2] * vf[2])))
    return out

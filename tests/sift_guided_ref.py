"""numpy restatement of feature/sift.cc:1092-1162 MatchGuidedSiftFeaturesCPU (test infrastructure): the distance matrix
of sift.cc:171-204 from the C oracle, the guided filter in float32 in the order of the reference's Eigen code (numpy
float32: one rounding per operation, no contraction), rejected pairs set to 0, then the one-way scans of sift.cc:55-107
and the cross check of :109-144 (acos through the host libm's acosf, as the C oracle does)."""
import ctypes
import ctypes.util

import numpy as np

_LIBM = ctypes.CDLL(ctypes.util.find_library("m"))
_LIBM.acosf.restype = ctypes.c_float
_LIBM.acosf.argtypes = [ctypes.c_float]
F32 = np.float32


def guided_reject(loc1, loc2, H=None, F=None, h_max_residual=16.0, f_max_residual=16.0):
    """[n1][n2] bool: True where the guided filter rejects (i1, i2)"""
    loc1 = np.asarray(loc1, F32).reshape(-1, 2)
    loc2 = np.asarray(loc2, F32).reshape(-1, 2)
    x1, y1 = loc1[:, 0][:, None], loc1[:, 1][:, None]
    x2, y2 = loc2[:, 0][None, :], loc2[:, 1][None, :]
    rej = np.zeros((loc1.shape[0], loc2.shape[0]), bool)
    with np.errstate(all="ignore"):
        if H is not None:
            H = np.asarray(H, F32).reshape(3, 3)
            h = [(H[i, 0] * x1 + H[i, 1] * y1) + H[i, 2] for i in range(3)]
            d0 = h[0] / h[2] - x2
            d1 = h[1] / h[2] - y2
            rej |= (d0 * d0 + d1 * d1) > F32(h_max_residual)
        if F is not None:
            F = np.asarray(F, F32).reshape(3, 3)
            a = [(F[i, 0] * x1 + F[i, 1] * y1) + F[i, 2] for i in range(3)]
            b = [(F[0, j] * x2 + F[1, j] * y2) + F[2, j] for j in range(2)]
            e = (x2 * a[0] + y2 * a[1]) + a[2]
            den = ((a[0] * a[0] + a[1] * a[1]) + b[0] * b[0]) + b[1] * b[1]
            rej |= ((e * e) / den) > F32(f_max_residual)
    return rej


def _one_way(d, max_ratio, max_distance):
    """sift.cc:55-107 on the rows of d (int64 [rows][cols]): best-match index per row or -1"""
    rows, cols = d.shape
    m = np.full(rows, -1, np.int64)
    if rows == 0 or cols == 0:
        return m
    idx = np.argmax(d, axis=1)                    # first of equal maxima = the ascending strict-> scan
    best = d[np.arange(rows), idx]
    rest = d.copy()
    rest[np.arange(rows), idx] = np.iinfo(np.int64).min
    second = np.maximum(rest.max(axis=1), 0) if cols > 1 else np.zeros(rows, np.int64)
    norm = F32(1.0 / (512.0 * 512.0))
    for i in np.nonzero(best > 0)[0]:
        bn = _LIBM.acosf(float(min(norm * F32(best[i]), F32(1.0))))
        if F32(bn) > F32(max_distance):
            continue
        sn = _LIBM.acosf(float(min(norm * F32(second[i]), F32(1.0))))
        if F32(bn) >= F32(max_ratio) * F32(sn):
            continue
        m[i] = idx[i]
    return m


def match_from_dists(dists, max_ratio=0.8, max_distance=0.7, cross_check=True):
    d = np.asarray(dists, np.int64)
    n1, n2 = d.shape
    if n1 == 0 or n2 == 0:
        return np.zeros((0, 2), np.uint32)
    m12 = _one_way(d, max_ratio, max_distance)
    m21 = _one_way(d.T, max_ratio, max_distance)
    keep = m12 != -1
    if cross_check:
        ok = np.zeros(n1, bool)
        j = m12[keep]
        ok[keep] = m21[j] == np.nonzero(keep)[0]
        keep = ok
    i1 = np.nonzero(keep)[0]
    return np.stack([i1, m12[i1]], axis=1).astype(np.uint32).reshape(-1, 2)


def sift_match_guided(oracle, d1, loc1, d2, loc2, H=None, F=None, h_max_residual=16.0, f_max_residual=16.0,
                      max_ratio=0.8, max_distance=0.7, cross_check=True):
    """MatchGuidedSiftFeaturesCPU; with H = F = None: MatchSiftFeaturesCPUBruteForce"""
    d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 128)
    d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 128)
    if d1.shape[0] == 0 or d2.shape[0] == 0:
        return np.zeros((0, 2), np.uint32)
    dists = oracle.sift_distance_matrix(d1, d2).astype(np.int64)
    if H is not None or F is not None:
        dists[guided_reject(loc1, loc2, H, F, h_max_residual, f_max_residual)] = 0
    return match_from_dists(dists, max_ratio, max_distance, cross_check)


def two_view_scene(rng, n1, n2, shared=0.6, size=1000.0, noise=0.7):
    """locations with a real two-view geometry: two cameras (K, R | t) looking at random 3D points; a `shared` share of
    set 1's points is seen in set 2 too (set 2 rows = their projections + pixel noise), the rest are distractors.
    Returns loc1, loc2, F (x2^T F x1 = 0), H (the homography of the points' mean depth plane), corr [k][2]."""
    f = size
    K = np.array([[f, 0, size / 2], [0, f, size / 2], [0, 0, 1]])
    ang = rng.normal(0, 0.08, 3)
    cx, sx = np.cos(ang), np.sin(ang)
    Rx = np.array([[1, 0, 0], [0, cx[0], -sx[0]], [0, sx[0], cx[0]]])
    Ry = np.array([[cx[1], 0, sx[1]], [0, 1, 0], [-sx[1], 0, cx[1]]])
    Rz = np.array([[cx[2], -sx[2], 0], [sx[2], cx[2], 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    t = np.array([1.0, rng.normal(0, 0.2), rng.normal(0, 0.2)])
    def proj(P, R_, t_):
        q = (K @ (R_ @ P.T + t_[:, None])).T
        return q[:, :2] / q[:, 2:3]
    P = np.column_stack([rng.uniform(-4, 4, n1), rng.uniform(-4, 4, n1), rng.uniform(8, 14, n1)])
    loc1 = proj(P, np.eye(3), np.zeros(3))
    k = min(int(shared * min(n1, n2)), n1, n2)
    src = rng.permutation(n1)[:k]
    dst = rng.permutation(n2)[:k]
    loc2 = rng.uniform(0, size, (n2, 2))
    loc2[dst] = proj(P[src], R, t) + rng.normal(0, noise, (k, 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    Fm = Ki.T @ tx @ R @ Ki
    Fm /= np.linalg.norm(Fm)
    n = np.array([0, 0, 1.0])
    Hm = K @ (R + np.outer(t, n) / 11.0) @ Ki
    Hm /= Hm[2, 2]
    corr = np.stack([src, dst], axis=1)
    return loc1.astype(F32), loc2.astype(F32), Fm.astype(F32), Hm.astype(F32), corr

"""numpy restatement of Reconstruction::FilterPoints3D as pcd_ba_filter_points defines it, and of the compaction rule of
pcd_ba_remove_observations_device.  Written from the reference, one point and one pair at a time:
  stage 1  FilterPoints3DWithLargeReprojectionError     base/reconstruction.cc:1662-1712
  stage 2  FilterPoints3DWithSmallTriangulationAngle     base/reconstruction.cc:1600-1660
           ProjectionCenterFromPose                      base/pose.cc:164-171
           CalculateTriangulationAngle                   base/triangulation.cc:122-145
The squared reprojection errors and the depths are inputs (pcd_ba_observation_errors has its own tests).  The summary
follows the library's fixed-order reduction (k_ba_filter_tracks, k_ba_filter_summary: 64 lanes by butterfly, the 4
wavefronts of a workgroup pairwise, workgroups strided over 256 accumulators, those in order), so it can be compared
bit for bit."""
import math

import numpy as np

EPS = 2.220446049250313e-16
DEG = 0.0174532925199432954743716805978692718781530857086181640625   # util/math.h DegToRad
DROPPED = 0xFFFFFFFF


def proj_center(pose):
    """normalised quaternion (a zero one: the identity), conjugated, applied to -tvec by Eigen's quat * v: uv = 2 v x X,
    X + w uv + v x uv"""
    q = np.array(pose[:4], np.float64)
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    q = np.array([1.0, 0.0, 0.0, 0.0]) if n == 0.0 else q / n
    w, a, b, c = q[0], -q[1], -q[2], -q[3]
    X = [-pose[4], -pose[5], -pose[6]]
    cx, cy, cz = b * X[2] - c * X[1], c * X[0] - a * X[2], a * X[1] - b * X[0]
    ux, uy, uz = 2.0 * cx, 2.0 * cy, 2.0 * cz
    return np.array([X[0] + w * ux + (b * uz - c * uy) + 0.0, X[1] + w * uy + (c * ux - a * uz) + 0.0,
                     X[2] + w * uz + (a * uy - b * ux) + 0.0])


def tri_angle(c1, c2, X, acos=math.acos):
    """CalculateTriangulationAngle; an acos argument outside [-1, 1] gives NaN, as std::acos does"""
    b, r, s = c1 - c2, X - c1, X - c2
    base2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
    ray1 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    ray2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2]
    den = 2.0 * math.sqrt(ray1 * ray2)
    if den == 0.0:
        return 0.0
    x = (ray1 + ray2 - base2) / den
    angle = abs(acos(x)) if -1.0 <= x <= 1.0 else math.nan
    other = math.pi - angle
    return other if other < angle else angle          # std::min(angle, pi - angle): a NaN stays


def tracks(obs_point, P):
    """the observations of every point, ascending"""
    order = np.argsort(np.asarray(obs_point), kind="stable")
    bounds = np.searchsorted(np.asarray(obs_point)[order], np.arange(P + 1))
    return [order[bounds[p]:bounds[p + 1]] for p in range(P)]


def _reduce(v):
    """the fixed-order sum of one value per point"""
    v = np.asarray(v, np.float64)
    nb = max((len(v) + 255) // 256, 1)
    a = np.zeros(nb * 256)
    a[:len(v)] = v
    a = a.reshape(nb, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lane ^ off]
    w = a[:, :, 0]
    blk = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    acc = np.zeros(256)
    for b in range(nb):
        acc[b % 256] += blk[b]
    t = 0.0
    for i in range(256):
        t += acc[i]
    return t


def filter_points(sq_err, depth, obs_image, obs_point, poses, points, max_reproj_error, min_tri_angle_deg, acos=math.acos):
    """dict as BA.filter_points returns it, plus max_angle [P]: the largest pair angle over the survivors of every point
    stage 1 kept (NaN pairs left out; -1 where stage 2 did not run), for the tests' distance-from-the-threshold check"""
    sq_err, depth = np.asarray(sq_err, np.float64), np.asarray(depth, np.float64)
    P, O = len(points), len(obs_point)
    max_sq = max_reproj_error * max_reproj_error
    erase, pdel = np.zeros(O, np.uint8), np.zeros(P, np.uint8)
    perr, filtered, max_angle = np.zeros(P), np.zeros(P), np.full(P, -1.0)
    centers = [proj_center(p) for p in np.asarray(poses, np.float64).reshape(-1, 7)]
    thr = min_tri_angle_deg * DEG
    for p, tr in enumerate(tracks(obs_point, P)):
        ndel, total = 0, 0.0
        for o in tr:
            if sq_err[o] > max_sq:
                ndel += 1
                erase[o] = 1
            else:
                total += math.sqrt(sq_err[o])
        if len(tr) < 2 or ndel + 1 >= len(tr):          # :1677-1681, :1700-1702
            pdel[p], perr[p], filtered[p] = 1, -1.0, len(tr)
            erase[tr] = 1
            continue
        perr[p], filtered[p] = total / (len(tr) - ndel), ndel
        if not min_tri_angle_deg > 0:
            continue
        live = [o for o in tr if not erase[o]]
        keep = False
        for i1 in range(len(live)):
            c1 = centers[obs_image[live[i1]]]
            for i2 in range(i1):
                ang = tri_angle(c1, centers[obs_image[live[i2]]], np.asarray(points[p], np.float64), acos)
                if ang == ang:
                    max_angle[p] = max(max_angle[p], ang)
                keep = keep or ang >= thr
        if not keep:                                    # one per point: :1653-1656
            pdel[p], perr[p], filtered[p] = 1, -1.0, ndel + 1
            erase[tr] = 1
    alive = pdel == 0
    n = _reduce(alive.astype(np.float64))
    e = _reduce(np.where(alive, perr, 0.0))
    return dict(obs_erase=erase, obs_negative_depth=(depth < EPS).astype(np.uint8), point_delete=pdel, point_error=perr,
                num_filtered=int(_reduce(filtered)), mean_reproj_error=float(e / n) if n > 0 else 0.0,
                num_points_with_error=int(n), num_negative_depth=int((depth < EPS).sum()), max_angle=max_angle)


def fresh_args_after_remove(scene, obs_erase=None, point_delete=None):
    """(the description of a fresh handle, obs_map, info counts): observation o stays iff !erase[o] and
    !point_delete[obs_point[o]], term l iff !point_delete[lidar_point[l]]; kept rows keep their order"""
    O, P = len(scene["obs_point"]), len(scene["points"])
    erase = np.zeros(O, bool) if obs_erase is None else np.asarray(obs_erase) != 0
    pdel = np.zeros(P, bool) if point_delete is None else np.asarray(point_delete) != 0
    keep = ~erase & ~pdel[scene["obs_point"]]
    kw = dict(scene)
    kw.update(obs_image=np.asarray(scene["obs_image"])[keep], obs_point=np.asarray(scene["obs_point"])[keep],
              obs_xy=np.asarray(scene["obs_xy"]).reshape(-1, 2)[keep])
    obs_map = np.where(keep, np.cumsum(keep) - 1, DROPPED).astype(np.uint32)
    nl = len(scene["lidar_point"]) if scene.get("lidar_point") is not None else 0
    lkeep = np.zeros(0, bool)
    if nl:
        lkeep = ~pdel[scene["lidar_point"]]
        for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
            kw[k] = np.asarray(scene[k])[lkeep]
        if not lkeep.any():
            for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
                kw.pop(k)
    before = np.bincount(scene["obs_point"], minlength=P)
    after = np.bincount(kw["obs_point"], minlength=P)
    info = dict(num_obs=int(keep.sum()), num_obs_removed=int((~keep).sum()), num_lidar=int(lkeep.sum()),
                num_lidar_removed=int(nl - lkeep.sum()), num_points_emptied=int(((before > 0) & (after == 0)).sum()))
    return kw, obs_map, info, lkeep

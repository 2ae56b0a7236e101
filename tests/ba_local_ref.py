"""numpy restatement of the local round's selections (pcd_ba_local_bundle_device, pcd_ba_local_window_create_device,
DESIGN 4.3g), written from the reference, one fp64 operation at a time (the library is built without FMA contraction):
  IncrementalMapper::FindLocalBundle                      sfm/incremental_mapper.cc:1747-1914
    shared observations per ROW of the image (:1762-1772), candidates by count descending -- ties by image index
    ascending, the library's choice --, the copy path (:1798-1803), the 75th percentile of the triangulation angles
    over EVERY row of the image (:1857-1873), the eight relaxation passes (:1816-1890), the fill-up (:1895-1911)
  CalculateTriangulationAngles                            base/triangulation.cc:147-181 (tests/ba_filter_ref.tri_angle)
  Percentile                                              util/math.h:231-246; std::round is math.floor(x + 0.5) here
    (x >= 0; numpy's round goes to even), a NaN angle orders behind every number -- the library's choice
  AdjustLocalBundle / AddImageToProblem / AddPointToProblem / ParameterizePoints
                                                          sfm/incremental_mapper.cc:1004-1213,
                                                          optim/bundle_adjustment.cc:814-985, 1107-1131
fresh_args_local turns a scene description and the current parameters into the description of the handle pcd_ba_create
would build for the local sub-problem."""
import math

import numpy as np

from tests import ba_filter_ref as fr

NOT_IN = 0xFFFFFFFF
DIVISORS = (1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0)
FRACTIONS = (0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1)
FILL_UP = 8                                             # the "pass" number of the fill-up stage in `fired`


def std_round(x):
    """std::round for x >= 0: halves away from zero"""
    return int(math.floor(x + 0.5))


def percentile_index(n, p=75.0):
    idx = std_round(p / 100 * (n - 1))
    return max(0, min(n - 1, idx))


def percentile(angles, p=75.0):
    """the idx-th smallest, NaN behind every number"""
    a = np.sort(np.asarray(angles, np.float64))         # numpy sorts NaN to the end
    return float(a[percentile_index(len(a), p)])


def shared_counts(obs_image, obs_point, I, P, image):
    """(shared [I] int64, n): the pairs (row of image, row of j) on the same point; shared[image] = 0"""
    obs_image, obs_point = np.asarray(obs_image), np.asarray(obs_point)
    mine = obs_image == image
    mult = np.bincount(obs_point[mine], minlength=P)
    shared = np.bincount(obs_image, weights=mult[obs_point], minlength=I).astype(np.int64)
    shared[image] = 0
    return shared, int(mine.sum())


def candidates(shared):
    """images with shared > 0: shared descending, ties by image index ascending"""
    shared = np.asarray(shared)
    order = np.argsort(-shared, kind="stable")
    return [int(j) for j in order if shared[j] > 0]


def tri_percentile(c1, c2, X, acos=math.acos):
    """the 75th percentile of the angles between the centres c1, c2 and every row of X [n][3]"""
    return percentile([fr.tri_angle(c1, c2, x, acos) for x in np.asarray(X, np.float64).reshape(-1, 3)])


def select(cand, shared, n, tri_of, num_images, min_tri_angle_deg):
    """(bundle, fired, tri): the relaxation passes and the fill-up over the ordered candidates.  tri_of(j) computes the
    percentile of candidate j; tri[j] holds it for the candidates with shared >= 0.1 * n (-1 elsewhere, and everywhere
    on the copy path); fired = the passes (0 .. 7, FILL_UP) that appended an image"""
    num_eff = min(num_images - 1, len(cand))
    tri = {j: -1.0 for j in cand}
    if len(cand) == num_eff:
        return list(cand), [], tri
    for j in cand:
        if float(shared[j]) >= 0.1 * n:
            tri[j] = tri_of(j)
    m = min_tri_angle_deg * fr.DEG
    bundle, used, fired = [], set(), []
    for k, (d, f) in enumerate(zip(DIVISORS, FRACTIONS)):
        for j in cand:
            if float(shared[j]) < f * n:
                break
            if j in used:
                continue
            if tri[j] >= m / d:
                bundle.append(j); used.add(j)
                if k not in fired:
                    fired.append(k)
                if len(bundle) >= num_eff:
                    break
        if len(bundle) >= num_eff:
            break
    if len(bundle) < num_eff:
        for j in cand:
            if j not in used:
                bundle.append(j); used.add(j)
                if FILL_UP not in fired:
                    fired.append(FILL_UP)
                if len(bundle) >= num_eff:
                    break
    return bundle, fired, tri


def local_bundle(obs_image, obs_point, poses, points, image, num_images=6, min_tri_angle_deg=6.0, acos=math.acos):
    """dict(bundle, num, image_set [I] uint8, shared [I] uint32, tri_angle [I] float64, fired, n)"""
    poses, points = np.asarray(poses, np.float64).reshape(-1, 7), np.asarray(points, np.float64).reshape(-1, 3)
    I, P = len(poses), len(points)
    shared, n = shared_counts(obs_image, obs_point, I, P, image)
    cand = candidates(shared)
    X = points[np.asarray(obs_point)[np.asarray(obs_image) == image]]
    c1 = fr.proj_center(poses[image])
    bundle, fired, tri = select(cand, shared, n, lambda j: tri_percentile(c1, fr.proj_center(poses[j]), X, acos),
                                num_images, min_tri_angle_deg)
    tri_angle = np.full(I, -1.0)
    for j, t in tri.items():
        tri_angle[j] = t
    image_set = np.zeros(I, np.uint8)
    image_set[[image] + bundle] = 1
    return dict(bundle=np.array(bundle, np.int32), num=len(bundle), image_set=image_set, shared=shared.astype(np.uint32),
                tri_angle=tri_angle, fired=fired, n=n)


def angle_gap(tri_angle, min_tri_angle_deg=6.0):
    """the smallest |tri[j] - m / d| over the computed candidates and the eight divisors (inf when none is computed):
    how far the selection is from changing with the last bits of an angle"""
    t = np.asarray(tri_angle, np.float64)
    t = t[t >= 0]
    if not len(t):
        return math.inf
    m = min_tri_angle_deg * fr.DEG
    return float(min(np.min(np.abs(t - m / d)) for d in DIVISORS))


def variable_by_rule(obs_image, obs_point, P, image, max_track_length):
    """[P] uint8: observed by `image` and track length <= max_track_length (:1110-1134)"""
    obs_image, obs_point = np.asarray(obs_image), np.asarray(obs_point)
    length = np.bincount(obs_point, minlength=P)
    seen = np.zeros(P, bool)
    seen[obs_point[obs_image == image]] = True
    return (seen & (length <= max_track_length)).astype(np.uint8)


def fresh_args_local(desc, poses, points, opts):
    """(description of the equivalent fresh handle, obs_map [O] uint32, info counts, kept terms [L] bool, image_in,
    point_variable).  desc: the keyword arguments of pcdhip.BA the source was made from (its rows and terms as they are
    now); poses / points: the source's current parameters; opts: dict(image_set, and point_variable or image with
    max_track_length (1000)), with an optional extra_const_pose."""
    poses, points = np.asarray(poses, np.float64).reshape(-1, 7), np.asarray(points, np.float64).reshape(-1, 3)
    I, P = len(poses), len(points)
    inn = (np.asarray(opts["image_set"]) != 0).astype(np.uint8)
    obs_image, obs_point = np.asarray(desc["obs_image"]), np.asarray(desc["obs_point"])
    if opts.get("point_variable") is not None:
        V = (np.asarray(opts["point_variable"]) != 0).astype(np.uint8)
    else:
        V = variable_by_rule(obs_image, obs_point, P, opts["image"], opts.get("max_track_length", 1000))
    keep = (inn[obs_image] != 0) | (V[obs_point] != 0)
    length, kept = np.bincount(obs_point, minlength=P), np.bincount(obs_point[keep], minlength=P)
    held = np.zeros(P, bool) if desc.get("point_const") is None else (np.asarray(desc["point_const"]) != 0)
    part = (kept > 0) & (kept < length)
    cpose = np.zeros(I, bool) if desc.get("image_const_pose") is None else (np.asarray(desc["image_const_pose"]) != 0)
    cpose = cpose | (inn == 0)
    if opts.get("extra_const_pose") is not None:
        cpose = cpose | (np.asarray(opts["extra_const_pose"]) != 0)
    kw = dict(desc)
    kw.update(poses=poses.copy(), points=points.copy(), image_const_pose=cpose.astype(np.uint8),
              point_const=(held | part).astype(np.uint8),
              obs_image=obs_image[keep].astype(np.int32), obs_point=obs_point[keep].astype(np.int32),
              obs_xy=np.asarray(desc["obs_xy"], np.float64).reshape(-1, 2)[keep])
    obs_map = np.where(keep, np.cumsum(keep) - 1, NOT_IN).astype(np.uint32)
    nl = len(desc["lidar_point"]) if desc.get("lidar_point") is not None else 0
    lkeep = np.zeros(0, bool)
    if nl:
        lkeep = V[np.asarray(desc["lidar_point"])] != 0
        for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
            kw[k] = np.asarray(desc[k])[lkeep]
        if not lkeep.any():
            for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
                kw.pop(k)
    info = dict(num_images_in=int(inn.sum()), num_points_variable=int(V.sum()), num_points_fixed=int((part & ~held).sum()),
                num_obs=int(keep.sum()), num_lidar=int(lkeep.sum()), num_pose_rows=int((~cpose[kw["obs_image"]]).sum()))
    return kw, obs_map, info, lkeep, inn, V

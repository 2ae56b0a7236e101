"""numpy restatement of the sphere-window selection of pcd_ba_window_create_device, written from the
reference, one fp64 operation at a time (the library is built without FMA contraction, so the two agree bit for bit):
  IncrementalMapper::AdjustGlobalBundleByLidar           sfm/incremental_mapper.cc:1347-1408
    the centre of an image: -R(q)^T t with Eigen's Quaterniond(w, x, y, z).toRotationMatrix() on the STORED quaternion
    (not normalised), :1350-1357 and :1367-1373; in iff norm(c_latest - c_i) <= ba_spherical_search_radius, :1376-1378
    a point is variable iff an "in" image observes it, :1391-1408
  AddImageInSphereToProblem                               optim/bundle_adjustment.cc:694-806
    an observation takes part iff its point is variable (:734); those on outside images are constant-pose blocks
fresh_args_window turns a scene description and the current parameters into the description of the handle
pcd_ba_create would build for that sub-problem."""
import numpy as np

NOT_IN = 0xFFFFFFFF


def centers(poses):
    """[I][3]: c_k = -((R0k t0 + R1k t1) + R2k t2), every image at once, in the order of the scalar code"""
    p = np.asarray(poses, np.float64).reshape(-1, 7)
    w, x, y, z, t0, t1, t2 = (p[:, k] for k in range(7))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R00, R01, R02 = 1.0 - (tyy + tzz), txy - twz, txz + twy
    R10, R11, R12 = txy + twz, 1.0 - (txx + tzz), tyz - twx
    R20, R21, R22 = txz - twy, tyz + twx, 1.0 - (txx + tyy)
    return np.stack([-((R00 * t0 + R10 * t1) + R20 * t2), -((R01 * t0 + R11 * t1) + R21 * t2),
                     -((R02 * t0 + R12 * t1) + R22 * t2)], axis=1)


def centers_normalised(poses):
    """the same with the quaternion normalised first (ProjectionCenterFromPose, base/pose.cc:164-171, up to rounding):
    NOT what the selection uses; the tests show where the two part"""
    p = np.array(poses, np.float64).reshape(-1, 7)
    p[:, :4] /= np.linalg.norm(p[:, :4], axis=1, keepdims=True)
    return centers(p)


def distances(poses, center_image):
    c = centers(poses)
    d = c[center_image] - c
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def image_in(poses, center_image, radius):
    """[I] uint8: dist <= radius (:1378)"""
    with np.errstate(invalid="ignore"):
        return (distances(poses, center_image) <= radius).astype(np.uint8)


def point_active(obs_image, obs_point, P, in_flags):
    """[P] uint8: some observation of the point lies on an "in" image"""
    a = np.zeros(P, np.uint8)
    a[np.asarray(obs_point)[np.asarray(in_flags)[np.asarray(obs_image)] != 0]] = 1
    return a


def gap_radius(poses, center_image, k):
    """a radius in the middle of the gap behind the k nearest images (the centre image included), and the distance of
    the nearest image centre from that boundary relative to the radius"""
    d = np.sort(distances(poses, center_image))
    r = 0.5 * (d[k - 1] + d[k])
    return r, np.min(np.abs(distances(poses, center_image) - r)) / r


def fresh_args_window(desc, poses, points, opts):
    """(description of the equivalent fresh handle, obs_map [O] uint32, info counts, kept terms [L] bool, image_in,
    point_active).  desc: the keyword arguments of pcdhip.BA the source was made from (its rows and terms as they are
    now); poses / points: the source's current parameters; opts: dict(center_image, radius) or dict(image_set), with an
    optional extra_const_pose."""
    poses, points = np.asarray(poses, np.float64).reshape(-1, 7), np.asarray(points, np.float64).reshape(-1, 3)
    I, P = len(poses), len(points)
    if opts.get("image_set") is not None:
        inn = (np.asarray(opts["image_set"]) != 0).astype(np.uint8)
    else:
        inn = image_in(poses, opts["center_image"], opts["radius"])
    obs_image, obs_point = np.asarray(desc["obs_image"]), np.asarray(desc["obs_point"])
    act = point_active(obs_image, obs_point, P, inn)
    keep = act[obs_point] != 0
    cpose = np.zeros(I, np.uint8) if desc.get("image_const_pose") is None else (np.asarray(desc["image_const_pose"]) != 0)
    cpose = (cpose.astype(bool) | (inn == 0))
    if opts.get("extra_const_pose") is not None:
        cpose |= np.asarray(opts["extra_const_pose"]) != 0
    kw = dict(desc)
    kw.update(poses=poses.copy(), points=points.copy(), image_const_pose=cpose.astype(np.uint8),
              obs_image=obs_image[keep].astype(np.int32), obs_point=obs_point[keep].astype(np.int32),
              obs_xy=np.asarray(desc["obs_xy"], np.float64).reshape(-1, 2)[keep])
    obs_map = np.where(keep, np.cumsum(keep) - 1, NOT_IN).astype(np.uint32)
    nl = len(desc["lidar_point"]) if desc.get("lidar_point") is not None else 0
    lkeep = np.zeros(0, bool)
    if nl:
        lkeep = act[np.asarray(desc["lidar_point"])] != 0
        for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
            kw[k] = np.asarray(desc[k])[lkeep]
        if not lkeep.any():
            for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
                kw.pop(k)
    info = dict(num_images_in=int(inn.sum()), num_points_active=int(act.sum()), num_obs=int(keep.sum()),
                num_lidar=int(lkeep.sum()), num_pose_rows=int((~cpose[kw["obs_image"]]).sum()))
    return kw, obs_map, info, lkeep, inn, act

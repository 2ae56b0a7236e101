"""The depth-projection route of the local bundle adjustment (pcd_ba_project_lidar_device, include/pcdhip.h) in numpy:
the scene the tests use, the per-track selection (BundleAdjustmentConfig::MatchVariablePoint2LidarPoint,
optim/bundle_adjustment.cc:288-350, as shim/lidar_hip.h:315-350 has it) and the term list a handle ends up with.

Everything is scalar float64 arithmetic in the order of the C++ (numpy scalars do not contract into FMA), so the rows
are the expected BITS of the device rows, not an approximation of them."""
import numpy as np

from pcdhip import synth

WIDTH, HEIGHT = 4032, 3024
_CACHE = {}


def cloud():
    if "cloud" not in _CACHE:
        _CACHE["cloud"] = synth.cloud_planes(400_000, seed=5)
    return _CACHE["cloud"]


def _project(poses, pts):
    """exact OPENCV projection of pts [n][3] into every image: depth [I][n], x, y"""
    pc = synth._quat_rotate(poses[:, None, :4], pts[None, :, :]) + poses[:, None, 4:]
    z = pc[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = synth._opencv_project(synth.OPENCV_PARAMS, pc[..., 0] / z, pc[..., 1] / z)
    return z, x, y


def scene(P, seed=3, max_track=4):
    """P points near rows of the cloud, each observed by up to max_track cameras of synth.ba_scene(24, 8, seed=11)'s path:
    those that see the ROW at a depth of 3-25 m inside the 4032 x 3024 image.  The observation is the exact projection of
    the point.  Returns the arguments of pcdhip.BA (one shared OPENCV camera, no LiDAR terms)."""
    key = ("scene", P, seed, max_track)
    if key in _CACHE:
        return _CACHE[key]
    xyz, _ = cloud()
    poses = synth.ba_scene(24, 8, seed=11)["poses"]
    rng = np.random.default_rng(seed)
    points, obs_image, obs_point, obs_xy = [], [], [], []
    while len(points) < P:
        rows = rng.integers(0, xyz.shape[0], 4096)
        base = xyz[rows].astype(np.float64)
        z, x, y = _project(poses, base)
        sees = (z > 3.0) & (z < 25.0) & (x > 8) & (x < WIDTH - 8) & (y > 8) & (y < HEIGHT - 8)
        for j in np.flatnonzero(sees.sum(axis=0) >= 2):
            if len(points) == P:
                break
            cams = np.flatnonzero(sees[:, j])
            cams = np.sort(rng.permutation(cams)[:max_track])
            X = base[j] + rng.normal(0, 0.02, 3)
            zz, xx, yy = _project(poses[cams], X[None])
            if not ((zz[:, 0] > 0.5).all() and (xx[:, 0] > 0).all() and (xx[:, 0] < WIDTH).all() and (yy[:, 0] > 0).all()
                    and (yy[:, 0] < HEIGHT).all()):
                continue
            p = len(points)
            points.append(X)
            for k, c in enumerate(cams):
                obs_image.append(c); obs_point.append(p); obs_xy.append([xx[k, 0], yy[k, 0]])
    s = dict(cam_model=np.array([4], np.int32), cam_params_list=[list(synth.OPENCV_PARAMS)], poses=poses,
             image_camera=np.zeros(len(poses), np.int32), points=np.array(points), obs_image=np.array(obs_image, np.int32),
             obs_point=np.array(obs_point, np.int32), obs_xy=np.array(obs_xy, np.float64))
    _CACHE[key] = s
    return s


def proj_inputs(s, poses=None, image_select=None, width=WIDTH, height=HEIGHT):
    """what pcd_proj_set_new_images takes for the scene's SELECTED images: (images, feat_xy, feat_obs).  An image's
    features are its observations in ascending observation index; feat_obs [n_feat] is the observation of every feature.
    params: the camera's parameters, zero-filled to 8."""
    poses = s["poses"] if poses is None else poses
    I = len(poses)
    order = np.argsort(s["obs_image"], kind="stable")
    start = np.searchsorted(s["obs_image"][order], np.arange(I + 1))
    images, feat, feat_obs = [], [], []
    pos = 0
    for i in range(I):
        if image_select is not None and not image_select[i]:
            continue
        prm = list(s["cam_params_list"][int(s["image_camera"][i])])
        prm = (prm + [0.0] * 8)[:8]
        o = order[start[i]:start[i + 1]]
        images.append(dict(qvec=poses[i, :4].tolist(), tvec=poses[i, 4:].tolist(), params=prm, width=width, height=height,
                           feat_begin=pos, feat_end=pos + len(o), image=i))
        feat.append(s["obs_xy"][o])
        feat_obs.append(o)
        pos += len(o)
    feat = np.concatenate(feat) if feat else np.zeros((0, 2))
    feat_obs = np.concatenate(feat_obs).astype(np.int64) if feat_obs else np.zeros(0, np.int64)
    return images, feat, feat_obs


def candidates(s, feat_obs, found, lidar6):
    """per point, its candidates in ascending observation index: (observation, lidar6 row).  An observation counts when
    its feature found a winner; of several such observations of a point in one image only the first (map::insert)."""
    O = len(s["obs_image"])
    ok = np.zeros(O, bool)
    l6 = np.zeros((O, 6))
    ok[feat_obs] = np.asarray(found).astype(bool)
    l6[feat_obs] = lidar6
    out = [[] for _ in range(len(s["points"]))]
    seen = set()
    for o in range(O):
        key = (int(s["obs_point"][o]), int(s["obs_image"][o]))
        if not ok[o] or key in seen:
            continue
        seen.add(key)
        out[key[0]].append((o, l6[o]))
    return out


def pick(X, cands):
    """lidar_hip.h:318-346 on a list of 6-vectors: (index of the winner or -1, abcd [4], xyz [3])"""
    X = np.asarray(X, np.float64)
    angle, best, which = np.float64(360), None, -1
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, c in enumerate(cands):
            c = np.asarray(c, np.float64)
            v = [X[0] - c[0], X[1] - c[1], X[2] - c[2]]
            dot = v[0] * c[3] + v[1] * c[4] + v[2] * c[5]
            nn = np.sqrt(c[3] * c[3] + c[4] * c[4] + c[5] * c[5])
            vn = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            a = np.abs(dot / (nn * vn))
            if a < angle:
                angle, best, which = a, c, k
        if which < 0:
            return -1, np.zeros(4), np.zeros(3)
        norm = np.sqrt(best[3] * best[3] + best[4] * best[4] + best[5] * best[5])
        a, b, c = best[3] / norm, best[4] / norm, best[5] / norm
        d = 0 - a * best[0] - b * best[1] - c * best[2]
    return which, np.array([a, b, c, d]), np.array(best[:3])


def dist_angle(X, abcd, xyz):
    """LidarPoint::dist / angle of a Proj association (lidar_hip.h:344-346)"""
    a, b, c, d = abcd
    w = [X[0] - xyz[0], X[1] - xyz[1], X[2] - xyz[2]]
    return (np.abs((X[0] * a + X[1] * b + X[2] * c) + d),
            np.abs((a * w[0] + b * w[1] + c * w[2]) / np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])))


def proj_rows(s, points, feat_obs, found, lidar6, point_mode=None):
    """the rows (type [P] uint8, abcd [P][4], xyz [P][3]) of the points of mode 1 (every point without point_mode); the
    others have type 0"""
    P = len(points)
    cands = candidates(s, feat_obs, found, lidar6)
    typ, abcd, xyz = np.zeros(P, np.uint8), np.zeros((P, 4)), np.zeros((P, 3))
    for p in range(P):
        if point_mode is not None and point_mode[p] != 1:
            continue
        which, r, x = pick(points[p], [c for _, c in cands[p]])
        if which >= 0:
            typ[p], abcd[p], xyz[p] = 3, r, x
    return typ, abcd, xyz


def merge_rows(proj, assoc, point_mode):
    """mode 1 -> the Proj row, mode 2 -> the association's row, mode 0 -> no term"""
    typ, abcd, xyz = (a.copy() for a in proj)
    if point_mode is not None:
        nn = np.asarray(point_mode) == 2
        typ[nn], abcd[nn], xyz[nn] = assoc["type"][nn], assoc["abcd"][nn], assoc["lidar_xyz"][nn]
        typ[np.asarray(point_mode) == 0] = 0
    return typ, abcd, xyz

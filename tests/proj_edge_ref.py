"""(test infrastructure, CPU only)  Scenes and a second reference for the edge cases of the depth-projection
association (csrc/proj.hip; the reference's lidar/pcd_projection.cc).

Three things live here, all plain numpy and none of them sharing code with oracle/proj_oracle.c:
  frustum_cloud   a cloud that fills one camera's frustum (synth.cloud_planes leaves most feature pixels empty)
  census          per (image, point): camera transform, scale branch, splat window, bitmap-word span, row count,
                  submap cull -- the proof, on the CPU, that a scene reaches the kernel path its GPU test is named for
  winners_numpy   brute-force winner per feature pixel, O(features x points): minimum of (norm bits, rank in
                  (submap key, cloud row) order) over the live points whose window covers the pixel
and the named scene builders of tests/test_proj_edge_cpu.py / tests/test_proj_edge_gpu.py, each returning
(xyz, nrm, images, feat, option keywords for oracle.proj_options)."""
import numpy as np

from pcdhip import synth

F32 = np.float32
NEAR, FAR, NEGATIVE, TOO_CLOSE, BEHIND = 0, 1, 2, 3, 4
BRANCH = {NEAR: "near", FAR: "far", NEGATIVE: "negative", TOO_CLOSE: "too close", BEHIND: "behind"}


def _c_round(x):
    """C round()/roundf(): halves away from zero (np.round goes to even); x - trunc(x) is exact"""
    t = np.trunc(x)
    return (t + np.where(np.abs(x - t) >= 0.5, np.copysign(1.0, x), 0.0)).astype(x.dtype)


def _sum3(a0, b0, a1, b1, a2, b2):
    # Eigen's fixed-size three-term reduction: t0 + (t1 + t2), every operand float32
    return a0 * b0 + (a1 * b1 + a2 * b2)


def _rotation(q):
    # Eigen::Quaterniond(w, x, y, z).toRotationMatrix() in double: no normalisation
    w, x, y, z = [float(v) for v in q]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], np.float64)


def _plane(a, b, c):
    ab, ac = a - b, a - c
    n0 = ab[1] * ac[2] - ab[2] * ac[1]
    n1 = ab[2] * ac[0] - ab[0] * ac[2]
    n2 = ab[0] * ac[1] - ab[1] * ac[0]
    d = n0 * a[0] + n1 * a[1]
    d = d + n2 * a[2]
    return np.array([n0, n1, n2, -d], F32)


def _camera(image, opt):
    """SetNewImage head + SearchSubMap (pcd_projection.cc:13-59, 258-297): scaled size, float pose, five planes"""
    s = float(opt.depth_image_scale)
    prm = [float(v) for v in image["params"]]
    w, h = int(float(image["width"]) * s), int(float(image["height"]) * s)
    R = _rotation(image["qvec"]).astype(F32)
    t = np.asarray(image["tvec"], np.float64).astype(F32)
    ifx, ify, icx, icy = prm[0] * s, prm[1] * s, prm[2] * s, prm[3] * s
    Rt = R.T
    twc = np.array([_sum3(-Rt[r, 0], t[0], -Rt[r, 1], t[1], -Rt[r, 2], t[2]) for r in range(3)], F32)
    xb = (F32(-icx / ifx), F32((float(w) - icx) / ifx))
    yb = (F32(-icy / ify), F32((float(h) - icy) / ify))
    far = F32(opt.choose_meter)
    corner = []
    for dx, dy in ((xb[1], yb[1]), (xb[1], yb[0]), (xb[0], yb[0]), (xb[0], yb[1])):
        corner.append(np.array([twc[r] + _sum3(Rt[r, 0], dx, Rt[r, 1], dy, Rt[r, 2], F32(1)) * far for r in range(3)],
                               F32))
    planes = [_plane(corner[0], corner[3], corner[2]), _plane(twc, corner[0], corner[1]),
              _plane(twc, corner[1], corner[2]), _plane(twc, corner[2], corner[3]), _plane(twc, corner[3], corner[0])]
    near = [int(float(opt.max_proj_scale) * (prm[k] / 3039.0) * (s / 0.2)) for k in (0, 1)]
    return dict(s=s, w=w, h=h, R=R, t=t, prm=prm, planes=planes, sx_near=near[0], sy_near=near[1])


def submap_keys(xyz, opt):
    """GetKeyType (pcd_projection.h:71-78): x with length, y with height, z with width.  Returns the finite-row mask
    and the int64 keys of every row (garbage on non-finite rows)."""
    xyz = np.asarray(xyz, F32)
    finite = np.isfinite(xyz).all(axis=1)
    size = np.array([opt.submap_length, opt.submap_height, opt.submap_width], F32)
    with np.errstate(all="ignore"):
        k = _c_round(np.where(finite[:, None], xyz, F32(0)) / size)
    return finite, k.astype(np.int64)


def census(xyz, image, options, coeffs):
    """Per point of `xyz` for one image: dict of arrays
         live     the kernel splats a non-empty window for this point (finite row, submap inside the five planes,
                  scale branch near/far with non-negative half-widths, finite projection, window meets the image)
         span     bitmap words per row, (uhi >> 5) - (ulo >> 5) + 1   (0 where not live)
         rows     vhi - vlo + 1                                       (0 where not live)
         branch   NEAR / FAR / NEGATIVE / TOO_CLOSE / BEHIND, from the camera-frame depth alone
         in_frustum, finite, window (live without the cull), sx, sy, u0, v0, ulo, uhi, vlo, vhi, zc, norm, key"""
    xyz = np.asarray(xyz, F32)
    cam = _camera(image, options)
    R, t, w, h, s = cam["R"], cam["t"], cam["w"], cam["h"], cam["s"]
    fx, fy, cx, cy, k1, k2, p1, p2 = cam["prm"]
    a_x, b_x, a_y, b_y = [float(v) for v in coeffs]
    lo_d, hi_d = float(options.min_lidar_proj_dist), float(options.min_proj_dist)
    finite, key = submap_keys(xyz, options)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        xc = _sum3(R[0, 0], x, R[0, 1], y, R[0, 2], z) + t[0]
        yc = _sum3(R[1, 0], x, R[1, 1], y, R[1, 2], z) + t[1]
        zc = _sum3(R[2, 0], x, R[2, 1], y, R[2, 2], z) + t[2]
        depth = zc.astype(np.float64)
        behind = zc < 0
        close = ~behind & (depth < lo_d)
        near = ~behind & ~close & (lo_d <= depth) & (depth <= hi_d)
        far = ~behind & ~close & ~near & (depth > hi_d)
        fsx, fsy = np.trunc(a_x * depth + b_x), np.trunc(a_y * depth + b_y)
        sx = np.where(near, cam["sx_near"], np.where(far & np.isfinite(fsx), fsx, -1)).astype(np.int64)
        sy = np.where(near, cam["sy_near"], np.where(far & np.isfinite(fsy), fsy, -1)).astype(np.int64)
        negative = far & ((sx < 0) | (sy < 0))
        u_ori = fx * (xc / zc).astype(np.float64) + cx
        v_ori = fy * (yc / zc).astype(np.float64) + cy
        # DistortOpenCV, pcd_projection.cc:561-594
        xn, yn = (u_ori - cx) / fx, (v_ori - cy) / fy
        r2 = xn * xn + yn * yn
        radial = 1. + k1 * r2 + k2 * r2 * r2
        dtx = 2. * p1 * xn * yn + p2 * (r2 + 2. * xn * xn)
        dty = p1 * (r2 + 2. * yn * yn) + 2. * p2 * xn * yn
        ud = (xn * radial * 1.0 + dtx) * fx + cx
        vd = (yn * radial * 1.0 + dty) * fy + cy
        ur, vr = _c_round(ud * s), _c_round(vd * s)
        ok = (np.abs(ur) < 1e9) & (np.abs(vr) < 1e9)
        u0 = np.where(ok, ur, 0).astype(np.int64)
        v0 = np.where(ok, vr, 0).astype(np.int64)
        norm = np.sqrt(xc * xc + (yc * yc + zc * zc))
        # SearchImageMap, pcd_projection.cc:523-553: the key centre against the five planes, float
        size = np.array([options.submap_length, options.submap_height, options.submap_width], F32)
        c = key.astype(F32) * size
        inside = np.ones(xyz.shape[0], bool)
        for pl in cam["planes"]:
            v = pl[0] * c[:, 0] + pl[1] * c[:, 1]
            v = v + pl[2] * c[:, 2]
            v = v + pl[3]
            inside &= v <= 0
    ulo, uhi = np.maximum(u0 - sx, 0), np.minimum(u0 + sx, w - 1)
    vlo, vhi = np.maximum(v0 - sy, 0), np.minimum(v0 + sy, h - 1)
    window = ok & (near | far) & ~negative & (ulo <= uhi) & (vlo <= vhi) & (w > 0) & (h > 0)
    inside &= finite & (w > 0) & (h > 0)
    live = finite & window & inside
    branch = np.select([behind, close, near, negative, far], [BEHIND, TOO_CLOSE, NEAR, NEGATIVE, FAR], default=BEHIND)
    return dict(live=live, span=np.where(live, (uhi >> 5) - (ulo >> 5) + 1, 0), rows=np.where(live, vhi - vlo + 1, 0),
                branch=branch, in_frustum=inside, finite=finite, window=window, sx=sx, sy=sy, u0=u0, v0=v0, ulo=ulo,
                uhi=uhi, vlo=vlo, vhi=vhi, zc=zc, norm=norm.astype(F32), key=key, w=w, h=h)


def feature_pixels(feat, scale, w, h):
    """pcd_projection.cc:35-36: (xy * scale).cast<int>() and the bounds check.  Outside +-2e9 (and NaN) the cast is
    undefined in the reference; such a feature is no feature pixel (the project's documented choice)."""
    with np.errstate(all="ignore"):
        f = np.asarray(feat, np.float64).reshape(-1, 2) * scale
        sane = (np.abs(f) < 2e9).all(axis=1)
        uv = np.trunc(np.where(sane[:, None], f, -1.0)).astype(np.int64)
    ok = sane & (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
    return ok, uv[:, 0], uv[:, 1]


def winners_numpy(xyz, images, feat, options, coeffs, chunk=128):
    """Brute force: found, index (cloud row), dist (float32 norm) per feature, and the surviving (image, submap) pairs"""
    xyz = np.asarray(xyz, F32)
    feat = np.asarray(feat, np.float64).reshape(-1, 2)
    nf = feat.shape[0]
    found, index, dist = np.zeros(nf, np.uint8), np.full(nf, 0xFFFFFFFF, np.uint32), np.zeros(nf, F32)
    finite, key = submap_keys(xyz, options)
    rows = np.arange(xyz.shape[0])
    order = np.lexsort((rows, key[:, 2], key[:, 1], key[:, 0]))      # (key, cloud row): the reference's walk
    order = order[finite[order]]
    rank = np.zeros(xyz.shape[0], np.uint64)
    rank[order] = np.arange(order.size, dtype=np.uint64)
    pairs = 0
    for im in images:
        c = census(xyz, im, options, coeffs)
        pairs += np.unique(key[c["in_frustum"]], axis=0).shape[0]
        cand = np.flatnonzero(c["live"])
        b, e = im["feat_begin"], im["feat_end"]
        ok, u, v = feature_pixels(feat[b:e], float(options.depth_image_scale), c["w"], c["h"])
        fid = b + np.flatnonzero(ok)
        if cand.size == 0 or fid.size == 0:
            continue
        u, v = u[ok], v[ok]
        k64 = (c["norm"][cand].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rank[cand]
        ulo, uhi, vlo, vhi = [c[n][cand] for n in ("ulo", "uhi", "vlo", "vhi")]
        none = np.uint64(0xFFFFFFFFFFFFFFFF)
        for i in range(0, fid.size, chunk):
            uu, vv = u[i:i + chunk, None], v[i:i + chunk, None]
            cover = (ulo <= uu) & (uu <= uhi) & (vlo <= vv) & (vv <= vhi)
            masked = np.where(cover, k64, none)
            best = masked.argmin(axis=1)
            hit = cover[np.arange(best.size), best]
            g = fid[i:i + chunk][hit]
            found[g] = 1
            index[g] = cand[best[hit]]
            dist[g] = c["norm"][cand[best[hit]]]
    return found, index, dist, pairs


# ------------------------------------------------------------------------------------------------------ clouds ---
def frustum_cloud(image, n, zmax, rng, margin=0.1, margin_px=0.0):
    """n points that fill the image's frustum: pixels U(image grown by `margin` of its size + `margin_px` on every
    side), depths U(0.2, zmax), back-projected (pinhole, distortion ignored) into world coordinates.  Normals are
    random unit vectors, so a zero ray/plane denominator has probability zero."""
    fx, fy, cx, cy = [float(v) for v in image["params"][:4]]
    W, H = float(image["width"]), float(image["height"])
    u = rng.uniform(-margin * W - margin_px, (1 + margin) * W + margin_px, n)
    v = rng.uniform(-margin * H - margin_px, (1 + margin) * H + margin_px, n)
    z = rng.uniform(0.2, zmax, n)
    pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    q = np.asarray(image["qvec"], np.float64)
    R = _rotation(q / np.linalg.norm(q))
    pw = (pc - np.asarray(image["tvec"], np.float64)) @ R          # R^T (pc - t)
    nn = rng.normal(size=(n, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    return pw.astype(F32), nn.astype(F32)


def _clouds(images, n, zmax, rng, **kw):
    parts = [frustum_cloud(im, n, zmax, rng, **kw) for im in images]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _opts(oracle, images, okw):
    oo = oracle.proj_options(**okw)
    return oo, oracle.proj_scale_coeffs(oo, images[0]["params"][0], images[0]["params"][1])


def _pixel_feats(u, v, scale, frac=0.5):
    return np.stack([(np.asarray(u, np.float64) + frac) / scale, (np.asarray(v, np.float64) + frac) / scale], axis=1)


def _set_ranges(images, feats):
    pos = 0
    for im, f in zip(images, feats):
        im["feat_begin"], im["feat_end"] = pos, pos + len(f)
        pos += len(f)
    return np.concatenate(feats) if feats else np.zeros((0, 2))


# ------------------------------------------------------------------------------------------------------ scenes ---
def scene_wide(seed=1, feats=2000):
    """max_proj_scale = 40 on the default camera: splats up to 81 pixels wide, three and four bitmap words"""
    rng = np.random.default_rng(seed)
    images, feat = synth.proj_scene(2, feats, seed=seed)
    xyz, nrm = _clouds(images, 15000, 48.0, rng)
    return xyz, nrm, images, feat, dict(max_proj_scale=40)


def scene_point(oracle, max_proj_scale=0, min_proj_scale=0, seed=1):
    """the wide scene's cloud with splats of one pixel (scales 0/0) or 3 x 3 (1/1); a tenth of the features sit on
    the projected pixel of a live point so that some are found whatever the density"""
    xyz, nrm, images, feat, _ = scene_wide(seed, feats=1500)
    okw = dict(max_proj_scale=max_proj_scale, min_proj_scale=min_proj_scale)
    oo, c4 = _opts(oracle, images, okw)
    rng = np.random.default_rng(seed + 100)
    for im in images:
        c = census(xyz, im, oo, c4)
        pick = rng.choice(np.flatnonzero(c["live"] & (c["u0"] >= 0) & (c["u0"] < c["w"]) & (c["v0"] >= 0)
                                         & (c["v0"] < c["h"])), 150, replace=False)
        b = im["feat_begin"]
        feat[b:b + 150] = _pixel_feats(c["u0"][pick], c["v0"][pick], oo.depth_image_scale, rng.uniform(0.05, 0.95))
    return xyz, nrm, images, feat, okw


def scene_borders(oracle, seed=2):
    """one default-camera image, a cloud reaching 10 % past every border (splats clipped left, right, top, bottom:
    even row counts and every rows % 4 class), features along row 0, row H-1, column 0, column W-1, the four
    corners, and features at x = -0.5 / scale and y = -0.5 / scale: truncation toward zero puts them in pixel 0"""
    rng = np.random.default_rng(seed)
    images, feat = synth.proj_scene(1, 600, seed=seed)
    xyz, nrm = _clouds(images, 30000, 30.0, rng)
    okw = dict()
    oo, c4 = _opts(oracle, images, okw)
    c = census(xyz, images[0], oo, c4)
    s, w, h = oo.depth_image_scale, c["w"], c["h"]
    n = 300
    edge = [_pixel_feats(rng.integers(0, w, n), np.zeros(n), s, rng.uniform(0.01, 0.99, n)),
            _pixel_feats(rng.integers(0, w, n), np.full(n, h - 1), s, rng.uniform(0.01, 0.99, n)),
            _pixel_feats(np.zeros(n), rng.integers(0, h, n), s, rng.uniform(0.01, 0.99, n)),
            _pixel_feats(np.full(n, w - 1), rng.integers(0, h, n), s, rng.uniform(0.01, 0.99, n)),
            _pixel_feats([0, w - 1, 0, w - 1], [0, 0, h - 1, h - 1], s)]
    # by construction: points whose window reaches column 0 / row 0; the feature has a negative coordinate
    left = np.flatnonzero(c["live"] & (c["ulo"] == 0) & (c["v0"] >= 0) & (c["v0"] < h))[:20]
    top = np.flatnonzero(c["live"] & (c["vlo"] == 0) & (c["u0"] >= 0) & (c["u0"] < w))[:20]
    neg = [np.stack([np.full(left.size, -0.5 / s), (c["v0"][left] + 0.5) / s], axis=1),
           np.stack([(c["u0"][top] + 0.5) / s, np.full(top.size, -0.5 / s)], axis=1),
           np.stack([np.full(left.size, -1.0 / s), (c["v0"][left] + 0.5) / s], axis=1)]   # pixel -1: never found
    feat = _set_ranges(images, [np.concatenate([feat] + edge + neg)])
    info = dict(neg_begin=600 + 4 * n + 4, n_left=left.size, n_top=top.size)
    return xyz, nrm, images, feat, okw, info


NARROW_WIDTHS = (1, 31, 32, 33, 64)
NARROW_POINTS = 300


def scene_narrow(seed=3):
    """five images whose scaled widths are 1, 31, 32, 33 and 64 (row_words 1 / 1 / 1 / 2 / 2, partial and full last
    words), 96 scaled rows, depth_image_scale 0.5 so the sizes are exact; EVERY pixel is a feature, so each column
    and each word edge is pinned; splat half-widths 0 to 4 across, 2 to 6 down"""
    rng = np.random.default_rng(seed)
    prm = [200.0, 200.0, 0.0, 96.0, 0.02, -0.01, 1e-4, -1e-4]
    poses, _ = synth.proj_scene(len(NARROW_WIDTHS), 0, seed=seed, width=2, height=192, params=prm)
    images, feats, clouds = [], [], []
    for im, ws in zip(poses, NARROW_WIDTHS):
        im = dict(im, width=2 * ws, params=[prm[0], prm[1], float(ws), prm[3]] + prm[4:])
        images.append(im)
        clouds.append(frustum_cloud(im, NARROW_POINTS, 20.0, rng, margin=0.0, margin_px=8.0))
        uu, vv = np.meshgrid(np.arange(ws), np.arange(96))
        feats.append(_pixel_feats(uu.ravel(), vv.ravel(), 0.5, rng.uniform(0.01, 0.99, uu.size)))
    feat = _set_ranges(images, feats)
    xyz, nrm = np.concatenate([c[0] for c in clouds]), np.concatenate([c[1] for c in clouds])
    okw = dict(depth_image_scale=0.5, max_proj_scale=30, min_proj_scale=2, submap=0.05, choose_meter=25.0)
    return xyz, nrm, images, feat, okw


def scene_duplicates(oracle, seed=4, groups=60, copies=5):
    """the borders cloud; `groups` pixels under live points, each holding `copies` features at different sub-pixel
    positions (feature index g * copies + k)"""
    xyz, nrm, images, _, okw, _ = scene_borders(oracle, seed)
    oo, c4 = _opts(oracle, images, okw)
    c = census(xyz, images[0], oo, c4)
    rng = np.random.default_rng(seed + 7)
    pick = rng.choice(np.flatnonzero(c["live"] & (c["u0"] >= 0) & (c["u0"] < c["w"]) & (c["v0"] >= 0)
                                     & (c["v0"] < c["h"])), groups, replace=False)
    u, v = np.repeat(c["u0"][pick], copies), np.repeat(c["v0"][pick], copies)
    f = (np.stack([u, v], axis=1) + rng.uniform(0.0, 0.999, (u.size, 2))) / oo.depth_image_scale
    f[::copies] = np.stack([c["u0"][pick], c["v0"][pick]], axis=1) / oo.depth_image_scale     # exactly on the corner
    feat = _set_ranges(images, [f])
    return xyz, nrm, images, feat, okw


BOUNDARY_PRM = [1519.5, 1519.5, 2015.0, 1510.0, 0.0, 0.0, 0.0, 0.0]


def boundary_depths(min_proj_dist, min_lidar_proj_dist, coeffs):
    """the depths (float32) of the boundary classes, by name"""
    f = lambda v: F32(v)
    up = lambda v: np.nextafter(F32(v), F32(np.inf))
    down = lambda v: np.nextafter(F32(v), F32(-np.inf))
    a_x, b_x = float(coeffs[0]), float(coeffs[1])
    # first float32 depth beyond min_proj_dist at which (int)(a_x * d + b_x) is 0 / negative: walk up from the real
    # root of a_x * d + b_x = 1 (resp. = -1 + tiny) a few ulps either side
    def first(pred, guess):
        d = F32(guess)
        for _ in range(64):
            d = down(d)
        for _ in range(200):
            if pred(int(np.trunc(a_x * float(d) + b_x))):
                return d
            d = up(d)
        raise AssertionError("no boundary near %r" % guess)
    zero = first(lambda k: k == 0, (1.0 - b_x) / a_x)
    negative = first(lambda k: k < 0, (-1.0 - b_x) / a_x)
    return {"at min_proj_dist": f(min_proj_dist), "just past min_proj_dist": up(min_proj_dist),
            "at min_lidar_proj_dist": f(min_lidar_proj_dist), "just below min_lidar_proj_dist": down(min_lidar_proj_dist),
            "zero": f(0.0), "minus zero": f(-0.0), "behind": f(-0.04), "first zero scale": zero,
            "last positive scale": down(zero), "first negative scale": negative, "last zero scale": down(negative)}


NEAR_CLASSES = ("at min_proj_dist", "just past min_proj_dist", "at min_lidar_proj_dist", "just below min_lidar_proj_dist",
                "zero", "minus zero", "behind")
FAR_CLASSES = ("first zero scale", "last positive scale", "first negative scale", "last zero scale")


def scene_boundary(oracle, min_lidar_proj_dist=0.5, part="near"):
    """identity pose (zc == z exactly), one point per boundary class, each in its own 160 x 150 pixel cell of the
    scaled image; per point a feature on the centre pixel and on the pixels up to and just past the right and bottom
    edge of the widest splat.  fx = fy = 3039 / 2 makes a_x = -0.5, b_x = 21, b_y = 22 exact (b_y carries the
    reference's unscaled min_proj_scale), so the near branch (20, 20) and the far branch just past min_proj_dist
    (19, 20) differ.
    part "near": the classes around min_proj_dist, min_lidar_proj_dist and depth 0, in 0.1 m submaps (each point's
    submap centre is next to it, inside the frustum).
    part "far": the classes where (int)(a * d + b) reaches 0 (d just past 40) and -1 (d = 44).  submap_width (the z
    axis) is 18 there: the centre z = 36 is inside the far plane at choose_meter = 40 while its cell runs to z = 45.
    With 1 m submaps no point deeper than 40.5 survives the cull and the kernel's `sx < 0` test never sees one."""
    okw = dict(max_proj_scale=40, min_proj_scale=2, min_proj_dist=2.0, min_lidar_proj_dist=min_lidar_proj_dist)
    okw.update(dict(submap=0.1) if part == "near" else dict(submap_length=1.0, submap_height=1.0, submap_width=18.0))
    images = [dict(qvec=[1.0, 0.0, 0.0, 0.0], tvec=[0.0, 0.0, 0.0], params=list(BOUNDARY_PRM), width=4032,
                   height=3024, feat_begin=0, feat_end=0)]
    oo, c4 = _opts(oracle, images, okw)
    depths = boundary_depths(okw["min_proj_dist"], min_lidar_proj_dist, c4)
    names = list(NEAR_CLASSES if part == "near" else FAR_CLASSES)
    extra = {}
    if part == "far":
        # 48 more depths from 41 to 44.95 (scales (0, 1), (0, 0) and (-1, 0)), 12 pixels apart so that their feature
        # sets overlap: the kernel's `sx < 0 || sy < 0` skip sees a few dozen points, not one per class
        extra = {"sweep %d" % j: F32(d) for j, d in enumerate(np.linspace(41.0, 44.95, 48))}
        names += list(extra)
        depths = dict(depths, **extra)
    xyz, feats = [], []
    for k, name in enumerate(names):
        d = float(depths[name])
        uc, vc = 80 + 160 * (k % 5), 75 + 150 * (k // 5)          # target scaled pixel
        if name in extra:
            j = k - len(FAR_CLASSES)
            uc, vc = 100 + 12 * (j % 24), 300 + 40 * (j // 24)
        x = (uc * 5 + 2.0 - BOUNDARY_PRM[2]) / BOUNDARY_PRM[0] * d
        y = (vc * 5 + 2.0 - BOUNDARY_PRM[3]) / BOUNDARY_PRM[1] * d
        if name == "zero":
            x, y = 0.0, 0.0                                        # 0 / 0: NaN pixel
        if name == "minus zero":
            x, y = 0.03, -0.02                                     # x / -0: infinite pixel
        xyz.append([x, y, d])
        offs = [(0, 0)] + [(o, 0) for o in range(-1, 23)] + [(0, o) for o in range(1, 24)]
        feats.append(_pixel_feats([uc + o[0] for o in offs], [vc + o[1] for o in offs], 0.2))
    xyz = np.array(xyz, F32)
    nrm = np.tile(np.array([0.0, 0.6, -0.8], F32), (xyz.shape[0], 1))
    feat = _set_ranges(images, [np.concatenate(feats)])
    return xyz, nrm, images, feat, okw, names


def shift_world(images, d):
    """move every camera centre by d (world frame)"""
    out = []
    for im in images:
        q = np.asarray(im["qvec"], np.float64)
        R = _rotation(q / np.linalg.norm(q))
        out.append(dict(im, tvec=(np.asarray(im["tvec"], np.float64) - R @ np.asarray(d, np.float64)).tolist()))
    return out


def scene_anisotropic(seed=5):
    """submaps 0.7 x 2.1 x 1.3 (length, height, width), a uniform cloud centred on the origin (negative keys on every
    axis), rows on exact half-cell borders, duplicated rows (equal norms, cloud order decides), NaN / +inf / -inf rows"""
    rng = np.random.default_rng(seed)
    box = np.array([30.0, 12.0, 30.0])
    xyz = ((rng.random((20000, 3)) - 0.5) * box).astype(F32)
    size = np.array([0.7, 2.1, 1.3], F32)
    border = ((rng.integers(-8, 8, (300, 3)).astype(F32) + F32(0.5)) * size).astype(F32)
    mixed = border.copy()
    mixed[:, 1:] = xyz[:300, 1:]                                  # on a border along x only
    xyz = np.concatenate([xyz, border, mixed])
    xyz = np.concatenate([xyz, xyz[4000:6000][::-1]])             # duplicates, later rows
    bad = rng.choice(xyz.shape[0], 45, replace=False)
    for k, r in enumerate(bad):
        xyz[r, k % 3] = [np.nan, np.inf, -np.inf][(k // 3) % 3]
    nn = rng.normal(size=xyz.shape)
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    prm = [500.0, 505.0, 322.0, 238.0, 0.03, -0.01, 2e-4, -1e-4]
    images, feat = synth.proj_scene(3, 1200, seed=seed, scene_box=box, width=640, height=480, params=prm)
    images = shift_world(images, -box / 2)
    okw = dict(max_proj_scale=40, min_proj_scale=6, choose_meter=15.0, submap_length=0.7, submap_height=2.1,
               submap_width=1.3)
    return xyz, nn.astype(F32), images, feat, okw


CHUNK_PRM = [500.0, 498.0, 321.0, 239.0, 0.02, -0.005, 1e-4, -1e-4]


def scene_chunked(n_images=130, feats=40, seed=6):
    """300 000 uniform points in 0.1 m submaps (nearly one submap per point), 130 small images: the pair list of one
    chunk holds 32 Mi / n_sub images (the test asserts that this is under 130 and at least 65), so the batch takes
    two trips through the chunk loop"""
    xyz, nrm = synth.cloud_uniform(300_000, seed=seed)
    images, feat = synth.proj_scene(n_images, feats, seed=seed, width=640, height=480, params=CHUNK_PRM)
    return xyz, nrm, images, feat, dict(submap=0.1)


def scene_feature_stride(seed=7, many=270_000, few=10):
    """one image with more features than the 1024 x 256 threads of the feature kernels' capped grid, one with ten"""
    rng = np.random.default_rng(seed)
    images, _ = synth.proj_scene(2, 0, seed=seed)
    xyz, nrm = _clouds(images, 4000, 30.0, rng)
    W, H = images[0]["width"], images[0]["height"]
    feats = [np.stack([rng.uniform(-0.02 * W, 1.02 * W, k), rng.uniform(-0.02 * H, 1.02 * H, k)], axis=1)
             for k in (many, few)]
    feat = _set_ranges(images, feats)
    return xyz, nrm, images, feat, dict()


def scene_small_images(images, seed=8, feats=60):
    """the first camera of `images` on a much smaller sensor (same intrinsics, so the latched coefficients agree)"""
    rng = np.random.default_rng(seed)
    im = dict(images[0], width=1003, height=701)
    f = np.stack([rng.uniform(0, 1003, feats), rng.uniform(0, 701, feats)], axis=1)
    small = [im]
    return small, _set_ranges(small, [f])

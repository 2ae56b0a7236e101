"""The BA point and image passes where their load order can go wrong (k_ba_points, k_ba_images, k_ba_cost).

Both Jacobian-pass kernels issue their loads ahead of use: k_ba_images reads the workgroup's pose and camera once and
prefetches the next iteration's indices (clamped to the segment's last observation) and point; k_ba_points reads every
row's image one row ahead (slots past the slice replaced by slot 0) and the first LiDAR term of a track from a
track-ordered copy.  What that can break: the last iteration of a segment, a segment boundary, an image without a
segment, a clamped prefetch at the very end of the arrays, padding slots and a half without a row in a slice, tracks
with 0-3 LiDAR terms, handles without LiDAR terms or without observations, and values cached across launches.

Scenes: small-rotation cameras looking along +z at points 5-12 m in front of all of them (so any image may observe
any point), observations re-projected through the oracle's camera models (tests/ba_schur_ref.reproject).
Bound: the project's 1e-9 relative with the per-column / per-block scales of tests/ba_edge_ref.py, as
tests/test_ba_edge_gpu.py; two calls in a row are bitwise equal."""
import numpy as np
import pytest

from tests import ba_edge_ref as er
from tests import ba_schur_ref as sr

pytestmark = pytest.mark.gpu
WANT = ("cost", "H_img", "g_img", "H_pt", "g_pt", "W")

# observations per image: the last iteration of a segment (1023, 1025), a segment boundary (1024, 1025), less than one
# wavefront, one iteration exactly (256), no segment (0).  The image with the highest index owns the last observation
# of the image-major arrays: 1025 (a second segment of one observation), 1024 (a full last iteration of a full segment),
# 256 (one full iteration)
COUNTS = ([0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025],
          [1025, 0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024],
          [1024, 1025, 0, 1, 63, 65, 255, 257, 1023, 64, 256])
CONST_IMAGE = 5                      # 255 / 65 / 65 observations, between two variable images
CAMERAS = {"shared": (4,), "shared_radial": (3,), "one_model": (4, 4, 4), "mixed": (4, 1, 7, 2)}


def _base(rng, I, P, models):
    poses = np.stack([er._generic_pose(rng) for _ in range(I)])
    points = np.stack([rng.uniform(-2, 2, P), rng.uniform(-1.5, 1.5, P), rng.uniform(5, 12, P)], axis=1)
    return dict(cam_model=np.array(models, np.int32),
                cam_params_list=[sr.camera_params(m, 1.0 + 2e-3 * k) for k, m in enumerate(models)], poses=poses,
                image_camera=(np.arange(I) % len(models)).astype(np.int32), points=points)


def _lidar(rng, s, lidar_point):
    lp = np.asarray(lidar_point, np.int32)
    nrm = rng.normal(size=(len(lp), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    near = s["points"][lp] + rng.normal(0, 0.05, (len(lp), 3))
    s.update(lidar_point=lp, lidar_abcd=np.concatenate([nrm, -np.sum(nrm * near, 1, keepdims=True)], axis=1),
             lidar_weight=np.where(rng.random(len(lp)) < 0.35, 1000.0, 100.0))


def image_scene(oracle, cams, order, k):
    """11 images with COUNTS[k] observations of 129 points (three 64-track slices, the last workgroup's second slice
    absent); image CONST_IMAGE constant, constant tvec components on four images, every 7th point constant, a LiDAR
    term on two points in three"""
    rng = np.random.default_rng(4100 + 10 * k + len(cams))
    counts = COUNTS[k]
    I, P = len(counts), 129
    s = _base(rng, I, P, CAMERAS[cams])
    obs_image = np.repeat(np.arange(I), counts).astype(np.int32)
    obs_point = rng.integers(0, P, len(obs_image)).astype(np.int32)
    obs_point[-1] = P - 1
    if order == "point":
        perm = np.argsort(obs_point, kind="stable")
    elif order == "shuffled":
        perm = rng.permutation(len(obs_image))
    else:
        perm = np.arange(len(obs_image))
    s.update(obs_image=obs_image[perm], obs_point=obs_point[perm])
    cpose = np.zeros(I, np.uint8); cpose[CONST_IMAGE] = 1
    tv = np.zeros(I, np.uint8); tv[[2, 4, 8, 10]] = [0b001, 0b110, 0b010, 0b101]
    pc = (np.arange(P) % 7 == 3).astype(np.uint8)
    s.update(image_const_pose=cpose, image_const_tvec=tv, point_const=pc)
    _lidar(rng, s, np.flatnonzero(np.arange(P) % 3 != 1))
    assert counts[CONST_IMAGE] > 0 and counts[CONST_IMAGE - 1] > 0 and counts[CONST_IMAGE + 1] > 0 and counts[-1] > 0
    return sr.reproject(oracle, s, rng)


def track_scene(oracle, P, cams="shared", lidar=True, obs=True):
    """P tracks of mixed lengths 1..9 over 10 images (one slice then holds padding slots and, behind a track of length
    1, a half without a row); 0, 1, 2 and 3 LiDAR terms per point in turn, the terms of a point far apart in the term
    list; point P // 2 has LiDAR terms and no observation; the last point carries a term; image 3 constant, every 5th
    point constant"""
    rng = np.random.default_rng(5200 + P)
    I = 10
    s = _base(rng, I, P, CAMERAS[cams])
    length = rng.permutation(np.arange(P) % 9 + 1) if obs else np.zeros(P, np.int64)
    nterm = np.arange(P) % 4
    nterm[P - 1] = max(nterm[P - 1], 1)
    if P >= 3:
        length[P // 2], nterm[P // 2] = 0, 2
    obs_point = np.repeat(np.arange(P), length).astype(np.int32)
    j = np.arange(len(obs_point)) - np.repeat(np.cumsum(length) - length, length)
    s.update(obs_image=((obs_point + j) % I).astype(np.int32), obs_point=obs_point)
    cpose = np.zeros(I, np.uint8); cpose[3] = 1
    s.update(image_const_pose=cpose, point_const=(np.arange(P) % 5 == 2).astype(np.uint8))
    if lidar:
        _lidar(rng, s, rng.permutation(np.repeat(np.arange(P), nterm)))
    s["obs_xy"] = np.zeros((0, 2))
    return sr.reproject(oracle, s, rng) if len(obs_point) else s


def check(oracle, gpu, kw, ba=None):
    """the normal equations with W and the residual-only cost against the oracle; a second call bitwise equal"""
    cost, Himg, gimg, Hpt, gpt, W = oracle.BA(**kw).normal_equations(want_w=True)
    own = ba is None
    if own:
        ba = gpu.BA(**kw)
    got = ba.evaluate(WANT)
    assert abs(got["cost"][0] - cost) <= er.REL * abs(cost)
    er.block_close(got["H_img"], Himg, "H_img")
    er.col_close(got["g_img"], gimg, "g_img")
    er.block_close(got["H_pt"], Hpt, "H_pt")
    er.col_close(got["g_pt"], gpt, "g_pt")
    er.block_close(got["W"], W, "W")
    c1 = ba.evaluate(("cost",))["cost"][0]                       # the cost-only pass
    assert abs(c1 - cost) <= er.REL * abs(cost) and c1 == ba.evaluate(("cost",))["cost"][0]
    again = ba.evaluate(WANT)
    for k in WANT:
        assert np.array_equal(again[k], got[k]), k
    if own:
        ba.close()
    return got, (Himg, Hpt, W)


@pytest.mark.parametrize("order", ["image", "point", "shuffled"])
@pytest.mark.parametrize("cams", list(CAMERAS))
def test_image_segments(gpu, oracle, cams, order):
    k = (list(CAMERAS).index(cams) + ["image", "point", "shuffled"].index(order)) % 3
    kw = image_scene(oracle, cams, order, k)
    got, (Himg, Hpt, W) = check(oracle, gpu, kw)
    counts = np.array(COUNTS[k])
    assert not got["H_img"][counts == 0].any() and not got["g_img"][counts == 0].any()
    assert not got["H_img"][CONST_IMAGE].any() and np.abs(Himg[CONST_IMAGE - 1]).max() > 0
    assert not got["W"][kw["obs_image"] == CONST_IMAGE].any()
    assert not got["W"][kw["point_const"][kw["obs_point"]] == 1].any()
    assert not got["H_pt"][kw["point_const"] == 1].any()
    # the observation the clamped prefetch lands on -- the last one of the last image -- is a live one
    last = np.flatnonzero(kw["obs_image"] == len(counts) - 1)[-1]
    assert kw["point_const"][kw["obs_point"][last]] == 1 or np.abs(W[last]).max() > 0


@pytest.mark.parametrize("cams", ["shared", "one_model", "mixed"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_tracks(gpu, oracle, P, cams):
    kw = track_scene(oracle, P, cams)
    got, (Himg, Hpt, W) = check(oracle, gpu, kw)
    nterm = np.bincount(kw["lidar_point"], minlength=P)
    assert nterm[P - 1] >= 1 and (P < 8 or set(nterm) == {0, 1, 2, 3})
    if P >= 3:
        q = P // 2                                               # LiDAR terms and no observation
        assert not (kw["obs_point"] == q).any() and nterm[q] == 2
        assert kw["point_const"][q] == 1 or np.abs(got["H_pt"][q]).max() > 0


@pytest.mark.parametrize("which", ["no_lidar", "no_obs"])
def test_handles_without_terms(gpu, oracle, which):
    for P in (65, 129):
        check(oracle, gpu, track_scene(oracle, P, lidar=which != "no_lidar", obs=which != "no_obs"))


@pytest.mark.parametrize("cams", ["shared", "mixed"])
def test_updated_parameters_are_read(gpu, oracle, cams):
    """set_parameters and set_camera_parameters between launches: pose, points and camera are read at every launch"""
    kw = image_scene(oracle, cams, "image", 0)
    ba = gpu.BA(**kw)
    first, _ = check(oracle, gpu, kw, ba)
    rng = np.random.default_rng(9)
    kw2 = dict(kw)
    kw2["poses"] = kw["poses"] + rng.normal(0, 2e-3, kw["poses"].shape)
    kw2["points"] = kw["points"] + rng.normal(0, 1e-2, kw["points"].shape)
    ba.set_parameters(kw2["poses"], kw2["points"])
    moved, _ = check(oracle, gpu, kw2, ba)
    assert not np.array_equal(moved["H_img"], first["H_img"]) and not np.array_equal(moved["H_pt"], first["H_pt"])
    kw3 = dict(kw2)
    kw3["cam_params_list"] = [c * np.where(np.arange(len(c)) < 2, 1.003, 0.9) for c in kw["cam_params_list"]]
    ba.set_camera_parameters(kw3["cam_params_list"])
    cam, _ = check(oracle, gpu, kw3, ba)
    assert not np.array_equal(cam["H_img"], moved["H_img"]) and not np.array_equal(cam["W"], moved["W"])
    ba.close()

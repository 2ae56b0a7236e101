"""The image blocks of the normal equations summed on the fp64 matrix pipe (csrc/ba.hip k_ba_images):
H_img, g_img and the fused W against the Jet oracle on hand-built scenes whose per-image observation counts sit on
every edge of the kernel's tiling -- the wavefront tail (63 / 64 / 65), the workgroup iteration of 256 and the segment
of kImgSeg = 1024 observations, up to an image split over three segments.

Tolerances are the existing test's (tests/test_ba_gpu.py test_normal_equations_and_cost): 1e-9 relative with an
absolute floor of 1e-9 x max |reference| on the blocks, 1e-11 relative on the cost, 1e-13 between the fused and the raw W.
"""
import numpy as np
import pytest

from pcdhip import synth

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 63, 64, 65, 127, 255, 256, 257, 1023, 1024, 1025, 2049]
P = 2049                                   # every image observes the first n_i of these points
LOSSES = [(0, 1.0), (1, 1.0), (2, 2.5)]    # the three of test_normal_equations_and_cost
SIMPLE_RADIAL = [3039.0, 2016.0, 1512.0, -0.05]


def _close(a, b, rtol, what):
    scale = float(np.abs(b).max()) if b.size else 0.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, err_msg=what)


def _scene(order="point", two_models=False, seed=5):
    """len(COUNTS) images side by side looking along +z at one cloud in front of all of them; image i observes points
    0 .. COUNTS[i]-1 at their exact OPENCV projection + U(-2, 2) px; the poses are then perturbed (what BA starts from).
    order = "point": the caller's observations are grouped by point; "image": image-major (contiguous W path)."""
    rng = np.random.default_rng(seed)
    I = len(COUNTS)
    depth = rng.uniform(6, 30, P)
    pts = np.stack([rng.uniform(-0.3, 0.3, P) * depth, rng.uniform(-0.25, 0.25, P) * depth, depth], axis=1)
    ang = rng.normal(0, 0.02, (I, 3))
    q = np.concatenate([np.ones((I, 1)), 0.5 * ang], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([np.linspace(-0.6, 0.6, I), rng.normal(0, 0.05, I), rng.normal(0, 0.05, I)], axis=1)
    obs_image = np.concatenate([np.full(n, i, np.int32) for i, n in enumerate(COUNTS)])
    obs_point = np.concatenate([np.arange(n, dtype=np.int32) for n in COUNTS])
    Pc = synth._quat_rotate(q[obs_image], pts[obs_point]) + t[obs_image]
    assert Pc[:, 2].min() > 4.0
    x, y = synth._opencv_project(synth.OPENCV_PARAMS, Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2])
    obs_xy = np.stack([x, y], axis=1) + rng.uniform(-2, 2, (len(x), 2))
    if order == "point":
        perm = np.argsort(obs_point, kind="stable")
        obs_image, obs_point, obs_xy = obs_image[perm], obs_point[perm], obs_xy[perm]
    poses = np.concatenate([q, t], axis=1)
    dq = np.concatenate([np.ones((I, 1)), 0.5 * rng.normal(0, np.deg2rad(0.3), (I, 3))], axis=1)
    poses[:, :4] = _qmul(dq, poses[:, :4])
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    poses[:, 4:] += rng.normal(0, 0.02, (I, 3))
    s = dict(cam_model=np.array([4], np.int32), cam_params_list=[synth.OPENCV_PARAMS], poses=poses,
             image_camera=np.zeros(I, np.int32), points=pts, obs_image=obs_image, obs_point=obs_point, obs_xy=obs_xy)
    if two_models:     # odd images through a SIMPLE_RADIAL camera: the problem no longer has one compiled-in model
        s["cam_model"] = np.array([4, 2], np.int32)
        s["cam_params_list"] = [synth.OPENCV_PARAMS, SIMPLE_RADIAL]
        s["image_camera"] = (np.arange(I) % 2).astype(np.int32)
    return s


def _qmul(a, b):
    w1, v1, w2, v2 = a[:, :1], a[:, 1:], b[:, :1], b[:, 1:]
    return np.concatenate([w1 * w2 - np.sum(v1 * v2, 1, keepdims=True), w1 * v2 + w2 * v1 + np.cross(v1, v2)], axis=1)


def _masks():
    """constant pose on the images with 65 and 1025 observations, the two tvec masks of the issue on the images with
    257 and 2049, every 13th point constant"""
    I = len(COUNTS)
    cp = np.zeros(I, np.uint8); cp[COUNTS.index(65)] = 1; cp[COUNTS.index(1025)] = 1
    tv = np.zeros(I, np.uint8); tv[COUNTS.index(257)] = 0b001; tv[COUNTS.index(2049)] = 0b110
    pc = np.zeros(P, np.uint8); pc[::13] = 1
    return dict(image_const_pose=cp, image_const_tvec=tv, point_const=pc)


_ref_cache = {}


def _reference(oracle, order, two_models, loss):
    """oracle blocks of one scene, computed once and shared (read-only) by the tests that compare against them"""
    key = (order, two_models, loss)
    if key not in _ref_cache:
        s = _scene(order, two_models)
        kw = dict(_masks(), loss_type=loss[0], loss_scale=loss[1])
        cost, Himg, gimg, _, _, W = oracle.BA(**s, **kw).normal_equations(want_w=True)
        for a in (Himg, gimg, W):
            a.setflags(write=False)
        _ref_cache[key] = (s, kw, cost, Himg, gimg, W)
    return _ref_cache[key]


def _check_structure(s, kw, H, g, W):
    """what must be exactly zero: blocks and W rows of constant-pose images, rows / columns of masked tvec
    components, W of constant points"""
    cp, tv, pc = kw["image_const_pose"].astype(bool), kw["image_const_tvec"], kw["point_const"].astype(bool)
    assert cp.any() and not H[cp].any() and not g[cp].any()
    if W is not None:
        assert not W[cp[s["obs_image"]]].any()
        assert pc[s["obs_point"]].any() and not W[pc[s["obs_point"]]].any()
    for i in np.flatnonzero(tv):
        if cp[i] or COUNTS[i] == 0:
            continue
        for k in range(3):
            if (int(tv[i]) >> k) & 1:
                assert not H[i, 3 + k, :].any() and not H[i, :, 3 + k].any() and g[i, 3 + k] == 0.0
                if W is not None:
                    assert not W[s["obs_image"] == i][:, 3 + k, :].any()
            else:
                assert H[i, 3 + k, 3 + k] > 0.0
    assert not H[COUNTS.index(0)].any() and not g[COUNTS.index(0)].any()      # an image without observations


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("order", ["point", "image"])
def test_image_blocks_and_w_on_tiling_edges(gpu, oracle, order, loss):
    s, kw, cost, Himg, gimg, W = _reference(oracle, order, False, loss)
    ba = gpu.BA(**s, **kw)
    got = ba.evaluate(("cost", "H_img", "g_img", "W"))
    print("cost rel err %.3e  H_img max err %.3e / scale %.3e  g_img %.3e / %.3e  W %.3e / %.3e" % (
        abs(got["cost"][0] - cost) / abs(cost), np.abs(got["H_img"] - Himg).max(), np.abs(Himg).max(),
        np.abs(got["g_img"] - gimg).max(), np.abs(gimg).max(), np.abs(got["W"] - W).max(), np.abs(W).max()))
    assert abs(got["cost"][0] - cost) <= 1e-11 * abs(cost)
    _close(got["H_img"], Himg, 1e-9, "H_img")
    _close(got["g_img"], gimg, 1e-9, "g_img")
    _close(got["W"], W, 1e-9, "W")
    assert np.array_equal(got["H_img"], np.transpose(got["H_img"], (0, 2, 1)))
    _check_structure(s, kw, got["H_img"], got["g_img"], got["W"])
    # W alone comes from the raw kernel instead of riding on the image pass: same blocks
    _close(ba.evaluate(("W",))["W"], got["W"], 1e-13, "W raw vs fused")
    # bitwise reproducible: fixed-order sums, no atomics
    again = ba.evaluate(("H_img", "g_img", "W"))
    assert np.array_equal(again["H_img"], got["H_img"]) and np.array_equal(again["g_img"], got["g_img"])
    # without W: the WANT_W = false instantiation
    now = ba.evaluate(("H_img", "g_img"))
    _close(now["H_img"], Himg, 1e-9, "H_img without W")
    _close(now["g_img"], gimg, 1e-9, "g_img without W")
    _check_structure(s, kw, now["H_img"], now["g_img"], None)
    again = ba.evaluate(("H_img", "g_img"))
    assert np.array_equal(again["H_img"], now["H_img"]) and np.array_equal(again["g_img"], now["g_img"])
    ba.close()


@pytest.mark.parametrize("order", ["point", "image"])
def test_two_camera_models_in_one_problem(gpu, oracle, order):
    """OPENCV and SIMPLE_RADIAL cameras together: the generic (per-observation switch) instantiation"""
    s, kw, cost, Himg, gimg, W = _reference(oracle, order, True, LOSSES[1])
    ba = gpu.BA(**s, **kw)
    got = ba.evaluate(("cost", "H_img", "g_img", "W"))
    assert abs(got["cost"][0] - cost) <= 1e-11 * abs(cost)
    _close(got["H_img"], Himg, 1e-9, "H_img")
    _close(got["g_img"], gimg, 1e-9, "g_img")
    _close(got["W"], W, 1e-9, "W")
    _check_structure(s, kw, got["H_img"], got["g_img"], got["W"])
    _close(ba.evaluate(("W",))["W"], got["W"], 1e-13, "W raw vs fused")
    again = ba.evaluate(("H_img", "g_img", "W"))
    assert np.array_equal(again["H_img"], got["H_img"]) and np.array_equal(again["g_img"], got["g_img"])
    now = ba.evaluate(("H_img", "g_img"))
    _close(now["H_img"], Himg, 1e-9, "H_img without W")
    _close(now["g_img"], gimg, 1e-9, "g_img without W")
    ba.close()

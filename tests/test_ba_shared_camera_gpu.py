"""The shared-camera path of the BA kernels (csrc/ba.hip: BaCam<MODEL, SHARED>, the image-uniform pose read of k_ba_cost,
k_sum_partials) against the per-image path, bit for bit.

When every image of a handle maps to one camera, k_ba_points, k_ba_cost, k_ba_raw, k_ba_raw_compact and k_ba_obs_errors
read the camera once through wave-uniform addresses; otherwise they gather it per observation.  Both feed the same
arithmetic, so the same problem stated with one camera and with two cameras of identical parameters (images alternating
between them) must give identical bits in every output.  The scene is the smallest that has three sliced-ELL slices with
a ragged last one, cost-pass wavefronts that straddle two images, and LiDAR terms.
"""
import numpy as np
import pytest

from pcdhip import synth

pytestmark = pytest.mark.gpu

F = 1200.0
CAMS = {0: [F, 2016.0, 1512.0],                                                   # SIMPLE_PINHOLE
        4: list(synth.OPENCV_PARAMS),                                             # OPENCV
        5: [F, 1.1 * F, 2016.0, 1512.0, 0.01, -0.02, 0.003, 0.001]}               # OPENCV_FISHEYE


def _outputs(ba):
    """every output the two paths must agree on"""
    out = dict(ba.evaluate(("cost", "H_img", "g_img", "H_pt", "g_pt", "W")))                 # k_ba_points, k_ba_images
    out["cost_only"] = ba.evaluate(("cost",))["cost"]                                          # k_ba_cost
    out.update(ba.evaluate(("residuals", "jac_q", "jac_t", "jac_X")))                          # k_ba_raw
    out["W_raw"] = ba.evaluate(("W",))["W"]
    out["records"] = ba.evaluate_blocks_compact()["records"]                                   # k_ba_raw_compact
    bl = ba.evaluate_blocks()
    for k in ("residuals", "jac_q", "jac_t", "jac_X"):
        out["blocks_" + k] = bl[k]
    out["sq_err"], out["depth"] = ba.observation_errors()                                      # k_ba_obs_errors
    return out


def _evaluate(gpu, s):
    ba = gpu.BA(**s)
    try:
        return _outputs(ba)
    finally:
        ba.close()


def _assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.size, k
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), k


def _one_camera(s, model):
    return dict(s, cam_model=np.array([model], np.int32), cam_params_list=[CAMS[model]])


def _two_cameras(s, model):
    """the same problem on the per-image path: two cameras of identical parameters, images alternate between them"""
    n = len(s["poses"])
    return dict(s, cam_model=np.array([model, model], np.int32), cam_params_list=[CAMS[model], CAMS[model]],
                image_camera=(np.arange(n) % 2).astype(np.int32))


@pytest.fixture(scope="module")
def scenes():
    img = synth.ba_scene(num_cams=5, num_points=130, order="image")
    assert len(img["points"]) > 128 and len(img["lidar_point"]) > 0          # three slices, the last one ragged
    per_image = np.bincount(img["obs_image"], minlength=5)
    assert (np.cumsum(per_image)[:-1] % 64 != 0).all()                       # wavefronts of the cost pass straddle images
    return dict(image=img, point=synth.ba_scene(num_cams=5, num_points=130, order="point"),
                single=synth.ba_scene(num_cams=1, num_points=130, order="image"))


@pytest.mark.parametrize("order", ["image", "point", "single"])
@pytest.mark.parametrize("model", [0, 4, 5])
def test_shared_camera_equals_per_image_path(gpu, scenes, model, order):
    s = scenes[order]
    if order == "single":
        assert len(s["poses"]) == 1 and len(s["obs_image"]) > 64
        # one image cannot alternate between two cameras: a second, unused camera and a second image without
        # observations put the handle on the per-image path
        two = dict(s, cam_model=np.array([model, model], np.int32), cam_params_list=[CAMS[model], CAMS[model]],
                   poses=np.concatenate([s["poses"], s["poses"]]), image_camera=np.array([0, 1], np.int32),
                   image_const_pose=np.concatenate([s["image_const_pose"], s["image_const_pose"]]))
        a, b = _evaluate(gpu, _one_camera(s, model)), _evaluate(gpu, two)
        for k in ("H_img", "g_img"):          # the extra image has no observations: its blocks are zero
            assert not b[k][1:].any()
            b[k] = b[k][:1]
        _assert_same_bits(a, b)
        return
    _assert_same_bits(_evaluate(gpu, _one_camera(s, model)), _evaluate(gpu, _two_cameras(s, model)))


@pytest.mark.parametrize("order", ["image", "point"])
def test_shared_camera_with_mixed_models(gpu, scenes, order):
    """cameras of different models compile no model in (MODEL = -1): every image on the OPENCV camera (shared) against
    images alternating between two OPENCV cameras (per image); the SIMPLE_PINHOLE camera is there and unused"""
    s = scenes[order]
    n = len(s["poses"])
    shared = dict(s, cam_model=np.array([4, 0], np.int32), cam_params_list=[CAMS[4], CAMS[0]],
                  image_camera=np.zeros(n, np.int32))
    generic = dict(s, cam_model=np.array([4, 4, 0], np.int32), cam_params_list=[CAMS[4], CAMS[4], CAMS[0]],
                   image_camera=(np.arange(n) % 2).astype(np.int32))
    _assert_same_bits(_evaluate(gpu, shared), _evaluate(gpu, generic))


@pytest.mark.parametrize("model", [0, 4, 5])
def test_camera_parameter_updates_are_seen(gpu, scenes, model):
    s = _one_camera(scenes["image"], model)
    perturbed = [p * (1.0 + 1e-3 * (k + 1)) for k, p in enumerate(CAMS[model])]
    ba = gpu.BA(**s)
    try:
        before = _outputs(ba)
        ba.set_camera_parameters([perturbed])
        after = _outputs(ba)
    finally:
        ba.close()
    fresh = _evaluate(gpu, dict(s, cam_params_list=[perturbed]))
    _assert_same_bits(after, fresh)
    assert not np.array_equal(before["residuals"], after["residuals"])


@pytest.mark.parametrize("model", [0, 4, 5])
def test_several_cameras_all_images_on_one(gpu, scenes, model):
    s = scenes["image"]
    n = len(s["poses"])
    others = [[p * 1.25 for p in CAMS[model]], [p * 0.75 for p in CAMS[model]]]
    three = dict(s, cam_model=np.array([model] * 3, np.int32), cam_params_list=others + [CAMS[model]],
                 image_camera=np.full(n, 2, np.int32))
    _assert_same_bits(_evaluate(gpu, three), _evaluate(gpu, _one_camera(s, model)))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 4097, 22000])
def test_sum_of_n_cost_partials(gpu, n):
    """k_sum_partials on n partials that are whole numbers, so every order of the additions gives the same double:
    LiDAR terms only, point at the origin, plane z + d = 0 with weight 1 -> each term adds d^2 / 2, d even; the cost pass
    makes one partial per 256 terms"""
    L = 256 * (n - 1) + 1
    d = 2.0 * (np.arange(L) % 7 + 1)
    abcd = np.zeros((L, 4)); abcd[:, 2] = 1.0; abcd[:, 3] = d
    ba = gpu.BA([0], [CAMS[0]], [[1, 0, 0, 0, 0, 0, 0]], [0], [[0.0, 0.0, 0.0]], [], [], np.zeros((0, 2)),
                lidar_point=np.zeros(L, np.int32), lidar_abcd=abcd, lidar_weight=np.ones(L))
    try:
        cost = ba.evaluate(("cost",))["cost"][0]
        again = ba.evaluate(("cost",))["cost"][0]
    finally:
        ba.close()
    expect = int((d.astype(np.int64) ** 2 // 2).sum())
    assert expect < 2 ** 53
    assert cost == float(expect)
    assert again == cost

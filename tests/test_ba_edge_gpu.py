"""Every BA kernel that evaluates a camera model, at the models' branch points, against the Jet oracle.

Scenes: tests/ba_edge_ref.py's catalogue, one camera model per scene (all 11, several cameras of different parameters
each) and the mixed scene (FOV small-omega, FOV large-omega, OPENCV_FISHEYE, THIN_PRISM_FISHEYE, OPENCV in one handle:
the per-observation switch runs over different branches inside one wavefront), the latter also padded with a
synth.ba_scene so that the edge observations sit at varied lane positions and two images hold more than 1024
observations.  About a third of the images carry off-unit quaternions.

Bound: the project's 1e-9 relative (tests/test_ba_gpu.py), applied per column (ba_edge_ref.col_close /
block_close): a wrong-signed d/d(omega) of magnitude 1e-6 cannot hide behind a focal-length column of magnitude 650.
tests/test_ba_edge_cpu.py measures the oracle against 50-digit arithmetic at every catalogue entry: the worst figure is
1.8e-14 of a column scale (FOV general branch, d/d(omega)), the cancellation region r ~ eps of the fisheye models
stays at 3.5e-16, so four times that adds nothing visible to 1e-9 and no column carries an allowance.

Kernels: k_ba_raw, k_ba_cam_jac, k_ba_lidar_raw (raw blocks); k_ba_points<., true>, k_ba_images<., WANT_W>, k_ba_cost
(normal equations, cost-only pass); k_ba_cameras, k_ba_cam_w (camera blocks); k_ba_obs_errors, k_ba_filter_tracks
(filters) -- compiled-in models 0-4 in the single-model scenes, the generic switch for 5-10 and the mixed scene."""
import numpy as np
import pytest

from tests import ba_edge_ref as er

pytestmark = pytest.mark.gpu
SCENES = er.SCENES
RAW = ("residuals", "jac_q", "jac_t", "jac_X", "jac_lidar", "jac_cam")
DBL_MAX = np.finfo(np.float64).max


@pytest.mark.parametrize("name", SCENES)
def test_raw_blocks(gpu, oracle, name):
    kw = er.scene(oracle, name)
    ba = gpu.BA(**kw)
    got = ba.evaluate(RAW)
    er.check_raw(oracle, kw, got)
    # the camera block's zero pattern at the catalogue observations: d/dk of theta_d is about f u r^2 just above
    # r = eps (1e-44 .. 1e-20, nothing a column-scaled bound can see) and exactly zero at r <= eps, so the pattern
    # tells which side of the threshold the device took
    Jc = er.pad12(oracle.BA(**kw).evaluate_raw()[4])
    for o, e in er.named_scene(oracle, name)["_edge"]:
        assert np.array_equal(got["jac_cam"][o] == 0, Jc[o] == 0), (e, got["jac_cam"][o], Jc[o])
    again = ba.evaluate(RAW)
    for k in RAW:
        assert np.array_equal(again[k], got[k]), k
    ba.close()


@pytest.mark.parametrize("loss", [(0, 1.0), (1, 1.0), (2, 2.5)], ids=["trivial", "soft_l1", "cauchy"])
@pytest.mark.parametrize("name", SCENES)
def test_normal_equations(gpu, oracle, name, loss):
    kw = er.scene(oracle, name, loss_type=loss[0], loss_scale=loss[1])
    cost, Himg, gimg, Hpt, gpt, W = oracle.BA(**kw).normal_equations(want_w=True)
    ba = gpu.BA(**kw)
    want = ("cost", "H_img", "g_img", "H_pt", "g_pt", "W")
    got = ba.evaluate(want)
    assert abs(got["cost"][0] - cost) <= er.REL * abs(cost)
    er.block_close(got["H_img"], Himg, "H_img")
    er.col_close(got["g_img"], gimg, "g_img")
    er.block_close(got["H_pt"], Hpt, "H_pt")
    er.col_close(got["g_pt"], gpt, "g_pt")
    er.block_close(got["W"], W, "W fused")
    er.block_close(ba.evaluate(("W",))["W"], W, "W raw")
    c1 = ba.evaluate(("cost",))["cost"][0]                       # the cost-only pass
    assert abs(c1 - cost) <= er.REL * abs(cost) and c1 == ba.evaluate(("cost",))["cost"][0]
    again = ba.evaluate(want)
    for k in want:
        assert np.array_equal(again[k], got[k]), k
    cp, pc = kw["image_const_pose"].astype(bool), kw["point_const"].astype(bool)
    assert cp.any() and pc.any() and not got["H_img"][cp].any() and not got["H_pt"][pc].any()
    ba.close()


@pytest.mark.parametrize("name", SCENES)
def test_camera_blocks(gpu, oracle, name):
    kw = er.scene(oracle, name, loss_type=1, loss_scale=2.0)
    ob = oracle.BA(**kw)
    want = ("H_cam", "g_cam", "E_cam", "W_cam")
    for flags in [(True, False, True), (False, False, True), (True, True, True), (True, False, False)]:
        mask = gpu.camera_refine_mask(kw["cam_model"], *flags, constant_cameras=(1,))
        H, g, E, Wc = ob.camera_blocks(mask, want_w=True)
        ba = gpu.BA(**kw, camera_refine=mask)
        got = ba.evaluate(want)
        er.block_close(got["H_cam"], H, "H_cam %r" % (flags,))
        er.col_close(got["g_cam"], g, "g_cam %r" % (flags,))
        er.block_close(got["E_cam"], E, "E_cam %r" % (flags,))
        er.block_close(got["W_cam"], Wc, "W_cam %r" % (flags,))
        assert not got["H_cam"][1].any() and (np.abs(H).max() > 0 or not mask.any())
        again = ba.evaluate(want)
        for k in want:
            assert np.array_equal(again[k], got[k]), k
        ba.close()


@pytest.mark.parametrize("name", SCENES)
def test_filters(gpu, oracle, name):
    """tolerances of tests/test_filters_gpu.py"""
    kw = er.scene(oracle, name)
    ob = oracle.BA(**kw)
    esq, edepth = ob.observation_errors()
    ba = gpu.BA(**kw)
    gsq, gdepth = ba.observation_errors()
    behind = edepth < np.finfo(np.float64).eps
    assert np.array_equal(gsq == DBL_MAX, behind)
    np.testing.assert_allclose(gdepth, edepth, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gsq[~behind], esq[~behind], rtol=1e-9, atol=1e-9)
    assert np.array_equal(gsq > 4.0 ** 2, esq > 4.0 ** 2)
    g2, d2 = ba.observation_errors()
    assert np.array_equal(g2, gsq) and np.array_equal(d2, gdepth)
    fin = np.sqrt(esq[esq < 1e300])
    P = kw["points"].shape[0]
    for max_err in (float(np.quantile(fin, 0.7)), float(np.quantile(fin, 0.3)), 4.0):
        exp = oracle.filter_tracks(esq, edepth, kw["obs_point"], P, max_err)
        got = ba.filter_tracks(max_err)
        for k in ("obs_erase", "obs_negative_depth", "point_delete"):
            assert np.array_equal(got[k], exp[k]), (max_err, k)
        for k in ("num_filtered", "num_points_with_error", "num_negative_depth"):
            assert got[k] == exp[k], (max_err, k, got[k], exp[k])
        np.testing.assert_allclose(got["point_error"], exp["point_error"], rtol=1e-12, atol=1e-12)
        assert abs(got["mean_reproj_error"] - exp["mean_reproj_error"]) <= 1e-12 * max(1.0, exp["mean_reproj_error"])
    ba.close()


def test_fov_omega_column_sign_named_case(gpu, oracle):
    """the same ray on either side of omega^2 = 1e-4: the camera column d(x)/d(omega) changes sign with the branch
    (tests/test_ba_edge_cpu.py pins the oracle's values against mpmath); omega = 1e-3 sits between 1e-4 and 1e-2, where
    a test of omega instead of omega^2 goes wrong."""
    for om, sign in ((0.0099, -1.0), (0.0101, 1.0), (1e-3, -1.0)):
        cam = er.cam_params(7, extra=[om])
        kw = dict(cam_model=[7], cam_params_list=[cam], poses=[[1, 0, 0, 0, 0, 0, 1.0]], image_camera=[0],
                  points=[[0.0404, 0.0, 3.0]], obs_image=[0], obs_point=[0], obs_xy=[[390.0, 511.0]])
        Jc = oracle.BA(**kw).evaluate_raw()[4]
        ba = gpu.BA(**kw)
        got = ba.evaluate(("jac_cam",))["jac_cam"]
        ba.close()
        assert np.sign(Jc[0, 0, 4]) == sign and np.sign(got[0, 0, 4]) == sign, (om, Jc[0, 0, 4], got[0, 0, 4])
        assert abs(got[0, 0, 4] - Jc[0, 0, 4]) <= er.REL * abs(Jc[0, 0, 4])


@pytest.mark.parametrize("ray", [(0.0099, 0.0), (0.007, -0.007), (0.0101, 0.0), (0.0072, -0.0072)])
def test_fov_radius_threshold_named_case(gpu, oracle, ray):
    """one observation on either side of radius^2 = 1e-4 at omega = 0.9 (camera_models.h:1105-1160).  The
    small-radius formula is the Taylor expansion of the general one, so just below the threshold the two agree closely:
    50-digit evaluation of both gives relative differences of 8e-9 in d(x)/d(u), 1e-4 in d(x)/d(v) at ray
    (0.007, -0.007), 5e-8 in d(x, y)/d(omega) -- invisible at a column scale set by a wide ray, visible at 1e-9 of
    the entry itself.  Pins the threshold of both headers: jac_q / jac_t / jac_X (ba_math.h), jac_cam (ba_cam_jac.h),
    and the camera and pose blocks built from them."""
    cam = er.cam_params(7, extra=[0.9])
    assert er.formula_branch(7, cam, *ray) == ("small_radius" if ray in ((0.0099, 0.0), (0.007, -0.007)) else "general")
    kw = dict(cam_model=[7], cam_params_list=[cam], poses=[[1.25, 0, 0, 0, 0, 0, 1.0]], image_camera=[0],
              points=[[4 * ray[0], 4 * ray[1], 3.0]], obs_image=[0], obs_point=[0], obs_xy=[[390.0, 509.0]],
              camera_refine=np.ones(5, np.uint8))
    ob = oracle.BA(**{k: v for k, v in kw.items() if k != "camera_refine"})
    res, Jq, Jt, JX, Jc, _ = ob.evaluate_raw()
    H, g, E, Wc = ob.camera_blocks(np.ones(5, np.uint8), want_w=True)
    _, Himg, gimg, Hpt, gpt, W = ob.normal_equations(want_w=True)
    ba = gpu.BA(**kw)
    got = ba.evaluate(RAW + ("H_cam", "g_cam", "E_cam", "W_cam", "H_img", "g_img", "H_pt", "g_pt", "W"))
    ba.close()
    for k, r in (("residuals", res), ("jac_q", Jq), ("jac_t", Jt), ("jac_X", JX), ("jac_cam", er.pad12(Jc)), ("H_cam", H),
                 ("g_cam", g), ("E_cam", E), ("W_cam", Wc), ("H_img", Himg), ("g_img", gimg), ("H_pt", Hpt), ("g_pt", gpt),
                 ("W", W)):
        er.entry_close(got[k], r, "%s at ray %r" % (k, ray))
    assert Jc[0, 0, 4] != 0 and (ray[1] == 0 or JX[0, 0, 1] != 0)


def test_non_finite_containment(gpu, oracle):
    """one observation with P.z == 0 exactly: the cost, that image's H_img / g_img block and that point's H_pt / g_pt
    block are non-finite on the device and on the oracle alike; every other block is finite and within the bound.
    Block granularity only: which entries are inf and which NaN is not compared."""
    kw, o_bad, im_bad, pt_bad = er.pz_zero_scene(oracle)
    cost, Himg, gimg, Hpt, gpt, _ = oracle.BA(**kw).normal_equations()
    ba = gpu.BA(**kw)
    got = ba.evaluate(("cost", "H_img", "g_img", "H_pt", "g_pt"))
    ba.close()
    assert not np.isfinite(cost) and not np.isfinite(got["cost"][0])
    for ref, dev, bad in ((Himg, got["H_img"], im_bad), (gimg, got["g_img"], im_bad), (Hpt, got["H_pt"], pt_bad),
                          (gpt, got["g_pt"], pt_bad)):
        assert not np.isfinite(ref[bad]).all() and not np.isfinite(dev[bad]).all()
        keep = np.arange(ref.shape[0]) != bad
        (er.block_close if ref.ndim == 3 else er.col_close)(dev[keep], ref[keep], "blocks next to the singular one")

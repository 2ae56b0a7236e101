"""The Ceres route (pcd_ba_evaluate_blocks: pinned buffers, pose rows packed by k_pack_rows, pose_row /
num_pose_rows) and the refined-intrinsics update (pcd_ba_set_camera_parameters) against the Jet oracle.

Bound: tests/ba_edge_ref.col_close, the project's 1e-9 relative per column (see tests/test_ba_edge_gpu.py)."""
import numpy as np
import pytest

from pcdhip import synth
from tests import ba_edge_ref as er

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
RAW = ("residuals", "jac_q", "jac_t", "jac_X", "jac_lidar", "jac_cam")


def _reorder(s, order, seed=3):
    s = dict(s)
    O = len(s["obs_image"])
    if order == "shuffled":
        perm = np.random.default_rng(seed).permutation(O)
        s["obs_image"], s["obs_point"], s["obs_xy"] = s["obs_image"][perm], s["obs_point"][perm], s["obs_xy"][perm]
    return s


def _check_blocks(gpu, oracle, kw, ba=None):
    """one pcd_ba_evaluate_blocks call against the oracle and against pcd_ba_evaluate's rows"""
    own = ba is None
    ba = ba or gpu.BA(**kw)
    O, L = len(kw["obs_image"]), 0 if kw.get("lidar_point") is None else len(kw["lidar_point"])
    cpose = np.zeros(np.asarray(kw["poses"]).reshape(-1, 7).shape[0], bool) if kw.get("image_const_pose") is None \
        else np.asarray(kw["image_const_pose"]).astype(bool)
    const_obs = cpose[np.asarray(kw["obs_image"], np.int64)] if O else np.zeros(0, bool)
    bl = ba.evaluate_blocks(True, True)
    row = bl["pose_row"]
    V = int((~const_obs).sum())
    assert bl["num_pose_rows"] == V and row.dtype == np.uint32 and row.shape == (O,)
    assert (row[const_obs] == NONE).all()
    assert np.array_equal(row[~const_obs], np.arange(V, dtype=np.uint32))       # ascending packing in observation order
    assert bl["jac_q"].shape == (V, 2, 4) and bl["jac_t"].shape == (V, 2, 3)
    assert bl["bytes_d2h"] == 8 * (2 * O + L + 14 * V + 6 * O + 3 * L + 24 * O)
    # un-packed: constant-pose observations have no pose blocks (zero rows in the oracle's / pcd_ba_evaluate's layout)
    full = dict(bl)
    full["jac_q"] = np.zeros((O, 2, 4)); full["jac_q"][~const_obs] = bl["jac_q"]
    full["jac_t"] = np.zeros((O, 2, 3)); full["jac_t"][~const_obs] = bl["jac_t"]
    if O:
        er.check_raw(oracle, kw, full, "blocks ")
    else:
        res, _, _, _, _, JL = oracle.BA(**kw).evaluate_raw()
        er.col_close(bl["residuals"], res, "lidar residuals")
        er.col_close(bl["jac_lidar"], JL, "jac_lidar")
    ev = ba.evaluate(RAW)
    for k in RAW:
        assert np.array_equal(full[k], ev[k]), k + ": packed rows differ from pcd_ba_evaluate's"
    # residuals only: NULL Jacobian pointers (None), fewer bytes
    r0 = ba.evaluate_blocks(False, False)
    assert all(r0[k] is None for k in RAW[1:]) and np.array_equal(r0["residuals"], bl["residuals"])
    assert r0["bytes_d2h"] == 8 * (2 * O + L) and (r0["bytes_d2h"] < bl["bytes_d2h"] or O + L == 0)
    assert np.array_equal(r0["pose_row"], row) and r0["num_pose_rows"] == V
    nc = ba.evaluate_blocks(True, False)
    assert nc["jac_cam"] is None and np.array_equal(nc["jac_q"], bl["jac_q"]) and np.array_equal(nc["jac_X"], bl["jac_X"])
    assert nc["bytes_d2h"] == bl["bytes_d2h"] - 8 * 24 * O
    if own:
        ba.close()
    return bl


@pytest.mark.parametrize("order", ["point", "image", "shuffled"])
@pytest.mark.parametrize("frac", [0.0, 0.25, 1.0])
def test_blocks_on_synthetic_scenes(gpu, oracle, frac, order):
    s = synth.ba_scene(9, 700, seed=61, const_pose_frac=frac, order="image" if order == "image" else "point")
    s = _reorder(s, order)
    if frac == 0.25:
        assert 0 < s["image_const_pose"].sum() < 9
    bl = _check_blocks(gpu, oracle, s)
    assert (bl["num_pose_rows"] == 0) == (frac == 1.0) and (bl["num_pose_rows"] == len(s["obs_image"])) == (frac == 0.0)


@pytest.mark.parametrize("name", ["mixed", "mixed_padded"])
def test_blocks_on_the_mixed_edge_scene(gpu, oracle, name):
    kw = er.scene(oracle, name)
    bl = _check_blocks(gpu, oracle, kw)
    assert 0 < bl["num_pose_rows"] < len(kw["obs_image"])


def test_blocks_follow_set_parameters(gpu, oracle):
    s = synth.ba_scene(7, 500, seed=62, const_pose_frac=0.25)
    s["image_const_pose"][2] = 1
    ba = gpu.BA(**s)
    first = _check_blocks(gpu, oracle, s, ba)                    # copies: nothing of the first call is read later
    s2 = dict(s)
    s2["poses"] = s["poses"].copy(); s2["poses"][:, 4:] += 0.01; s2["poses"][::2, :4] *= 1.2
    s2["points"] = s["points"] + 0.02
    ba.set_parameters(poses=s2["poses"], points=s2["points"])
    second = _check_blocks(gpu, oracle, s2, ba)
    assert not np.array_equal(first["residuals"], second["residuals"])
    assert np.array_equal(first["pose_row"], second["pose_row"])
    ba.close()


def test_blocks_edge_sizes(gpu, oracle):
    s = synth.ba_scene(4, 60, seed=63)
    # no observations, LiDAR terms only
    a = dict(s)
    a["obs_image"], a["obs_point"], a["obs_xy"] = s["obs_image"][:0], s["obs_point"][:0], s["obs_xy"][:0]
    bl = _check_blocks(gpu, oracle, a)
    assert bl["num_pose_rows"] == 0 and bl["pose_row"].shape == (0,) and bl["jac_lidar"].shape[0] == len(a["lidar_point"]) > 0
    assert bl["jac_q"].shape == (0, 2, 4) and bl["jac_X"].shape == (0, 2, 3)
    # every pose constant
    b = dict(s); b["image_const_pose"] = np.ones(4, np.uint8)
    bl = _check_blocks(gpu, oracle, b)
    assert bl["num_pose_rows"] == 0 and (bl["pose_row"] == NONE).all() and len(bl["pose_row"]) > 0
    # a single observation, variable and constant pose, no LiDAR
    for cp in (0, 1):
        c = dict(cam_model=s["cam_model"], cam_params_list=s["cam_params_list"], poses=s["poses"][s["obs_image"][:1]],
                 image_camera=[0], points=s["points"][s["obs_point"][:1]], obs_image=[0], obs_point=[0],
                 obs_xy=s["obs_xy"][:1], image_const_pose=[cp])
        bl = _check_blocks(gpu, oracle, c)
        assert bl["num_pose_rows"] == 1 - cp and list(bl["pose_row"]) == [NONE if cp else 0]


def _perturbed_cameras(kw):
    """every camera's parameters moved; the FOV camera at omega = 0.9 goes to omega = 1e-6 (general / small-radius
    branches -> small-omega branch) and the one at 1e-6 to 0.5"""
    new = []
    for m, p in zip(kw["cam_model"], kw["cam_params_list"]):
        q = np.array(p, np.float64) * (1.0 + 2e-3)
        if m == 7:
            q[4] = 1e-6 if p[4] == 0.9 else 0.5
        new.append(q)
    return new


@pytest.mark.parametrize("name", ["m7", "m4", "mixed"])
def test_set_camera_parameters(gpu, oracle, name):
    kw = er.scene(oracle, name, loss_type=1, loss_scale=2.0)
    new = _perturbed_cameras(kw)
    assert name == "m4" or any(m == 7 and p[4] == 0.9 and q[4] == 1e-6
                               for m, p, q in zip(kw["cam_model"], kw["cam_params_list"], new))
    kw2 = dict(kw); kw2["cam_params_list"] = new
    mask = gpu.camera_refine_mask(kw["cam_model"], True, True, True, constant_cameras=(1,))
    want = RAW + ("H_cam", "g_cam", "E_cam", "W_cam", "cost")
    ba = gpu.BA(**kw, camera_refine=mask)
    before = ba.evaluate(want)
    ba.set_camera_parameters(new)
    got = ba.evaluate(want)
    fresh_ba = gpu.BA(**kw2, camera_refine=mask)
    fresh = fresh_ba.evaluate(want)
    for k in want:
        assert np.array_equal(got[k], fresh[k]), k + ": updated handle differs from a fresh one"
    assert not np.array_equal(before["residuals"], got["residuals"])
    er.check_raw(oracle, kw2, got, "after the update ")
    H, g, E, Wc = oracle.BA(**kw2).camera_blocks(mask, want_w=True)
    er.block_close(got["H_cam"], H, "H_cam"); er.col_close(got["g_cam"], g, "g_cam")
    er.block_close(got["E_cam"], E, "E_cam"); er.block_close(got["W_cam"], Wc, "W_cam")
    # the Ceres route sees the new intrinsics too
    bl = ba.evaluate_blocks(True, True)
    assert np.array_equal(bl["residuals"], fresh["residuals"]) and np.array_equal(bl["jac_cam"], fresh["jac_cam"])
    # and back: the original parameters give the original numbers
    ba.set_camera_parameters(kw["cam_params_list"])
    back = ba.evaluate(want)
    for k in want:
        assert np.array_equal(back[k], before[k]), k
    ba.close(); fresh_ba.close()
    # a handle created without camera_refine (all intrinsics constant): same effect on the residuals
    plain = gpu.BA(**kw)
    plain.set_camera_parameters(np.concatenate(new))             # packed form
    out = plain.evaluate(("residuals", "jac_cam", "H_cam"))
    assert np.array_equal(out["residuals"], fresh["residuals"]) and np.array_equal(out["jac_cam"], fresh["jac_cam"])
    assert not out["H_cam"].any()
    plain.close()

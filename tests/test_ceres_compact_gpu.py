"""The compact Ceres route on the device (pcd_ba_evaluate_blocks_compact: k_ba_raw_compact, k_ba_pack_cam_jac) against
the full route (pcd_ba_evaluate_blocks) of the same handle.

Records are {r0, r1, M row-major 2x3}, M = dr/dP.  r and M are the very values the full kernel multiplies out, so they are
compared BITWISE: records[:, :2] with the full route's residuals, records[:, 2:] with its jac_t on variable-pose rows
(jac_t = M).  On every row, constant poses included, M D(q) formed in numpy must give the full route's jac_X under
tests/ba_edge_ref.col_close (the project's 1e-9 relative per column; numpy's product order differs from the device's).
Observation counts sit where wave_store_rows and the grid tail can go wrong: 1, 63, 64, 65 and 257 (more than one
256-thread workgroup, a last wavefront of one lane).  Every second quaternion of the synthetic scenes is scaled by 1.2
(the Jacobians are those of the un-normalised polynomial); the mixed scene holds both kinds."""
import os
import subprocess

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_edge_ref as er

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
COUNTS = (1, 63, 64, 65, 257)
_SYNTH = {}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _synth_scene(frac, order):
    """built once per (const-pose fraction, order); callers trim copies"""
    key = (frac, order)
    if key not in _SYNTH:
        s = synth.ba_scene(9, 300, seed=81, const_pose_frac=frac, order="image" if order == "image" else "point")
        if order == "shuffled":
            perm = np.random.default_rng(5).permutation(len(s["obs_image"]))
            s["obs_image"], s["obs_point"], s["obs_xy"] = s["obs_image"][perm], s["obs_point"][perm], s["obs_xy"][perm]
        s["poses"] = s["poses"].copy()
        s["poses"][::2, :4] *= 1.2
        assert len(s["obs_image"]) >= max(COUNTS)
        _SYNTH[key] = s
    return _SYNTH[key]


def _trim(s, O):
    s = dict(s)
    s["obs_image"], s["obs_point"], s["obs_xy"] = s["obs_image"][:O], s["obs_point"][:O], s["obs_xy"][:O]
    return s


def _num_params(kw):
    K = np.array([er.NUM_PARAMS[int(m)] for m in kw["cam_model"]])
    per_obs = K[np.asarray(kw["image_camera"], np.int64)[np.asarray(kw["obs_image"], np.int64)]]
    return int(K.max()), per_obs


def _check(gpu, kw, ba=None):
    """one handle: the compact call against the full one"""
    own = ba is None
    if own:
        ba = gpu.BA(**kw, camera_refine=gpu.camera_refine_mask(kw["cam_model"], True, True, True))
    O, L = len(kw["obs_image"]), 0 if kw.get("lidar_point") is None else len(kw["lidar_point"])
    poses = np.asarray(kw["poses"], np.float64).reshape(-1, 7)
    cpose = np.zeros(poses.shape[0], bool) if kw.get("image_const_pose") is None \
        else np.asarray(kw["image_const_pose"]).astype(bool)
    oi = np.asarray(kw["obs_image"], np.int64)
    const_obs = cpose[oi] if O else np.zeros(0, bool)
    cs, K = _num_params(kw)
    full = ba.evaluate_blocks(True, True)
    c = ba.evaluate_blocks_compact(True, True)
    rec = c["records"]
    assert rec.shape == (O, 8) and c["residuals"] is None and c["cam_stride"] == cs
    assert _bits(rec[:, :2].reshape(-1), full["residuals"][:2 * O]), "r differs from the full route's residuals"
    assert _bits(rec[~const_obs, 2:], full["jac_t"].reshape(-1, 6)), "M differs from the full route's jac_t"
    if O:
        D = np.stack([er.rotation_matrix_poly(q) for q in poses[:, :4]])
        er.col_close(rec[:, 2:].reshape(O, 2, 3) @ D[oi], full["jac_X"], "M D(q) against jac_X")
        assert np.abs(rec[:, 2:]).max(axis=1).min() > 0           # constant-pose rows keep their M
    assert _bits(c["lidar_residuals"], full["residuals"][2 * O:]) and _bits(c["jac_lidar"], full["jac_lidar"])
    assert c["bytes_d2h"] == 8 * (8 * O + 4 * L) + 16 * cs * O
    assert c["jac_cam"].shape == (O, 2, cs)
    cols = np.arange(cs)[None, None, :] < K[:, None, None]
    assert _bits(np.where(cols, c["jac_cam"], 0.0), np.where(cols, full["jac_cam"][:, :, :cs], 0.0)), "jac_cam[..., :K]"
    assert not np.where(cols, 0.0, c["jac_cam"]).any(), "jac_cam padding"
    assert O == 0 or np.abs(c["jac_cam"]).max() > 0
    nc = ba.evaluate_blocks_compact(True, False)
    assert nc["jac_cam"] is None and _bits(nc["records"], rec) and nc["bytes_d2h"] == 8 * (8 * O + 4 * L)
    r0 = ba.evaluate_blocks_compact(False, False)
    assert r0["records"] is None and r0["jac_lidar"] is None and r0["jac_cam"] is None
    assert _bits(r0["residuals"], full["residuals"][:2 * O]) and _bits(r0["lidar_residuals"], full["residuals"][2 * O:])
    assert r0["bytes_d2h"] == 8 * (2 * O + L)
    again = ba.evaluate_blocks(True, True)                         # the two routes share the pinned buffer
    assert all(_bits(again[k], full[k]) for k in ("residuals", "jac_q", "jac_t", "jac_X", "jac_lidar", "jac_cam"))
    if own:
        ba.close()
    return c


@pytest.mark.parametrize("order", ["point", "image", "shuffled"])
@pytest.mark.parametrize("frac", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("O", COUNTS)
def test_compact_on_synthetic_scenes(gpu, O, frac, order):
    s = _trim(_synth_scene(frac, order), O)
    if frac == 0.25:
        assert 0 < _synth_scene(frac, order)["image_const_pose"].sum() < 9
    _check(gpu, s)


@pytest.mark.parametrize("O", (1, 63, 64, 65, None))
def test_compact_on_the_mixed_edge_scene(gpu, oracle, O):
    """five camera models in one handle (the per-observation model switch), cam_stride 12, constant pose and scaled
    quaternions among the images; None = the whole scene"""
    kw = er.scene(oracle, "mixed")
    assert len(kw["obs_image"]) > 65 and kw["image_const_pose"].any()
    c = _check(gpu, kw if O is None else _trim(kw, O))
    assert c["cam_stride"] == 12


@pytest.mark.parametrize("name", ["m0", "m7"])
def test_compact_on_uniform_edge_scenes(gpu, oracle, name):
    """a compiled-in model with the narrowest camera (cam_stride 3, odd) and a uniform model outside the dispatch table"""
    c = _check(gpu, er.scene(oracle, name))
    assert c["cam_stride"] == er.NUM_PARAMS[int(name[1:])]


def test_compact_without_observations(gpu):
    s = _trim(synth.ba_scene(4, 60, seed=63), 0)
    c = _check(gpu, s)
    assert c["records"].shape == (0, 8) and c["jac_lidar"].shape[0] == len(s["lidar_point"]) > 0


def test_compact_follows_parameter_updates(gpu):
    s = _trim(synth.ba_scene(7, 500, seed=62, const_pose_frac=0.25), 257)
    s["image_const_pose"][2] = 1
    ba = gpu.BA(**s)
    first = _check(gpu, s, ba)
    s2 = dict(s)
    s2["poses"] = s["poses"].copy(); s2["poses"][:, 4:] += 0.01; s2["poses"][::2, :4] *= 1.2
    s2["points"] = s["points"] + 0.02
    s2["cam_params_list"] = [np.asarray(p, np.float64) * (1.0 + 2e-3) for p in s["cam_params_list"]]
    ba.set_parameters(poses=s2["poses"], points=s2["points"])
    moved = _check(gpu, s2, ba)
    assert not _bits(first["records"], moved["records"])
    ba.set_camera_parameters(s2["cam_params_list"])
    second = _check(gpu, s2, ba)
    assert not _bits(moved["records"], second["records"]) and not _bits(moved["jac_cam"], second["jac_cam"])
    fresh_ba = gpu.BA(**s2)
    fresh = fresh_ba.evaluate_blocks_compact(True, True)
    for k in ("records", "lidar_residuals", "jac_lidar", "jac_cam"):
        assert _bits(second[k], fresh[k]), k + ": updated handle differs from a fresh one"
    ba.close(); fresh_ba.close()


def test_adapter_modes_are_bit_identical():
    """shim/test_ceres_compact --gpu: HipEvaluation on a ShimParameterSource scene with compact off and on, and
    HipBlockRecorder::Finalize under COLMAP_PCD_HIP_COMPACT: every block's Evaluate output, residuals and all Jacobians,
    constant-pose images and refined cameras included, bit for bit"""
    subprocess.check_call(["make", "-s", "-C", PKG, "shim/test_ceres_compact"])
    r = subprocess.run([os.path.join(PKG, "shim", "test_ceres_compact"), "--gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

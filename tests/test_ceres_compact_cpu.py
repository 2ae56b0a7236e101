"""Host half of the compact Ceres route (colmap-pcd_amd/shim/ceres_compact.h and the compact mode of ceres_adapter.h),
without a GPU: shim/test_ceres_compact rebuilds jac_q / jac_t / jac_X from {r, M = dr/dP} and the evaluation point, and
the result is held against the Jet oracle's blocks.

Cases come from oracle.BA(...).evaluate_raw() with every pose variable, so the oracle's jac_t IS M for every observation
(the constant-pose functor has no jac_t to take it from).  Bound: tests/ba_edge_ref.col_close, the project's 1e-9 relative
per column."""
import os
import subprocess

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_edge_ref as er

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "-C", PKG, "shim/test_ceres_compact"])
    return os.path.join(PKG, "shim", "test_ceres_compact")


def _scenes(oracle):
    mixed = er.scene(oracle, "mixed")
    s = synth.ba_scene(7, 500, seed=71)
    s["poses"] = s["poses"].copy()
    s["poses"][::2, :4] *= 1.2                      # the Jacobian is that of the un-normalised polynomial
    return {"mixed": mixed, "synth_scaled": s}


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """per scene: (file of {q, X, {r, jac_t}} records, the oracle's jac_q, jac_t, jac_X)"""
    d = tmp_path_factory.mktemp("compact")
    out = {}
    for name, kw in _scenes(oracle).items():
        kw = dict(kw)
        I = np.asarray(kw["poses"]).reshape(-1, 7).shape[0]
        kw["image_const_pose"] = np.zeros(I, np.uint8)
        res, Jq, Jt, JX, _, _ = oracle.BA(**kw).evaluate_raw()
        O = len(kw["obs_image"])
        assert O > 50 and Jt.shape == (O, 2, 3) and np.abs(Jt).max() > 0
        q = np.asarray(kw["poses"], np.float64).reshape(-1, 7)[np.asarray(kw["obs_image"], np.int64), :4]
        X = np.asarray(kw["points"], np.float64).reshape(-1, 3)[np.asarray(kw["obs_point"], np.int64)]
        rec = np.concatenate([res[:2 * O].reshape(O, 2), Jt.reshape(O, 6)], axis=1)
        path = str(d / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(np.int64(O).tobytes())
            f.write(np.ascontiguousarray(np.concatenate([q, X, rec], axis=1), np.float64).tobytes())
        out[name] = (path, Jq, Jt, JX)
    return out


@pytest.mark.parametrize("name", ["mixed", "synth_scaled"])
def test_expansion_matches_the_oracle(prog, cases, tmp_path, name):
    path, Jq, Jt, JX = cases[name]
    res = str(tmp_path / "out.bin")
    r = subprocess.run([prog, "expand", path, res], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(res, np.float64).reshape(-1, 20)
    assert got.shape[0] == Jq.shape[0]
    assert np.array_equal(got[:, 8:14].reshape(-1, 2, 3), Jt)          # jac_t = M, copied
    er.col_close(got[:, :8].reshape(-1, 2, 4), Jq, name + " jac_q")
    er.col_close(got[:, 14:].reshape(-1, 2, 3), JX, name + " jac_X")


@pytest.mark.parametrize("name", ["mixed", "synth_scaled"])
def test_adapter_on_hand_filled_buffers(prog, cases, name):
    """HipReprojectionBlock::Evaluate in compact mode: variable-pose and constant-pose (block order 3, K) blocks,
    jacobians == NULL, every single NULL entry, a jac_cam row at cam_stride 5 < 12, a residual-only pass; guard entries
    behind every destination, nothing written through a NULL pointer"""
    r = subprocess.run([prog, "adapter", cases[name][0]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


def test_python_binding_declares_the_entry_point(pcdhip):
    assert "pcd_ba_evaluate_blocks_compact" in pcdhip.ABI_SYMBOLS
    assert hasattr(pcdhip.lib(), "pcd_ba_evaluate_blocks_compact") and hasattr(pcdhip.BA, "evaluate_blocks_compact")

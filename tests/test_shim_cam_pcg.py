"""The linear solver of BundleAdjusterHip::Solve with refined intrinsics (shim/ba_problem.h, BundleAdjustmentOptions::
refined_linear_solver_type), driven through shim/test_ba_solve_cam_pcg.cc.  Without a GPU: the default is DIRECT whatever
linear_solver_type says, and AUTO picks by the number of images in the config (1000 direct, 1001 iterative).  With one:
ITERATIVE makes Solve equal pcd_ba_solve(PCD_LINEAR_PCG_CAM, refine_intrinsics = 1) through the C ABI bit for bit, with the
camera in the Reconstruction updated, and the default equals the Cholesky route bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "colmap-pcd_amd")
EXE = os.path.join(PKG, "shim", "test_ba_solve_cam_pcg")


def _run(*args):
    subprocess.check_call(["make", "-s", "-C", PKG, "shim/test_ba_solve_cam_pcg"])
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    return r


def test_solver_choice_on_the_host():
    r = _run()
    assert r.returncode == 0 and "ALL OK" in r.stdout


@pytest.mark.gpu
def test_solve_equals_the_c_abi(gpu):
    r = _run("--gpu")
    assert r.returncode == 0 and "ALL OK" in r.stdout
    assert "bordered PCG" in r.stdout and "Cholesky (the default)" in r.stdout

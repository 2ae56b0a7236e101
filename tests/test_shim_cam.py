"""BundleAdjusterHip::Solve with refined intrinsics (shim/ba_problem.h, BundleAdjustmentOptions::
refine_intrinsics_on_device), driven through shim/test_ba_solve_cam.cc.  Without a GPU: with the option off a refined
problem is refused as before.  With one: option on, refine_focal_length, Solve equals pcd_ba_solve through the C ABI bit
for bit, the camera in the Reconstruction is updated, and one refined camera per image (nine of them) makes Solve return
false."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "colmap-pcd_amd")
EXE = os.path.join(PKG, "shim", "test_ba_solve_cam")


def _run(*args):
    subprocess.check_call(["make", "-s", "-C", PKG, "shim/test_ba_solve_cam"])
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    return r


def test_option_off_refuses_as_before():
    r = _run()
    assert r.returncode == 0 and "ALL OK" in r.stdout


@pytest.mark.gpu
def test_solve_with_refined_intrinsics(gpu):
    r = _run("--gpu")
    assert r.returncode == 0 and "ALL OK" in r.stdout and "focal length refined" in r.stdout

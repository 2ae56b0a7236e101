"""ISA of the camera-row kernels of the reduced system (csrc/ba_solve_cam.hip), checked without a GPU and
from the kernel metadata only: no scratch (a spill would put per-lane fp64 traffic on the memory path these kernels are
bound by), the VGPR counts of the gfx950 build pinned from above, and LDS.  The two wavefront-per-block kernels hold 36
fp64 accumulators as k_schur_blocks does: k_schur_cam_border with the 2 x 18 doubles of an observation (158 VGPRs, 3
wavefronts per SIMD), k_schur_cam_partials with the 9 + 36 doubles of a point (188 VGPRs, 2 wavefronts per SIMD)."""
import os
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPRS = {                     # counts of the gfx950 build (hipcc -O3); (VGPRs, LDS bytes)
    "k_schur_cam_pointsILb1E": (128, 0),      # one shared camera: no camera test
    "k_schur_cam_pointsILb0E": (104, 0),
    "k_schur_cam_partials": (188, 0),
    "k_schur_cam_reduce": (8, 0),
    "k_schur_cam_border": (158, 0),
    "k_chol_fill_cam": (16, 0),
    "k_schur_cam_dense": (18, 0),
    "k_schur_cam_back": (92, 32),
    "k_schur_cam_model_decrease": (18, 0),
    "k_ba_plus_cam": (8, 0),
    "k_ba_cam_grad_max": (11, 0),
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba_solve_cam.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba_solve_cam.hip"), "-o", str(out)])
    return _kernels(out.read_text())


def test_every_kernel_of_the_unit_has_a_row(isa):
    meta, _ = isa
    for k in meta:
        assert sum(("%d%s" % (len(p.split("I")[0]), p)) in k for p in VGPRS) == 1, k
    assert len(meta) == len(VGPRS)


@pytest.mark.parametrize("part", sorted(VGPRS))
def test_camera_kernel_resources(isa, part):
    meta, body = isa
    ks = [k for k in meta if ("%d%s" % (len(part.split("I")[0]), part)) in k]
    assert len(ks) == 1, ks
    k = ks[0]
    m = meta[k]
    vgpr, lds = VGPRS[part]
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    assert m["vgpr"] <= vgpr, (k, m)
    assert m["lds"] <= lds, (k, m)

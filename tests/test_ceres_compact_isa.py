"""ISA of the compact Ceres-route kernels (csrc/ba.hip: k_ba_raw_compact, k_ba_pack_cam_jac), checked without a GPU:
they compile for gfx950 with no scratch and need no more VGPRs than k_ba_raw of the same compile -- the compact kernel
drops D = dP/dX, dPdq and the three products, so it must not be the heavier of the two."""
import os
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
MODELS = ("ILi0E", "ILi1E", "ILi2E", "ILi3E", "ILi4E", "ILin1E")      # the dispatched instantiations, -1 = per observation
SHARED = ("Lb0EE", "Lb1EE")                                           # second template argument: per-image / shared camera


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba.hip"), "-o", str(out)])
    return _kernels(out.read_text())


def _one(meta, part):
    ks = [k for k in meta if part in k]
    assert len(ks) == 1, (part, ks)
    return ks[0]


@pytest.mark.parametrize("model", MODELS)
def test_compact_kernel_is_leaner_than_the_full_one(isa, model):
    meta, body = isa
    for shared in SHARED:
        full = _one(meta, "8k_ba_raw" + model + shared)
        k = _one(meta, "16k_ba_raw_compact" + model + shared)
        m = meta[k]
        assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
        assert m["vgpr"] <= meta[full]["vgpr"], (k, m, meta[full])


def test_packed_camera_kernel(isa):
    meta, body = isa
    k = _one(meta, "17k_ba_pack_cam_jac")
    m = meta[k]
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    for model in MODELS:
        for shared in SHARED:
            assert m["vgpr"] <= meta[_one(meta, "8k_ba_raw" + model + shared)]["vgpr"], (k, m)

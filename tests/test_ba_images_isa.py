"""Resources of the image pass of the normal equations (csrc/ba.hip k_ba_images), checked on the
gfx950 code object's metadata without a GPU.  The bench scene's instantiation (OPENCV, with W) sums its 27 block entries
on the fp64 matrix pipe instead of in 54 registers of per-lane sums: it must stay at 4 wavefronts per SIMD (<= 128
VGPRs, which its launch bound asks for) without paying for that in scratch, and at 4 workgroups' LDS per CU."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

BENCH_KERNEL = "k_ba_imagesILi4ELb1EE"      # k_ba_images<4, true>


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba.hip"), "-o", str(out)])
    return _kernels(out.read_text())


def test_image_pass_resources(isa):
    meta, body = isa
    ks = [k for k in meta if BENCH_KERNEL in k]
    assert len(ks) == 1, ks
    k = ks[0]
    m = meta[k]
    print(k, m)
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    assert m["lds"] <= 40 * 1024, (k, m)                   # four workgroups per CU
    assert m["vgpr"] <= 128, (k, m)                        # __launch_bounds__(256, 4): four wavefronts per SIMD


def test_image_pass_sums_on_the_matrix_pipe(isa):
    """every instantiation: 16 fp64 MFMAs per iteration (8 staged rows each), no spill, LDS for 4 workgroups per CU"""
    meta, body = isa
    ks = [k for k in meta if "11k_ba_imagesILi" in k]
    assert len(ks) == 12, ks                               # 5 compiled-in models + the generic one, with and without W
    for k in ks:
        assert len(re.findall(r"\bv_mfma_f64_16x16x4_f64\b", body[k])) == 16, k
        assert meta[k]["scratch"] == 0 and "scratch_" not in body[k], (k, meta[k])
        assert meta[k]["lds"] <= 40 * 1024, (k, meta[k])

"""ISA of the guided SIFT walks (csrc/sift.hip k_sift_guided_stripe / k_sift_guided_batch), checked without a GPU: no
scratch (a reload in the tile loop would be a VMEM operation the hand-counted vmcnt waits miscount), the stated VGPR
budget, the tile loop's own LDS-DMA count, and no fused multiply-add outside the correctly rounded division of the
F test (the filter must round every operation as the reference's float Eigen code does)."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPR_BUDGET = 168   # 3 wavefronts per SIMD (the guided walk needs 139)


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "sift.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "sift.hip"), "-o", str(out)])
    return _kernels(out.read_text())


@pytest.mark.parametrize("part", ["k_sift_guided_stripe", "k_sift_guided_batch"])
def test_guided_walk_resources(isa, part):
    meta, body = isa
    ks = [k for k in meta if part in k]
    assert len(ks) == 1, ks
    k = ks[0]
    m, b = meta[k], body[k]
    assert m["scratch"] == 0 and "scratch_" not in b, (k, m)
    assert m["vgpr"] <= VGPR_BUDGET, (k, m)
    assert m["lds"] <= 80 * 1024, (k, m)
    # prologue + loop: 2 descriptor DMAs per wavefront + 1 record DMA (wavefronts 2 .. 4)
    assert len(re.findall(r"\bglobal_load_lds_dwordx4\b", b)) == 2 * 3, k
    assert len(re.findall(r"\bv_mfma_i32_32x32x32_i8\b", b)) == 4 * 8, k


@pytest.mark.parametrize("part", ["k_sift_guided_stripe", "k_sift_guided_batch", "k_sift_guide_prep"])
def test_no_fma_outside_the_division(isa, part):
    meta, body = isa
    k = [k for k in body if part in k][0]
    b = body[k]
    assert not re.findall(r"\bv_(?:mac|mad|pk_fma|fma_mix|fma_f16|fma_f64|fmac_f16|fmac_f64)\w*", b), k
    fma = len(re.findall(r"\bv_fma_f32\b", b)) + len(re.findall(r"\bv_fmac_f32\w*", b))
    fmas = len(re.findall(r"\bv_div_fmas_f32\b", b))
    fixup = len(re.findall(r"\bv_div_fixup_f32\b", b))
    assert fixup > 0, k
    # each correctly rounded division: 2 v_div_scale, v_rcp, 5 v_fma / v_fmac, v_div_fmas, v_div_fixup -- no other FMA
    assert fmas == fixup and fma == 5 * fixup, (k, fma, fmas, fixup)
    assert len(re.findall(r"\bv_div_scale_f32\b", b)) == 2 * fixup, k


def test_unguided_walks_keep_their_shape(isa):
    """the unguided kernels are the GUIDED = false instantiation: no record DMA, no division"""
    meta, body = isa
    for part in ("k_sift_scores_stripe", "k_sift_scores_batch"):
        k = [k for k in body if part in k][0]
        assert len(re.findall(r"\bglobal_load_lds_dwordx4\b", body[k])) == 2 * 2, k
        assert "v_div_fixup_f32" not in body[k], k
        assert meta[k]["vgpr"] <= 128, (k, meta[k])

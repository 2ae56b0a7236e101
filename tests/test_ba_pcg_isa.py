"""ISA of the reduced-solve kernels (csrc/ba_solve.hip: the block-sparse PCG, the gradient max-norm and the LM record,
DESIGN 4.3a), checked without a GPU: they compile for gfx950 with no scratch, and their VGPR counts are pinned from
above at what the build gives.  k_pcg_spmv holds one 6x6 block (36 fp64) per lane plus the partner's direction and six
accumulators: 120 VGPRs, 4 wavefronts per SIMD; k_pcg_init keeps the block's factor and its inverse in registers."""
import os
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPRS = {                     # counts of the gfx950 build (hipcc -O3)
    "k_pcg_init": 93,
    "k_pcg_begin": 32,
    "k_pcg_spmv": 120,
    "k_pcg_update": 74,
    "k_pcg_step": 40,
    "k_pcg_finish": 9,
    "k_ba_grad_max": 16,
    "k_ba_lm_record": 30,
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba_solve.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba_solve.hip"), "-o", str(out)])
    return _kernels(out.read_text())


@pytest.mark.parametrize("part", sorted(VGPRS))
def test_pcg_kernel_resources(isa, part):
    meta, body = isa
    ks = [k for k in meta if ("%d%s" % (len(part), part)) in k]
    assert len(ks) == 1, ks
    k = ks[0]
    m = meta[k]
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    assert m["vgpr"] <= VGPRS[part], (k, m)
    assert m["lds"] <= 2048, (k, m)

"""ISA of the kernels of csrc/ba_solve.hip (the point elimination, the manifold update, the gradient max-norm and the LM
record), checked without a GPU: no scratch (a spill would
put per-lane fp64 traffic on the memory path these kernels are bound by) and the VGPR counts stated below, pinned from
above so that growth shows up here rather than as a loss of wavefronts in flight.  k_schur_blocks holds 36 fp64
accumulators plus the 2 x 18 doubles of an entry: 156 VGPRs, 3 wavefronts per SIMD."""
import os
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPRS = {                     # counts of the gfx950 build (hipcc -O3), DESIGN 4.3a
    "k_schur_points": 44,
    "k_schur_obs": 118,
    "k_schur_blocks": 156,
    "k_schur_dense": 18,
    "k_schur_back": 76,
    "k_schur_model_decrease": 42,
    "k_sum_u32": 8,
    "k_ba_plus": 58,
    "k_ba_grad_max": 16,
    "k_ba_lm_record": 30,
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba_solve.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba_solve.hip"), "-o", str(out)])
    return _kernels(out.read_text())


@pytest.mark.parametrize("part", sorted(VGPRS))
def test_schur_kernel_resources(isa, part):
    meta, body = isa
    ks = [k for k in meta if ("%d%s" % (len(part), part)) in k]
    assert len(ks) == 1, ks
    k = ks[0]
    m = meta[k]
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    assert m["vgpr"] <= VGPRS[part], (k, m)
    assert m["lds"] <= 2048, (k, m)

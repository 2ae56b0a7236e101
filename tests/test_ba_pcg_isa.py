"""ISA of the PCG kernels on the reduced camera system, plain and bordered (csrc/ba_pcg.hip), checked
without a GPU and from the kernel metadata only: they compile for gfx950 with no scratch, and their VGPR counts and LDS
are pinned from above at what the build gives.  k_pcg_spmv holds one 6x6 block (36 fp64) per lane plus the partner's
direction and six accumulators: 120 VGPRs, 4 wavefronts per SIMD; k_pcg_init keeps the block's factor and its inverse in
registers.  k_pcg_cam_init works on one 12 x 12 block per wavefront through LDS (A, L and L^-1: 3 x 1152 bytes, and two
12-vectors) instead of 144 doubles per thread; k_pcg_cam_spmv is k_pcg_spmv (a 6 x 6 block per lane) plus six
accumulators and one row of B."""
import os
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPRS = {                     # counts of the gfx950 build (hipcc -O3); (VGPRs, LDS bytes)
    "k_pcg_init": (93, 2048),
    "k_pcg_begin": (32, 2048),
    "k_pcg_spmv": (120, 2048),
    "k_pcg_update": (74, 2048),
    "k_pcg_step": (40, 2048),
    "k_pcg_finish": (9, 2048),
    "k_pcg_cam_init": (48, 3648),
    "k_pcg_cam_spmv": (122, 0),
    "k_pcg_cam_rows": (24, 0),
    "k_pcg_cam_update": (98, 128),
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba_pcg.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba_pcg.hip"), "-o", str(out)])
    return _kernels(out.read_text())


def test_every_kernel_of_the_unit_has_a_row(isa):
    meta, _ = isa
    for k in meta:
        assert sum(("%d%s" % (len(p), p)) in k for p in VGPRS) == 1, k
    assert len(meta) == len(VGPRS)


@pytest.mark.parametrize("part", sorted(VGPRS))
def test_pcg_kernel_resources(isa, part):
    meta, body = isa
    ks = [k for k in meta if ("%d%s" % (len(part), part)) in k]
    assert len(ks) == 1, ks
    k = ks[0]
    m = meta[k]
    vgpr, lds = VGPRS[part]
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    assert m["vgpr"] <= vgpr, (k, m)
    assert m["lds"] <= lds, (k, m)

"""ISA of the dense factor-and-solve kernels (csrc/ba_chol.hip), checked without a GPU: they compile for
gfx950 with no scratch, and their VGPR counts are pinned from above at what the build gives.  k_chol_panel holds 24
columns of a row (48 VGPRs) per thread in workgroups of 512, so it has to stay at or below 128; k_chol_update holds a
48 x 48 accumulator per wavefront (72 VGPRs) and two steps of operands: 168, 3 wavefronts per SIMD.  The trailing
update must really run on the fp64 matrix pipe."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPRS = {                     # counts of the gfx950 build (hipcc -O3)
    "k_chol_clear": 10,
    "k_chol_fill_dense": 10,
    "k_chol_panel": 124,
    "k_chol_update": 168,
    "k_chol_back": 38,
    "k_chol_finish": 13,
}
LDS = {"k_chol_panel": 2 * 128 * 8, "k_chol_back": (96 * 96 + 96) * 8}   # column buffers; diagonal block + x_j


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba_chol.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba_chol.hip"), "-o", str(out)])
    return _kernels(out.read_text())


def _one(meta, part):
    ks = [k for k in meta if ("%d%s" % (len(part), part)) in k]
    assert len(ks) == 1, ks
    return ks[0]


def test_every_kernel_is_pinned(isa):
    meta, _ = isa
    assert sorted(_one(meta, p) for p in VGPRS) == sorted(meta)


@pytest.mark.parametrize("part", sorted(VGPRS))
def test_chol_kernel_resources(isa, part):
    meta, body = isa
    k = _one(meta, part)
    m = meta[k]
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    assert m["vgpr"] <= VGPRS[part], (k, m)
    assert m["lds"] == LDS.get(part, 0), (k, m)


def test_panel_kernel_fits_its_workgroup(isa):
    """512 threads are 2 wavefronts per SIMD: more than 256 VGPRs could not launch, more than 128 halves what runs"""
    meta, _ = isa
    assert meta[_one(meta, "k_chol_panel")]["vgpr"] <= 128


def test_trailing_update_runs_on_the_matrix_pipe(isa):
    meta, body = isa
    b = body[_one(meta, "k_chol_update")]
    n = len(re.findall(r"\bv_mfma_f64_16x16x4_f64\b", b))
    assert n == 9 * 24, n          # 3 x 3 tiles per wavefront, 96 / 4 steps, fully unrolled
    assert not re.findall(r"\bv_fma_f64\b", b)       # no product left on the vector pipe
    for part in ("k_chol_panel", "k_chol_back"):     # and the other kernels do not pretend to use it
        assert "v_mfma" not in body[_one(meta, part)]

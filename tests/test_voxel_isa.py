"""Resources of the voxel-downsampling kernels (csrc/voxel.hip) from the code-object metadata hipcc emits for gfx950 (no
GPU needed): no kernel spills (the reduce kernels keep a whole piece's records in registers: a spill would turn the
gather's 16 loads in flight into scratch traffic), and the register counts stay where this build has them -- the short
reduce kernel within 64 VGPRs (8 wavefronts per SIMD: at a handful of rows per voxel it lives on wavefronts in flight),
the long one within 128 (4 per SIMD, each with 16 gathers outstanding)."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# VGPRs of every k_voxel_* kernel as built, pinned from above
VGPR_PINS = {
    "k_voxel_keys": 9, "k_voxel_heads": 6, "k_voxel_segments": 8, "k_voxel_keep": 13, "k_voxel_long_list": 4,
    "k_voxel_reduce_short": 61, "k_voxel_reduce_long": 117, "k_voxel_map": 8,
}


@pytest.fixture(scope="module")
def voxel_meta(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "voxel.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "voxel.hip"), "-o", str(out)])
    meta, _ = _kernels(out.read_text())
    return {re.search(r"k_voxel_[a-z_]+?(?=E[PK])", k).group(0): m for k, m in meta.items() if "k_voxel_" in k}


def test_voxel_kernels_have_no_scratch(voxel_meta):
    assert sorted(voxel_meta) == sorted(VGPR_PINS)          # every kernel of the file is pinned below
    for name, m in voxel_meta.items():
        assert m["scratch"] == 0 and m["lds"] == 0, (name, m)


def test_voxel_kernels_vgpr_counts(voxel_meta):
    for name, pin in VGPR_PINS.items():
        assert voxel_meta[name]["vgpr"] <= pin, (name, voxel_meta[name])
    assert voxel_meta["k_voxel_reduce_short"]["vgpr"] <= 64
    assert voxel_meta["k_voxel_reduce_long"]["vgpr"] <= 128

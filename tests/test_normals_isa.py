"""ISA of the normal-estimation kernels (csrc/normals.hip), checked without a GPU: they compile for gfx950
with no scratch (the pass loop counts its vector-memory operations by hand: a spill reload would be miscounted), the VGPR
counts are pinned from above at what the build gives, the LDS of the pair kernel leaves room for 4 workgroups per CU,
and the distance test holds no fused multiply-add (the neighbour predicate is FLANN's separate multiply / add)."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

VGPRS = {                     # counts of the gfx950 build (hipcc -O3)
    "k_normals_passes": 14,
    "k_normals_items": 12,
    "k_normals_unindexed": 12,
    "k_normals_brick": 62,    # 8 wavefronts per SIMD by registers; the LDS tiles allow 4 workgroups = 4 per SIMD
    "k_normals_totals": 38,
}
BRICK_LDS = 4 * 2 * 256 * 16 + 4 * 8 * 8      # two 256-point tiles per wavefront + the block's counters


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "normals.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "normals.hip"), "-o", str(out)])
    return _kernels(out.read_text())


def _one(meta, part):
    ks = [k for k in meta if ("%d%s" % (len(part), part)) in k]
    assert len(ks) == 1, ks
    return ks[0]


@pytest.mark.parametrize("part", sorted(VGPRS))
def test_normals_kernel_resources(isa, part):
    meta, body = isa
    k = _one(meta, part)
    m = meta[k]
    assert m["scratch"] == 0 and "scratch_" not in body[k], (k, m)
    assert m["vgpr"] <= VGPRS[part], (k, m)
    if part == "k_normals_brick":
        assert m["lds"] == BRICK_LDS and 4 * m["lds"] <= 160 * 1024, (k, m)      # 4 workgroups per CU
    else:
        assert m["lds"] <= 16 * 1024, (k, m)


def test_pair_kernel_arithmetic(isa):
    meta, body = isa
    b = body[_one(meta, "k_normals_brick")]
    fma = re.findall(r"\bv_(?:fma|mad|fmac|pk_fma|mac)\w*_f32", b)
    assert not fma, fma[:3]
    # the moments are fp64: 3 widenings and 6 fused second moments per staged point, 4 points per LDS read group
    assert len(re.findall(r"\bv_cvt_f64_f32", b)) >= 4 * 3
    assert len(re.findall(r"\bv_(?:fma|fmac)_f64", b)) >= 4 * 6
    assert len(re.findall(r"\bglobal_load_lds_dwordx4\b", b)) == 2 * 4            # prologue + loop, 4 per tile


def test_pass_loop_has_only_its_own_vmem_operations(isa):
    """between a tile's 4 LDS-DMA instructions and the counted wait that covers them the kernel issues no other
    vector-memory instruction: `s_waitcnt vmcnt(4)` means "all but the 4 DMAs of the next tile" """
    meta, body = isa
    lines = body[_one(meta, "k_normals_brick")].split("\n")
    waits = [i for i, ln in enumerate(lines) if "s_waitcnt vmcnt(4)" in ln]
    assert len(waits) == 1, waits
    seen, j = 0, waits[0] - 1
    while j >= 0 and seen < 4:
        ln = lines[j].strip()
        if ln.startswith("global_load_lds_dwordx4"):
            seen += 1
        elif re.match(r"(global|buffer|flat|scratch)_(load|store|atomic)", ln):
            raise AssertionError(f"`{ln}` between a tile's DMAs and its counted wait (line {j})")
        j -= 1
    assert seen == 4

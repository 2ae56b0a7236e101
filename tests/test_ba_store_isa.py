"""Store policies of the BA evaluation (csrc/ba.hip StorePolicy), checked on the gfx950 ISA without a GPU.

W of the bench scene's image pass, k_ba_images<4, true>, leaves with non-temporal 16-byte stores on both of its paths
(nine per row of 144 B on the contiguous path, nine on the scattered one); the policy must cost neither the fourth
wavefront per SIMD nor scratch, there or in k_ba_points<4, true, true>.  The kernels whose outputs are read back
straight away (pinned-buffer copies of the raw / Ceres route, the camera coupling blocks) keep plain stores."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

IMAGES = "11k_ba_imagesILi4ELb1EE"          # k_ba_images<4, true>
POINTS = "11k_ba_pointsILi4ELb1ELb1EE"      # k_ba_points<4, true, true>
PLAIN = ("8k_ba_rawILi", "16k_ba_raw_compactILi", "10k_ba_cam_wILi")
STORE = re.compile(r"^\s*((?:global|flat|buffer|scratch)_store_\w+)\s([^\n;]*)", re.M)
MODIFIER = re.compile(r"\b(nt|sc0|sc1)\b")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "ba.s"
    subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", "ba.hip"), "-o", str(out)])
    return _kernels(out.read_text())


def _one(meta, part):
    ks = [k for k in meta if part in k]
    assert len(ks) == 1, (part, ks)
    return ks[0]


def _stores(body):
    """(instruction, sorted cache modifiers) of every vector store"""
    return [(op, tuple(sorted(MODIFIER.findall(args)))) for op, args in STORE.findall(body)]


def test_w_leaves_with_non_temporal_16_byte_stores(isa):
    meta, body = isa
    k = _one(meta, IMAGES)
    wide = [s for s in _stores(body[k]) if s[0].endswith("dwordx4")]
    print(k, meta[k], wide)
    assert len(wide) >= 9, wide
    assert all(s == ("global_store_dwordx4", ("nt",)) for s in wide), wide
    # nothing of W leaves in narrower pieces: the only other store is the segment's 27 sums, 8 bytes per lane, plain
    rest = [s for s in _stores(body[k]) if not s[0].endswith("dwordx4")]
    assert rest == [("global_store_dwordx2", ())], rest


def test_policy_costs_no_occupancy(isa):
    meta, body = isa
    for part in (IMAGES, POINTS):
        k = _one(meta, part)
        print(k, meta[k])
        assert meta[k]["vgpr"] <= 128, (k, meta[k])            # four wavefronts per SIMD
        assert meta[k]["scratch"] == 0 and "scratch_" not in body[k], (k, meta[k])


def test_outputs_read_back_at_once_keep_plain_stores(isa):
    meta, body = isa
    for part in PLAIN:
        ks = [k for k in meta if part in k]
        assert ks, part
        for k in ks:
            st = _stores(body[k])
            assert any(op.endswith("dwordx4") for op, _ in st), (k, st)
            assert all(mod == () for _, mod in st), (k, st)
    # the point pass writes H_pt / g_pt plain as well (non-temporal there doubled its time: DESIGN 5)
    assert all(mod == () for _, mod in _stores(body[_one(meta, POINTS)]))

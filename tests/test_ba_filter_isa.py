"""Resources of the kernels of pcd_ba_filter_points (csrc/ba.hip) and pcd_ba_remove_observations_device
(csrc/ba_edit.hip) from the code-object metadata hipcc emits for gfx950 (no GPU needed): none of them uses scratch memory
(the pair loop of k_ba_filter_tri_angle keeps its centres and the point in registers: no runtime-indexed array), and
k_ba_filter_tri_angle stays within the 128 VGPRs at which its 256-thread workgroups keep 4 wavefronts on every SIMD."""
import os
import subprocess

import pytest

from tests.test_kernel_isa import FLAGS, HIPCC, ROOT, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
FILTER = ("k_ba_proj_centers", "k_ba_filter_tri_angle")
EDIT = ("k_edit_obs_flag", "k_edit_term_flag", "k_edit_list_flag", "k_edit_vobs_flag", "k_edit_compact_obs",
        "k_edit_compact_terms", "k_edit_compact_list", "k_edit_starts", "k_edit_lengths", "k_edit_slice_width",
        "k_edit_seg_count", "k_edit_segs", "k_edit_record")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    out = {}
    for unit in ("ba", "ba_edit"):
        path = tmp_path_factory.mktemp("isa") / (unit + ".s")
        subprocess.check_call([HIPCC] + FLAGS + [os.path.join(ROOT, "colmap-pcd_amd", "csrc", unit + ".hip"), "-o", str(path)])
        out.update(_kernels(path.read_text())[0])
    return out


def _one(meta, name):
    hits = [k for k in meta if ("3pcd%d%sE" % (len(name), name)) in k]
    assert len(hits) == 1, (name, hits)
    return meta[hits[0]]


def test_new_kernels_use_no_scratch(meta):
    for name in FILTER + EDIT:
        assert _one(meta, name)["scratch"] == 0, (name, _one(meta, name))


def test_tri_angle_register_budget(meta):
    m = _one(meta, "k_ba_filter_tri_angle")
    assert m["vgpr"] <= 128, m

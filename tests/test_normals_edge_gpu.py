"""The normal estimation (csrc/normals.hip) where its suite did not reach: range tables of more than 64 quad rows (the B
registers of k_normals_brick), clouds far from the origin and of a wide extent (the binning slack in the reach), the reach
refusal, and the rules of pcdhip.h on the device -- the orientation tie, ORIENT_NONE off a plane, the only_missing
threshold, min_neighbors below 3, nearly collinear neighbourhoods, the tails of the pair loop and of the query passes.

Scenes and references: tests/normals_ref.py (checked on their own by tests/test_normals_cpu.py).  Tolerances: those of
tests/test_normals_gpu.py, unchanged.  normals_ref.range_table_geometry only proves that a scene reaches the branch it
is about; it never predicts device output."""
import numpy as np
import pytest

from tests import normals_ref as nr
from tests.test_normals_gpu import _check_info, _cloud, _compare

pytestmark = pytest.mark.gpu


def _run(gpu, name, check_info=True):
    """an edge scene through the host entry point: (handle info, device result, downloaded normals, reference)"""
    xyz, cell, r, opts, vectors, _ = nr.edge_scene(name)
    ref = nr.edge_ref(name)
    c = _cloud(gpu, xyz, cell)
    info = c.info()
    out = c.estimate_normals(radius=r, **opts)
    _, nrm_dev = c.download()
    c.close()
    _compare(out, nrm_dev, ref, vectors=vectors)
    if check_info:
        _check_info(out["info"], ref, info["num_indexed"])
    return info, out, nrm_dev, ref


# ------------------------------------------------------------------------------------------- B. wide reach ----
def test_wide_dense_fills_both_halves_of_the_range_table(gpu):
    xyz, cell, r = nr.edge_scene("wide_dense")[:3]
    info = _run(gpu, "wide_dense")[0]
    assert info["dims"] == [3, 26, 24]
    geo = nr.range_table_geometry(xyz, info, r)
    assert (geo["R"], geo["Rq"]) == (9, 5)
    assert np.any(geo["nrows"] > 64) and np.any(geo["nrows"] == 64) and geo["nrows"].max() == 121
    assert any(n > 64 and w[64:].sum() > 0 for n, w in zip(geo["nrows"], geo["rows"]))      # the B rows hold points


def test_wide_sparse_empty_rows_in_the_second_half(gpu):
    xyz, cell, r = nr.edge_scene("wide_sparse")[:3]
    info = _run(gpu, "wide_sparse")[0]
    geo = nr.range_table_geometry(xyz, info, r)
    wide = [w for n, w in zip(geo["nrows"], geo["rows"]) if n > 64]
    assert any(w[64:].sum() == 0 for w in wide)                                  # T == TA: every B row is empty
    assert any(np.any((w[64:-1] == 0) & (w[65:] > 0)) for w in wide)              # an empty range before a full one, in B


def test_smallest_reach_that_crosses_64_rows(gpu):
    """r = 7 cells: Rq = 4, a window of 9 x 9 quad rows"""
    xyz, cell, r = nr.edge_scene("wide_dense_r7")[:3]
    info = _run(gpu, "wide_dense_r7")[0]
    geo = nr.range_table_geometry(xyz, info, r)
    assert geo["Rq"] == 4 and geo["nrows"].max() == 81 and np.any(geo["nrows"] == 64)


# ----------------------------------------------------------------------- C. far origin and wide extent ----
def test_far_from_origin_the_slack_widens_the_reach(gpu):
    xyz, cell, r = nr.edge_scene("far")[:3]
    info, out, nrm_dev, ref = _run(gpu, "far")
    geo = nr.range_table_geometry(xyz, info, r)
    assert geo["R_noslack"] == 2 and geo["R"] == 3 and 3.7e-3 < geo["slack"] < 3.9e-3
    assert ref["dot_rel"][ref["ok"]].min() > 1e-6            # the viewpoint inside the cloud decides every sign


def test_wide_extent(gpu):
    xyz, cell, r = nr.edge_scene("wide_extent")[:3]
    info = _run(gpu, "wide_extent")[0]
    assert 40009 <= info["dims"][0] <= 40011 and info["dims"][1:] == [10, 10]
    geo = nr.range_table_geometry(xyz, info, r)
    assert geo["R_noslack"] == 2 and geo["R"] == 3


# --------------------------------------------------------------------------------- D. the reach refusal ----
def test_reach_refusal_touches_nothing(gpu):
    """radius == 8 h passes the guard, but with a slack of one cell it reaches 10: refused by both entry points before
    anything is launched -- stored normals (the Inf row's too) and device outputs stay as they were"""
    import torch
    xyz, cell, r, _, _, _ = nr.edge_scene("reach_0.7")
    n = xyz.shape[0]
    given = np.tile(np.array([0, 1, 0], np.float32), (n, 1))
    c = _cloud(gpu, xyz, cell, nrm=given)
    assert np.float32(0.8) == np.float32(8.0) * np.float32(c.info()["cell_size"])
    d_count = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_curv = torch.full((n,), -7.25, dtype=torch.float64, device="cuda")
    with pytest.raises(gpu.PcdError) as e:
        c.estimate_normals(radius=0.8)
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "reaches" in str(e.value)
    assert np.array_equal(c.download()[1].view(np.uint32), given.view(np.uint32))
    for only_missing in (False, True):
        with pytest.raises(gpu.PcdError) as e:
            c.estimate_normals_device(d_count, d_curv, radius=0.8, only_missing=only_missing,
                                      stream=torch.cuda.current_stream().cuda_stream)
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "reaches" in str(e.value)
        torch.cuda.synchronize()
        assert np.array_equal(c.download()[1].view(np.uint32), given.view(np.uint32))
        assert bool((d_count == 0x5A5A5A5A).all()) and bool((d_curv == -7.25).all())
    # the same handle at 7 cells: R = 9, accepted
    geo = nr.range_table_geometry(xyz, c.info(), r)
    assert geo["R"] == 9 and geo["R_noslack"] == 8 and geo["nrows"].max() > 64
    ref = nr.edge_ref("reach_0.7")
    out = c.estimate_normals(radius=r)
    _, nrm_dev = c.download()
    _compare(out, nrm_dev, ref)
    _check_info(out["info"], ref, n - 1)
    assert np.all(nrm_dev[-1] == 0) and out["count"][-1] == 0 and out["curvature"][-1] == 0      # the Inf row
    c.close()


# ------------------------------------------------------------------------------ E. rules on the device ----
def test_orientation_tie_on_the_device(gpu):
    """the viewpoint lies in the plane: every dot product is exactly 0, the largest component decides"""
    info, out, nrm_dev, ref = _run(gpu, "tie_plane")
    assert np.all(ref["dot_rel"] == 0)
    assert np.array_equal(nrm_dev, np.tile(np.array([0, 0, 1], np.float32), (nrm_dev.shape[0], 1)))


def test_orient_none_off_a_plane(gpu):
    xyz, ref = nr.orient_none_ref()
    sure = nr.orient_none_sure(ref)
    assert sure.sum() >= 0.95 * ref["ok"].sum()
    c = _cloud(gpu, xyz, 0.1)
    out = c.estimate_normals(radius=0.25, orient=nr.ORIENT_NONE, viewpoint=(1.0, 1.0, 1.0))     # the viewpoint is unused
    _, nrm_dev = c.download()
    c.close()
    _compare(out, nrm_dev, ref, sure=sure)
    _check_info(out["info"], ref, xyz.shape[0])


def test_only_missing_threshold_and_inf_rows(gpu):
    xyz, stored = nr.only_missing_scene()
    ref = nr.edge_ref("only_missing")
    fin = ref["finite"]
    kept = nr.kept_mask(stored)
    assert np.array_equal(kept[:7], [False, False, False, True, True, False, True])
    c = _cloud(gpu, xyz, 0.1, nrm=stored)
    m = c.info()["num_indexed"]
    assert m == 25
    out = c.estimate_normals(radius=0.1, only_missing=True)
    _, nrm_dev = c.download()
    assert np.array_equal(nrm_dev[kept].view(np.uint32), stored[kept].view(np.uint32))          # bit-identical
    # counts and curvature on every row (kept rows report theirs too); the vectors of the replaced rows are the device's,
    # the kept ones (an Inf among them) were compared above
    _compare(out, np.where(kept[:, None], ref["normal"].astype(np.float32), nrm_dev), ref)
    i = out["info"]
    assert i["num_kept"] == int((kept & fin).sum()) == 10
    assert i["num_estimated"] == int((ref["ok"] & ~kept).sum()) == 15
    assert i["num_kept"] + i["num_estimated"] + i["num_too_few"] + i["num_degenerate"] == m
    # the rows with an Inf coordinate: count 0, curvature 0, in no counter; a stored normal is kept, a missing one stays 0
    assert np.all(out["count"][~fin] == 0) and np.all(out["curvature"][~fin] == 0)
    assert np.array_equal(nrm_dev[~fin], np.array([[0, 0, 1], [0, 0, 0]], np.float32))
    # without only_missing everything is replaced, the Inf rows by 0
    out = c.estimate_normals(radius=0.1)
    _, nrm_dev = c.download()
    c.close()
    _compare(out, nrm_dev, ref)
    _check_info(out["info"], ref, m)
    assert np.all(nrm_dev[~fin] == 0)


@pytest.mark.parametrize("min_nb", [0, 1, 2])
def test_min_neighbors_below_three_is_three(gpu, min_nb):
    for scene in nr.degenerate_scenes():
        name, xyz, r, _, (est, few, deg), bare = scene
        if name not in ("two_points", "isolated"):
            continue
        ref = nr.estimate(xyz, r, min_neighbors=3)
        c = _cloud(gpu, xyz, 0.1)
        out = c.estimate_normals(radius=r, min_neighbors=min_nb)
        _, nrm_dev = c.download()
        c.close()
        i = out["info"]
        assert (i["num_estimated"], i["num_too_few"], i["num_degenerate"]) == (est, few, deg), name
        assert np.all(nrm_dev[bare] == 0) and np.all(out["curvature"][bare] == 0)
        _compare(out, nrm_dev, ref)


@pytest.mark.parametrize("jitter", nr.NEAR_LINE_JITTER)
def test_nearly_collinear_is_estimated(gpu, jitter):
    """l1 / l2 of 1e-7 .. 1e-5: two and more decades above the rule's 1e-10, every row has a normal"""
    info, out, nrm_dev, ref = _run(gpu, "near_line_%g" % jitter)
    assert ref["ok"].all() and out["info"]["num_degenerate"] == 0
    assert not np.any((ref["rank"] > 1e-12) & (ref["rank"] < 1e-8))


@pytest.mark.parametrize("n", nr.TAIL_SIZES)
def test_pass_and_tile_tails(gpu, n):
    """one leaf of n points: n % 4 is the tail of the pair loop, n % 64 the clamp of the last query pass, 256 the tile"""
    info, out, nrm_dev, ref = _run(gpu, "tail_%d" % n)
    assert info["dims"] == [1, 1, 1] and ref["count"].min() >= 10
    assert out["info"]["pair_tests"] == n * n

"""The numpy reference of the normal estimation (tests/normals_ref.py) checked on its own, without a GPU: its neighbour
sets against scipy's k-d tree, its sensitivity to the summation order against the tolerances the device test uses, the
eigenvalue gaps of the parity clouds those tolerances rely on, the hand cases, the same checks on the scenes of
tests/test_normals_edge_gpu.py with the figures and range-table branches those tests quote, and the entry point's
refusal on a box without a device."""
import ctypes as C

import numpy as np
import pytest

from tests import normals_ref as nr

PARITY = [("planes", r) for r in nr.PLANES_RADII] + [("uniform", r) for r in nr.UNIFORM_RADII]


@pytest.mark.parametrize("name,r", PARITY)
def test_bruteforce_neighbours_equal_kdtree(name, r):
    xyz, pairs = nr.parity_pairs(name)
    I, J = pairs[r]
    Ik, Jk = nr.pairs_kdtree(xyz, r)
    assert np.array_equal(I, Ik) and np.array_equal(J, Jk)
    assert np.all(np.bincount(I, minlength=xyz.shape[0]) >= 1)      # every row is its own neighbour


@pytest.mark.parametrize("name,r", PARITY)
def test_summation_order_stays_within_the_device_tolerances(name, r):
    """the tolerances of tests/test_normals_gpu.py are about the order of the fp64 sums only: the reference with its pair
    list shuffled stays inside them"""
    xyz, ref = nr.parity_ref(name, r)
    I, J = nr.parity_pairs(name)[1][r]
    perm = np.random.default_rng(5).permutation(I.shape[0])
    alt = nr.from_pairs(xyz, I, J, perm=perm)
    assert np.array_equal(alt["count"], ref["count"])
    assert np.array_equal(alt["ok"], ref["ok"])
    dc = np.abs(alt["curvature"] - ref["curvature"])
    print("max curvature move / tol", float(np.max(dc / nr.curvature_tol(ref))))
    assert np.all(dc <= nr.curvature_tol(ref))
    wide = ref["ok"] & (ref["gap"] >= nr.GAP_MIN)
    dn = np.abs(alt["normal"].astype(np.float32).astype(np.float64) - ref["normal"].astype(np.float32))
    print("max normal move", float(dn[wide].max()))
    assert np.all(dn[wide] <= nr.normal_tol(ref)[wide, None])


@pytest.mark.parametrize("name,r", PARITY)
def test_parity_clouds_have_the_gaps_the_device_test_relies_on(name, r):
    xyz, ref = nr.parity_ref(name, r)
    narrow = ref["ok"] & (ref["gap"] < nr.GAP_MIN)
    k = ref["count"]
    print(name, r, "mean k %.1f max k %d, k<3: %d, gap<1e-3: %.3f %%, gap<1e-2: %.3f %%" % (
        k.mean(), k.max(), int((k < 3).sum()), 100.0 * narrow.mean(), 100.0 * (ref["ok"] & (ref["gap"] < 1e-2)).mean()))
    assert narrow.mean() <= 0.01
    # no row within a factor 100 of the rank rule l1 <= 1e-10 l2
    assert not np.any((ref["rank"] > 1e-12) & (ref["rank"] < 1e-8))


def test_lattice_hand_cases():
    xyz = nr.lattice()
    idx = np.arange(12 ** 3).reshape(12, 12, 12)
    for r, interior, corner in ((0.125, 7, 4), (0.25, 33, 11)):
        ref = nr.estimate(xyz, r)
        assert np.all(ref["count"][idx[2:-2, 2:-2, 2:-2].ravel()] == interior)      # the boundary `<=` is included
        assert ref["count"][idx[0, 0, 0]] == corner
        assert np.allclose(ref["curvature"][idx[2:-2, 2:-2, 2:-2].ravel()], 1.0 / 3.0, rtol=0, atol=1e-14)


def test_plane_hand_cases():
    xyz = nr.plane_lattice()
    for vp, orient, nz in (((0, 0, 10), nr.ORIENT_VIEWPOINT, 1.0), ((0, 0, 0), nr.ORIENT_NONE, 1.0),
                           ((0, 0, -10), nr.ORIENT_VIEWPOINT, -1.0)):
        ref = nr.estimate(xyz, 0.1, orient=orient, viewpoint=vp)
        assert ref["ok"].all()
        assert np.allclose(ref["normal"], [0.0, 0.0, nz], rtol=0, atol=1e-12)
        assert np.all(np.abs(ref["curvature"]) <= 1e-15)


@pytest.mark.parametrize("scene", nr.degenerate_scenes(), ids=lambda s: s[0])
def test_degenerate_hand_cases(scene):
    name, xyz, r, min_nb, (est, few, deg), bare = scene
    ref = nr.estimate(xyz, r, min_neighbors=min_nb)
    assert (int(ref["ok"].sum()), int(ref["too_few"].sum()), int(ref["degenerate"].sum())) == (est, few, deg)
    assert np.all(ref["normal"][bare] == 0) and np.all(ref["curvature"][bare] == 0)


def test_orientation_tie_rule():
    """a dot product of exactly 0 falls back to the largest component, ties to the lowest axis"""
    xyz = nr.plane_lattice(n=9, spacing=0.125, z=0.0)     # the viewpoint (0,0,0) lies in the plane: n . (v - p) = 0
    ref = nr.estimate(xyz, 0.3)
    assert ref["ok"].all() and np.allclose(ref["normal"], [0, 0, 1], atol=1e-12)


# ---- the scenes of tests/test_normals_edge_gpu.py: the same four checks, and the figures their tests quote ----
@pytest.mark.parametrize("name", nr.EDGE_SCENES)
def test_edge_scene_reference(name):
    xyz, cell, r, opts, vectors, expect = nr.edge_scene(name)
    ref = nr.edge_ref(name)
    I, J = nr.edge_pairs(name)
    Ik, Jk = nr.pairs_kdtree(xyz, r)
    assert np.array_equal(I, Ik) and np.array_equal(J, Jk)
    k = ref["count"][ref["finite"]]
    narrow = ref["ok"] & (ref["gap"] < nr.GAP_MIN)
    print(name, "estimated / too few / degenerate %d %d %d, k %d .. %d, gap<1e-3: %d rows, rank %.3g .. %.3g" % (
        ref["ok"].sum(), ref["too_few"].sum(), ref["degenerate"].sum(), k.min(), k.max(), narrow.sum(),
        ref["rank"][ref["finite"]].min(), ref["rank"][ref["finite"]].max()))
    est, few, deg, kmin, kmax = expect
    assert (int(ref["ok"].sum()), int(ref["too_few"].sum()), int(ref["degenerate"].sum())) == (est, few, deg)
    assert kmin is None or (int(k.min()), int(k.max())) == (kmin, kmax)
    assert k.min() >= 10 or not name.startswith("tail_")
    assert not np.any((ref["rank"] > 1e-12) & (ref["rank"] < 1e-8))
    if vectors:                                                # the share is capped wherever vectors are compared
        assert narrow.sum() <= 0.01 * ref["ok"].sum()
    # another summation order stays inside the device tolerances
    alt = nr.from_pairs(xyz, I, J, perm=np.random.default_rng(5).permutation(I.shape[0]), **opts)
    assert np.array_equal(alt["count"], ref["count"]) and np.array_equal(alt["ok"], ref["ok"])
    assert np.all(np.abs(alt["curvature"] - ref["curvature"]) <= nr.curvature_tol(ref))
    norm = np.linalg.norm(alt["normal"].astype(np.float32).astype(np.float64), axis=1)
    assert np.all(np.abs(norm[ref["ok"]] - 1.0) <= 2.0 ** -22)
    if vectors:
        wide = ref["ok"] & ~narrow
        dn = np.abs(alt["normal"].astype(np.float32).astype(np.float64) - ref["normal"].astype(np.float32))
        assert np.all(dn[wide] <= nr.normal_tol(ref)[wide, None])


def test_near_line_ranks_are_decades_from_the_rule():
    for j, (lo, hi) in zip(nr.NEAR_LINE_JITTER, ((3e-8, 4e-7), (3e-6, 4e-5))):
        rank = nr.edge_ref("near_line_%g" % j)["rank"]
        assert lo <= rank.min() and rank.max() <= hi


def test_orient_none_reference():
    xyz, ref = nr.orient_none_ref()
    _, with_vp = nr.parity_ref("uniform", 0.25)
    big = ref["normal"][np.arange(xyz.shape[0]), np.argmax(np.abs(ref["normal"]), axis=1)]
    assert np.all(big[ref["ok"]] > 0)
    assert np.array_equal(np.abs(ref["normal"]), np.abs(with_vp["normal"]))      # the same vectors up to the sign
    assert (ref["normal"] != with_vp["normal"]).any()
    assert nr.orient_none_sure(ref).sum() >= 0.95 * ref["ok"].sum()


def test_kept_mask_threshold():
    xyz, stored = nr.only_missing_scene()
    kept = nr.kept_mask(stored)
    assert np.array_equal(kept[:7], [False, False, False, True, True, False, True])
    assert int(kept[:25].sum()) == 10 and list(kept[25:]) == [True, False]
    assert float(stored[2, 0]) == 9.999999974752427e-07


def test_range_table_geometry_hand_cases():
    # one leaf: a table of one row that holds every point
    xyz, cell, r = nr.edge_scene("tail_65")[:3]
    geo = nr.range_table_geometry(xyz, nr.grid_info(xyz, cell), r)
    assert geo["leaves"].tolist() == [[0, 0, 0]] and geo["nrows"].tolist() == [1] and geo["rows"][0].tolist() == [65]
    # one point in the middle of every cell of 2 x 60 x 60 (30 x 30 quads), r = 8 cells: R = 9, Rq = 5
    h = 0.125
    g = [(np.arange(n) + 0.5) * h for n in (2, 60, 60)]
    xyz = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    info = nr.grid_info(xyz, h)
    assert info["dims"] == [2, 60, 60]
    geo = nr.range_table_geometry(xyz, info, 1.0)
    assert (geo["R"], geo["Rq"], geo["R_noslack"]) == (9, 5, 9) and geo["leaves"].shape[0] == 900
    at = {tuple(l): i for i, l in enumerate(geo["leaves"].tolist())}
    i = at[(0, 15, 15)]
    assert geo["nrows"][i] == 121 and np.all(geo["rows"][i] == 8)               # 2 x cells of 4 cells a quad
    assert geo["nrows"][at[(0, 0, 0)]] == 36 and geo["nrows"][at[(0, 3, 29)]] == 9 * 6
    assert geo["nrows"].max() == 121
    # the dims of the last row: lattice points bin as the device bins them (one per cell)
    assert sum(int(w.sum()) for w in geo["rows"]) == sum(8 * n for n in geo["nrows"])


def test_edge_scenes_reach_their_branches():
    """what the GPU tests assert from the handle's info, here from the grid a handle of that cell size gets"""
    geo = {n: nr.range_table_geometry(nr.edge_scene(n)[0], nr.grid_info(*nr.edge_scene(n)[:2]), nr.edge_scene(n)[2])
           for n in ("wide_dense", "wide_dense_r7", "wide_sparse", "far", "wide_extent", "reach_0.7")}
    d = geo["wide_dense"]
    col = np.unique(d["leaves"][:, 1:], axis=0, return_index=True)[1]             # one leaf per (y, z) column
    nrows = d["nrows"][col]
    assert ((nrows > 64).sum(), (nrows == 64).sum(), (nrows < 64).sum(), nrows.max()) == (96, 4, 56, 121)
    assert (d["R"], d["Rq"]) == (9, 5)
    assert geo["wide_dense_r7"]["Rq"] == 4 and geo["wide_dense_r7"]["nrows"].max() == 81
    wide = [w for n, w in zip(geo["wide_sparse"]["nrows"], geo["wide_sparse"]["rows"]) if n > 64]
    assert any(w[64:].sum() == 0 for w in wide)
    assert any(np.any((w[64:-1] == 0) & (w[65:] > 0)) for w in wide)
    for n in ("far", "wide_extent"):
        assert (geo[n]["R_noslack"], geo[n]["R"]) == (2, 3) and 3.7e-3 < geo[n]["slack"] < 3.9e-3
    assert nr.grid_info(*nr.edge_scene("wide_extent")[:2])["dims"] == [40010, 10, 10]
    assert (geo["reach_0.7"]["R_noslack"], geo["reach_0.7"]["R"]) == (8, 9)
    # radius = 8 h on that handle: 10 cells
    xyz, cell = nr.edge_scene("reach_0.7")[:2]
    assert nr.range_table_geometry(xyz, nr.grid_info(xyz, cell), 0.8)["R"] == 10


def test_entry_point_refuses_without_a_device(pcdhip):
    L = pcdhip.lib()
    if pcdhip.device_count() > 0:
        # on a GPU box the argument checks come first: a null handle is invalid
        assert L.pcd_cloud_estimate_normals(None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
        assert L.pcd_cloud_estimate_normals_device(None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
        return
    # "no gfx950 device" is the first guard: no handle can exist on this box, so every call ends there
    o = pcdhip.normals_options()
    assert (o.radius, o.min_neighbors, o.orient, list(o.viewpoint), o.only_missing) == (
        np.float32(0.15), 3, pcdhip.NORMALS_ORIENT_VIEWPOINT, [0.0, 0.0, 0.0], 0)
    assert L.pcd_cloud_estimate_normals(None, C.byref(o), None, None, None) == pcdhip.PCD_ERR_NO_DEVICE
    assert L.pcd_cloud_estimate_normals_device(None, C.byref(o), None, None, None) == pcdhip.PCD_ERR_NO_DEVICE
    assert b"no HIP device" in L.pcd_last_error()
    with pytest.raises(pcdhip.PcdError) as e:
        pcdhip.Cloud(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), raw_lidar_frame=False)
    assert e.value.status == pcdhip.PCD_ERR_NO_DEVICE

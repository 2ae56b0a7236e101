"""GPU parity of the normal estimation (pcd_cloud_estimate_normals, csrc/normals.hip) against the numpy reference of
its definition (tests/normals_ref.py).

Tolerances, computed from the reference's own k_i and gap_i = (l1 - l0) / l2, never from device output:
  counts      exact;
  curvature   |d| <= 64 k 2^-53: the eigenvalue perturbation under a reordered fp64 sum of k terms, relative to the trace;
  normals     on rows with gap >= 1e-3, per component |n_dev - float32(n_ref)| <= 2^-23 + 128 k 2^-53 / gap: one float
              rounding plus Davis-Kahan; the sign is compared only where |n_ref . (v - p)| > 1e-6 |v - p|;
  other rows  finite, | |n| - 1 | <= 2^-22; their share is asserted <= 1 % wherever the vectors are compared
              (tests/test_normals_cpu.py shows the reference clouds keep to that on their own).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import normals_ref as nr

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")


def _cloud(gpu, xyz, cell_size, nrm=None):
    c = gpu.Cloud(xyz, np.zeros_like(xyz) if nrm is None else nrm, raw_lidar_frame=False, cell_size=cell_size)
    assert abs(c.info()["cell_size"] - np.float32(cell_size)) < 1e-9      # r / h is what the test says it is
    return c


def _compare(out, nrm_dev, ref, rows=None, vectors=True, sure=None):
    """device result (estimate_normals' dict + the downloaded normals) against the reference on `rows` (default all);
    sure: the rows whose sign must be the reference's (default: where the viewpoint decides it)"""
    n = ref["count"].shape[0]
    sel = np.ones(n, bool) if rows is None else np.isin(np.arange(n), rows)
    assert np.array_equal(out["count"][sel], ref["count"][sel])
    bare = sel & ~ref["ok"]
    assert np.all(nrm_dev[bare] == 0) and np.all(out["curvature"][bare] == 0)
    dc = np.abs(out["curvature"] - ref["curvature"])
    tol_c = nr.curvature_tol(ref)
    print("curvature: max |d| / tol = %.3g" % float(np.max(dc[sel] / np.maximum(tol_c[sel], 1e-300), initial=0.0)))
    assert np.all(dc[sel] <= tol_c[sel])
    ok = sel & ref["ok"]
    assert np.all(np.isfinite(nrm_dev))
    norm = np.linalg.norm(nrm_dev.astype(np.float64), axis=1)
    assert np.all(np.abs(norm[ok] - 1.0) <= 2.0 ** -22)
    if not vectors:
        return
    wide = ok & (ref["gap"] >= nr.GAP_MIN)
    assert (ok & ~wide).sum() <= 0.01 * max(int(ok.sum()), 1)
    ref32 = ref["normal"].astype(np.float32).astype(np.float64)
    dev = nrm_dev.astype(np.float64)
    same = np.abs(dev - ref32).max(axis=1)
    mirrored = np.abs(dev + ref32).max(axis=1)
    if sure is None:
        sure = ref["dot_rel"] > 1e-6                     # the orientation is decided: signs must agree
    err = np.where(sure, same, np.minimum(same, mirrored))
    tol_n = nr.normal_tol(ref)
    print("normals: max err / tol = %.3g over %d rows" % (float(np.max(err[wide] / tol_n[wide], initial=0.0)),
                                                          int(wide.sum())))
    assert np.all(err[wide] <= tol_n[wide])


def _check_info(info, ref, m):
    assert info["num_estimated"] == int(ref["ok"].sum())
    assert info["num_too_few"] == int(ref["too_few"].sum())
    assert info["num_degenerate"] == int(ref["degenerate"].sum())
    assert info["num_kept"] == 0
    assert info["max_neighbors"] == int(ref["count"].max(initial=0))
    assert abs(info["mean_neighbors"] - ref["count"].sum() / max(m, 1)) <= 1e-12 * max(info["mean_neighbors"], 1.0)
    assert info["pair_tests"] >= int(ref["count"].sum()) and info["ms"] > 0


@pytest.mark.parametrize("name,cell,r", [("planes", 0.2, 0.08), ("planes", 0.2, 0.2), ("planes", 0.2, 0.5),
                                         ("uniform", 0.1, 0.25), ("uniform", 0.3, 0.25)])
def test_parity(gpu, name, cell, r):
    xyz, ref = nr.parity_ref(name, r)
    c = _cloud(gpu, xyz, cell)
    out = c.estimate_normals(radius=r)
    _, nrm_dev = c.download()
    _compare(out, nrm_dev, ref)
    _check_info(out["info"], ref, xyz.shape[0])
    c.close()


@pytest.mark.parametrize("cell", [0.125, 0.25])
def test_lattice_ties(gpu, cell):
    """points exactly on cell faces, neighbours at exactly r"""
    xyz = nr.lattice()
    idx = np.arange(12 ** 3).reshape(12, 12, 12)
    inner = idx[2:-2, 2:-2, 2:-2].ravel()
    c = _cloud(gpu, xyz, cell)
    for r, k in ((0.125, 7), (0.25, 33)):
        ref = nr.estimate(xyz, r)
        out = c.estimate_normals(radius=r)
        _, nrm_dev = c.download()
        assert np.all(out["count"][inner] == k)
        assert np.all(np.abs(out["curvature"][inner] - 1.0 / 3.0) <= 64 * k * nr.EPS)
        _compare(out, nrm_dev, ref, vectors=False)           # edges and corners too; the lattice's eigenvalues tie
    c.close()


@pytest.mark.parametrize("viewpoint,orient,nz", [((0, 0, 10), nr.ORIENT_VIEWPOINT, 1.0), ((0, 0, 0), nr.ORIENT_NONE, 1.0),
                                                 ((0, 0, -10), nr.ORIENT_VIEWPOINT, -1.0)])
def test_exact_plane(gpu, viewpoint, orient, nz):
    xyz = nr.plane_lattice()
    c = _cloud(gpu, xyz, 0.1)
    out = c.estimate_normals(radius=0.1, orient=orient, viewpoint=viewpoint)
    _, nrm_dev = c.download()
    assert np.array_equal(nrm_dev, np.tile(np.array([0, 0, nz], np.float32), (xyz.shape[0], 1)))
    assert np.all(np.abs(out["curvature"]) <= 1e-15)
    assert np.array_equal(out["count"], nr.estimate(xyz, 0.1)["count"])
    c.close()


@pytest.mark.parametrize("scene", nr.degenerate_scenes(), ids=lambda s: s[0])
def test_degenerate(gpu, scene):
    name, xyz, r, min_nb, (est, few, deg), bare = scene
    ref = nr.estimate(xyz, r, min_neighbors=min_nb)
    ones = np.tile(np.array([0, 1, 0], np.float32), (xyz.shape[0], 1))      # whatever was stored is replaced
    c = _cloud(gpu, xyz, 0.1, nrm=ones)
    out = c.estimate_normals(radius=r, min_neighbors=min_nb)
    _, nrm_dev = c.download()
    i = out["info"]
    assert (i["num_estimated"], i["num_too_few"], i["num_degenerate"]) == (est, few, deg)
    assert np.all(nrm_dev[bare] == 0) and np.all(out["curvature"][bare] == 0)
    _compare(out, nrm_dev, ref)
    c.close()


def test_dense_brick(gpu):
    """12 000 points of a thin sheet inside ONE cell: dozens of tiles, 188 passes of 64 queries over the same leaf"""
    rng = np.random.default_rng(11)
    xyz = np.stack([rng.uniform(0.05, 0.45, 12000), rng.uniform(0.05, 0.45, 12000),
                    0.25 + rng.normal(0, 0.002, 12000)], axis=1).astype(np.float32)
    ref = nr.estimate(xyz, 0.08)
    assert ref["count"].max() > 1000
    c = _cloud(gpu, xyz, 0.5)
    assert c.info()["dims"] == [1, 1, 1]
    out = c.estimate_normals(radius=0.08)
    _, nrm_dev = c.download()
    _compare(out, nrm_dev, ref)
    _check_info(out["info"], ref, xyz.shape[0])
    assert out["info"]["pair_tests"] == 12000 * 12000
    c.close()


def test_grid_border_and_largest_radius(gpu):
    """odd cell dimensions (padded quads), queries in corner cells, the largest admissible reach: r = 8 cells"""
    rng = np.random.default_rng(12)
    xyz = (rng.random((3000, 3)) * np.array([1.1, 0.85, 0.6])).astype(np.float32)
    c = _cloud(gpu, xyz, 0.125)
    assert c.info()["dims"] == [9, 7, 5]
    ref = nr.estimate(xyz, 1.0)
    out = c.estimate_normals(radius=1.0)                   # 8 cells exactly: accepted
    _, nrm_dev = c.download()
    _compare(out, nrm_dev, ref)
    ref = nr.estimate(xyz, 0.1)
    out = c.estimate_normals(radius=0.1)
    _, nrm_dev = c.download()
    _compare(out, nrm_dev, ref)
    with pytest.raises(gpu.PcdError) as e:
        c.estimate_normals(radius=8.5 * 0.125)
    assert e.value.status == gpu.PCD_ERR_INVALID and "cell_size" in str(e.value) and "8.5" in str(e.value)
    c.close()


def test_only_missing(gpu):
    from pcdhip import synth
    xyz, given = synth.cloud_uniform(4000, seed=3, box=2.0)
    _, ref = nr.parity_ref("uniform", 0.25)
    has = np.arange(xyz.shape[0]) % 2 == 0
    start = np.where(has[:, None], given, np.float32(0)).astype(np.float32)
    c = _cloud(gpu, xyz, 0.1, nrm=start)
    out = c.estimate_normals(radius=0.25, only_missing=True)
    _, nrm_dev = c.download()
    assert np.array_equal(nrm_dev[has].view(np.uint32), start[has].view(np.uint32))      # bit-identical
    _compare(out, np.where(has[:, None], ref["normal"].astype(np.float32), nrm_dev), ref)  # counts / curvature: all rows
    _compare(out, nrm_dev, ref, rows=np.flatnonzero(~has))
    i = out["info"]
    assert i["num_kept"] == int(has.sum()) and i["num_estimated"] == int((ref["ok"] & ~has).sum())
    assert i["num_kept"] + i["num_estimated"] + i["num_too_few"] + i["num_degenerate"] == xyz.shape[0]
    c.close()


def _two_patches():
    """one horizontal patch (normal along y: ground for bundle_adjustment.cc:381) and one vertical"""
    rng = np.random.default_rng(21)
    g = (np.arange(40) - 20) * 0.04
    u, v = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    w = rng.normal(0, 0.002, (2, u.shape[0]))
    ground = np.stack([3.0 + u, 1.5 + w[0], 4.0 + v], axis=1)
    wall = np.stack([6.0 + w[1], 0.5 + u, 4.0 + v], axis=1)
    xyz = np.concatenate([ground, wall]).astype(np.float32)
    q = xyz[rng.integers(0, xyz.shape[0], 1500)].astype(np.float64) + rng.normal(0, 0.05, (1500, 3))
    return xyz, q


def test_end_to_end_association(gpu, oracle):
    """a cloud without normals associates nothing; after the estimation the association is the oracle's on the
    downloaded normals, field by field"""
    xyz, q = _two_patches()
    c = gpu.Cloud(xyz, np.zeros_like(xyz), raw_lidar_frame=False)
    before = c.associate(q, 1.5, gpu.GATE_MAPPER_LOCAL)
    assert np.all(before["type"] == 0)
    out = c.estimate_normals(radius=0.15)
    assert out["info"]["num_estimated"] == xyz.shape[0]
    _, nrm = c.download()
    got = c.associate(q, 1.5, gpu.GATE_MAPPER_LOCAL)
    idx, sq, found = oracle.nn_bruteforce(xyz, q)
    assert np.array_equal(got["nn_idx"], idx) and np.array_equal(got["nn_sqdist"].view(np.uint32), sq.view(np.uint32))
    out6, ok = oracle.search_nearest_neibor(xyz, nrm, idx, found)
    abcd, typ, dist, ang, d2p = oracle.associate(q, out6, ok, 1.5, 0)
    assert np.array_equal(got["type"], typ)
    assert (typ == gpu.LIDAR_ICP).sum() > 100 and (typ == gpu.LIDAR_ICP_GROUND).sum() > 100
    np.testing.assert_array_equal(got["lidar_xyz"][ok.astype(bool)], out6[ok.astype(bool), :3])
    np.testing.assert_allclose(got["abcd"], abcd, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(got["dist"], dist, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(got["angle"], ang, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(got["dist2plane"], d2p, rtol=1e-12, atol=1e-15)
    c.close()


def test_repeatability_and_device_outputs(gpu):
    import torch
    xyz, ref = nr.parity_ref("uniform", 0.25)
    c = _cloud(gpu, xyz, 0.1)
    a = c.estimate_normals(radius=0.25)
    na = c.download()[1]
    b = c.estimate_normals(radius=0.25)
    nb = c.download()[1]
    assert np.array_equal(na.view(np.uint32), nb.view(np.uint32))
    assert np.array_equal(a["count"], b["count"])
    assert np.array_equal(a["curvature"].view(np.uint64), b["curvature"].view(np.uint64))
    d_count = torch.zeros(xyz.shape[0], dtype=torch.int32, device="cuda")
    d_curv = torch.zeros(xyz.shape[0], dtype=torch.float64, device="cuda")
    c.estimate_normals_device(d_count, d_curv, radius=0.25, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_count.cpu().numpy().view(np.uint32), a["count"])
    assert np.array_equal(d_curv.cpu().numpy().view(np.uint64), a["curvature"].view(np.uint64))
    assert np.array_equal(c.download()[1].view(np.uint32), na.view(np.uint32))
    c.estimate_normals_device(None, None, radius=0.25)      # both outputs are optional
    torch.cuda.synchronize()
    assert np.array_equal(c.download()[1].view(np.uint32), na.view(np.uint32))
    c.close()


def test_guards(gpu, oracle):
    from pcdhip import synth
    xyz, nrm = synth.cloud_uniform(2000, seed=4, box=2.0)
    L = gpu.lib()
    # shards and strided handles: their neighbourhoods cross handle borders
    sh = gpu.ShardedCloud(xyz, nrm, [0, 0], raw_lidar_frame=False)
    L.pcd_cloud_shards_get.restype = C.c_void_p
    L.pcd_cloud_shards_get.argtypes = [C.c_void_p, C.c_int]
    o = gpu.normals_options()
    h = C.c_void_p(L.pcd_cloud_shards_get(sh._h, 0))
    assert L.pcd_cloud_estimate_normals(h, C.byref(o), None, None, None) == gpu.PCD_ERR_UNSUPPORTED
    assert L.pcd_cloud_estimate_normals_device(h, C.byref(o), None, None, None) == gpu.PCD_ERR_UNSUPPORTED
    assert b"download, then shard" in L.pcd_last_error()
    sh.close()
    strided = gpu.Cloud(xyz[::2], nrm[::2], raw_lidar_frame=False, index_stride=2)
    with pytest.raises(gpu.PcdError) as e:
        strided.estimate_normals()
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    strided.close()
    # bad options
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, cell_size=0.1)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(min_neighbors=-1), dict(orient=7), dict(radius=0.81)):
        with pytest.raises(gpu.PcdError) as e:
            c.estimate_normals(**kw)
        assert e.value.status == gpu.PCD_ERR_INVALID, kw
    assert L.pcd_cloud_estimate_normals(None, C.byref(o), None, None, None) == gpu.PCD_ERR_INVALID
    # nothing was touched: the stored normals are the given ones, and the handle still answers
    assert np.array_equal(c.download()[1], nrm)
    q = synth.queries(xyz, 500, seed=6, sigma=0.05, box=np.array([2.0, 2.0, 2.0]))
    idx, sq, found = c.nn(q)
    eidx, esq, _ = oracle.nn_bruteforce(xyz, q)
    assert np.array_equal(idx, eidx) and np.array_equal(sq.view(np.uint32), esq.view(np.uint32))
    c.estimate_normals(radius=0.2)
    idx, sq, found = c.nn(q)
    assert np.array_equal(idx, eidx)
    assert (c.associate(q, 1.5, gpu.GATE_MAPPER_LOCAL)["type"] != 0).sum() > 400
    c.close()
    # an empty cloud: OK, zero counts
    e0 = gpu.Cloud(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), raw_lidar_frame=False)
    out = e0.estimate_normals()
    assert out["count"].shape == (0,) and out["info"]["num_estimated"] == 0 and out["info"]["pair_tests"] == 0
    e0.close()


def test_capturing_stream_is_refused(gpu):
    """an eager entry point (scratch growth, one host synchronisation): refused inside a graph capture, untouched after"""
    import torch
    xyz, _ = nr.parity_ref("uniform", 0.25)
    c = _cloud(gpu, xyz, 0.1)
    c.estimate_normals(radius=0.25)
    before = c.download()[1]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                c.estimate_normals_device(None, None, radius=0.2, stream=side.cuda_stream)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
        c.estimate_normals_device(None, None, radius=0.25, stream=side.cuda_stream)
        side.synchronize()
    assert np.array_equal(c.download()[1].view(np.uint32), before.view(np.uint32))
    c.close()


def test_shim_estimates_missing_normals(gpu, tmp_path):
    subprocess.check_call(["make", "-s", "-C", PKG, "shim/test_normals"])
    r = subprocess.run([os.path.join(PKG, "shim", "test_normals"), str(tmp_path / "scan.ply")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

"""GPU parity of the voxel-grid downsampling (pcd_cloud_voxel_downsample, csrc/voxel.hip) against the numpy reference of
its definition (tests/voxel_ref.py).

Tolerances, computed from the reference's own values, never from device output (k = rows of the voxel):
  partition   row_voxel, counts and output order: exact;
  position    per component |c_dev - f32(c_ref)| <= 2^-23 |c_ref| + 2 k 2^-53 max_j |p_j|: one float rounding boundary
              plus a reordered fp64 sum and the divide;
  normal      voxels with |s_ref| >= 1e-3 k max_j |n_j|: |n_dev - f32(s_ref / |s_ref|)| <= 2^-23 + 8 k 2^-53 max_j |n_j| /
              |s_ref|; voxels with s_ref = 0 exactly (a two-row cancellation, all-zero normals): zeros; the rest: finite,
              and zero or | |n| - 1 | <= 2^-22.  The share of "the rest" is asserted <= 1 % wherever vectors are compared
              (tests/test_voxel_cpu.py shows the clouds keep to that on their own).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import normals_ref as nr
from tests import voxel_ref as vr

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
INFO_COUNTS = ("num_input", "num_voxels", "num_output", "num_dropped_rows")


def _downsample(gpu, xyz, nrm, leaf, min_points=0, cell_size=0.0):
    """(out xyz, out nrm, info, row_voxel) of one call on a fresh handle"""
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    out, info, rv = c.voxel_downsample(leaf, min_points=min_points, cell_size=cell_size, want_map=True)
    assert len(out) == info["num_output"]
    p, q = out.download()
    out.close()
    c.close()
    return p, q, info, rv


def _check_info(info, ref):
    for k in INFO_COUNTS:
        assert info[k] == ref[k], (k, info[k], ref[k])
    assert info["max_points_per_voxel"] == ref["max_points"]
    assert info["min_b"] == ref["min_b"] and info["dims"] == ref["dims"]
    assert info["ms"] > 0 and info["build_ms"] > 0


def _compare(p, q, info, rv, ref, vectors=True):
    """device rows, info and map against the reference (its kept voxels, in key order)"""
    _check_info(info, ref)
    assert np.array_equal(rv, ref["row_voxel"])
    keep = ref["keep"]
    assert p.shape[0] == int(keep.sum())
    # counts per output row, recovered from the device's own map
    got_counts = np.bincount(rv[rv != vr.NONE].astype(np.int64), minlength=p.shape[0])
    assert np.array_equal(got_counts, ref["counts"][keep])
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(q))
    dp = np.abs(p.astype(np.float64) - ref["pos32"][keep].astype(np.float64))
    tol_p = vr.pos_tol(ref)[keep]
    print("position: max |d| / tol = %.3g over %d voxels" % (float(np.max(dp / np.maximum(tol_p, 1e-300), initial=0.0)),
                                                             p.shape[0]))
    assert np.all(dp <= tol_p)
    strong, zero, rest = (m[keep] for m in vr.normal_classes(ref))
    assert np.all(q[zero] == 0)
    qn = np.linalg.norm(q.astype(np.float64), axis=1)
    assert np.all((qn[rest] == 0) | (np.abs(qn[rest] - 1.0) <= 2.0 ** -22))
    assert np.all(np.abs(qn[strong] - 1.0) <= 2.0 ** -22)
    if not vectors:
        return
    assert rest.sum() <= 0.01 * max(rest.size, 1)
    dn = np.abs(q.astype(np.float64) - ref["nrm32"][keep].astype(np.float64)).max(axis=1)
    tol_n = vr.normal_tol(ref)[keep]
    print("normals: max err / tol = %.3g over %d voxels" % (float(np.max(dn[strong] / tol_n[strong], initial=0.0)),
                                                            int(strong.sum())))
    assert np.all(dn[strong] <= tol_n[strong])


# ------------------------------------------------------------------------------------------------ 1. parity ----
@pytest.mark.parametrize("name", ["planes", "uniform"])
@pytest.mark.parametrize("leaf", vr.PARITY_LEAVES, ids=str)
def test_parity(gpu, name, leaf):
    xyz, nrm, ref = vr.parity_ref(name, leaf)
    _compare(*_downsample(gpu, xyz, nrm, leaf), ref)


# ------------------------------------------------------------------------------------- 2. faces and signs ----
@pytest.mark.parametrize("spacing", [0.125, 0.05])
def test_lattice_on_voxel_faces(gpu, spacing):
    """spacing = leaf: every point on a face.  0.125 is exact; at 0.05 the float product decides the voxel"""
    xyz = vr.lattice(spacing)
    nrm = vr.unit_normals(xyz.shape[0], 3)
    ref = vr.voxelize(xyz, nrm, spacing)
    if spacing == 0.125:
        assert ref["num_voxels"] == xyz.shape[0] and ref["min_b"] == [-3, -3, -3]
    p, q, info, rv = _downsample(gpu, xyz, nrm, spacing)
    _compare(p, q, info, rv, ref)


def test_cloud_straddling_the_origin(gpu):
    """floor, not truncation: truncation would merge the voxels -1 and 0 of every axis"""
    xyz, nrm = vr.straddle_cloud()
    ref = vr.voxelize(xyz, nrm, 0.05)
    assert ref["min_b"] == [-6, -6, -6] and ref["dims"] == [12, 12, 12]
    p, q, info, rv = _downsample(gpu, xyz, nrm, 0.05)
    _compare(p, q, info, rv, ref)
    assert rv[-3] != rv[-2]                        # (-0.01, -0.01, -0.01) and the origin are different voxels


# --------------------------------------------------------------------------------------- 3. segment lengths ----
def test_segment_lengths(gpu):
    xyz, nrm = vr.segments_cloud()
    ref = vr.voxelize(xyz, nrm, 1.0)
    assert tuple(ref["counts"]) == vr.SEGMENT_LENGTHS
    p, q, info, rv = _downsample(gpu, xyz, nrm, 1.0)
    _compare(p, q, info, rv, ref)
    assert info["max_points_per_voxel"] == 20000


# ---------------------------------------------------------------------------------------------- 4. extremes ----
def test_extremes(gpu):
    xyz, nrm = vr.uniform_cloud()
    # one voxel for the whole cloud
    ref = vr.voxelize(xyz, nrm, 16.0)
    assert ref["num_voxels"] == 1
    _compare(*_downsample(gpu, xyz, nrm, 16.0), ref)
    # every row in its own voxel
    lat = vr.lattice(0.125)
    ln = vr.unit_normals(lat.shape[0], 4)
    ref = vr.voxelize(lat, ln, 0.0625)
    assert ref["num_voxels"] == lat.shape[0]
    p, q, info, rv = _downsample(gpu, lat, ln, 0.0625)
    _compare(p, q, info, rv, ref)
    assert np.array_equal(p[rv], lat)              # a voxel of one row is that row
    # an empty cloud, and a cloud of Inf rows only
    for cloud in (np.zeros((0, 3), np.float32), np.full((5, 3), np.inf, np.float32)):
        p, q, info, rv = _downsample(gpu, cloud, np.zeros_like(cloud), 0.05)
        assert p.shape == (0, 3) and all(info[k] == 0 for k in INFO_COUNTS) and info["max_points_per_voxel"] == 0
        assert rv.shape[0] == cloud.shape[0] and np.all(rv == vr.NONE)
    # Inf rows mixed in
    mixed = xyz.copy()
    bad = np.arange(7, mixed.shape[0], 97)
    mixed[bad, np.arange(bad.size) % 3] = np.array([np.inf, -np.inf], np.float32)[np.arange(bad.size) % 2]
    ref = vr.voxelize(mixed, nrm, 0.2)
    p, q, info, rv = _downsample(gpu, mixed, nrm, 0.2)
    _compare(p, q, info, rv, ref)
    assert np.all(rv[bad] == vr.NONE) and info["num_input"] == mixed.shape[0] - bad.size


def test_output_handle_of_an_empty_source_answers(gpu):
    c = gpu.Cloud(np.full((3, 3), np.inf, np.float32), np.zeros((3, 3), np.float32), raw_lidar_frame=False)
    out, info = c.voxel_downsample(0.05)
    assert len(out) == 0 and out.info()["num_indexed"] == 0
    idx, sq, found = out.nn(np.zeros((4, 3)))
    assert not found.any()
    out.close()
    c.close()


# -------------------------------------------------------------------------------------------------- 5. keys ----
def test_keys_above_32_bits_and_refusals(gpu):
    xyz, nrm = vr.sparse_cloud()
    ref = vr.voxelize(xyz, nrm, 0.01)
    assert max(ref["keys"]) > 2 ** 32
    _compare(*_downsample(gpu, xyz, nrm, 0.01), ref)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    L = gpu.lib()
    for leaf in (1e-6, (1e-8, 1.0, 1.0)):          # 2^63 voxels or more; one axis alone leaves the int32 range
        with pytest.raises(ValueError):
            vr.voxelize(xyz, nrm, leaf)
        o = gpu.voxel_options(leaf)
        h = C.c_void_p(0xDEAD)
        assert L.pcd_cloud_voxel_downsample(c._h, C.byref(o), None, C.byref(h), None) == gpu.PCD_ERR_INVALID
        assert h.value is None                     # *out is NULL
    # the source is still usable
    _compare(*_run_on(c, 0.01), ref)
    c.close()


def _run_on(c, leaf, **kw):
    out, info, rv = c.voxel_downsample(leaf, want_map=True, **kw)
    p, q = out.download()
    out.close()
    return p, q, info, rv


# -------------------------------------------------------------------------------------------- 6. min_points ----
@pytest.mark.parametrize("min_points", [0, 1, 2, 5])
def test_min_points(gpu, min_points):
    xyz, nrm = vr.planes_cloud()
    ref = vr.voxelize(xyz, nrm, 0.1, min_points=min_points)
    p, q, info, rv = _downsample(gpu, xyz, nrm, 0.1, min_points=min_points)
    _compare(p, q, info, rv, ref)
    full = vr.voxelize(xyz, nrm, 0.1)
    dropped_rows = np.flatnonzero(full["counts"][full["row_vid"]] < min_points)
    assert np.all(rv[dropped_rows] == vr.NONE) and info["num_dropped_rows"] == dropped_rows.size
    kept = rv[rv != vr.NONE]
    assert info["num_input"] == kept.size + info["num_dropped_rows"]
    assert info["num_output"] == (np.unique(kept).size if kept.size else 0) <= info["num_voxels"] == full["num_voxels"]
    if min_points >= 2:
        assert 0 < info["num_output"] < info["num_voxels"]
    # survivors stay in key order: their keys, read through the map, ascend with the output row
    first_row = np.full(info["num_output"], -1, np.int64)
    first_row[kept[::-1]] = np.flatnonzero(rv != vr.NONE)[::-1]
    keys = np.asarray(full["keys"], dtype=object)[full["row_vid"][first_row]]
    assert all(a < b for a, b in zip(keys, keys[1:]))


# ----------------------------------------------------------------------------------------------- 7. normals ----
def test_normals(gpu):
    xyz, nrm = vr.mixed_normals_cloud()
    ref = vr.voxelize(xyz, nrm, 1.0)
    strong, zero, rest = vr.normal_classes(ref)
    assert zero.sum() == 43 and strong.sum() >= 250
    p, q, info, rv = _downsample(gpu, xyz, nrm, 1.0)
    _compare(p, q, info, rv, ref)
    assert np.all(q[:40] == 0)                     # the opposed pairs
    # a cloud without normals stays without them
    p, q, info, rv = _downsample(gpu, xyz, np.zeros_like(nrm), 1.0)
    assert np.all(q == 0)
    _compare(p, q, info, rv, vr.voxelize(xyz, np.zeros_like(nrm), 1.0))


# ---------------------------------------------------------------------------------------- 8. bitwise repeat ----
def test_bitwise_repeat(gpu):
    from pcdhip import synth
    xyz, nrm = vr.segments_cloud()
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    a = _run_on(c, 1.0)
    b = _run_on(c, 1.0)
    c.nn(synth.queries(xyz, 500, seed=2))          # an unrelated call on the source in between
    c.estimate_normals(radius=0.05)                # (rewrites the source's normals: the positions must not move)
    d = _run_on(c, 1.0)
    for x, y in ((a, b), (a, d)):
        assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[3], y[3])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    c.close()
    xyz, nrm, _ = vr.parity_ref("planes", 0.05)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    a = _run_on(c, 0.05)
    c.nn(synth.queries(xyz, 500, seed=2))
    b = _run_on(c, 0.05)
    for k in (0, 1):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
    assert np.array_equal(a[3], b[3])
    c.close()


def test_device_form_gives_the_same_rows_and_map(gpu):
    import torch
    xyz, nrm, ref = vr.parity_ref("planes", (0.05, 0.1, 0.2))
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    host = _run_on(c, (0.05, 0.1, 0.2))
    d_map = torch.zeros(xyz.shape[0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out, info = c.voxel_downsample_device(d_map, (0.05, 0.1, 0.2), stream=side.cuda_stream)
    p, q = out.download()
    assert np.array_equal(d_map.cpu().numpy().view(np.uint32), host[3])
    assert np.array_equal(p.view(np.uint32), host[0].view(np.uint32))
    assert np.array_equal(q.view(np.uint32), host[1].view(np.uint32))
    _check_info(info, ref)
    out.close()
    out, info = c.voxel_downsample_device(None, (0.05, 0.1, 0.2))      # the map is optional
    assert np.array_equal(out.download()[0].view(np.uint32), host[0].view(np.uint32))
    out.close()
    c.close()


# ------------------------------------------------------------------------------- 9. the output is a real handle ----
def _nn_bruteforce(rows, q):
    """FLANN L2_Simple in float32 over `rows`, ties to the lowest index"""
    q32 = q.astype(np.float32)
    idx = np.empty(q.shape[0], np.uint32)
    sq = np.empty(q.shape[0], np.float32)
    for s in range(0, q.shape[0], 256):
        d = q32[s:s + 256, None, :] - rows[None, :, :]
        d2 = d[:, :, 0] * d[:, :, 0]
        d2 = d2 + d[:, :, 1] * d[:, :, 1]
        d2 = d2 + d[:, :, 2] * d[:, :, 2]
        i = np.argmin(d2, axis=1)                  # first of equal minima
        idx[s:s + 256] = i
        sq[s:s + 256] = d2[np.arange(i.size), i]
    return idx, sq


def test_output_is_a_real_handle(gpu):
    from pcdhip import synth
    from tests.test_normals_gpu import _compare as compare_normals
    xyz, nrm = vr.planes_cloud()
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    out, info = c.voxel_downsample(0.1, cell_size=0.2)
    assert abs(out.info()["cell_size"] - np.float32(0.2)) < 1e-9 and out.info()["num_indexed"] == len(out)
    rows, _ = out.download()
    q = synth.queries(rows, 2000, seed=8)
    q[:50] = rows[:50].astype(np.float64)          # exact hits
    q[50:60] = (rows[100:110].astype(np.float64) + rows[101:111].astype(np.float64)) / 2
    idx, sq, found = out.nn(q)
    eidx, esq = _nn_bruteforce(rows, q)
    assert found.all() and np.array_equal(idx, eidx) and np.array_equal(sq.view(np.uint32), esq.view(np.uint32))
    ref = nr.estimate(rows, 0.3)
    est = out.estimate_normals(radius=0.3)
    compare_normals(est, out.download()[1], ref)
    out.close()
    c.close()


# --------------------------------------------------------------------------------------- 10. source untouched ----
def test_source_untouched(gpu):
    from pcdhip import synth
    xyz, nrm = vr.planes_cloud()
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    q = synth.queries(xyz, 2000, seed=6)
    before = c.download(), c.nn(q), c.info()
    for leaf, mp in ((0.05, 0), (1.0, 3)):
        out, _ = c.voxel_downsample(leaf, min_points=mp)
        out.close()
    after = c.download(), c.nn(q), c.info()
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert before[2] == after[2] and len(c) == xyz.shape[0]
    c.close()


# ---------------------------------------------------------------------------------------------- 11. refusals ----
def test_refusals(gpu):
    xyz, nrm = vr.uniform_cloud()
    L = gpu.lib()
    o = gpu.voxel_options(0.1)
    sh = gpu.ShardedCloud(xyz, nrm, [0, 0], raw_lidar_frame=False)
    L.pcd_cloud_shards_get.restype = C.c_void_p
    L.pcd_cloud_shards_get.argtypes = [C.c_void_p, C.c_int]
    hs = C.c_void_p(L.pcd_cloud_shards_get(sh._h, 0))
    h = C.c_void_p(0xDEAD)
    assert L.pcd_cloud_voxel_downsample(hs, C.byref(o), None, C.byref(h), None) == gpu.PCD_ERR_UNSUPPORTED
    assert h.value is None and b"download, then shard" in L.pcd_last_error()
    assert L.pcd_cloud_voxel_downsample_device(hs, C.byref(o), None, None, C.byref(h), None) == gpu.PCD_ERR_UNSUPPORTED
    sh.close()
    strided = gpu.Cloud(xyz[::2], nrm[::2], raw_lidar_frame=False, index_stride=2)
    with pytest.raises(gpu.PcdError) as e:
        strided.voxel_downsample(0.1)
    assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    strided.close()
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    for kw in (dict(leaf=0.0), dict(leaf=-0.05), dict(leaf=float("nan")), dict(leaf=float("inf")),
               dict(leaf=(0.05, 0.0, 0.05)), dict(leaf=0.05, min_points=-1)):
        with pytest.raises(gpu.PcdError) as e:
            c.voxel_downsample(**kw)
        assert e.value.status == gpu.PCD_ERR_INVALID, kw
    assert L.pcd_cloud_voxel_downsample(None, C.byref(o), None, C.byref(h), None) == gpu.PCD_ERR_INVALID
    assert L.pcd_cloud_voxel_downsample(c._h, C.byref(o), None, None, None) == gpu.PCD_ERR_INVALID
    # NULL options are the defaults (leaf 0.05)
    assert L.pcd_cloud_voxel_downsample(c._h, None, None, C.byref(h), None) == gpu.PCD_OK
    d = gpu.Cloud._from_handle(h)
    assert len(d) == vr.voxelize(xyz, nrm, 0.05)["num_output"]
    d.close()
    c.close()


def test_capturing_stream_is_refused(gpu):
    """an eager entry point (allocations, host synchronisations): refused inside a graph capture, the handle works after"""
    import torch
    xyz, nrm, ref = vr.parity_ref("uniform", 1.0)
    c = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                c.voxel_downsample_device(None, 1.0, stream=side.cuda_stream)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
        out, info = c.voxel_downsample_device(None, 1.0, stream=side.cuda_stream)
        side.synchronize()
    _check_info(info, ref)
    out.close()
    _compare(*_run_on(c, 1.0), ref)
    c.close()


# -------------------------------------------------------------------------------------------------- 12. shim ----
def test_shim_downsample_then_normals(gpu, tmp_path):
    subprocess.check_call(["make", "-s", "-C", PKG, "shim/test_voxel"])
    r = subprocess.run([os.path.join(PKG, "shim", "test_voxel"), str(tmp_path / "scan.ply")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

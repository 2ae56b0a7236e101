"""Plain numpy restatement of the cloud build (csrc/cloud.hip, csrc/grid.h) and of the shard split and refine
predicate (csrc/shards.hip, k_prepare<kPrepRefine> in csrc/nn.hip).  No device code: tests/test_cloud_ref_cpu.py pins these
functions on hand-computed cases, the GPU tests compare the library with them bit for bit.

Every function takes the cloud in the HANDLE's frame: rows already transformed and NaN-filtered, float32."""
import math

import numpy as np

MAX_CELLS = 1 << 26          # cloud.hip kMaxCells
KEY_CAP = 2097151            # shards.hip: 21 bits per axis of the sort key
FLT_MAX_BITS = 0x7F7FFFFF    # nn.hip kKeyInit >> 32: the distance a key without a result carries into the refine


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _qf(q):
    """queries are double in the ABI and rounded to float first (ply.cc:92); past the float range they are Inf"""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(q, np.float64).reshape(-1, 3).astype(np.float32)


def finite_rows(xyz):
    return np.isfinite(_f32(xyz)).all(axis=1)


def _ordered(a):
    """float32 -> int32 in the order of the floats, -0.0 below +0.0 (cloud.hip f2ord)"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7FFFFFFF))


def _unordered(i):
    i = np.asarray(i, np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(np.float32)


def tight_box(xyz):
    """(m, lo, hi): number of finite rows and their float32 minimum / maximum per axis, zeros when there is none.
    Signed zeros are ordered (-0.0 < +0.0) as the device's integer atomics order them, so the bits are defined."""
    x = _f32(xyz)
    fin = finite_rows(x)
    m = int(fin.sum())
    if m == 0:
        return 0, np.zeros(3, np.float32), np.zeros(3, np.float32)
    o = _ordered(x[fin])
    return m, _unordered(o.min(axis=0)), _unordered(o.max(axis=0))


def grid_dims(lo, hi, h):
    e = np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)
    c = np.floor(e / np.float64(np.float32(h))).astype(np.int64) + 1
    return np.maximum(c, 1)


def cell_coords(xyz, origin, h, dims):
    """the binning of grid.h in float32, one operation at a time; finite rows only"""
    x = _f32(xyz)
    o = np.asarray(origin, np.float32)
    inv_h = np.float32(1) / np.float32(h)
    t = np.floor(((x - o).astype(np.float32) * inv_h).astype(np.float32))
    d = np.asarray(dims, np.int64)
    return np.clip(t.astype(np.float64), 0, (d - 1).astype(np.float64)).astype(np.int64)


def grid_info(xyz, h):
    """what pcd_cloud_get_info must report for a grid of cell size h over `xyz`"""
    x = _f32(xyz)
    m, lo, hi = tight_box(x)
    dims = grid_dims(lo, hi, h)
    occupied = 0
    if m:
        c = cell_coords(x[finite_rows(x)], lo, h, dims)
        occupied = int(np.unique((c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]).size)
    return dict(len=x.shape[0], num_indexed=m, bbox_lo=lo, bbox_hi=hi, origin=lo.copy(),
                dims=[int(v) for v in dims], block_dims=[int((v + 3) // 4) for v in dims], occupied_cells=occupied)


def budget_min_cell(ext):
    """smallest cell edge the cell budget allows (cloud.hip min_h_for_budget), double"""
    h = np.cbrt((ext[0] + 1e-3) * (ext[1] + 1e-3) * (ext[2] + 1e-3) / float(MAX_CELLS))
    for _ in range(64):
        cells = (math.floor(ext[0] / h) + 1.0) * (math.floor(ext[1] / h) + 1.0) * (math.floor(ext[2] / h) + 1.0)
        if cells <= float(MAX_CELLS):
            break
        h *= 1.05
    return float(h)


def effective_cell_size(lo, hi, m, user_h):
    """the cell size choose_cell_size (cloud.hip) settles on for a user value > 0, as float32"""
    assert user_h > 0
    user_h = np.float32(user_h)
    ext = [float(np.float64(np.float32(hi[d])) - np.float64(np.float32(lo[d]))) for d in range(3)]
    maxext = max(ext)
    if m == 0 or maxext <= 0:
        return user_h
    hmin = max(budget_min_cell(ext), 1e-6 * max(maxext, 1e-3))
    return np.float32(max(float(user_h), hmin))


def shard_keys(xyz):
    """sort key of pcd_cloud_create_sharded: 1 m cells relative to the finite minimum, z-major, 21 bits per axis;
    rows with a non-finite coordinate get key 0"""
    x = _f32(xyz).astype(np.float64)
    fin = np.isfinite(x).all(axis=1)
    lo = x[fin].min(axis=0) if fin.any() else np.zeros(3)
    c = np.zeros(x.shape, np.uint64)
    if fin.any():
        c[fin] = np.minimum(np.floor(x[fin] - lo), float(KEY_CAP)).astype(np.uint64)
    return (c[:, 2] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 0]


def shard_split(xyz, ndev):
    """(order, cuts, boxes): shard s holds rows order[cuts[s]:cuts[s + 1]] in that order, under their ORIGINAL
    indices; boxes[s] = (lo, hi) of its finite rows in float32, (+inf, -inf) for a shard without one"""
    x = _f32(xyz)
    m = x.shape[0]
    order = np.argsort(shard_keys(x), kind="stable").astype(np.uint32)
    cuts = [(m * s) // ndev for s in range(ndev + 1)]
    boxes = np.empty((ndev, 6), np.float32)
    for s in range(ndev):
        k, lo, hi = tight_box(x[order[cuts[s]:cuts[s + 1]]])
        boxes[s, :3] = lo if k else np.inf
        boxes[s, 3:] = hi if k else -np.inf
    return order, cuts, boxes


def _l2_simple3(q, p):
    d = (q - p).astype(np.float32)
    r = (d[:, 0] * d[:, 0]).astype(np.float32)
    r = (r + (d[:, 1] * d[:, 1]).astype(np.float32)).astype(np.float32)
    return (r + (d[:, 2] * d[:, 2]).astype(np.float32)).astype(np.float32)


def box_distance(q, box_lo, box_hi):
    """float32 squared distance from float32(q) to its clamp into the box, FLANN order ((dx*dx)+dy*dy)+dz*dz"""
    qf = _qf(q)
    lo, hi = np.asarray(box_lo, np.float32), np.asarray(box_hi, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return _l2_simple3(qf, np.fmin(np.fmax(qf, lo), hi))


def point_distance(q, p):
    qf = _qf(q)
    with np.errstate(invalid="ignore", over="ignore"):
        return _l2_simple3(qf, _f32(p))


def refine_active(q, box_lo, box_hi, incoming_sqdist_bits):
    """k_prepare<kPrepRefine>: a finite query stays active in a shard iff the float distance to the shard's box does not
    exceed the distance it comes in with (equality kept: a lower index at the same distance may live there)"""
    qf = _qf(q)
    inc = np.ascontiguousarray(incoming_sqdist_bits, np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(qf).all(axis=1) & (box_distance(q, box_lo, box_hi) <= inc)

"""Which rows of an association become LiDAR terms of a BA handle (pcd_ba_set_lidar_device, include/pcdhip.h), in numpy.

A restatement of the rule, nothing else: row q becomes a term iff its type is not 0 and none of its four abcd values
is NaN (an Inf passes); an unselected row counts as type 0; the term's point is point[q] (row q is point q without a
point array), its weight is weight[type]; terms keep the order of the rows."""
import numpy as np


def terms(type, abcd, weight, point=None, lidar_xyz=None, select=None):
    """dict of lidar_point [L] int32, lidar_abcd [L][4], lidar_weight [L] (the arguments of a fresh handle), type [L]
    uint8, lidar_xyz [L][3] (zeros without lidar_xyz) and rows [L] (the row of every term)"""
    t = np.asarray(type, np.uint8).copy()
    Q = t.shape[0]
    abcd = np.asarray(abcd, np.float64).reshape(Q, 4)
    if select is not None:
        t[np.asarray(select).astype(bool) == 0] = 0
    keep = (t != 0) & ~np.isnan(abcd).any(axis=1)
    pt = np.arange(Q, dtype=np.int32) if point is None else np.asarray(point, np.int32)
    xyz = np.zeros((Q, 3)) if lidar_xyz is None else np.asarray(lidar_xyz, np.float64).reshape(Q, 3)
    w = np.asarray(weight, np.float64)
    return dict(lidar_point=pt[keep], lidar_abcd=abcd[keep], lidar_weight=w[t[keep]], type=t[keep], lidar_xyz=xyz[keep],
                rows=np.flatnonzero(keep))


def terms_loop(type, abcd, weight, point=None, lidar_xyz=None, select=None):
    """the same, one row at a time"""
    lp, la, lw, lt, lx, rows = [], [], [], [], [], []
    for q in range(len(type)):
        t = int(type[q])
        if select is not None and not select[q]:
            t = 0
        if t == 0:
            continue
        if any(v != v for v in abcd[q]):
            continue
        lp.append(q if point is None else int(point[q]))
        la.append([float(v) for v in abcd[q]])
        lw.append(float(weight[t]))
        lt.append(t)
        lx.append([0.0, 0.0, 0.0] if lidar_xyz is None else [float(v) for v in lidar_xyz[q]])
        rows.append(q)
    return dict(lidar_point=np.array(lp, np.int32), lidar_abcd=np.array(la, np.float64).reshape(-1, 4),
                lidar_weight=np.array(lw, np.float64), type=np.array(lt, np.uint8),
                lidar_xyz=np.array(lx, np.float64).reshape(-1, 3), rows=np.array(rows, np.int64))


def fresh_args(scene, t):
    """the scene with the term list t in place of its own LiDAR terms"""
    kw = {k: v for k, v in scene.items() if k not in ("lidar_point", "lidar_abcd", "lidar_weight")}
    if len(t["lidar_point"]):
        kw.update(lidar_point=t["lidar_point"], lidar_abcd=t["lidar_abcd"], lidar_weight=t["lidar_weight"])
    return kw


def same_bits(a, b):
    """np.array_equal on the bit patterns: equal shapes and equal bytes (a NaN equals the same NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8),
                                                                         b.reshape(-1).view(np.uint8))

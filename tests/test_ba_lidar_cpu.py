"""What of the device re-association of a handle's LiDAR terms can be checked without a GPU (pcd_ba_set_lidar_device,
pcd_ba_get_lidar, pcd_ba_lidar_device, pcd_ba_assoc_opts_default, pcd_ba_associate_lidar_device): the symbols, the
documented defaults, the argument checks that come before any device is touched, and the numpy restatement of the term
rule (tests/ba_lidar_ref.py) against a literal per-row loop.  A real handle cannot exist here, so every call passes a
NULL handle: PCD_ERR_INVALID with the message of the check that fired, never a crash."""
import ctypes as C

import numpy as np

from tests import ba_lidar_ref as lr

NEW_SYMBOLS = ["pcd_ba_set_lidar_device", "pcd_ba_get_lidar", "pcd_ba_lidar_device", "pcd_ba_assoc_opts_default",
               "pcd_ba_associate_lidar_device"]


def test_new_symbols_declared_and_exported(pcdhip):
    from tests.test_abi import _declared_symbols
    declared = _declared_symbols()
    lib = pcdhip.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and s in pcdhip.ABI_SYMBOLS and hasattr(lib, s), s


def test_assoc_opts_default(pcdhip):
    o = pcdhip.BAAssocOpts()
    C.memset(C.byref(o), 0xAB, C.sizeof(o))
    pcdhip.lib().pcd_ba_assoc_opts_default(C.byref(o))
    assert o.gate_mode == pcdhip.GATE_MAPPER_GLOBAL == 1
    assert (o.icp_weight, o.icp_ground_weight) == (100.0, 1000.0)          # shim/ba_problem.h:71-72
    assert o.d_max_range is None and o.d_select is None and o.max_range_count == 0
    assert list(o.reserved) == [0] * 8
    pcdhip.lib().pcd_ba_assoc_opts_default(None)                           # tolerated, as the other *_default are not asked to be
    # the struct is the header's: 4 (+4) + 8 + 8 + 8 + 8 + 8 + 32
    assert C.sizeof(pcdhip.BAAssocOpts) == 80 and C.sizeof(pcdhip.BAAssocInfo) == 48


def _err(pcdhip):
    return pcdhip.lib().pcd_last_error().decode()


def test_argument_checks_return_invalid(pcdhip):
    L = pcdhip.lib()
    o = pcdhip.BAAssocOpts()
    L.pcd_ba_assoc_opts_default(C.byref(o))
    info = pcdhip.BAAssocInfo()
    # an otherwise valid opts, a NULL handle
    assert L.pcd_ba_associate_lidar_device(None, None, C.byref(o), None, C.byref(info)) == pcdhip.PCD_ERR_INVALID
    assert "null handle" in _err(pcdhip)
    assert info.num_terms == 0 and info.num_queries == 0
    assert L.pcd_ba_associate_lidar_device(None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
    assert "null options" in _err(pcdhip)
    for bad in (3, -1, 7 | pcdhip.GATE_BOUNDED_SEARCH, 0x200):
        o.gate_mode = bad
        assert L.pcd_ba_associate_lidar_device(None, None, C.byref(o), None, None) == pcdhip.PCD_ERR_INVALID
        assert "gate_mode" in _err(pcdhip), bad
    for ok in (0, 1, 2, 2 | pcdhip.GATE_BOUNDED_SEARCH):                   # a valid mode gets as far as the handle check
        o.gate_mode = ok
        assert L.pcd_ba_associate_lidar_device(None, None, C.byref(o), None, None) == pcdhip.PCD_ERR_INVALID
        assert "null handle" in _err(pcdhip), ok
    w = (C.c_double * 4)(0, 100, 1000, 1)
    n = C.c_uint64(77)
    assert L.pcd_ba_set_lidar_device(None, 0, None, None, None, None, w, None, C.byref(n)) == pcdhip.PCD_ERR_INVALID
    assert "null handle" in _err(pcdhip) and n.value == 77
    assert L.pcd_ba_get_lidar(None, C.byref(n), None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
    assert L.pcd_ba_lidar_device(None, C.byref(n), None, None, None, None, None) == pcdhip.PCD_ERR_INVALID
    assert n.value == 77


def test_reference_agrees_with_a_per_row_loop():
    rng = np.random.default_rng(20)
    Q, P = 200, 37
    typ = rng.integers(0, 4, Q).astype(np.uint8)
    abcd = rng.normal(size=(Q, 4))
    for k in range(4):
        abcd[rng.choice(Q, 6, replace=False), k] = np.nan
    abcd[rng.choice(Q, 5, replace=False), 3] = np.inf
    abcd[rng.choice(Q, 3, replace=False), 0] = -np.inf
    point = rng.integers(0, P, Q).astype(np.int32)
    xyz = rng.normal(size=(Q, 3))
    select = (rng.random(Q) < 0.7).astype(np.uint8)
    weight = np.array([np.nan, 100.0, 1000.0, 1.0])
    for kw in (dict(point=point, lidar_xyz=xyz), dict(point=point), dict(lidar_xyz=xyz, select=select),
               dict(point=point, lidar_xyz=xyz, select=select), {}):
        a, b = lr.terms(typ, abcd, weight, **kw), lr.terms_loop(typ, abcd, weight, **kw)
        assert 0 < len(a["rows"]) < Q
        for k in a:
            assert lr.same_bits(a[k], b[k].astype(a[k].dtype)), (k, kw)
        assert np.isinf(a["lidar_abcd"]).any() and not np.isnan(a["lidar_abcd"]).any()
        assert not np.isnan(a["lidar_weight"]).any()
        assert (np.diff(a["rows"]) > 0).all()
    # the edge shapes
    for Q in (0, 1):
        a = lr.terms(typ[:Q], abcd[:Q], weight)
        b = lr.terms_loop(typ[:Q], abcd[:Q], weight)
        for k in a:
            assert lr.same_bits(a[k], b[k].astype(a[k].dtype)), (k, Q)

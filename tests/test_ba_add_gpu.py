"""Observations and points added to a live BA handle on the device (pcd_ba_add_observations_device).

The contract is equality with a FRESH handle built from the concatenated description (tests/ba_add_ref.
fresh_args_after_add): every result of tests/test_ba_filter_gpu.all_results -- evaluate with every output, both block
routes, the Schur blocks, both solves, the filters, the co-visibility structure, get_lidar -- bit for bit.  There is no
tolerance anywhere.

Shapes: the scenes of tests/test_ba_lidar_gpu (P = 65 / 130: two and three 64-track slices), track scenes cut so that P
crosses a slice edge (60 -> 64, 64 -> 65, 64 -> 128), a two-image scene whose image 0 crosses the kImgSeg = 1024 segment
edge, and both sides of the sizes at which rocPRIM's radix sort of the new rows changes algorithm (one block up to 1024
rows, merge sort up to 2^20, Onesweep above), and one handle taken through the removal, the addition and
set_lidar_device in turn (three images, one constant; P 70 -> 140 across a slice edge; through L = 0), each rebuild
working in the buffers the others retired."""
import os
import subprocess

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_add_ref as ar
from tests import ba_filter_ref as fr
from tests import ba_lidar_ref as lr
from tests import ba_schur_ref as sr
from tests import test_ba_filter_gpu as fg
from tests import test_ba_lidar_gpu as bl
from tests import test_ba_load_order_gpu as lo

pytestmark = pytest.mark.gpu
WEIGHT = bl.WEIGHT
_CACHE = {}


def full_scene(oracle, cams):
    s, many = bl.scene(oracle, cams)
    return dict(s, **many)


def rows_of(add):
    return add["obs_image"], add["obs_point"], add["obs_xy"], add.get("new_points")


def check_added(gpu, a, desc, add, meta=None, solves=True):
    """add on the live handle `a` (whose description is `desc`, at desc's parameters; its set_lidar_device rows' meta in
    `meta`), build the fresh handle, compare everything; returns the fresh description"""
    kw, info_ref = ar.fresh_args_after_add(desc, desc["points"], add, add.get("new_points"))
    info = a.add_observations(*rows_of(add))
    assert {k: info[k] for k in info_ref} == info_ref
    assert (a.O, a.P) == (info_ref["num_obs"], info_ref["num_points"])
    if meta is not None:                                # terms that came from set_lidar_device keep type / lidar_xyz
        b = gpu.BA(**{k: v for k, v in kw.items() if not k.startswith("lidar_")})
        b.set_lidar_device(meta["type"], kw["lidar_abcd"], WEIGHT, point=kw["lidar_point"], lidar_xyz=meta["lidar_xyz"])
        t = a.get_lidar()
        assert lr.same_bits(t["type"], meta["type"]) and lr.same_bits(t["lidar_xyz"], meta["lidar_xyz"])
    else:
        b = gpu.BA(**kw)
    bl.assert_same(fg.all_results(gpu, a, kw, solves), fg.all_results(gpu, b, kw, solves))
    b.close()
    return kw


# ---- random additions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("cams", ["shared", "two"])
def test_random_additions_equal_a_fresh_handle(gpu, oracle, cams, shuffle):
    s = full_scene(oracle, cams)
    base, add = ar.split(s, 0.3, 5, seed=41, shuffle=shuffle)
    P, Pb = len(s["points"]), len(base["points"])
    A = len(add["obs_image"])
    assert Pb == P - 5 and 0.25 * len(s["obs_image"]) < A and (add["obs_point"] >= Pb).any() and (add["obs_point"] < Pb).any()
    # the scene is in point order: the image keys always need the sort, the point keys when the rows are shuffled
    assert (np.diff(add["obs_image"]) < 0).any() and (np.diff(add["obs_point"]) < 0).any() == shuffle
    before = np.bincount(base["obs_point"], minlength=P)
    after = before + np.bincount(add["obs_point"], minlength=P)
    assert not np.array_equal(np.argsort(before, kind="stable"), np.argsort(after, kind="stable"))   # the tracks reorder
    a = gpu.BA(**base)
    fg.in_use(gpu, a)
    kw = check_added(gpu, a, base, add)
    a.schur(1e-3, want=("cost",))
    # the same call on a second handle, its rows given as device tensors: repeatable, bit for bit
    import torch
    c = gpu.BA(**base)
    c.add_observations(torch.from_numpy(add["obs_image"]).cuda(), torch.from_numpy(add["obs_point"]).cuda(),
                       torch.from_numpy(np.ascontiguousarray(add["obs_xy"])).cuda(), torch.from_numpy(add["new_points"]).cuda())
    bl.assert_same(fg.all_results(gpu, c, kw), fg.all_results(gpu, a, kw))
    a.schur(1e-3, want=("cost",))
    a.add_observations(add["obs_image"][:1], add["obs_point"][:1], add["obs_xy"][:1])    # any addition drops the Schur state
    with pytest.raises(gpu.PcdError) as e:
        a.schur_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    a.close(); c.close()


# ---- layout boundaries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,held", [(64, 4), (65, 1), (128, 64)])
def test_points_across_a_slice_edge(gpu, oracle, P, held):
    """P 60 -> 64: one slice without padding; 64 -> 65: a second slice with 63 padding threads; 64 -> 128"""
    if ("track", P) not in _CACHE:
        _CACHE["track", P] = lo.track_scene(oracle, P)
    s = _CACHE["track", P]
    base, add = ar.split(s, 0.2, held, seed=P, shuffle=True)
    assert len(base["points"]) == P - held and (P - held + 63) // 64 == 1 and (P + 63) // 64 == (1 if P == 64 else 2)
    a = gpu.BA(**base)
    fg.in_use(gpu, a)
    check_added(gpu, a, base, add)
    a.close()


def two_image_scene():
    """1030 points seen by images 0 and 1, observations moved by N(0, 0.5 px); no constant pose: the handle has no
    packed pose rows"""
    if "seg" not in _CACHE:
        rng = np.random.default_rng(91)
        P = 1030
        points = np.stack([rng.uniform(-2, 2, P), rng.uniform(-1.5, 1.5, P), rng.uniform(5, 12, P)], axis=1)
        p = np.arange(P)
        s = fg.hand_scene([[0, 0, 0], [0.5, 0, 0]], points, np.concatenate([np.zeros(P, np.int64), np.ones(P, np.int64)]),
                          np.concatenate([p, p]))
        s["obs_xy"] = s["obs_xy"] + rng.normal(0, 0.5, s["obs_xy"].shape)
        _CACHE["seg"] = s
    return _CACHE["seg"]


@pytest.mark.parametrize("start,n", [(1020, 4), (1024, 1), (1020, 10)])
def test_image_segments_after_an_addition(gpu, start, n):
    """image 0 grows 1020 -> 1024 (one full segment), 1024 -> 1025 (a second segment of one row), 1020 -> 1030"""
    s = two_image_scene()
    of0 = np.flatnonzero(s["obs_image"] == 0)
    assert len(of0) == 1030
    keep = np.ones(len(s["obs_image"]), bool)
    keep[of0[start:]] = False
    base = dict(s, obs_image=s["obs_image"][keep], obs_point=s["obs_point"][keep], obs_xy=s["obs_xy"][keep])
    rows = of0[start:start + n][::-1]                   # descending point ids
    add = dict(obs_image=s["obs_image"][rows], obs_point=s["obs_point"][rows], obs_xy=s["obs_xy"][rows])
    assert "image_const_pose" not in s
    assert ((start + 1023) // 1024, (start + n + 1023) // 1024) in ((1, 1), (1, 2))
    a = gpu.BA(**base)
    fg.in_use(gpu, a)
    kw = check_added(gpu, a, base, add)
    assert (kw["obs_image"] == 0).sum() == start + n
    a.close()


def point_and_image_cases(s):
    P, xy = len(s["points"]), s["obs_xy"].mean(axis=0)
    i32 = lambda v: np.asarray(v, np.int32)
    assert not (s["obs_point"] == P // 2).any() and (s["lidar_point"] == P // 2).any()
    assert s["point_const"][2] == 1 and s["image_const_pose"][3] == 1 and s["image_const_pose"].sum() == 1
    new = np.array([[0.1, 0.2, 8.0], [-0.4, 0.3, 7.0], [0.5, -0.2, 9.0]])
    none = dict(obs_image=i32([]), obs_point=i32([]), obs_xy=np.zeros((0, 2)))
    return {
        "a point without observations": dict(obs_image=i32([0]), obs_point=i32([P // 2]), obs_xy=xy[None]),
        "a constant point": dict(obs_image=i32([1]), obs_point=i32([2]), obs_xy=xy[None]),
        "a new point of length 1": dict(obs_image=i32([2]), obs_point=i32([P]), obs_xy=xy[None], new_points=new[:1]),
        "new points without rows": dict(none, new_points=new),
        "rows only": dict(obs_image=i32([5, 0, 9, 0, 4, 7, 0]), obs_point=i32([7, 64, 0, 7, 33, 7, 1]),
                          obs_xy=xy + np.arange(14.0).reshape(7, 2)),
        "a row on the constant image": dict(obs_image=i32([3]), obs_point=i32([10]), obs_xy=xy[None]),
        "all rows on constant images": dict(obs_image=i32([3, 3, 3, 3]), obs_point=i32([P + 1, 0, P, 64]),
                                            obs_xy=xy + np.arange(8.0).reshape(4, 2), new_points=new[:2]),
    }


CASES = ["a point without observations", "a constant point", "a new point of length 1", "new points without rows",
         "rows only", "a row on the constant image", "all rows on constant images"]


@pytest.mark.parametrize("case", CASES)
def test_point_and_image_cases(gpu, oracle, case):
    s = full_scene(oracle, "shared")
    add = point_and_image_cases(s)[case]
    a = gpu.BA(**s)
    fg.in_use(gpu, a)
    rows0 = int((s["image_const_pose"][s["obs_image"]] == 0).sum())
    check_added(gpu, a, s, add)
    got = a.evaluate_blocks(True, False)                # the packed pose rows of the grown handle
    variable = int((s["image_const_pose"][add["obs_image"]] == 0).sum())
    assert int((got["pose_row"] != 0xFFFFFFFF).sum()) == rows0 + variable
    if "constant image" in case:
        assert variable == 0
    a.close()


def test_a_handle_without_observations_receives_every_row(gpu, oracle):
    s = full_scene(oracle, "two")
    base = dict(s, obs_image=np.zeros(0, np.int32), obs_point=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2)))
    add = {k: s[k] for k in ("obs_image", "obs_point", "obs_xy")}
    a = gpu.BA(**base)
    assert a.O == 0 and a.evaluate(("cost",))["cost"][0] > 0
    kw = check_added(gpu, a, base, add)
    assert np.array_equal(kw["obs_point"], s["obs_point"])
    a.close()


# ---- the sizes at which the sort of the new rows changes algorithm ---------------------------------------------------
def synth_scene(which):
    if which not in _CACHE:
        _CACHE[which] = synth.ba_scene(8, 1000, seed=5) if which == "small" else synth.ba_scene(100, 300000, seed=5)
    return _CACHE[which]


@pytest.mark.parametrize("which,A", [("small", 1024), ("small", 1025), ("large", 1 << 20), ("large", (1 << 20) + 1)])
def test_sort_size_boundaries(gpu, which, A):
    """solves=False; the large scene (1.3 M rows) compares the normal equations, the cost pass, the track filter and the
    structure: every derived layout is read by one of them"""
    s = synth_scene(which)
    O = len(s["obs_image"])
    assert O > A + 200
    rows = np.random.default_rng(A).permutation(O)[:A]
    keep = np.ones(O, bool)
    keep[rows] = False
    base = dict(s, obs_image=s["obs_image"][keep], obs_point=s["obs_point"][keep], obs_xy=s["obs_xy"][keep])
    add = dict(obs_image=s["obs_image"][rows], obs_point=s["obs_point"][rows], obs_xy=s["obs_xy"][rows])
    kw, info_ref = ar.fresh_args_after_add(base, base["points"], add)
    a = gpu.BA(**base)
    info = a.add_observations(*rows_of(add))
    assert {k: info[k] for k in info_ref} == info_ref
    b = gpu.BA(**kw)

    def results(h):
        if which == "small":
            out = fg.all_results(gpu, h, kw, solves=False)
        else:
            out = dict(evaluate=h.evaluate(("cost", "residuals", "H_img", "g_img", "H_pt", "g_pt")), cost_only=h.evaluate(("cost",)),
                       filter=h.filter_tracks(4.0))
        out["structure"] = h.schur_structure()
        return out
    bl.assert_same(results(a), results(b))
    a.close(); b.close()


# ---- compositions ---------------------------------------------------------------------------------------------------
def test_remove_then_add_is_a_merge(gpu, oracle):
    """two points deleted, one added with the union of their rows"""
    s = full_scene(oracle, "two")
    P = len(s["points"])
    p, q = 7, 41
    pdel = np.zeros(P, np.uint8); pdel[[p, q]] = 1
    rows = np.flatnonzero(np.isin(s["obs_point"], [p, q]))
    assert len(rows) >= 2 and (s["lidar_point"] == q).any()
    a = gpu.BA(**s)
    fg.in_use(gpu, a)
    kw1, _, _ = fg.check_removed(gpu, a, s, None, pdel)
    add = dict(obs_image=s["obs_image"][rows], obs_point=np.full(len(rows), P, np.int32), obs_xy=s["obs_xy"][rows],
               new_points=(s["points"][p] + s["points"][q])[None] / 2)
    fg.in_use(gpu, a)
    kw2 = check_added(gpu, a, kw1, add)
    assert len(kw2["obs_point"]) == len(s["obs_point"]) and len(kw2["points"]) == P + 1
    a.close()


def test_add_then_remove_and_add_twice(gpu, oracle):
    s = full_scene(oracle, "two")
    base, add1 = ar.split(s, 0.2, 5, seed=51, shuffle=True)
    base0, add0 = ar.split(base, 0.2, 3, seed=52, shuffle=False)
    a = gpu.BA(**base0)
    fg.in_use(gpu, a)
    kw1 = check_added(gpu, a, base0, add0)
    fg.in_use(gpu, a)
    kw2 = check_added(gpu, a, kw1, add1)                # the swapped buffers of the first call are the second's scratch
    assert len(kw2["obs_point"]) == len(s["obs_point"]) and np.array_equal(kw2["points"], s["points"])
    erase, pdel = fg.random_flags(kw2, 53, 0.2, 4)
    pdel[len(pdel) - 2] = 1                             # one of the added points goes again
    fg.in_use(gpu, a)
    kw3, _, _ = fg.check_removed(gpu, a, kw2, erase, pdel)
    fg.in_use(gpu, a)
    check_added(gpu, a, kw3, dict(obs_image=add1["obs_image"][:9], obs_point=add1["obs_point"][:9], obs_xy=add1["obs_xy"][:9]))
    a.close()


def test_add_then_associate_lidar(gpu, oracle):
    s = full_scene(oracle, "shared")
    base, add = ar.split(s, 0.3, 5, seed=61)
    Pb = len(base["points"])
    kw, _ = ar.fresh_args_after_add(base, base["points"], add, add["new_points"])
    cloud = gpu.Cloud(*bl.fitted_cloud(), raw_lidar_frame=False)
    a, b = gpu.BA(**base), gpu.BA(**kw)
    a.associate_lidar(cloud, max_range=0.5)             # the scratch of the handle at its old size
    a.add_observations(*rows_of(add))
    assert not (a.get_lidar()["point"] >= Pb).any()     # new points carry no term yet
    ia, ib = a.associate_lidar(cloud, max_range=0.5), b.associate_lidar(cloud, max_range=0.5)
    strip = lambda d: {k: v for k, v in d.items() if not k.endswith("_ms")}
    bl.assert_same(strip(ia), strip(ib))
    assert ia["num_queries"] == len(kw["points"]) and (a.get_lidar()["point"] >= Pb).any()     # and now they do
    bl.assert_same(a.get_lidar(), b.get_lidar())
    bl.assert_same(fg.all_results(gpu, a, kw), fg.all_results(gpu, b, kw))
    a.close(); b.close(); cloud.close()


def test_set_lidar_terms_keep_their_meta(gpu, oracle):
    s0, _ = bl.scene(oracle, "shared")
    base0, add = ar.split(s0, 0.3, 5, seed=71, shuffle=True)
    point, typ, abcd, xyz = bl.make_rows(base0, 200, "shuffled", 5, False)
    y = lr.terms(typ, abcd, WEIGHT, point, xyz)
    desc = dict(base0, lidar_point=y["lidar_point"], lidar_abcd=y["lidar_abcd"], lidar_weight=y["lidar_weight"])
    a = gpu.BA(**base0)
    a.set_lidar_device(typ, abcd, WEIGHT, point=point, lidar_xyz=xyz)
    assert a.L == len(y["lidar_point"]) > 0 and y["type"].any()
    fg.in_use(gpu, a)
    check_added(gpu, a, desc, add, meta=dict(type=y["type"], lidar_xyz=y["lidar_xyz"]))
    a.close()


def chain_scene(oracle):
    """140 tracks of 1 .. 3 observations over 3 images (279 rows), image 1 constant, every 5th point constant, 0 .. 3
    LiDAR terms per point"""
    if "chain" not in _CACHE:
        rng = np.random.default_rng(97)
        I, P = 3, 140
        s = lo._base(rng, I, P, lo.CAMERAS["shared"])
        length = rng.permutation(np.arange(P) % 3 + 1)
        obs_point = np.repeat(np.arange(P), length).astype(np.int32)
        j = np.arange(len(obs_point)) - np.repeat(np.cumsum(length) - length, length)
        cpose = np.zeros(I, np.uint8); cpose[1] = 1
        s.update(obs_image=((obs_point + j) % I).astype(np.int32), obs_point=obs_point, image_const_pose=cpose,
                 point_const=(np.arange(P) % 5 == 2).astype(np.uint8))
        lo._lidar(rng, s, rng.permutation(np.repeat(np.arange(P), np.arange(P) % 4)))
        _CACHE["chain"] = sr.reproject(oracle, s, rng)
    return _CACHE["chain"]


def check_terms(gpu, a, desc, Q, seed):
    """set_lidar_device with Q rows on the live handle `a` (whose description is `desc`), compare with a fresh handle that
    holds the terms of those rows; returns (fresh description, meta)"""
    bare = {k: v for k, v in desc.items() if not k.startswith("lidar_")}
    point, typ, abcd, xyz = bl.make_rows(bare, Q, "shuffled", seed, False)
    y = lr.terms(typ, abcd, WEIGHT, point, xyz)
    assert a.set_lidar_device(typ, abcd, WEIGHT, point=point, lidar_xyz=xyz) == len(y["lidar_point"]) == a.L > 0
    kw = dict(bare, lidar_point=y["lidar_point"], lidar_abcd=y["lidar_abcd"], lidar_weight=y["lidar_weight"])
    b = gpu.BA(**bare)
    b.set_lidar_device(y["type"], y["lidar_abcd"], WEIGHT, point=y["lidar_point"], lidar_xyz=y["lidar_xyz"])
    bl.assert_same(fg.all_results(gpu, a, kw), fg.all_results(gpu, b, kw))
    b.close()
    return kw, dict(type=y["type"], lidar_xyz=y["lidar_xyz"])


def test_every_rebuild_in_turn_on_one_handle(gpu, oracle):
    """removal, addition and set_lidar_device alternate on one handle, so each works in the buffers the others retired:
    created with terms (no type / lidar_xyz yet), through a handle without any term, P 70 -> 90 -> 130 -> 140"""
    s = chain_scene(oracle)
    s2, add3 = ar.split(s, 0.1, 10, seed=101, shuffle=True)
    s1, add2 = ar.split(s2, 0.1, 40, seed=102, shuffle=True)
    s0, add1 = ar.split(s1, 0.1, 20, seed=103, shuffle=True)
    assert len(s0["points"]) == 70 and s0["image_const_pose"].sum() == 1 and len(s["obs_point"]) == 279
    a = gpu.BA(**s0)
    L0 = a.L
    fg.in_use(gpu, a)
    erase, pdel = fg.random_flags(s0, 104, 0.1, 3)
    pdel[np.flatnonzero(np.bincount(s0["lidar_point"], minlength=70) == 3)[0]] = 1
    kw, _, _ = fg.check_removed(gpu, a, s0, erase, pdel)                # 2: has_lidar_meta is still false
    assert 0 < a.L < L0
    fg.in_use(gpu, a)
    kw = check_added(gpu, a, kw, add1)                                  # 3
    L1 = a.L
    kw, meta = check_terms(gpu, a, kw, 20, 105)                         # 4: fewer terms, on points 1 .. 10
    assert a.L < min(L1, 20) and kw["lidar_point"].max() <= 10
    fg.in_use(gpu, a)
    kw = check_added(gpu, a, kw, add2, meta=meta)                       # 5: two slices become three
    assert (a.P + 63) // 64 == 3
    fg.in_use(gpu, a)
    pdel = np.zeros(a.P, np.uint8); pdel[kw["lidar_point"]] = 1
    kw, meta, _ = fg.check_removed(gpu, a, kw, None, pdel, meta=meta)   # 6: every term goes
    assert a.L == 0 and a.O > 100
    kw, meta = check_terms(gpu, a, kw, 200, 106)                        # 7
    fg.in_use(gpu, a)
    kw = check_added(gpu, a, kw, add3, meta=meta)                       # 8
    assert a.P == 140 and a.L == len(meta["type"]) > 20
    a.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_untouched(gpu, oracle):
    s = full_scene(oracle, "two")
    base, add = ar.split(s, 0.3, 5, seed=81, shuffle=True)
    I, P = len(s["poses"]), len(s["points"])
    a = gpu.BA(**base)
    fg.in_use(gpu, a)
    before, dims, ptrs = fg.all_results(gpu, a, base), (a.O, a.P, a.L), a.lidar_device()

    def bad(k, row, v):
        d = dict(add, **{k: add[k].copy()})
        d[k][row] = v
        return d
    many = {k: np.concatenate([add[k]] * 4)[:300] for k in ("obs_image", "obs_point", "obs_xy")}
    many["new_points"] = add["new_points"]
    last = dict(many, obs_point=many["obs_point"].copy())
    last["obs_point"][299] = P
    assert len(last["obs_point"]) == 300
    for d in (bad("obs_image", 3, I), bad("obs_image", 0, -1), bad("obs_point", 5, P), bad("obs_point", 2, -1), last):
        with pytest.raises(gpu.PcdError) as e:
            a.add_observations(*rows_of(d))
        assert e.value.status == gpu.PCD_ERR_INVALID and "out of range" in str(e.value)
        assert (a.O, a.P, a.L) == dims and a.lidar_device() == ptrs
    with pytest.raises(gpu.PcdError) as e:              # a point the handle does not have yet, without new points
        a.add_observations(add["obs_image"], add["obs_point"], add["obs_xy"])
    assert e.value.status == gpu.PCD_ERR_INVALID and a.lidar_device() == ptrs
    bl.assert_same(fg.all_results(gpu, a, base), before)
    check_added(gpu, a, base, add)                      # and a valid addition still equals the fresh handle
    a.close()


def test_the_empty_call_and_a_capturing_stream(gpu, oracle):
    import ctypes as C
    import torch
    L = gpu.lib()
    assert L.pcd_ba_add_observations_device(None, None, 0, None, None, None, 0, None, None) == gpu.PCD_ERR_INVALID
    s = full_scene(oracle, "shared")
    base, add = ar.split(s, 0.3, 5, seed=82)
    a = gpu.BA(**base)
    before = fg.all_results(gpu, a, base)
    a.schur(1e-3, want=("cost",))
    ptrs = a.lidar_device()
    info = a.add_observations(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    assert (info["num_obs"], info["num_obs_added"], info["num_points"], info["num_points_added"]) == (a.O, 0, a.P, 0)
    assert info["num_pose_rows"] == int((base["image_const_pose"][base["obs_image"]] == 0).sum())
    assert a.lidar_device() == ptrs
    a.schur_solve_pcg()                                 # the Schur state is still there
    # a count with a NULL array
    null = C.c_void_p(None)
    assert L.pcd_ba_add_observations_device(a._h, null, 2, null, null, null, 0, null, None) == gpu.PCD_ERR_INVALID
    assert L.pcd_ba_add_observations_device(a._h, null, 0, null, null, null, 3, null, None) == gpu.PCD_ERR_INVALID
    # a capturing stream: refused before anything is allocated, as tests/test_capture_gpu.py has it for the others
    rows = [torch.from_numpy(np.ascontiguousarray(add[k])).cuda() for k in ("obs_image", "obs_point", "obs_xy", "new_points")]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                a.add_observations(*rows)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
    assert (a.O, a.P) == (len(base["obs_point"]), len(base["points"])) and a.lidar_device() == ptrs
    bl.assert_same(fg.all_results(gpu, a, base), before)
    check_added(gpu, a, base, add)                      # the handle works afterwards
    a.close()


# ---- the loop -------------------------------------------------------------------------------------------------------
def test_refine_filter_with_a_completion_callback(gpu, oracle):
    s = fg.filter_scene(oracle, "two")
    base, add = ar.split(s, 0.2, 3, seed=83, shuffle=True)
    A = len(add["obs_image"])
    opts = dict(max_num_iterations=4, linear_solver="cholesky")
    strip = lambda d: {k: v for k, v in d.items() if not k.endswith("_ms")}
    desc, manual = dict(base), []
    for r in range(8):                                  # the same steps by hand, a new handle for each of them
        h = gpu.BA(**desc)
        num_obs = h.O
        summary, _its = gpu.ba_solve(h, **opts)
        poses, points = h.get_parameters()
        h.close()
        desc, ainfo = dict(desc, poses=poses, points=points), None
        if r == 0:
            desc, ainfo = ar.fresh_args_after_add(desc, points, add, add["new_points"])
        h = gpu.BA(**desc)
        f = h.filter_points(8.0, 1.5)
        h.close()
        desc, _, info, _ = fr.fresh_args_after_remove(desc, f["obs_erase"], f["point_delete"])
        changed = (float(f["num_filtered"]) + (A if r == 0 else 0)) / num_obs
        manual.append((summary, f, info, ainfo, changed))
        if changed < 0.0005:
            break
    calls = []

    def complete(ba, r):
        calls.append((r, ba.O))
        return add if r == 0 else None
    ba = gpu.BA(**base)
    rounds = gpu.refine_filter(ba, max_refinements=8, complete=complete, **opts)
    assert len(rounds) == len(manual) >= 2 and [c[0] for c in calls] == list(range(len(rounds)))
    assert calls[0][1] == len(base["obs_point"])        # invoked behind the solve, ahead of the filter and the removal
    assert rounds[0][1]["changed"] >= A / len(base["obs_point"])
    for (sm, fl, info, added), (msm, mf, minfo, mainfo, mchanged) in zip(rounds, manual):
        bl.assert_same(strip(sm), strip(msm))
        bl.assert_same(fg.summary_keys(fl), fg.summary_keys(mf))
        assert fl["changed"] == mchanged and {k: info[k] for k in minfo} == minfo
        assert (added is None) == (mainfo is None) and (added is None or {k: added[k] for k in mainfo} == mainfo)
    poses, points = ba.get_parameters()
    assert lr.same_bits(poses, desc["poses"]) and lr.same_bits(points, desc["points"])
    assert (ba.O, ba.P) == (len(desc["obs_point"]), len(s["points"]))
    ba.close()
    # a callback that never adds, and none at all: today's results
    x, y = gpu.BA(**s), gpu.BA(**s)
    rx = gpu.refine_filter(x, max_refinements=3, complete=lambda ba, r: None, **opts)
    ry = gpu.refine_filter(y, max_refinements=3, **opts)
    assert len(rx) == len(ry) and all(len(t) == 4 and t[3] is None for t in rx) and all(len(t) == 3 for t in ry)
    for tx, ty in zip(rx, ry):
        bl.assert_same(strip(tx[0]), strip(ty[0]))
        bl.assert_same(tx[1], ty[1])
        bl.assert_same(strip(tx[2]), strip(ty[2]))
    x.close(); y.close()


def test_shim_add_observations(gpu):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_add"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_add"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr

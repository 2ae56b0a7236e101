"""LiDAR terms of a BA handle rebuilt on the device (pcd_ba_set_lidar_device, pcd_ba_associate_lidar_device).

The contract is equality with a FRESH handle: after the call every result on the handle -- evaluate with every output,
both block routes, the Schur blocks, the track filter, a 3-iteration LM solve with the PCG and with the Cholesky -- has
the bits of the result on a handle that pcd_ba_create built from the same scene with the new term list.  The expected
term list comes from tests/ba_lidar_ref.py (the type / NaN / weight rule in numpy).  Equality is np.array_equal on the
bit patterns (ba_lidar_ref.same_bits), so a NaN that both handles compute compares equal.

Scenes: tests/test_ba_load_order_gpu.track_scene at P = 65 (one shared camera) and P = 130 (two cameras): two and three
64-track slices, so the thread-order fill crosses a slice edge and padding lanes.  Rows: type-0 rows, a NaN in each of
the four abcd positions, all three types, points with 0, 1 and 3 terms, in shuffled and in ascending point order (the
sort path and the no-sort path), Q = 0, 1, 64, 65, 1000 (several scan workgroups).  The Inf row (kept, as the reference
keeps it) rides in the one-camera runs: it makes the cost Inf and the steps NaN, identically on both handles; the
two-camera runs carry none, so there the compared solves are finite, which the test asserts.  weight[0] is NaN: it is
never read."""
import numpy as np
import pytest

from pcdhip import synth
from tests import ba_lidar_ref as lr
from tests import test_ba_load_order_gpu as lo

pytestmark = pytest.mark.gpu
lo.CAMERAS.setdefault("two", (4, 1))
SCENES = {"shared": 65, "two": 130}
WEIGHT = np.array([np.nan, 100.0, 1000.0, 1.0])
EVERY = ("cost", "residuals", "jac_q", "jac_t", "jac_X", "jac_lidar", "H_img", "g_img", "H_pt", "g_pt", "W", "jac_cam",
         "H_cam", "g_cam", "E_cam", "W_cam")
_CACHE = {}


def scene(oracle, cams):
    """the scene without LiDAR terms, and the terms track_scene gives it ("many")"""
    if cams not in _CACHE:
        s = lo.track_scene(oracle, SCENES[cams], cams=cams)
        many = {k: s.pop(k) for k in ("lidar_point", "lidar_abcd", "lidar_weight")}
        _CACHE[cams] = (s, many)
    return _CACHE[cams]


def make_rows(s, Q, order, seed, inf_row, keep_every=1, none=False):
    """Q rows (point, type, abcd, lidar_xyz).  Candidates: 0, 1, 3, 1 rows for the points in turn, types 1, 2, 3 in turn,
    planes through a point near their own.  From 16 rows on: two type-0 rows, one row with a NaN in each abcd position and
    (inf_row) one with an Inf; rows beyond the candidates are of type 0.  keep_every > 1 turns all candidates but every
    keep_every-th into type 0; none turns every candidate and the Inf row into type 0 (the NaN rows keep their types)."""
    rng = np.random.default_rng(seed)
    P = len(s["points"])
    special = (6 + int(inf_row)) if Q >= 16 else 0
    per_point = np.array([0, 1, 3, 1])[np.arange(P) % 4]
    cand = np.repeat(np.arange(P), per_point)[:Q - special]
    fill = Q - special - len(cand)                      # rows beyond the candidates: type 0, any point
    point = np.concatenate([cand, rng.integers(0, P, fill + special)]).astype(np.int32)
    typ = (np.arange(Q) % 3 + 1).astype(np.uint8)
    typ[len(cand):Q - special] = 0
    nrm = rng.normal(size=(Q, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    xyz = s["points"][point] + rng.normal(0, 0.05, (Q, 3))
    abcd = np.concatenate([nrm, -np.sum(nrm * xyz, axis=1, keepdims=True)], axis=1)
    if keep_every > 1:
        typ[:len(cand)][np.arange(len(cand)) % keep_every != 0] = 0
    if none:
        typ[:len(cand)] = 0
    if special:
        b = Q - special
        typ[b:b + 2] = 0
        for k in range(4):
            abcd[b + 2 + k, k] = np.nan
        if inf_row:
            abcd[b + 6, 3] = np.inf
            typ[b + 6] = 0 if none else 1
    perm = rng.permutation(Q) if order == "shuffled" else np.argsort(point, kind="stable")
    return point[perm], typ[perm], abcd[perm], xyz[perm]


def results(gpu, ba, s):
    """every result the contract names, at the scene's parameters; the solves start from them again"""
    out = dict(evaluate=ba.evaluate(EVERY), blocks=ba.evaluate_blocks(True, True),
               compact=ba.evaluate_blocks_compact(True, True), compact_trial=ba.evaluate_blocks_compact(False),
               cost_only=ba.evaluate(("cost",)), filter=ba.filter_tracks(4.0))
    sch = ba.schur(1e-3, want=("cost", "S_diag", "S_off", "rhs", "num_skipped"))
    out["schur"] = {k: v.cpu().numpy() for k, v in sch.items()}
    for solver in ("pcg", "cholesky"):
        ba.set_parameters(s["poses"], s["points"])
        summary, its = gpu.ba_solve(ba, max_num_iterations=3, linear_solver=solver)
        poses, points = ba.get_parameters()
        out["solve_" + solver] = dict(
            summary={k: v for k, v in summary.items() if not k.endswith("_ms")}, poses=poses, points=points,
            iterations=[{k: np.float64(v) if isinstance(v, float) else v for k, v in it.items()} for it in its])
    ba.set_parameters(s["poses"], s["points"])
    return out


def assert_same(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            assert_same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, f"{path}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, path
    elif isinstance(a, (np.ndarray, np.floating, float)):
        assert lr.same_bits(np.asarray(a, np.float64) if not isinstance(a, np.ndarray) else a,
                            np.asarray(b, np.float64) if not isinstance(b, np.ndarray) else b), path
    else:
        assert a == b, path


def handle(gpu, s, t):
    return gpu.BA(**lr.fresh_args(s, t))


FEW = 3
KINDS = ("none_some", "some_none", "few_many", "many_few")
CASES = [(k, Q, o, c) for k in KINDS for Q in (0, 1, 64, 65, 1000) for o in ("ascending", "shuffled") for c in SCENES
         if Q > 1 or o == "ascending"]


@pytest.mark.parametrize("kind,Q,order,cams", CASES)
def test_set_lidar_equals_a_fresh_handle(gpu, oracle, kind, Q, order, cams):
    s, many = scene(oracle, cams)
    if kind == "none_some":
        x = {}
    elif kind == "few_many":
        x = {k: v[:FEW] for k, v in many.items()}
    else:
        x = many
    inf_row = cams == "shared"
    point, typ, abcd, xyz = make_rows(s, Q, order, 7000 + Q, inf_row, keep_every=8 if kind == "many_few" else 1,
                                      none=kind == "some_none")
    y = lr.terms(typ, abcd, WEIGHT, point, xyz)
    if Q >= 64:   # the rows are what the issue asks for
        assert (typ == 0).any() and np.isnan(abcd).any(axis=1).sum() == 4 and np.isinf(abcd).any() == inf_row
        if kind in ("none_some", "few_many"):
            per = np.bincount(y["lidar_point"], minlength=len(s["points"]))
            assert {0, 1, 3} <= set(per.tolist()) and set(y["type"].tolist()) == {1, 2, 3}
            assert (np.diff(y["lidar_point"]) < 0).any() == (order == "shuffled")
    if kind == "some_none":
        assert len(y["lidar_point"]) == 0
    a = gpu.BA(**s, **x)
    a.evaluate(("cost", "H_pt"))                       # a handle in use: staging and the Schur state belong to X
    a.schur(1e-3, want=("cost",))
    n = a.set_lidar_device(typ, abcd, WEIGHT, point=point, lidar_xyz=xyz)
    assert n == len(y["lidar_point"]) == a.L
    with pytest.raises(gpu.PcdError) as e:             # the Schur state of X is dropped, the structure is not
        a.schur_solve_pcg()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    got_terms = a.get_lidar()
    for k, ky in (("point", "lidar_point"), ("abcd", "lidar_abcd"), ("weight", "lidar_weight"), ("type", "type"),
                  ("lidar_xyz", "lidar_xyz")):
        assert lr.same_bits(got_terms[k], y[ky]), k
    b = handle(gpu, s, y)
    ra, rb = results(gpu, a, s), results(gpu, b, s)
    assert_same(ra, rb)
    if not inf_row:
        for solver in ("solve_pcg", "solve_cholesky"):
            assert np.isfinite(ra[solver]["summary"]["final_cost"]) and np.isfinite(ra[solver]["points"]).all()
    a.close()
    b.close()


def test_get_lidar_of_a_created_handle(gpu, oracle):
    s, many = scene(oracle, "shared")
    ba = gpu.BA(**s, **many)
    t = ba.get_lidar()
    assert lr.same_bits(t["point"], many["lidar_point"]) and lr.same_bits(t["abcd"], many["lidar_abcd"])
    assert lr.same_bits(t["weight"], many["lidar_weight"])
    assert not t["type"].any() and not t["lidar_xyz"].any()      # pcd_ba_create knows neither
    L, ptrs = ba.lidar_device()
    assert L == len(many["lidar_point"]) and all(ptrs.values())
    ba.close()


def test_refusals_leave_the_handle_untouched(gpu, oracle):
    import torch
    s, many = scene(oracle, "two")
    P = len(s["points"])
    ba = gpu.BA(**s, **many)
    before = ba.evaluate(EVERY)
    point, typ, abcd, xyz = make_rows(s, 65, "shuffled", 1, False)
    assert (typ == 1).any()
    bad_point, bad_low, bad_type = point.copy(), point.copy(), typ.copy()
    bad_point[40] = P
    bad_low[3] = -1
    bad_type[np.flatnonzero(typ == 0)[0]] = 4          # a type above 3 is refused in any row
    w_nan = WEIGHT.copy(); w_nan[1] = np.nan
    calls = [lambda: ba.set_lidar_device(typ, abcd, WEIGHT, point=bad_point),
             lambda: ba.set_lidar_device(typ, abcd, WEIGHT, point=bad_low),
             lambda: ba.set_lidar_device(bad_type, abcd, WEIGHT, point=point),
             lambda: ba.set_lidar_device(typ, abcd, w_nan, point=point),
             lambda: ba.set_lidar_device(typ, abcd, WEIGHT)]            # no point array and Q != P
    for call in calls:
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_INVALID, str(e.value)
        assert ba.L == len(many["lidar_point"])
        assert_same(ba.evaluate(EVERY), before)
    # a capturing stream: refused before anything is allocated, as tests/test_capture_gpu.py has it for the others
    cloud = gpu.Cloud(*synth.cloud_planes(20000), raw_lidar_frame=False)
    dt, da = torch.from_numpy(typ).cuda(), torch.from_numpy(abcd).cuda()
    dp = torch.from_numpy(point).cuda()
    one = torch.ones(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            for call in (lambda: ba.set_lidar_device(dt, da, WEIGHT, point=dp),
                         lambda: ba.associate_lidar(cloud, max_range=one)):
                with pytest.raises(gpu.PcdError) as e:
                    call()
                assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
    assert_same(ba.evaluate(EVERY), before)
    # a weight that is not finite for a type that does NOT occur is not read
    only2 = np.where(typ != 0, 2, 0).astype(np.uint8)
    assert ba.set_lidar_device(only2, abcd, w_nan, point=point) == len(lr.terms(only2, abcd, w_nan, point)["rows"])
    cloud.close()
    ba.close()


# ---- associate_lidar ------------------------------------------------------------------------------------------------
def fitted_cloud():
    """synth.cloud_planes(20000) moved and scaled (one factor) into the box the scenes' points fill, so that the points
    have neighbours: normals stay as they are"""
    if "cloud" not in _CACHE:
        xyz, nrm = synth.cloud_planes(20000)
        lo_c, hi_c = xyz.min(axis=0), xyz.max(axis=0)
        box_lo, box_hi = np.array([-2.0, -1.5, 5.0]), np.array([2.0, 1.5, 12.0])
        f = np.float32(((box_hi - box_lo) / (hi_c - lo_c)).min())
        _CACHE["cloud"] = (((xyz - (lo_c + hi_c) / 2) * f + ((box_lo + box_hi) / 2).astype(np.float32)).astype(np.float32), nrm)
    return _CACHE["cloud"]


def max_ranges(P, which):
    if which == "one":
        return 0.3
    if which == "none_pass":
        return np.zeros(P)                       # rejects everything: no term
    return np.where(np.arange(P) % 3 == 0, 0.05, np.where(np.arange(P) % 3 == 1, 0.2, 0.5))


ASSOC = [(gpu_mode, bounded, sel, mr) for gpu_mode in (0, 1, 2) for bounded in (False, True) for sel in (False, True)
         for mr in ("per_point",)] + [(1, False, False, "one"), (1, True, True, "none_pass"), (0, False, False, "none_pass")]


@pytest.mark.parametrize("mode,bounded,use_select,mr", ASSOC)
def test_associate_lidar_equals_the_composition(gpu, oracle, mode, bounded, use_select, mr):
    cams = "two" if use_select else "shared"
    s, many = scene(oracle, cams)
    P = len(s["points"])
    cloud = gpu.Cloud(*fitted_cloud(), raw_lidar_frame=False)
    gate = mode | (gpu.GATE_BOUNDED_SEARCH if bounded else 0)
    rng = max_ranges(P, mr)
    select = (np.arange(P) % 4 != 1).astype(np.uint8) if use_select else None
    ref = cloud.associate(s["points"], None if mode == gpu.GATE_CONTROLLER else rng, gate)
    w = [0.0, 70.0, 900.0, 0.0]
    y = lr.terms(ref["type"], ref["abcd"], w, None, ref["lidar_xyz"], select)
    a = gpu.BA(**s, **many)
    info = a.associate_lidar(cloud, max_range=rng, gate_mode=gate, select=select, icp_weight=70.0, icp_ground_weight=900.0)
    n1, n2 = int((y["type"] == 1).sum()), int((y["type"] == 2).sum())
    assert (info["num_terms"], info["num_icp"], info["num_icp_ground"]) == (len(y["rows"]), n1, n2)
    assert info["num_icp"] + info["num_icp_ground"] == info["num_terms"] == a.L
    assert info["num_queries"] == (P if select is None else int(select.sum()))
    if mr == "none_pass" and mode != gpu.GATE_CONTROLLER:
        assert info["num_terms"] == 0
    elif mr == "per_point":
        # both types occur and some selected points are rejected
        assert n1 > 0 and n2 > 0 and info["num_terms"] < info["num_queries"]
    t = a.get_lidar()
    for k, ky in (("point", "lidar_point"), ("abcd", "lidar_abcd"), ("weight", "lidar_weight"), ("type", "type"),
                  ("lidar_xyz", "lidar_xyz")):
        assert lr.same_bits(t[k], y[ky]), k
    assert lr.same_bits(t["type"], ref["type"][y["rows"]]) and lr.same_bits(t["lidar_xyz"], ref["lidar_xyz"][y["rows"]])
    again = a.associate_lidar(cloud, max_range=rng, gate_mode=gate, select=select, icp_weight=70.0, icp_ground_weight=900.0)
    assert_same(a.get_lidar(), t)                     # twice in a row without a solve: identical terms
    assert again["num_terms"] == info["num_terms"]
    b = handle(gpu, s, y)
    assert_same(results(gpu, a, s), results(gpu, b, s))
    a.close(); b.close(); cloud.close()


def test_associate_lidar_refuses_a_strided_cloud(gpu, oracle):
    s, many = scene(oracle, "shared")
    xyz, nrm = fitted_cloud()
    ba = gpu.BA(**s, **many)
    before = ba.get_lidar()
    for kw in (dict(index_stride=2), dict(index_base=5)):
        part = gpu.Cloud(xyz, nrm, raw_lidar_frame=False, **kw)
        with pytest.raises(gpu.PcdError) as e:
            ba.associate_lidar(part, max_range=0.3)
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
        part.close()
    assert_same(ba.get_lidar(), before)
    ba.close()


def test_register_refine_equals_a_new_handle_per_round(gpu, oracle):
    s, _ = scene(oracle, "two")
    P = len(s["points"])
    cloud = gpu.Cloud(*fitted_cloud(), raw_lidar_frame=False)
    select = (np.arange(P) % 5 != 0).astype(np.uint8)
    opts = dict(max_num_iterations=6, linear_solver="cholesky")
    sched = dict(kd_max=0.5, kd_min=0.1, drop=0.2)      # near neighbours only: the first steps are accepted
    # the manual loop: associate on the host route, a new handle per round from the downloaded parameters
    poses, points = s["poses"], s["points"]
    manual = []
    for r in range(2):
        rng = float(gpu.search_range_schedule(np.array([r], np.int32), **sched)[0])
        ref = cloud.associate(points, rng, gpu.GATE_MAPPER_GLOBAL)
        y = lr.terms(ref["type"], ref["abcd"], [0.0, 100.0, 1000.0, 0.0], None, ref["lidar_xyz"], select)
        assert len(y["rows"]) > 0
        h = gpu.BA(**lr.fresh_args(dict(s, poses=poses, points=points), y))
        gpu.ba_solve(h, **opts)
        poses, points = h.get_parameters()
        manual.append((poses, points, len(y["rows"])))
        h.close()
    ba = gpu.BA(**s)
    got = []
    for r in range(2):                                  # one round at a time, to look at the parameters in between
        (info, summary, its), = gpu.register_refine(ba, cloud, 1, kd_max=float(gpu.search_range_schedule(
            np.array([r], np.int32), **sched)[0]), kd_min=0.1, select=select, **opts)
        assert summary["num_accepted"] >= 1
        got.append((*ba.get_parameters(), info["num_terms"]))
    for r in range(2):
        assert got[r][2] == manual[r][2]
        assert lr.same_bits(got[r][0], manual[r][0]) and lr.same_bits(got[r][1], manual[r][1]), r
    assert not lr.same_bits(got[0][1], s["points"])     # the solve moved the points: round 2 re-associated other queries
    # and the loop as one call
    ba.set_parameters(s["poses"], s["points"])
    rounds = gpu.register_refine(ba, cloud, 2, select=select, **sched, **opts)
    assert [r[0]["num_terms"] for r in rounds] == [m[2] for m in manual]
    assert [r[0]["max_range"] for r in rounds] == [float(v) for v in gpu.search_range_schedule(np.arange(2, dtype=np.int32), **sched)]
    poses2, points2 = ba.get_parameters()
    assert lr.same_bits(poses2, manual[1][0]) and lr.same_bits(points2, manual[1][1])
    ba.close(); cloud.close()


# ---- shim -----------------------------------------------------------------------------------------------------------
def read_blocks(path):
    """the file shim/test_ba_reassoc writes: 'name dtype count' lines, each followed by the raw array"""
    out = {}
    with open(path, "rb") as f:
        while True:
            head = f.readline()
            if not head:
                return out
            name, dtype, count = head.decode().split()
            dt = np.dtype("<" + dtype)
            out[name] = np.frombuffer(f.read(int(count) * dt.itemsize), dt).copy()


def test_shim_reassociate_and_the_python_route(gpu, tmp_path):
    import os
    import re
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_reassoc"])
    path = str(tmp_path / "scene.bin")
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_reassoc"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    m = re.search(r"^ROUND1 (\d+) (\S+) (\S+)$", r.stdout, re.M)
    terms, initial, final = int(m.group(1)), float(m.group(2)), float(m.group(3))
    # the same scene through the Python binding: associate on the handle, then the solve the shim asks for
    b = read_blocks(path)
    off = list(b["cam_off"]) + [len(b["cam_params"])]
    ba = gpu.BA(b["cam_model"], [b["cam_params"][off[c]:off[c + 1]] for c in range(len(b["cam_model"]))], b["poses"],
                b["image_camera"], b["points"], b["obs_image"], b["obs_point"], b["obs_xy"],
                image_const_pose=b["image_const_pose"], image_const_tvec=b["image_const_tvec"], point_const=b["point_const"])
    cloud = gpu.Cloud(b["cloud_xyz"], b["cloud_nrm"])     # a raw scan, as PointCloudProcess indexes it
    info = ba.associate_lidar(cloud, max_range=0.6, gate_mode=gpu.GATE_MAPPER_GLOBAL, icp_weight=40.0, icp_ground_weight=300.0)
    assert info["num_terms"] == terms and 0 < info["num_icp_ground"] < terms
    summary, _ = gpu.ba_solve(ba, max_num_iterations=10, function_tolerance=0.0, gradient_tolerance=0.0,
                              linear=dict(max_iterations=200))
    assert summary["initial_cost"] == initial and summary["final_cost"] == final
    ba.close(); cloud.close()

"""GPU parity of the point elimination (pcd_ba_schur*) against the numpy reference built from the oracle's
normal equations (tests/ba_schur_ref.py).

Bounds: S_diag, S_off, rhs and the dense S within 1e-9 relative (scale-aware floor, as test_ba_gpu.py); the step
(GPU Schur -> numpy solve -> GPU back-substitution) within 1e-8 of the dense solve of the whole damped system where that
system is well conditioned, and within 1e-8 of the reference back-substitution of the same pose step everywhere;
plus within 1e-14."""
import ctypes as C

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_schur_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _close(a, b, rtol, what):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, err_msg=what)


def _scene(seed, I=6, P=150, order="point", loss=0, lidar=True, const=True, tvec=True):
    s = synth.ba_scene(I, P, seed=seed, const_pose_frac=0.3 if const else 0.0, order=order,
                       lidar_frac=1.0 if lidar else 0.0)
    if not lidar:
        for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
            s.pop(k)
    rng = np.random.default_rng(seed)
    if tvec:
        s["image_const_tvec"] = (rng.integers(1, 8, I) * (rng.random(I) < 0.4)).astype(np.uint8)
    if const:
        s["point_const"] = (rng.random(P) < 0.1).astype(np.uint8)
        s["image_const_pose"][0] = 1
    s["loss_type"], s["loss_scale"] = loss, 2.0
    return s


def _run(gpu, s, mu, mode):
    ba = gpu.BA(**s)
    out = ba.schur(mu, damping=mode, dense=True)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    return ba, res


def _check_blocks(ne, st, res):
    sb = ne.schur_blocks()
    assert np.array_equal(st["pairs"], sb["pairs"])
    _close(res["S_diag"], sb["S_diag"], 1e-9, "S_diag")
    off = np.stack([sb["S_off"][tuple(p)] for p in sb["pairs"]]) if len(sb["pairs"]) else np.zeros((0, 6, 6))
    _close(res["S_off"], off, 1e-9, "S_off")
    _close(res["rhs"], sb["rhs"], 1e-9, "rhs")
    _close(res["S"], sb["S"], 1e-9, "dense S")
    assert int(res["num_skipped"][0]) == int(ne.skipped.sum())
    return sb


def _step(ba, res, ne, well_conditioned):
    dev = torch.device("cuda", ba.device)
    dpose = np.linalg.solve(res["S"], res["rhs"].reshape(-1)).reshape(-1, 6)
    dpoint, md = ba.back_substitute(torch.from_numpy(dpose).to(dev))
    dpoint = dpoint.cpu().numpy()
    _close(dpoint, ne.back_substitute(dpose), 1e-8, "back-substitution")
    _close(md.cpu().numpy()[0], ne.model_decrease(dpose, dpoint), 1e-8, "model decrease")
    assert not dpoint[ne.skipped | (ne.pr["point_const"] == 1)].any()
    if well_conditioned:
        dp_ref, dx_ref = ne.dense_solve()
        _close(dpose, dp_ref, 1e-8, "pose step vs dense solve")
        _close(dpoint, dx_ref, 1e-8, "point step vs dense solve")
    return dpose, dpoint


CASES = [  # (loss, order, lidar, const, mode, mu, well conditioned)
    (0, "point", True, True, "marquardt", 1e-4, True),
    (1, "point", True, True, "marquardt", 1e-4, True),
    (2, "image", True, True, "marquardt", 1e-4, True),
    (0, "image", False, True, "marquardt", 1.0, True),
    (1, "point", True, False, "levenberg", 1.0, False),
    (2, "point", True, True, "levenberg", 1e-4, False),
    (0, "image", True, True, "marquardt", 0.0, False),
    (0, "point", True, True, "levenberg", 0.0, False),
    (0, "point", True, True, "marquardt", 1.0, True),
    (2, "image", True, True, "levenberg", 1.0, False),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_schur_parity(gpu, oracle, case):
    loss, order, lidar, const, mode, mu, wc = CASES[case]
    s = _scene(30 + case, order=order, loss=loss, lidar=lidar, const=const)
    ba, res = _run(gpu, s, mu, mode)
    ne = ref.NormalEquations(oracle, s, mu, mode)
    np.testing.assert_allclose(res["cost"][0], ne.cost, rtol=1e-9)
    st = ba.schur_structure()
    assert np.array_equal(st["image_slot"], ne.pr["slot"])
    _check_blocks(ne, st, res)
    dpose, dpoint = _step(ba, res, ne, wc)
    # plus
    poses, points = ba.plus(torch.from_numpy(dpose).cuda(ba.device), torch.from_numpy(dpoint).cuda(ba.device))
    rp, rx = ref.plus(s, dpose, dpoint)
    _close(poses.cpu().numpy(), rp, 1e-14, "plus (poses)")
    _close(points.cpu().numpy(), rx, 1e-14, "plus (points)")
    cpose = np.flatnonzero(s["image_const_pose"]) if s.get("image_const_pose") is not None else []
    assert np.array_equal(poses.cpu().numpy()[cpose], np.asarray(s["poses"])[cpose])
    ba.close()


def test_schur_and_evaluate_share_the_normal_equations(gpu):
    """pcd_ba_evaluate and pcd_ba_schur reach the point and image passes through the same launches: on one handle the
    Schur call's cost is the evaluated cost bit for bit, and its S and rhs at mu = 0 are what the reference builds from
    the evaluated blocks -- W in the caller's order there, image-major inside the Schur call.  The scene
    (ref.shared_launch_scene) takes every launch: two point slices, two segments in one image, a constant pose, a
    constant point, LiDAR terms; test_ba_schur_cpu.py checks that the reference skips none of its 70 points."""
    s = ref.shared_launch_scene()
    ba = gpu.BA(**s)
    ev = ba.evaluate(("cost", "H_img", "g_img", "H_pt", "g_pt", "W"))
    ns = 2
    out = dict(cost=np.full(1, np.nan), rhs=np.full((ns, 6), np.nan), S=np.full((6 * ns, 6 * ns), np.nan),
               num_skipped=np.full(1, 2 ** 63, np.uint64))
    o = gpu.BASchurOut(*[gpu._ptr(out.get(n)) for n, _ in gpu.BASchurOut._fields_])
    gpu._check(gpu.lib().pcd_ba_schur(ba._h, C.byref(gpu.BASchurOpts(0.0, gpu.DAMP_MARQUARDT)), C.byref(o)))
    assert ba.schur_structure()["num_slots"] == ns
    assert out["cost"].view(np.uint64)[0] == ev["cost"].view(np.uint64)[0]
    ne = ref.NormalEquations(None, s, 0.0, blocks=[ev[k] for k in ("cost", "H_img", "g_img", "H_pt", "g_pt", "W")])
    assert not ne.skipped.any() and int(out["num_skipped"][0]) == 0
    sb = ne.schur_blocks()
    _close(out["S"], sb["S"], 1e-9, "dense S from the evaluated blocks")
    _close(out["rhs"], sb["rhs"], 1e-9, "rhs from the evaluated blocks")
    ba.close()


def test_structure_brute_force(gpu):
    s = _scene(7, I=10, P=400)
    ob_img, ob_pt = np.asarray(s["obs_image"]), np.asarray(s["obs_point"])
    s["obs_image"] = np.concatenate([ob_img, ob_img[:5]]).astype(np.int32)   # a few points seen twice by one image
    s["obs_point"] = np.concatenate([ob_pt, ob_pt[:5]]).astype(np.int32)
    s["obs_xy"] = np.concatenate([s["obs_xy"], s["obs_xy"][:5] + 3.0])
    ba = gpu.BA(**s)
    st = ba.schur_structure()
    slot = np.full(10, -1)
    var = np.flatnonzero(s["image_const_pose"] == 0)
    slot[var] = np.arange(var.size)
    assert np.array_equal(st["image_slot"], slot) and st["num_slots"] == var.size
    pairs = set()
    for p in range(400):
        if s["point_const"][p]:
            continue
        sl = sorted({int(slot[i]) for i in s["obs_image"][s["obs_point"] == p] if slot[i] >= 0})
        pairs |= {(a, b) for k, a in enumerate(sl) for b in sl[k + 1:]}
    assert [tuple(p) for p in st["pairs"]] == sorted(pairs)
    info = ba.schur_stats()
    assert info["build_ms"] > 0 and info["num_entries"] > 0
    ba.close()


def test_bitwise_repeatable(gpu):
    s = _scene(11, I=8, P=500, order="image")
    ba = gpu.BA(**s)
    dev = torch.device("cuda", ba.device)
    a = ba.schur(1e-3, dense=True)
    dpose = torch.linalg.solve(a["S"], a["rhs"].reshape(-1)).reshape(-1, 6)
    x1, m1 = ba.back_substitute(dpose)
    x1, m1 = x1.clone(), m1.clone()
    b = ba.schur(1e-3, dense=True)
    x2, m2 = ba.back_substitute(dpose)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(x1, x2) and torch.equal(m1, m2)
    assert x1.device == dev
    ba.close()


def test_rank_deficient_point_is_skipped(gpu, oracle):
    s = _scene(13, I=6, P=120)
    s["points"] = np.concatenate([s["points"], [[1.0, 2.0, 30.0]]])        # point 120: no observation, no LiDAR term
    s["point_const"] = np.concatenate([s["point_const"], [0]]).astype(np.uint8)
    ba, res = _run(gpu, s, 0.0, "marquardt")
    ne = ref.NormalEquations(oracle, s, 0.0, "marquardt")
    assert ne.skipped[120] and int(res["num_skipped"][0]) == int(ne.skipped.sum()) >= 1
    _check_blocks(ne, ba.schur_structure(), res)
    dpose = np.linalg.solve(res["S"], res["rhs"].reshape(-1)).reshape(-1, 6)
    dpoint, md = ba.back_substitute(torch.from_numpy(dpose).cuda(ba.device))
    assert not dpoint[120].any() and np.isfinite(dpoint.cpu().numpy()).all()
    ba.close()


def test_guards(gpu):
    s = _scene(17)
    s["camera_refine"] = gpu.camera_refine_mask(s["cam_model"], True, False, False)
    ba = gpu.BA(**s)
    z6 = torch.zeros((6, 6), dtype=torch.float64, device="cuda")
    z3 = torch.zeros((ba.P, 3), dtype=torch.float64, device="cuda")
    for call in (lambda: ba.schur_structure(), lambda: ba.schur(1e-3), lambda: ba.back_substitute(z6),
                 lambda: ba.plus(z6, z3)):
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    ba.close()
    s.pop("camera_refine")
    ba = gpu.BA(**s)
    with pytest.raises(gpu.PcdError) as e:
        ba.back_substitute(z6)
    assert e.value.status == gpu.PCD_ERR_INVALID          # no Schur call yet
    ba.close()


def test_capture_refused_then_eager_works(gpu):
    s = _scene(19)
    ba = gpu.BA(**s)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ref0 = ba.schur(1e-3, dense=True)                # eager: builds the structure
        dpose = torch.linalg.solve(ref0["S"], ref0["rhs"].reshape(-1)).reshape(-1, 6)
        x0, _ = ba.back_substitute(dpose)
        x0 = x0.clone()
        dpoint = torch.zeros_like(x0)
        poses_out = torch.empty((ba.I, 7), dtype=torch.float64, device="cuda")
        points_out = torch.empty((ba.P, 3), dtype=torch.float64, device="cuda")
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            calls = [lambda: ba.schur(1e-3, dense=True), lambda: ba.back_substitute(dpose, dpoint),
                     lambda: ba.plus(dpose, dpoint, poses_out, points_out),
                     lambda: ba.set_parameters_device(poses_out, points_out)]
            for call in calls:
                with pytest.raises(gpu.PcdError) as e:
                    call()
                assert e.value.status == gpu.PCD_ERR_UNSUPPORTED, str(e.value)
                assert "capturing" in str(e.value)
        finally:
            g.capture_end()
        again = ba.schur(1e-3, dense=True)
        x1, _ = ba.back_substitute(dpose)
        side.synchronize()
        for k in ref0:
            assert torch.equal(again[k], ref0[k]), k
        assert torch.equal(x1, x0)
    ba.close()


def test_config_b_sized_sample(gpu, oracle):
    """450 images / 400 k points (config B's size): a seeded sample of blocks against the reference"""
    s = synth.ba_scene(450, 400_000, seed=23, const_pose_frac=0.1, order="image")
    ba = gpu.BA(**s)
    out = ba.schur(1e-4)
    st = ba.schur_structure()
    ne = ref.NormalEquations(oracle, s, 1e-4)
    assert int(out["num_skipped"].item()) == int(ne.skipped.sum())
    Sd, So, rhs = out["S_diag"].cpu().numpy(), out["S_off"].cpu().numpy(), out["rhs"].cpu().numpy()
    rng = np.random.default_rng(5)
    for i in rng.choice(st["num_slots"], 6, replace=False):
        _close(Sd[i], ne.pair_block(i, i), 1e-9, f"S_diag[{i}]")
    for q in rng.choice(len(st["pairs"]), 12, replace=False):
        i, j = st["pairs"][q]
        _close(So[q], ne.pair_block(i, j), 1e-9, f"S_off[{i},{j}]")
    ba.close()


def _lm_scene():
    s = synth.ba_scene(12, 3000, seed=5, const_pose_frac=0.25)     # LiDAR terms on (lidar_frac 0.9)
    rng = np.random.default_rng(1005)
    s["points"] = s["points"] + rng.normal(0, 0.05, s["points"].shape)
    return s


def test_solve_lm_matches_numpy_lm(gpu, oracle):
    """ba_solve_lm against the same trust-region loop on the oracle; seed 5 keeps every rho far from 1e-3"""
    s = _lm_scene()
    want, final = ref.lm(oracle, s, 8)
    ba = gpu.BA(**s)
    got = gpu.ba_solve_lm(ba, max_iterations=8)
    assert [r["accepted"] for r in got] == [r["accepted"] for r in want]
    assert any(r["accepted"] for r in want) and not all(r["accepted"] for r in want)
    for g, w in zip(got, want):
        assert abs(w["rho"] - 1e-3) > 0.05
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
    costs = [r["cost"] for r in got]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    cost_final = ba.evaluate(("cost",))["cost"][0]
    np.testing.assert_allclose(cost_final, oracle.BA(**final).normal_equations()[0], rtol=1e-8)
    assert cost_final < got[0]["cost"]
    ba.close()

"""GPU tests of the direct reduced solve (pcd_ba_schur_solve_cholesky*, pcd_ba_solve with PCD_LINEAR_CHOLESKY,
ba_solve_lm(linear_solver="cholesky_hip"), BundleAdjusterHip with DIRECT / AUTO; csrc/ba_chol.hip).

Accuracy is asked as the backward error eta of tests/test_ba_chol_cpu.py against ETA_BOUND, which that module measures
on the numpy reference alone.  The sizes of the caller-supplied systems are built from SLOTS_PER_PANEL and every case
asserts info["panels"], so that a change of the panel width cannot silently move a case off its boundary.  Every test
prints its figures before it asserts."""
import os
import subprocess

import numpy as np
import pytest

from pcdhip import synth
from tests import ba_schur_ref as ref
from tests.test_ba_chol_cpu import ETA_BOUND, WELL_CONDITIONED, eta, first_failing_column
from tests.test_ba_pcg_gpu import _blocks, _case_scene, _lm_scene, _scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NB = 96                        # panel width of csrc/ba_chol.hip (kCholNB)
SLOTS_PER_PANEL = NB // 6
BOUNDARY_SLOTS = [1, SLOTS_PER_PANEL, SLOTS_PER_PANEL + 1, 3 * SLOTS_PER_PANEL + 1]
FAIL_SLOTS = 3 * SLOTS_PER_PANEL + 1


def _panels(ns):
    return -(-6 * ns // NB)


def _handle(gpu, ns):
    """a handle with exactly ns slots (no constant pose)"""
    ba = gpu.BA(**synth.ba_scene(ns, 40 * ns, seed=100 + ns))
    assert ba.schur_structure()["num_slots"] == ns
    return ba


def _system(ns):
    """S = G G^T + n I from a seeded G, x*, rhs = S x*"""
    n = 6 * ns
    rng = np.random.default_rng(7000 + ns)
    G = rng.normal(size=(n, n))
    S = G @ G.T + n * np.eye(n)
    S = 0.5 * (S + S.T)
    xs = rng.normal(size=n)
    return S, xs, S @ xs


def _lower_with_nan(S):
    """the lower triangle of S with NaN everywhere above the diagonal: the solve must not read it"""
    T = np.tril(S)
    T[np.triu_indices(S.shape[0], 1)] = np.nan
    return T


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dense(Sd, So, pairs):
    ns = Sd.shape[0]
    S = np.zeros((6 * ns, 6 * ns))
    for i in range(ns):
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Sd[i]
    for (i, j), blk in zip(pairs, So):
        S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blk
        S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = blk.T
    return S


@pytest.mark.parametrize("case", WELL_CONDITIONED)
def test_handles_own_blocks(gpu, case):
    s, mode, mu, wc = _case_scene(case)
    assert wc
    ba = gpu.BA(**s)
    Sd, So, pairs, rhs = _blocks(ba, mu, mode)
    x, info = ba.schur_solve_cholesky()
    xv = x.cpu().numpy()
    e = eta(_dense(Sd, So, pairs), rhs, xv)
    print(f"case {case}: n {rhs.size} eta {e:.3e} (bound {ETA_BOUND:.3e}) info {info}")
    assert info["status"] == gpu.CHOL_OK and info["failed_column"] == -1
    assert info["n"] == rhs.size and info["n_padded"] == NB * _panels(Sd.shape[0]) and info["panels"] == _panels(Sd.shape[0])
    assert e <= ETA_BOUND
    assert not xv[~ref.problem(s)["active"]].any()           # constant-tvec coordinates: exactly 0
    assert 0.0 < info["min_pivot"] <= info["max_pivot"]
    xh, ih = ba.schur_solve_cholesky_host()                   # the host form: the same solve, bit for bit
    assert np.array_equal(xh, xv) and ih == info
    ba.close()


@pytest.mark.parametrize("ns", BOUNDARY_SLOTS)
def test_panel_boundaries_with_callers_system(gpu, ns):
    ba = _handle(gpu, ns)
    S, xs, b = _system(ns)
    dS = _dev(_lower_with_nan(S))
    before = dS.clone()
    x, info = ba.schur_solve_cholesky(dS, _dev(b))
    xv = x.cpu().numpy().reshape(-1)
    e = eta(S, b, xv)
    d = np.diag(np.linalg.cholesky(S))       # the pivots: L's diagonal
    print(f"{ns} slots: n {6 * ns} panels {info['panels']} eta {e:.3e} (bound {ETA_BOUND:.3e}) "
          f"max |x - x*| {np.abs(xv - xs).max():.3e} pivots {info['min_pivot']:.6g} .. {info['max_pivot']:.6g}")
    assert info["status"] == gpu.CHOL_OK and info["failed_column"] == -1
    assert info["panels"] == _panels(ns) and info["n"] == 6 * ns and info["n_padded"] == NB * _panels(ns)
    assert info["n_padded"] // info["panels"] == NB          # the library's own panel width is the one assumed here
    assert np.isfinite(xv).all() and e <= ETA_BOUND
    np.testing.assert_allclose([info["min_pivot"], info["max_pivot"]], [d.min(), d.max()], rtol=1e-10)
    assert torch.equal(dS.view(torch.int64), before.view(torch.int64))       # the caller's matrix is not modified
    xh, ih = ba.schur_solve_cholesky_host(_lower_with_nan(S), b)
    assert np.array_equal(xh.reshape(-1), xv) and ih == info
    ba.close()


def test_larger_system(gpu):
    """450 slots (n = 2700): 29 panels, the full tile grid of the trailing update"""
    ns = 450
    ba = _handle(gpu, ns)
    S, xs, b = _system(ns)
    x, info = ba.schur_solve_cholesky(_dev(_lower_with_nan(S)), _dev(b))
    xv = x.cpu().numpy().reshape(-1)
    e = eta(S, b, xv)
    print(f"n {6 * ns} panels {info['panels']} eta {e:.3e} (bound {ETA_BOUND:.3e}) max |x - x*| {np.abs(xv - xs).max():.3e}")
    assert info["status"] == gpu.CHOL_OK and info["panels"] == _panels(ns) == 29
    assert e <= ETA_BOUND
    ba.close()


def test_failure_first_and_later_panel(gpu):
    ns = FAIL_SLOTS
    n = 6 * ns
    ba = _handle(gpu, ns)
    S, xs, b = _system(ns)
    L = np.linalg.cholesky(S)
    db = _dev(b)
    last = NB * (_panels(ns) - 1)
    assert _panels(ns) == 4 and last < n - 3
    for k in (5, n - 3):                       # a column of panel 0, a column of the last panel
        assert (k < NB) != (k >= last)
        T = _lower_with_nan(S)
        T[k, k] -= 2 * L[k, k] ** 2            # the pivot becomes -L_kk^2: far from rounding
        assert first_failing_column(np.tril(T)) == k
        x, info = ba.schur_solve_cholesky(_dev(T), db)
        print(f"pivot {k} lowered: {info}")
        assert info["status"] == gpu.CHOL_NOT_POSITIVE_DEFINITE and info["failed_column"] == k
        assert info["panels"] == 4
        xv = x.cpu().numpy()
        assert xv.shape == (ns, 6) and not xv.any() and not np.signbit(xv).any()
        # the state is not poisoned: the unmodified matrix solves right after
        x, info = ba.schur_solve_cholesky(_dev(_lower_with_nan(S)), db)
        assert info["status"] == gpu.CHOL_OK and info["failed_column"] == -1
        assert eta(S, b, x.cpu().numpy()) <= ETA_BOUND
    T = _lower_with_nan(S)
    T[100, 100] = np.nan
    x, info = ba.schur_solve_cholesky(_dev(T), db)
    assert info["status"] == gpu.CHOL_NOT_POSITIVE_DEFINITE and info["failed_column"] == 100
    assert not x.cpu().numpy().any()
    ba.close()


def test_bitwise_repeatable(gpu):
    ns = FAIL_SLOTS
    ba = _handle(gpu, ns)
    S, xs, b = _system(ns)
    dS, db = _dev(_lower_with_nan(S)), _dev(b)
    a, ia = ba.schur_solve_cholesky(dS, db)
    a = a.clone()
    c, ic = ba.schur_solve_cholesky(dS, db)
    assert torch.equal(a, c) and ia == ic and ia["panels"] == 4
    ba.close()


@pytest.fixture(scope="module")
def lm_reference(oracle):
    """ref.lm on the 12-image scene, computed once: (scene, history, cost at the final parameters)"""
    s = _lm_scene()
    want, final = ref.lm(oracle, s, 8)
    return s, want, oracle.BA(**final).normal_equations()[0]


def _check_lm(gpu, got, want):
    print("accepted", "".join("T" if r["accepted"] else "F" for r in got), "costs", [r["cost"] for r in got])
    assert [r["accepted"] for r in got] == [r["accepted"] for r in want]
    for g, w in zip(got, want):
        np.testing.assert_allclose(g["cost"], w["cost"], rtol=1e-8)
        np.testing.assert_allclose(g["radius"], w["radius"], rtol=1e-6)
        assert g["linear_iterations"] == 0 and g["linear_termination"] == gpu.CHOL_OK


@pytest.mark.parametrize("route", ["library", "python"])
def test_lm_parity(gpu, oracle, lm_reference, route):
    """pcd_ba_solve with the direct solver and ba_solve_lm with the library's solve in place of torch's, against the
    same loop on the oracle (np.linalg.cholesky)"""
    s, want, cost_final = lm_reference
    for w in want:
        assert abs(w["rho"] - 1e-3) > 0.05
    assert any(r["accepted"] for r in want) and not all(r["accepted"] for r in want)
    ba = gpu.BA(**s)
    if route == "library":
        summary, got = gpu.ba_solve(ba, max_num_iterations=8, linear_solver="cholesky")
        print(summary)
        assert summary["num_iterations"] == 8 and summary["termination"] == gpu.SOLVE_MAX_ITERATIONS
        assert summary["num_accepted"] == sum(r["accepted"] for r in want)
        assert summary["linear_solver_ms"] > 0
        np.testing.assert_allclose(summary["final_cost"], cost_final, rtol=1e-8)
    else:
        got = gpu.ba_solve_lm(ba, max_iterations=8, linear_solver="cholesky_hip")
    _check_lm(gpu, got, want)
    poses, points = ba.get_parameters()
    np.testing.assert_allclose(oracle.BA(**dict(s, poses=poses, points=points)).normal_equations()[0], cost_final, rtol=1e-8)
    ba.close()


def test_guards(gpu):
    s = _scene(17)
    ba = gpu.BA(**s)
    ns = ba.schur_structure()["num_slots"]
    S, xs, b = _system(ns)
    for kw in (dict(S=_dev(S)), dict(rhs=_dev(b))):            # one of the two without the other
        with pytest.raises(gpu.PcdError) as e:
            ba.schur_solve_cholesky(**kw)
        assert e.value.status == gpu.PCD_ERR_INVALID
    with pytest.raises(gpu.PcdError) as e:                     # the handle's own blocks: there are none yet
        ba.schur_solve_cholesky()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_solve_cholesky_host()
    assert e.value.status == gpu.PCD_ERR_INVALID and "no Schur state" in str(e.value)
    ba.schur(1e-3, want=("cost", "S_diag", "num_skipped"))     # S_diag went to caller memory
    with pytest.raises(gpu.PcdError) as e:
        ba.schur_solve_cholesky()
    assert e.value.status == gpu.PCD_ERR_INVALID and "S_diag" in str(e.value) and "S_off" not in str(e.value)
    _, info = ba.schur_solve_cholesky(_dev(S), _dev(b))        # a caller's system needs no Schur state
    assert info["status"] == gpu.CHOL_OK
    ba.schur(1e-3, want=("cost", "num_skipped"))
    _, info = ba.schur_solve_cholesky()
    assert info["status"] == gpu.CHOL_OK and info["panels"] == _panels(ns)
    with pytest.raises(gpu.PcdError) as e:
        gpu.ba_solve(ba, max_num_iterations=2, linear_solver=7)
    assert e.value.status == gpu.PCD_ERR_INVALID
    ba.close()
    s["camera_refine"] = gpu.camera_refine_mask(s["cam_model"], True, False, False)
    ba = gpu.BA(**s)
    for call in (lambda: ba.schur_solve_cholesky(_dev(S), _dev(b)), lambda: ba.schur_solve_cholesky_host(S, b),
                 lambda: gpu.ba_solve(ba, linear_solver="cholesky")):
        with pytest.raises(gpu.PcdError) as e:
            call()
        assert e.value.status == gpu.PCD_ERR_UNSUPPORTED
    ba.close()


def test_capture_refused_then_eager_works(gpu):
    s = _scene(19)
    ba = gpu.BA(**s)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ba.schur(1e-3, want=("cost", "num_skipped"))
        x0, i0 = ba.schur_solve_cholesky()
        x0 = x0.clone()
        buf = torch.empty_like(x0)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(gpu.PcdError) as e:
                ba.schur_solve_cholesky(dpose=buf)
            assert e.value.status == gpu.PCD_ERR_UNSUPPORTED and "capturing" in str(e.value)
        finally:
            g.capture_end()
        x1, i1 = ba.schur_solve_cholesky()
        side.synchronize()
        assert torch.equal(x1, x0) and i1 == i0 and i0["status"] == gpu.CHOL_OK
    ba.close()


def test_no_slots(gpu):
    s = _scene(41)
    s["image_const_pose"][:] = 1
    ba = gpu.BA(**s)
    ba.schur(1e-3, want=("cost", "num_skipped"))
    x, info = ba.schur_solve_cholesky()
    assert x.shape == (0, 6) and info["status"] == gpu.CHOL_OK and info["failed_column"] == -1 and info["panels"] == 0
    empty = torch.zeros((0, 0), dtype=torch.float64, device="cuda")
    x, info = ba.schur_solve_cholesky(empty, empty.reshape(0))
    assert x.shape == (0, 6) and info["status"] == gpu.CHOL_OK
    xh, ih = ba.schur_solve_cholesky_host()
    assert xh.shape == (0, 6) and ih["status"] == gpu.CHOL_OK
    summary, got = gpu.ba_solve(ba, max_num_iterations=2, linear_solver="cholesky")
    assert summary["num_iterations"] == 2 and all(r["linear_termination"] == gpu.CHOL_OK for r in got)
    ba.close()


def test_pcg_is_untouched(gpu):
    """a default-options ba_solve before and after Cholesky calls on the same handle: identical iteration records"""
    s = _lm_scene()
    poses0, points0 = np.array(s["poses"], np.float64), np.array(s["points"], np.float64)
    ba = gpu.BA(**s)
    _, before = gpu.ba_solve(ba, max_num_iterations=4)
    ba.set_parameters(poses0, points0)
    ba.schur(1e-4, want=("cost", "num_skipped"))
    _, info = ba.schur_solve_cholesky()
    assert info["status"] == gpu.CHOL_OK
    gpu.ba_solve(ba, max_num_iterations=2, linear_solver="cholesky")
    ba.set_parameters(poses0, points0)
    _, after = gpu.ba_solve(ba, max_num_iterations=4)
    assert len(before) == len(after) == 4 and any(r["linear_iterations"] > 0 for r in before)
    for a, c in zip(before, after):
        assert a == c, (a, c)
    ba.close()


def test_scratch_bytes(gpu):
    ns = SLOTS_PER_PANEL + 1
    ba = _handle(gpu, ns)
    S, xs, b = _system(ns)
    dS, db = _dev(S), _dev(b)
    base = ba.schur_stats()["scratch_bytes"]
    _, info = ba.schur_solve_cholesky(dS, db)
    first = ba.schur_stats()["scratch_bytes"]
    ba.schur_solve_cholesky(dS, db)
    second = ba.schur_stats()["scratch_bytes"]
    print(f"scratch bytes {base} -> {first} -> {second}, n_padded {info['n_padded']}")
    assert info["n_padded"] == 2 * NB
    assert first - base >= 8 * info["n_padded"] ** 2 and second == first
    ba.close()


def test_shim_direct_solve(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "colmap-pcd_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "shim/test_ba_cholesky"])
    r = subprocess.run([os.path.join(pkg, "shim", "test_ba_cholesky"), "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout

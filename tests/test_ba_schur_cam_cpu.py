"""The reference of the reduced system with refined intrinsics (tests/ba_schur_cam_ref.py) checked against itself, and
how the accuracy bound of the direct solve of the bordered system is measured; no GPU.

Cases: ba_schur_cam_ref.CAM_CASES (shared OPENCV focal only / all 8, PINHOLE all, FULL_OPENCV all 12, OPENCV +
SIMPLE_RADIAL all, OPENCV + SIMPLE_RADIAL with only camera 1 refined) on ba_schur_ref.camera_scene (I = 6, P = 150,
Cauchy loss), each at ba_schur_cam_ref.DAMPINGS.

The two routes (whole damped system by numpy.linalg.solve; block by block, then back-substitution) agree within 1e-9
where the system is well conditioned (Marquardt, mu = 1e-4: cond(S) 9e9 .. 1.7e11; measured agreement <= 1e-10).  With
Levenberg damping at mu = 0 and 1e-4 the gauge directions of these scenes are nearly free (cond(S) 1e14 .. 1e21, S not
even numerically positive definite in two cases at mu = 0): there the step of the block route is checked against the
bordered system it solves (the backward error below), not against another solve.

eta (tests/test_ba_chol_cpu.py) of np.linalg.cholesky plus two triangular substitutions on the bordered systems of all
those cases whose S numpy can factor (22 of 24), largest first: 2.2591e-15 (case 0, Levenberg 1e-4), 7.3639e-16
(case 5, Levenberg 1), 4.5887e-16 (case 2, Levenberg 0).  ETA_CAM_REFERENCE is that largest value with the last digit
rounded up; ETA_CAM_BOUND = 100 x it, the project's customary margin for a different order of the sums.  The bound
comes from the reference alone, not from the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ba_schur_cam_ref as cref
from tests.test_ba_chol_cpu import cholesky_solve, eta

ETA_CAM_REFERENCE = 2.2592e-15           # largest eta of the reference over the cases, see above
ETA_CAM_BOUND = 100 * ETA_CAM_REFERENCE  # 2.2592e-13

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pcdhip.h")
NEW_SYMBOLS = ("pcd_ba_camera_slots", "pcd_ba_schur_cam_device", "pcd_ba_schur_cam", "pcd_ba_schur_cam_solve_cholesky_device",
               "pcd_ba_schur_cam_back_substitute_device", "pcd_ba_plus_cam_device", "pcd_ba_get_camera_parameters")


def _close(a, b, rtol, what):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, err_msg=what)


@pytest.fixture(scope="module")
def systems(oracle):
    """(case, mode, mu) -> (CamNormalEquations, its blocks), computed once"""
    out = {}
    for case in range(len(cref.CAM_CASES)):
        for mode, mu in cref.DAMPINGS:
            s, refine = cref.cam_case_scene(oracle, case)
            ne = cref.CamNormalEquations(oracle, s, refine, mu, mode)
            out[(case, mode, mu)] = (ne, ne.schur_cam_blocks())
    return out


def test_the_two_routes_agree(systems):
    for (case, mode, mu), (ne, sb) in systems.items():
        n = 6 * ne.pr["slot_img"].size + 12 * ne.ncs
        assert sb["S"].shape == (n, n) and sb["rhs_full"].shape == (n,)
        _close(sb["S"], sb["S"].T, 1e-12, "S is symmetric")
        dead = np.concatenate([~ne.pr["active"].reshape(-1), ~ne.cam_active.reshape(-1)])
        assert np.array_equal(sb["S"][dead][:, dead], np.eye(int(dead.sum()))) and not sb["rhs_full"][dead].any()
        assert not sb["S"][dead][:, ~dead].any()
        if mode not in cref.WELL_CONDITIONED:
            continue
        dpose, dcam = ne.split(np.linalg.solve(sb["S"], sb["rhs_full"]))
        dpoint = ne.back_substitute_cam(dpose, dcam)
        rp, rc, rx = ne.dense_solve_cam()
        print(f"case {case} {mode} {mu}: ncs {ne.ncs} cond {np.linalg.cond(sb['S']):.2e}")
        _close(dpose, rp, 1e-9, "pose step")
        _close(dcam, rc, 1e-9, "camera step")
        _close(dpoint, rx, 1e-9, "point step")
        assert not dcam[~ne.cam_active].any()


def test_camera_slots_of_the_cases(oracle):
    ncs = []
    for case in range(len(cref.CAM_CASES)):
        s, refine = cref.cam_case_scene(oracle, case)
        slot, slot_cam, active, _ = cref.camera_slots(s, refine)
        ncs.append((slot.tolist(), active.sum(axis=1).tolist()))
    assert ncs == [([0], [2]), ([0], [8]), ([0], [4]), ([0], [12]), ([0, 1], [8, 4]), ([-1, 0], [4])]


def test_eta_of_the_reference(systems):
    """the measurement ETA_CAM_BOUND comes from, repeated"""
    worst, solved = 0.0, 0
    for (case, mode, mu), (ne, sb) in systems.items():
        try:
            x = cholesky_solve(sb["S"], sb["rhs_full"])
        except np.linalg.LinAlgError:
            print(f"case {case} {mode} {mu}: S is not numerically positive definite")
            continue
        e = eta(sb["S"], sb["rhs_full"], x)
        print(f"case {case} {mode} {mu}: n {x.size} eta {e:.4e}")
        worst, solved = max(worst, e), solved + 1
    print(f"largest eta of the reference {worst:.4e} over {solved} systems")
    assert solved >= 20
    # pinned from both sides: a much smaller eta of another numpy would leave ETA_CAM_BOUND far above 100 x the measurement
    assert 0.5 * ETA_CAM_REFERENCE <= worst <= ETA_CAM_REFERENCE
    assert ETA_CAM_BOUND == 100 * ETA_CAM_REFERENCE


def test_new_symbols_are_exported_and_declared(pcdhip):
    lib = pcdhip.lib()
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bpcd_status\s+" + name + r"\s*\(", text), name
    assert "#define PCD_BA_MAX_CAMERA_SLOTS 8" in text and pcdhip.MAX_CAMERA_SLOTS == 8
    for m in ("camera_slots", "schur_cam", "schur_cam_solve_cholesky", "back_substitute_cam", "plus_cam",
              "get_camera_parameters"):
        assert callable(getattr(pcdhip.BA, m)), m


def test_solve_opts_size_is_unchanged(pcdhip, tmp_path):
    """refine_intrinsics came out of reserved: 152 bytes as before (the binding's own assertion pins the Python side), the
    flag sits right behind linear_solver, and the defaults leave it 0"""
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pcdhip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(pcd_ba_solve_opts), '
                   'offsetof(pcd_ba_solve_opts, linear_solver), offsetof(pcd_ba_solve_opts, refine_intrinsics)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)])
    size, off_ls, off_ri = map(int, subprocess.check_output([str(exe)]).split())
    assert size == 152 == C.sizeof(pcdhip.BASolveOpts)
    assert off_ri == off_ls + 4 == pcdhip.BASolveOpts.refine_intrinsics.offset
    o = pcdhip.BASolveOpts()
    o.refine_intrinsics = 7
    pcdhip.lib().pcd_ba_solve_opts_default(C.byref(o))
    assert o.refine_intrinsics == 0 and o.linear_solver == pcdhip.LINEAR_PCG

"""How the accuracy bound of the direct reduced solve (pcd_ba_schur_solve_cholesky*) is measured; no GPU.

The measure is the normwise backward error of a solution x of S x = b,
    eta(S, b, x) = ||S x - b||_inf / (||S||_inf ||x||_inf + ||b||_inf),
which a backward-stable solver keeps at a small multiple of the unit roundoff whatever cond(S) is (1e8 ... 1e11 on
these systems), so it can be asked of the device without asking it to round like numpy.

The reference: S and rhs from the oracle (ba_schur_ref.NormalEquations.schur_blocks()) on the scenes of
tests/test_ba_pcg_gpu.CASES whose "well conditioned" flag is set, solved by np.linalg.cholesky and two triangular
substitutions.  Its eta per case: 2.86684e-17 (case 0), 1.0621e-18 (1), 7.7256e-19 (2), 1.1982e-18 (3), 2.1440e-18 (8).
Largest value measured: 2.86684e-17, 2.8669e-17 with the last digit rounded up.  ETA_BOUND = 100 x 2.8669e-17 =
2.8669e-15, the project's customary margin for a different order of the sums (the device factors in panels of 96
columns, right-looking, and scales a column by the reciprocal of its pivot's root).  The bound comes from the
reference alone, not from the device."""
import numpy as np

from tests import ba_schur_ref as ref
from tests.test_ba_pcg_gpu import CASES, _case_scene

ETA_REFERENCE = 2.8669e-17       # largest eta of the reference over the well-conditioned cases, see above
ETA_BOUND = 100 * ETA_REFERENCE  # 2.8669e-15

WELL_CONDITIONED = [c for c in range(len(CASES)) if CASES[c][6]]


def eta(S, b, x):
    S, b, x = np.asarray(S, np.float64), np.asarray(b, np.float64).reshape(-1), np.asarray(x, np.float64).reshape(-1)
    if b.size == 0:
        return 0.0
    return float(np.abs(S @ x - b).max() / (np.abs(S).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def cholesky_solve(S, b):
    """np.linalg.cholesky, then forward and backward substitution row by row"""
    L = np.linalg.cholesky(S)
    n = b.size
    y, x = np.zeros(n), np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def first_failing_column(S):
    """the column at which an unblocked Cholesky of the lower triangle meets a pivot that is <= 0 or not finite; -1: none"""
    A = np.tril(np.array(S, np.float64))
    n = A.shape[0]
    for j in range(n):
        with np.errstate(invalid="ignore"):
            piv = A[j, j] - A[j, :j] @ A[j, :j]
        if not (piv > 0.0 and np.isfinite(piv)):
            return j
        A[j, j] = np.sqrt(piv)
        A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    return -1


def test_eta_of_the_reference(oracle):
    """the measurement ETA_BOUND comes from, repeated"""
    assert WELL_CONDITIONED == [0, 1, 2, 3, 8]
    worst = 0.0
    for case in WELL_CONDITIONED:
        s, mode, mu, _ = _case_scene(case)
        sb = ref.NormalEquations(oracle, s, mu, mode).schur_blocks()
        S, b = sb["S"], sb["rhs"].reshape(-1)
        e = eta(S, b, cholesky_solve(S, b))
        print(f"case {case}: n {b.size} cond {np.linalg.cond(S):.2e} eta {e:.4e}")
        worst = max(worst, e)
    print(f"largest eta of the reference {worst:.4e}")
    # pinned from both sides: a much smaller eta of another numpy would leave ETA_BOUND far above 100 x the measurement
    assert 0.5 * ETA_REFERENCE <= worst <= ETA_REFERENCE
    assert ETA_BOUND == 100 * ETA_REFERENCE


def test_eta_is_a_backward_error():
    """eta is 0 for the exact solution of an exactly representable system, scale-free, and grows with a perturbation"""
    S = np.array([[4.0, 2.0], [2.0, 5.0]])
    x = np.array([1.0, -2.0])
    b = S @ x
    assert eta(S, b, x) == 0.0
    assert eta(1024 * S, 1024 * b, x) == 0.0
    e = eta(S, b, x + np.array([1e-8, 0.0]))
    assert 1e-9 < e < 1e-8
    np.testing.assert_allclose(eta(S, b, cholesky_solve(S, b)), 0.0, atol=1e-16)


def test_first_failing_column():
    rng = np.random.default_rng(3)
    G = rng.normal(size=(20, 20))
    S = G @ G.T + 20 * np.eye(20)
    assert first_failing_column(S) == -1
    L = np.linalg.cholesky(S)
    for k in (0, 7, 19):
        T = S.copy()
        T[k, k] -= 2 * L[k, k] ** 2
        assert first_failing_column(T) == k
    T = S.copy()
    T[5, 5] = np.nan
    assert first_failing_column(T) == 5

"""numpy reference of the block-sparse preconditioned CG on the reduced camera system (pcd_ba_schur_solve_pcg*,
include/pcdhip.h) and of the LM loop that uses it (pcd_ba_solve, ba_solve_lm(linear_solver="pcg")).

The system is given as block lists, the form the device keeps: S_diag [ns][6][6], S_off [npairs][6][6] for the slot
pairs i < j (ascending), rhs [ns][6].  The product walks every slot's row: the transposes of its (k, i) blocks, its
diagonal block and its (i, j) blocks, in ascending or descending partner slot (the switch measures how much the result
depends on the order of the sums; the device's own order differs from both by its lane-strided partial sums).
Test infrastructure: Python loops over blocks, small scenes only."""
import numpy as np

from tests import ba_schur_ref as ref

IDENTITY, SCHUR_JACOBI = 0, 1
MAX_ITERATIONS, Q_TOLERANCE, R_TOLERANCE, BREAKDOWN, ZERO_RHS = range(5)
DEFAULTS = dict(max_iterations=100, min_iterations=0, preconditioner=SCHUR_JACOBI, q_tolerance=0.1, r_tolerance=-1.0)


def rows(ns, pairs):
    """row lists: for slot i the (block, transposed, partner) of its row, ascending partner; block = ('d', i) or
    ('o', q)"""
    out = [[] for _ in range(ns)]
    for q, (i, j) in enumerate(pairs):
        out[j].append((("o", q), True, int(i)))
    for i in range(ns):
        out[i].append((("d", i), False, i))
    for q, (i, j) in enumerate(pairs):
        out[i].append((("o", q), False, int(j)))
    for i in range(ns):
        assert [e[2] for e in out[i]] == sorted(e[2] for e in out[i])
    return out


def product(S_diag, S_off, row_lists, x, descending=False):
    y = np.zeros_like(x)
    for i, lst in enumerate(row_lists):
        acc = np.zeros(6)
        for (kind, b), tr, j in (reversed(lst) if descending else lst):
            B = S_diag[b] if kind == "d" else S_off[b]
            acc = acc + (B.T if tr else B) @ x[j]
        y[i] = acc
    return y


def block_inverse(A):
    """inverse of a 6x6 block through its Cholesky factor, in the device's operation order; None when a pivot is not
    positive and finite"""
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j] - sum(L[j, k] * L[j, k] for k in range(j))
        if not (d > 0.0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        for a in range(j + 1, 6):
            L[a, j] = (A[a, j] - sum(L[a, k] * L[j, k] for k in range(j))) / L[j, j]
    M = np.zeros((6, 6))
    for j in range(6):
        M[j, j] = 1.0 / L[j, j]
        for a in range(j + 1, 6):
            M[a, j] = -sum(L[a, k] * M[k, j] for k in range(j, a)) / L[a, a]
    return M.T @ M


def preconditioner(S_diag, kind):
    """(M^-1 [ns][6][6], number of identity fallbacks)"""
    ns = S_diag.shape[0]
    Minv = np.tile(np.eye(6), (ns, 1, 1))
    fallbacks = 0
    if kind == SCHUR_JACOBI:
        for i in range(ns):
            inv = block_inverse(S_diag[i])
            if inv is None:
                fallbacks += 1
            else:
                Minv[i] = inv
    return Minv, fallbacks


def pcg(S_diag, S_off, pairs, rhs, max_iterations=100, min_iterations=0, preconditioner=SCHUR_JACOBI, q_tolerance=0.1,
        r_tolerance=-1.0, descending=False):
    """the PCG of include/pcdhip.h from x = 0.  Returns dict(x, iterations, termination, q, residual_norm, rhs_norm,
    step_dot_residual, zetas, precond_fallbacks)"""
    S_diag, S_off, rhs = np.asarray(S_diag, np.float64), np.asarray(S_off, np.float64), np.asarray(rhs, np.float64)
    ns = rhs.shape[0]
    rl = rows(ns, pairs)
    Minv, fb = globals()["preconditioner"](S_diag, preconditioner)
    x, r = np.zeros_like(rhs), rhs.copy()
    bb = float(np.sum(rhs * rhs))
    out = dict(x=x, iterations=0, termination=MAX_ITERATIONS, q=0.0, residual_norm=np.sqrt(bb), rhs_norm=np.sqrt(bb),
               step_dot_residual=0.0, zetas=[], precond_fallbacks=fb)
    if bb == 0.0:
        out["termination"] = ZERO_RHS
        return out
    z = np.einsum("iab,ib->ia", Minv, r)
    rho = float(np.sum(r * z))
    if not (np.isfinite(bb) and rho > 0.0 and np.isfinite(rho)):
        out["termination"] = BREAKDOWN
        return out
    if max_iterations <= 0:
        return out
    p = np.zeros_like(rhs)
    beta, q_prev, k = 0.0, 0.0, 0
    while True:
        p = z + beta * p
        w = product(S_diag, S_off, rl, p, descending)
        pw = float(np.sum(p * w))
        with np.errstate(all="ignore"):
            alpha = rho / pw if pw != 0.0 else np.inf
        if not (pw > 0.0 and np.isfinite(alpha)):
            out["termination"] = BREAKDOWN
            return out
        x_new = x + alpha * p
        r = r - alpha * w
        z = np.einsum("iab,ib->ia", Minv, r)
        rz, rr = float(np.sum(r * z)), float(np.sum(r * r))
        q = -0.5 * float(np.sum(x_new * (rhs + r)))
        if not (rz >= 0.0 and np.isfinite(rz) and np.isfinite(rr) and np.isfinite(q)):
            out["termination"] = BREAKDOWN
            return out
        x = x_new
        k += 1
        zeta = k * (q - q_prev) / q
        out["zetas"].append(zeta)
        out.update(x=x, iterations=k, q=q, residual_norm=np.sqrt(rr), step_dot_residual=float(np.sum(x * r)))
        if k >= min_iterations and q_tolerance >= 0.0 and zeta < q_tolerance:
            out["termination"] = Q_TOLERANCE
            return out
        if k >= min_iterations and r_tolerance >= 0.0 and np.sqrt(rr) <= r_tolerance * out["rhs_norm"]:
            out["termination"] = R_TOLERANCE
            return out
        if k >= max_iterations:
            out["termination"] = MAX_ITERATIONS
            return out
        beta, rho, q_prev = rz / rho, rz, q


# ---- the device's own operation order -----------------------------------------------------------------------------
# numpy's reductions (np.sum pairwise, BLAS mat-vec with fused multiply-adds) round in an order numpy chooses.  On the
# ill-conditioned reduced systems a last-bit difference in a CG scalar grows by many orders of magnitude in x within a
# few iterations, so a parity check at the level of the order sensitivity needs a reference whose every sum is in a
# stated order.  pcg_device_order() is the same algorithm with the order csrc/ba_pcg.hip documents: sums over the 6
# coordinates of a slot sequentially from 0, slots combined per 256-thread workgroup by the xor butterfly of each
# 64-lane wavefront and (w0 + w1) + (w2 + w3), workgroup partials strided over 256 threads and combined the same way,
# a row's blocks lane-strided and combined by the butterfly, no fused multiply-add (as ba_schur_ref.point_inverse
# follows k_schur_points' order).
_LANE = np.arange(64)


def _wave_tree(v):
    """xor butterfly over the last axis (64 lanes): what every lane holds at the end"""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ off]
    return v[..., 0]


def _block_sum256(v):
    """sum of up to 256 per-thread values in the order of block_sum256"""
    t = np.zeros(256)
    t[:len(v)] = v
    w = _wave_tree(t.reshape(4, 64))
    return float((w[0] + w[1]) + (w[2] + w[3]))


def _sum_strided(v):
    """block_sum_strided: thread t adds v[t], v[t + 256], ... in turn, then block_sum256"""
    v = np.asarray(v, np.float64)
    a = np.zeros(256)
    for m in range(0, len(v), 256):
        c = v[m:m + 256]
        a[:len(c)] = a[:len(c)] + c
    return _block_sum256(a)


def _sum_slots(per_slot):
    """a per-slot quantity summed as k_pcg_init / k_pcg_update (one partial per 256 slots) and k_pcg_begin / k_pcg_step"""
    per_slot = np.asarray(per_slot, np.float64)
    if per_slot.size == 0:
        return 0.0
    return _sum_strided([_block_sum256(per_slot[m:m + 256]) for m in range(0, len(per_slot), 256)])


def _seq6(terms):
    """[ns][6] -> [ns]: sequential sum over the coordinates from 0.0"""
    s = np.zeros(terms.shape[0])
    for k in range(terms.shape[1]):
        s = s + terms[:, k]
    return s


def _matvec6(M, v):
    """[ns][6][6] x [ns][6], every row a sequential sum over the columns from 0.0"""
    out = np.zeros_like(v)
    for c in range(6):
        out = out + M[:, :, c] * v[:, c][:, None]
    return out


def _block_inverse_device_order(A):
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not (d > 0.0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        for a in range(j + 1, 6):
            t = A[a, j]
            for k in range(j):
                t = t - L[a, k] * L[j, k]
            L[a, j] = t / L[j, j]
    M = np.zeros((6, 6))
    for j in range(6):
        M[j, j] = 1.0 / L[j, j]
        for a in range(j + 1, 6):
            t = 0.0
            for k in range(j, a):
                t = t + L[a, k] * M[k, j]
            M[a, j] = -t / L[a, a]
    inv = np.zeros((6, 6))
    for a in range(6):
        for c in range(a + 1):
            t = 0.0
            for k in range(a, 6):
                t = t + M[k, a] * M[k, c]
            inv[a, c] = inv[c, a] = t
    return inv


def _product_device_order(S_diag, S_off, row_lists, x):
    y = np.zeros_like(x)
    for i, lst in enumerate(row_lists):
        lanes = np.zeros((6, 64))
        for t, ((kind, b), tr, j) in enumerate(lst):
            B = S_diag[b] if kind == "d" else S_off[b]
            B = B.T if tr else B
            s = np.zeros(6)
            for c in range(6):
                s = s + B[:, c] * x[j, c]
            lanes[:, t % 64] = lanes[:, t % 64] + s
        y[i] = _wave_tree(lanes)
    return y


def pcg_device_order(S_diag, S_off, pairs, rhs, max_iterations=100, min_iterations=0, preconditioner=SCHUR_JACOBI,
                     q_tolerance=0.1, r_tolerance=-1.0):
    """pcg() with every sum in the device's stated order (see above); same return value"""
    S_diag, S_off, rhs = np.asarray(S_diag, np.float64), np.asarray(S_off, np.float64), np.asarray(rhs, np.float64)
    ns = rhs.shape[0]
    rl = rows(ns, pairs)
    Minv = np.tile(np.eye(6), (ns, 1, 1))
    fb = 0
    if preconditioner == SCHUR_JACOBI:
        for i in range(ns):
            inv = _block_inverse_device_order(S_diag[i])
            if inv is None:
                fb += 1
            else:
                Minv[i] = inv
    x, r = np.zeros_like(rhs), rhs.copy()
    z = _matvec6(Minv, r)
    rho, bb = _sum_slots(_seq6(r * z)), _sum_slots(_seq6(r * r))
    out = dict(x=x, iterations=0, termination=MAX_ITERATIONS, q=0.0, residual_norm=np.sqrt(bb), rhs_norm=np.sqrt(bb),
               step_dot_residual=0.0, zetas=[], precond_fallbacks=fb)
    if not bb > 0.0:
        out["termination"] = ZERO_RHS if bb == 0.0 else BREAKDOWN
        return out
    if not (rho > 0.0 and np.isfinite(rho)):
        out["termination"] = BREAKDOWN
        return out
    if max_iterations <= 0:
        return out
    p = np.zeros_like(rhs)
    beta, q_prev, k = 0.0, 0.0, 0
    while True:
        p = z + beta * p
        w = _product_device_order(S_diag, S_off, rl, p)
        pw = _sum_strided(_seq6(p * w))
        with np.errstate(all="ignore"):
            alpha = np.float64(rho) / np.float64(pw)
        if not (pw > 0.0 and np.isfinite(alpha)):
            out["termination"] = BREAKDOWN
            return out
        x_new = x + alpha * p
        r = r - alpha * w
        z = _matvec6(Minv, r)
        rz, rr = _sum_slots(_seq6(r * z)), _sum_slots(_seq6(r * r))
        xbr, xr = _sum_slots(_seq6(x_new * (rhs + r))), _sum_slots(_seq6(x_new * r))
        q = -0.5 * xbr
        if not (rz >= 0.0 and np.isfinite(rz) and np.isfinite(rr) and np.isfinite(q)):
            out["termination"] = BREAKDOWN
            return out
        x = x_new
        k += 1
        zeta = k * (q - q_prev) / q
        out["zetas"].append(zeta)
        out.update(x=x, iterations=k, q=q, residual_norm=np.sqrt(rr), step_dot_residual=xr)
        if k >= min_iterations and q_tolerance >= 0.0 and zeta < q_tolerance:
            out["termination"] = Q_TOLERANCE
            return out
        if k >= min_iterations and r_tolerance >= 0.0 and np.sqrt(rr) <= r_tolerance * out["rhs_norm"]:
            out["termination"] = R_TOLERANCE
            return out
        if k >= max_iterations:
            out["termination"] = MAX_ITERATIONS
            return out
        beta, rho, q_prev = rz / rho, rz, q


def block_lists(sb):
    """(S_diag, S_off [npairs][6][6], pairs, rhs) of NormalEquations.schur_blocks()"""
    off = np.stack([sb["S_off"][tuple(p)] for p in sb["pairs"]]) if len(sb["pairs"]) else np.zeros((0, 6, 6))
    return sb["S_diag"], off, sb["pairs"], sb["rhs"]


def true_residual(S_diag, S_off, pairs, rhs, x):
    """||rhs - S x|| / ||rhs|| by a block product (no dense S)"""
    y = product(np.asarray(S_diag), np.asarray(S_off), rows(rhs.shape[0], pairs), np.asarray(x))
    return float(np.linalg.norm(rhs - y) / np.linalg.norm(rhs))


def lm_pcg(oracle, scene, max_iterations, initial_radius=1e4, mode="marquardt", min_relative_decrease=1e-3,
           max_radius=1e16, **pcg_opts):
    """ba_schur_ref.lm with the PCG above as the linear solver (a BREAKDOWN is a rejected step).  Returns (history,
    final scene); every record also has linear_iterations, linear_termination and zetas."""
    scene = dict(scene)
    radius, factor = float(initial_radius), 2.0
    hist = []
    for _ in range(max_iterations):
        ne = ref.NormalEquations(oracle, scene, 1.0 / radius, mode)
        sol = pcg(*block_lists(ne.schur_blocks()), **pcg_opts)
        rec = dict(cost=ne.cost, candidate_cost=np.nan, rho=np.nan, accepted=False,
                   linear_iterations=sol["iterations"], linear_termination=sol["termination"], zetas=sol["zetas"])
        cand = None
        if sol["termination"] != BREAKDOWN:
            dpose = sol["x"]
            dpoint = ne.back_substitute(dpose)
            model = ne.model_decrease(dpose, dpoint)
            poses, points = ref.plus(scene, dpose, dpoint)
            cand = dict(scene, poses=poses, points=points)
            new_cost = oracle.BA(**cand).normal_equations()[0]
            rho = (ne.cost - new_cost) / model if model > 0 else -np.inf
            rec.update(candidate_cost=new_cost, rho=rho, accepted=bool(rho > min_relative_decrease))
        if rec["accepted"]:
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rec["rho"] - 1.0) ** 3))
            factor = 2.0
            scene = cand
        else:
            radius /= factor
            factor *= 2.0
        rec["radius"] = radius
        hist.append(rec)
    return hist, scene

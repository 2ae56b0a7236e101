"""numpy reference of the bordered PCG (pcd_ba_schur_cam_solve_pcg*, include/pcdhip.h) and of the LM loop
that uses it (pcd_ba_solve with PCD_LINEAR_PCG_CAM), built by import on tests/ba_pcg_ref.py (the plain PCG) and
tests/ba_schur_cam_ref.py (the bordered blocks).

The system: S = [[S_pose, B^T], [B, S_cam]] on x = [dpose (6 ns) | dcam (12 ncs)], b = [rhs | rhs_cam], as block lists:
S_diag / S_off / pairs / rhs of ba_pcg_ref, B [ns][ncs][12][6], S_cam [ncs][ncs][12][12], rhs_cam [ncs][12].

  pcg_cam               numpy's own summation order; `descending` walks the pose row lists, the slots of the camera-row sum
                        and the camera slots of the border term in descending order (the order-sensitivity switch)
  pcg_cam_device_order  every sum in the order csrc/ba_pcg.hip states for k_pcg_cam_init, k_pcg_cam_spmv,
                        k_pcg_cam_rows and k_pcg_cam_update (and for the plain kernels of the pose part), no fused multiply-add
  lm_cam_pcg            ba_schur_cam_ref.lm_cam with pcg_cam as its linear solver (a BREAKDOWN is a rejected step)
With ncs = 0 the first two are ba_pcg_ref.pcg / pcg_device_order bit for bit.  Test infrastructure: small scenes only."""
import numpy as np

from tests import ba_pcg_ref as pr
from tests import ba_schur_cam_ref as cref
from tests.ba_pcg_ref import BREAKDOWN, IDENTITY, MAX_ITERATIONS, Q_TOLERANCE, R_TOLERANCE, SCHUR_JACOBI, ZERO_RHS  # noqa: F401

S12 = cref.S12


def cam_block_lists(sb):
    """(S_diag, S_off, pairs, rhs, B, S_cam, rhs_cam) of CamNormalEquations.schur_cam_blocks()"""
    return pr.block_lists(sb) + (sb["B"], sb["S_cam"], sb["rhs_cam"])


def _arrays(S_diag, S_off, rhs, B, S_cam, rhs_cam):
    rhs = np.asarray(rhs, np.float64).reshape(-1, 6)
    ns = rhs.shape[0]
    rhs_cam = np.asarray(rhs_cam, np.float64).reshape(-1, S12)
    ncs = rhs_cam.shape[0]
    return (np.asarray(S_diag, np.float64).reshape(ns, 6, 6), np.asarray(S_off, np.float64).reshape(-1, 6, 6), rhs,
            np.asarray(B, np.float64).reshape(ns, ncs, S12, 6), np.asarray(S_cam, np.float64).reshape(ncs, ncs, S12, S12),
            rhs_cam, ns, ncs)


def block_inverse_n(A, device_order=False):
    """inverse of an n x n block through its Cholesky factor in the operation order of k_pcg_init (n = 6) and
    k_pcg_cam_init (n = 12); None when a pivot is not positive and finite.  device_order: every sum sequential from its
    first term; otherwise Python's sum() over the same terms (the form of ba_pcg_ref.block_inverse)."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        if device_order:
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
        else:
            d = A[j, j] - sum(L[j, k] * L[j, k] for k in range(j))
        if not (d > 0.0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        for a in range(j + 1, n):
            if device_order:
                t = A[a, j]
                for k in range(j):
                    t = t - L[a, k] * L[j, k]
            else:
                t = A[a, j] - sum(L[a, k] * L[j, k] for k in range(j))
            L[a, j] = t / L[j, j]
    M = np.zeros((n, n))
    for j in range(n):
        M[j, j] = 1.0 / L[j, j]
        for a in range(j + 1, n):
            t = 0.0
            for k in range(j, a):
                t = t + L[a, k] * M[k, j]
            M[a, j] = -t / L[a, a]
    if not device_order:
        return M.T @ M
    inv = np.zeros((n, n))
    for a in range(n):
        for c in range(a + 1):
            t = 0.0
            for k in range(a, n):
                t = t + M[k, a] * M[k, c]
            inv[a, c] = inv[c, a] = t
    return inv


def cam_preconditioner(S_cam, kind, device_order=False):
    """(M_cam^-1 [ncs][12][12] of the diagonal blocks S_cam[r][r], number of identity fallbacks)"""
    ncs = S_cam.shape[0]
    Minv = np.tile(np.eye(S12), (ncs, 1, 1))
    fb = 0
    if kind == SCHUR_JACOBI:
        for r in range(ncs):
            inv = block_inverse_n(S_cam[r, r], device_order)
            if inv is None:
                fb += 1
            else:
                Minv[r] = inv
    return Minv, fb


def product_cam(S_diag, S_off, row_lists, B, S_cam, p, pc, descending=False):
    """(w_pose [ns][6], w_cam [ncs][12]) of the bordered product"""
    ns, ncs = p.shape[0], pc.shape[0]
    w = pr.product(S_diag, S_off, row_lists, p, descending)
    wc = np.zeros_like(pc)
    order_r = range(ncs - 1, -1, -1) if descending else range(ncs)
    for i in (range(ns - 1, -1, -1) if descending else range(ns)):
        acc = np.zeros(6)
        for r in order_r:
            acc = acc + B[i, r].T @ pc[r]
        w[i] = w[i] + acc
        wc = wc + B[i] @ p[i]
    acc = np.zeros_like(pc)
    for q in order_r:
        acc = acc + np.einsum("rab,b->ra", S_cam[:, q], pc[q])
    return w, wc + acc


def _finish(out, ns):
    out["x_pose"], out["x_cam"] = out["x"][:6 * ns].reshape(ns, 6), out["x"][6 * ns:].reshape(-1, S12)
    return out


def pcg_cam(S_diag, S_off, pairs, rhs, B, S_cam, rhs_cam, max_iterations=100, min_iterations=0,
            preconditioner=SCHUR_JACOBI, q_tolerance=0.1, r_tolerance=-1.0, descending=False):
    """ba_pcg_ref.pcg on the bordered system.  Returns its dict with x [6 ns + 12 ncs] (and x_pose, x_cam views)."""
    S_diag, S_off, rhs, B, S_cam, rhs_cam, ns, ncs = _arrays(S_diag, S_off, rhs, B, S_cam, rhs_cam)
    if ncs == 0:
        out = pr.pcg(S_diag, S_off, pairs, rhs, max_iterations, min_iterations, preconditioner, q_tolerance, r_tolerance,
                     descending)
        out["x"] = out["x"].reshape(-1)
        return _finish(out, ns)
    rl = pr.rows(ns, pairs)
    Minv, fb = pr.preconditioner(S_diag, preconditioner)
    Mc, fbc = cam_preconditioner(S_cam, preconditioner)
    cat = lambda a, c: np.concatenate([a.reshape(-1), c.reshape(-1)])   # noqa: E731
    b = cat(rhs, rhs_cam)
    bb = float(np.sum(b * b))
    out = dict(x=np.zeros_like(b), iterations=0, termination=MAX_ITERATIONS, q=0.0, residual_norm=np.sqrt(bb),
               rhs_norm=np.sqrt(bb), step_dot_residual=0.0, zetas=[], precond_fallbacks=fb + fbc)
    if bb == 0.0:
        out["termination"] = ZERO_RHS
        return _finish(out, ns)
    precond = lambda r: cat(np.einsum("iab,ib->ia", Minv, r[:6 * ns].reshape(ns, 6)),   # noqa: E731
                            np.einsum("rab,rb->ra", Mc, r[6 * ns:].reshape(ncs, S12)))
    x, r = np.zeros_like(b), b.copy()
    z = precond(r)
    rho = float(np.sum(r * z))
    if not (np.isfinite(bb) and rho > 0.0 and np.isfinite(rho)):
        out["termination"] = BREAKDOWN
        return _finish(out, ns)
    if max_iterations <= 0:
        return _finish(out, ns)
    p = np.zeros_like(b)
    beta, q_prev, k = 0.0, 0.0, 0
    while True:
        p = z + beta * p
        w = cat(*product_cam(S_diag, S_off, rl, B, S_cam, p[:6 * ns].reshape(ns, 6), p[6 * ns:].reshape(ncs, S12),
                             descending))
        pw = float(np.sum(p * w))
        with np.errstate(all="ignore"):
            alpha = rho / pw if pw != 0.0 else np.inf
        if not (pw > 0.0 and np.isfinite(alpha)):
            out["termination"] = BREAKDOWN
            return _finish(out, ns)
        x_new = x + alpha * p
        r = r - alpha * w
        z = precond(r)
        rz, rr = float(np.sum(r * z)), float(np.sum(r * r))
        q = -0.5 * float(np.sum(x_new * (b + r)))
        if not (rz >= 0.0 and np.isfinite(rz) and np.isfinite(rr) and np.isfinite(q)):
            out["termination"] = BREAKDOWN
            return _finish(out, ns)
        x = x_new
        k += 1
        zeta = k * (q - q_prev) / q
        out["zetas"].append(zeta)
        out.update(x=x, iterations=k, q=q, residual_norm=np.sqrt(rr), step_dot_residual=float(np.sum(x * r)))
        if k >= min_iterations and q_tolerance >= 0.0 and zeta < q_tolerance:
            out["termination"] = Q_TOLERANCE
            return _finish(out, ns)
        if k >= min_iterations and r_tolerance >= 0.0 and np.sqrt(rr) <= r_tolerance * out["rhs_norm"]:
            out["termination"] = R_TOLERANCE
            return _finish(out, ns)
        if k >= max_iterations:
            out["termination"] = MAX_ITERATIONS
            return _finish(out, ns)
        beta, rho, q_prev = rz / rho, rz, q


# ---- the device's own operation order -----------------------------------------------------------------------------
def _lanes(terms):
    """[m][...] terms dealt lane-strided (term t to lane t % 64, in turn) and combined by the xor butterfly"""
    terms = np.asarray(terms, np.float64)
    lanes = np.zeros(terms.shape[1:] + (64,))
    for t in range(terms.shape[0]):
        lanes[..., t % 64] = lanes[..., t % 64] + terms[t]
    return pr._wave_tree(lanes)


def _seq(terms):
    """[m][k] -> [m]: sequential sum over the last axis from 0.0"""
    s = np.zeros(terms.shape[0])
    for k in range(terms.shape[1]):
        s = s + terms[:, k]
    return s


def _matvec(M, v):
    """[m][k][k] x [m][k], every row a sequential sum over the columns from 0.0"""
    out = np.zeros_like(v)
    for c in range(v.shape[1]):
        out = out + M[:, :, c] * v[:, c][:, None]
    return out


def _sum_parts(per_slot, per_cam):
    """k_pcg_begin / k_pcg_step over the partial list [pose workgroups (256 slots each, at least one) | camera slots]"""
    per_slot = np.asarray(per_slot, np.float64)
    pose = [pr._block_sum256(per_slot[m:m + 256]) for m in range(0, len(per_slot), 256)] or [0.0]
    return pr._sum_strided(pose + [float(v) for v in per_cam])


def _product_cam_device_order(S_diag, S_off, row_lists, B, S_cam, p, pc):
    ns, ncs = p.shape[0], pc.shape[0]
    nc = S12 * ncs
    w = pr._product_device_order(S_diag, S_off, row_lists, p)
    pcv = pc.reshape(-1)
    camw = np.zeros((nc, ns))
    for i in range(ns):
        Bi = B[i].reshape(nc, 6)
        camw[:, i] = _seq(Bi * p[i][None, :])                       # B[i]_t . p_i, c ascending
        w[i] = w[i] + _lanes(Bi * pcv[:, None])                     # B[i]_t p_cam[t], lane-strided rows t
    Sc = S_cam.transpose(0, 2, 1, 3).reshape(nc, nc)
    wc = np.array([_lanes(camw[e]) + _lanes(Sc[e] * pcv) for e in range(nc)])
    return w, wc.reshape(ncs, S12)


def pcg_cam_device_order(S_diag, S_off, pairs, rhs, B, S_cam, rhs_cam, max_iterations=100, min_iterations=0,
                         preconditioner=SCHUR_JACOBI, q_tolerance=0.1, r_tolerance=-1.0):
    """pcg_cam() with every sum in the device's stated order; same return value"""
    S_diag, S_off, rhs, B, S_cam, rhs_cam, ns, ncs = _arrays(S_diag, S_off, rhs, B, S_cam, rhs_cam)
    if ncs == 0:
        out = pr.pcg_device_order(S_diag, S_off, pairs, rhs, max_iterations, min_iterations, preconditioner, q_tolerance,
                                  r_tolerance)
        out["x"] = out["x"].reshape(-1)
        return _finish(out, ns)
    rl = pr.rows(ns, pairs)
    Minv = np.tile(np.eye(6), (ns, 1, 1))
    fb = 0
    if preconditioner == SCHUR_JACOBI:
        for i in range(ns):
            inv = pr._block_inverse_device_order(S_diag[i])
            if inv is None:
                fb += 1
            else:
                Minv[i] = inv
    Mc, fbc = cam_preconditioner(S_cam, preconditioner, device_order=True)
    cat = lambda a, c: np.concatenate([a.reshape(-1), c.reshape(-1)])   # noqa: E731
    x, xc = np.zeros_like(rhs), np.zeros_like(rhs_cam)
    r, rc = rhs.copy(), rhs_cam.copy()
    z, zc = _matvec(Minv, r), _matvec(Mc, rc)
    # k_pcg_cam_init: a camera slot's partial is a sequential sum over its 12 coordinates
    rho, bb = _sum_parts(_seq(r * z), _seq(rc * zc)), _sum_parts(_seq(r * r), _seq(rc * rc))
    out = dict(x=cat(x, xc), iterations=0, termination=MAX_ITERATIONS, q=0.0, residual_norm=np.sqrt(bb),
               rhs_norm=np.sqrt(bb), step_dot_residual=0.0, zetas=[], precond_fallbacks=fb + fbc)
    if not bb > 0.0:
        out["termination"] = ZERO_RHS if bb == 0.0 else BREAKDOWN
        return _finish(out, ns)
    if not (rho > 0.0 and np.isfinite(rho)):
        out["termination"] = BREAKDOWN
        return _finish(out, ns)
    if max_iterations <= 0:
        return _finish(out, ns)
    p, pc = np.zeros_like(rhs), np.zeros_like(rhs_cam)
    beta, q_prev, k = 0.0, 0.0, 0
    # k_pcg_cam_update: a camera slot's partial is block_sum256 over its 12 threads
    cam256 = lambda t: [pr._block_sum256(v) for v in t]   # noqa: E731
    while True:
        p, pc = z + beta * p, zc + beta * pc
        w, wc = _product_cam_device_order(S_diag, S_off, rl, B, S_cam, p, pc)
        pw = pr._sum_strided(np.concatenate([_seq(p * w), (pc * wc).reshape(-1)]))
        with np.errstate(all="ignore"):
            alpha = np.float64(rho) / np.float64(pw)
        if not (pw > 0.0 and np.isfinite(alpha)):
            out["termination"] = BREAKDOWN
            return _finish(out, ns)
        x_new, xc_new = x + alpha * p, xc + alpha * pc
        r, rc = r - alpha * w, rc - alpha * wc
        z, zc = _matvec(Minv, r), _matvec(Mc, rc)
        rz, rr = _sum_parts(_seq(r * z), cam256(rc * zc)), _sum_parts(_seq(r * r), cam256(rc * rc))
        xbr = _sum_parts(_seq(x_new * (rhs + r)), cam256(xc_new * (rhs_cam + rc)))
        xr = _sum_parts(_seq(x_new * r), cam256(xc_new * rc))
        q = -0.5 * xbr
        if not (rz >= 0.0 and np.isfinite(rz) and np.isfinite(rr) and np.isfinite(q)):
            out["termination"] = BREAKDOWN
            return _finish(out, ns)
        x, xc = x_new, xc_new
        k += 1
        zeta = k * (q - q_prev) / q
        out["zetas"].append(zeta)
        out.update(x=cat(x, xc), iterations=k, q=q, residual_norm=np.sqrt(rr), step_dot_residual=xr)
        if k >= min_iterations and q_tolerance >= 0.0 and zeta < q_tolerance:
            out["termination"] = Q_TOLERANCE
            return _finish(out, ns)
        if k >= min_iterations and r_tolerance >= 0.0 and np.sqrt(rr) <= r_tolerance * out["rhs_norm"]:
            out["termination"] = R_TOLERANCE
            return _finish(out, ns)
        if k >= max_iterations:
            out["termination"] = MAX_ITERATIONS
            return _finish(out, ns)
        beta, rho, q_prev = rz / rho, rz, q


def dense_system(S_diag, S_off, pairs, rhs, B, S_cam, rhs_cam):
    """(S [n][n], b [n]) of the block lists"""
    S_diag, S_off, rhs, B, S_cam, rhs_cam, ns, ncs = _arrays(S_diag, S_off, rhs, B, S_cam, rhs_cam)
    n0, nc = 6 * ns, S12 * ncs
    S = np.zeros((n0 + nc, n0 + nc))
    for i in range(ns):
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = S_diag[i]
    for q, (i, j) in enumerate(pairs):
        S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = S_off[q]
        S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = S_off[q].T
    Bd = B.reshape(ns, nc, 6).transpose(1, 0, 2).reshape(nc, n0)
    S[n0:, :n0], S[:n0, n0:] = Bd, Bd.T
    S[n0:, n0:] = S_cam.transpose(0, 2, 1, 3).reshape(nc, nc)
    return S, np.concatenate([rhs.reshape(-1), rhs_cam.reshape(-1)])


def true_residual(blocks, x):
    """||b - S x|| / ||b|| of the block lists `blocks` (cam_block_lists order)"""
    S, b = dense_system(*blocks)
    return float(np.linalg.norm(b - S @ np.asarray(x).reshape(-1)) / np.linalg.norm(b))


def lm_cam_pcg(oracle, scene, refine, max_iterations, initial_radius=1e4, mode="marquardt", min_relative_decrease=1e-3,
               max_radius=1e16, linear=None):
    """ba_schur_cam_ref.lm_cam with pcg_cam as the linear solver (a BREAKDOWN is a rejected step); linear: dict of
    pcg_cam options, as ba_solve's.  Returns (history, final scene); every record also has linear_iterations,
    linear_termination and zetas."""
    scene = cref.without_refine(scene)
    radius, factor = float(initial_radius), 2.0
    hist = []
    for _ in range(max_iterations):
        ne = cref.CamNormalEquations(oracle, scene, refine, 1.0 / radius, mode)
        sol = pcg_cam(*cam_block_lists(ne.schur_cam_blocks()), **(linear or {}))
        rec = dict(cost=ne.cost, candidate_cost=np.nan, rho=np.nan, accepted=False,
                   linear_iterations=sol["iterations"], linear_termination=sol["termination"], zetas=sol["zetas"])
        cand = None
        if sol["termination"] != BREAKDOWN:
            dpose, dcam = sol["x_pose"], sol["x_cam"]
            dpoint = ne.back_substitute_cam(dpose, dcam)
            model = ne.model_decrease_cam(dpose, dcam, dpoint)
            poses, points, cams = cref.plus_cam(scene, refine, dpose, dcam, dpoint)
            cand = dict(scene, poses=poses, points=points, cam_params_list=cams)
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

// ba_pcg.hip -- preconditioned conjugate gradients on the reduced camera system of bundle adjustment, from
// the blocks the last Schur call left in the handle:
//   plain     S x = rhs, x = dpose (6 ns)                                    pcd_ba_schur_solve_pcg*, PCD_LINEAR_PCG
//   bordered  S = [[S_pose, B^T], [B, S_cam]], x = [dpose | dcam (12 ncs)],
//             b = [rhs | rhs_cam], with the camera rows of refined intrinsics  pcd_ba_schur_cam_solve_pcg*, PCD_LINEAR_PCG_CAM
// No atomics, fp64, every sum in an order fixed by the structure: bitwise repeatable.  The launchers are ba_pcg.h's; the
// solver state, the batches and the entry points live in ba_solve.hip.
//
// An iteration is three plain launches (product, vector update, scalars); scalars, the iteration count and the done
// flag live in PcgState on the device and every kernel of an iteration returns at once when done is set, so the host
// enqueues a batch of iterations between two looks at the flag.  p and x are double-buffered (iteration it reads buffer
// it & 1 and writes the other): the product forms the new direction of a partner slot on the fly from z and the old p
// instead of waiting for a fourth launch, and a breakdown leaves the last finite x untouched.
//
// The bordered solve shares the recurrence, the scalars and the done flag: k_pcg_init, k_pcg_begin, k_pcg_step and
// k_pcg_finish run unchanged on the pose part and on partial lists that carry one more entry per camera slot, and the
// pose sums of its product and update kernels are the plain kernels' own bodies (pcg_row_product, pcg_slot_update), so
// its pose part is the plain sums, exactly.  Its iteration is four launches: k_pcg_cam_spmv, k_pcg_cam_rows,
// k_pcg_cam_update, k_pcg_step.  The camera rows have a launch of their own because w_cam sums over every pose slot:
// folded into the prologue of k_pcg_cam_update, each of its workgroups would repeat that whole cross-slot reduction.
//
// The kernels take their arrays as loose __restrict__ parameters, not through PcgVec: the members of a struct carry no
// such promise, and the loads of the update kernels are scheduled across their stores on the strength of it.
#include "ba_pcg.h"

#include "ba_solve_cam.h"

namespace pcd {

// ---- what both solves sum -----------------------------------------------------------------------------------------
// lane's share of row i: the row list (ascending partner slot; block, transposed flag) of B p_j with
// p_j = z_j + beta p_old_j, lane-strided blocks, into six accumulators
__device__ __forceinline__ void pcg_row_product(int ns, int i, int lane, double beta, const uint32_t* row_start,
                                                const uint32_t* row_blk, const uint32_t* row_col, const double* Sdiag,
                                                const double* Soff, const double* z, const double* p_old,
                                                double (&acc)[6]) {
  for (uint32_t t = row_start[i] + lane; t < row_start[i + 1]; t += 64) {
    const uint32_t blk = row_blk[t], cj = row_col[t];
    const bool tr = cj & 1u;
    const size_t j = cj >> 1;
    const double* B = blk < (uint32_t)ns ? Sdiag + 36 * (size_t)blk : Soff + 36 * (size_t)(blk - (uint32_t)ns);
    double bv[36], pj[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) bv[k] = B[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) pj[k] = z[6 * j + k] + beta * p_old[6 * j + k];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += (tr ? bv[6 * c + a] : bv[6 * a + c]) * pj[c];
      acc[a] += s;
    }
  }
}

// pose slot i: x_new = x_old + alpha p, r -= alpha w, z = M^-1 r and the slot's terms of r.z, r.r, x.(rhs + r), x.r
__device__ __forceinline__ void pcg_slot_update(int i, double alpha, const double* Minv, const double* rhs,
                                                const double* p, const double* w, const double* x_old, double* x_new,
                                                double* r, double* z, double& rz, double& rr, double& xbr, double& xr) {
  double rv[6], xv[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const size_t o = 6 * (size_t)i + k;
    xv[k] = x_old[o] + alpha * p[o];
    rv[k] = r[o] - alpha * w[o];
    x_new[o] = xv[k]; r[o] = rv[k];
  }
  const double* mi = Minv + 36 * (size_t)i;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s += mi[6 * a + c] * rv[c];
    z[6 * (size_t)i + a] = s;
    rz += rv[a] * s; rr += rv[a] * rv[a];
    xbr += xv[a] * (rhs[6 * (size_t)i + a] + rv[a]); xr += xv[a] * rv[a];
  }
}

// ---- the plain system, and the pose part of the bordered one ------------------------------------------------------
// thread = slot: M_i^-1 (SCHUR_JACOBI: inverse of the 6x6 diagonal block through its Cholesky factor, identity when a
// pivot is not positive and finite -- counted; IDENTITY: I), x = 0, r = rhs, z = M^-1 r, both direction buffers 0;
// partials [nb][4] of r.z, rhs.rhs and the fallback count.  An identity row / column of the block (constant tvec
// coordinate) gives an identity row / column of the factor and of the inverse, exactly.
__global__ __launch_bounds__(256) void k_pcg_init(int ns, int precond, const double* __restrict__ Sdiag,
                                                  const double* __restrict__ rhs, double* __restrict__ Minv,
                                                  double* __restrict__ x0, double* __restrict__ r, double* __restrict__ z,
                                                  double* __restrict__ p0, double* __restrict__ p1,
                                                  double* __restrict__ partial) {
  __shared__ double s_l[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double rz = 0.0, bb = 0.0, fb = 0.0;
  if (i < ns) {
    double mi[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) mi[k] = (k % 7 == 0) ? 1.0 : 0.0;
    if (precond != 0) {
      const double* A = Sdiag + 36 * (size_t)i;
      double L[36];
#pragma unroll
      for (int k = 0; k < 36; ++k) L[k] = 0.0;
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double d = A[7 * j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
        ok = ok && d > 0.0 && d <= 1.7976931348623157e308;
        const double ljj = ok ? sqrt(d) : 1.0;
        L[7 * j] = ljj;
#pragma unroll
        for (int a = j + 1; a < 6; ++a) {
          double s = A[6 * a + j];
#pragma unroll
          for (int k = 0; k < j; ++k) s -= L[6 * a + k] * L[6 * j + k];
          L[6 * a + j] = s / ljj;
        }
      }
      if (ok) {
        double M[36];   // L^-1, lower
#pragma unroll
        for (int k = 0; k < 36; ++k) M[k] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          M[7 * j] = 1.0 / L[7 * j];
#pragma unroll
          for (int a = j + 1; a < 6; ++a) {
            double s = 0.0;
#pragma unroll
            for (int k = j; k < a; ++k) s += L[6 * a + k] * M[6 * k + j];
            M[6 * a + j] = -s / L[7 * a];
          }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int c = 0; c <= a; ++c) {
            double s = 0.0;   // (M^T M)_ac, k from a (>= c) upwards
#pragma unroll
            for (int k = a; k < 6; ++k) s += M[6 * k + a] * M[6 * k + c];
            mi[6 * a + c] = s; mi[6 * c + a] = s;
          }
      } else {
        fb = 1.0;
      }
    }
    double* mo = Minv + 36 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 36; ++k) mo[k] = mi[k];
    double b[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = rhs[6 * (size_t)i + k];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += mi[6 * a + c] * b[c];
      const size_t o = 6 * (size_t)i + a;
      z[o] = s; r[o] = b[a]; x0[o] = 0.0; p0[o] = 0.0; p1[o] = 0.0;
      rz += b[a] * s; bb += b[a] * b[a];
    }
  }
  rz = block_sum256(rz, s_l); bb = block_sum256(bb, s_l); fb = block_sum256(fb, s_l);
  if (threadIdx.x == 0) {
    double* o = partial + 4 * (size_t)blockIdx.x;
    o[0] = rz; o[1] = bb; o[2] = fb; o[3] = 0.0;
  }
}

// one workgroup: the scalars of iteration 0.  ||rhs|| = 0 -> ZERO_RHS, max_iterations <= 0 -> MAX_ITERATIONS, x = 0
__global__ __launch_bounds__(256) void k_pcg_begin(int nb, const double* __restrict__ partial, PcgRule rule,
                                                   PcgState* __restrict__ st) {
  __shared__ double s_l[4];
  const double rz = block_sum_strided(partial, nb, 4, s_l);
  const double bb = block_sum_strided(partial + 1, nb, 4, s_l);
  const double fb = block_sum_strided(partial + 2, nb, 4, s_l);
  if (threadIdx.x != 0) return;
  PcgState s;
  s.rho = rz; s.alpha = 0.0; s.beta = 0.0; s.pw = 0.0; s.q = 0.0; s.rn2 = bb; s.bnorm = sqrt(bb); s.xr = 0.0;
  s.k = 0; s.done = 0; s.term = PCD_PCG_MAX_ITERATIONS; s.xsel = 0; s.fallbacks = (unsigned)fb; s.pad = 0;
  if (!(bb > 0.0)) {   // zero (or not a number: nothing to iterate on)
    s.done = 1; s.term = bb == 0.0 ? PCD_PCG_ZERO_RHS : PCD_PCG_BREAKDOWN;
  } else if (!(rz > 0.0) || !(rz <= 1.7976931348623157e308)) {
    s.done = 1; s.term = PCD_PCG_BREAKDOWN;
  } else if (rule.max_iterations <= 0) {
    s.done = 1;
  }
  *st = s;
}

// one wavefront per slot row: w_i = the row list's sum (pcg_row_product), xor butterfly.  Lane 0 stores the row's new
// direction, w_i and p_i . w_i.
__global__ __launch_bounds__(256) void k_pcg_spmv(int ns, const PcgState* __restrict__ st,
                                                  const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ row_blk,
                                                  const uint32_t* __restrict__ row_col, const double* __restrict__ Sdiag,
                                                  const double* __restrict__ Soff, const double* __restrict__ z,
                                                  const double* __restrict__ p_old, double* __restrict__ p_new,
                                                  double* __restrict__ w, double* __restrict__ pw_partial) {
  if (st->done) return;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= ns) return;
  const double beta = st->beta;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  pcg_row_product(ns, i, lane, beta, row_start, row_blk, row_col, Sdiag, Soff, z, p_old, acc);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[a] += __shfl_xor(acc[a], off);
  if (lane == 0) {
    double pw = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const size_t o = 6 * (size_t)i + k;
      const double pk = z[o] + beta * p_old[o];
      p_new[o] = pk; w[o] = acc[k];
      pw += pk * acc[k];
    }
    pw_partial[i] = pw;
  }
}

// thread = slot: alpha = rho / p.w (every workgroup sums the ns row partials in the same order), then the slot's update
// (pcg_slot_update) and the partials [nb][4] of r.z, r.r, x.(rhs + r), x.r.
// p.w <= 0 or a non-finite alpha: nothing is updated (k_pcg_step ends the solve with BREAKDOWN).
__global__ __launch_bounds__(256) void k_pcg_update(int ns, PcgState* __restrict__ st, const double* __restrict__ pw_partial,
                                                    const double* __restrict__ Minv, const double* __restrict__ rhs,
                                                    const double* __restrict__ p, const double* __restrict__ w,
                                                    const double* __restrict__ x_old, double* __restrict__ x_new,
                                                    double* __restrict__ r, double* __restrict__ z,
                                                    double* __restrict__ partial) {
  __shared__ double s_l[4];
  if (st->done) return;
  const double pw = block_sum_strided(pw_partial, ns, 1, s_l);
  const double alpha = st->rho / pw;
  const bool good = pw > 0.0 && alpha <= 1.7976931348623157e308 && alpha >= -1.7976931348623157e308;
  if (blockIdx.x == 0 && threadIdx.x == 0) { st->pw = pw; st->alpha = alpha; }
  if (!good) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  double rz = 0.0, rr = 0.0, xbr = 0.0, xr = 0.0;
  if (i < ns) pcg_slot_update(i, alpha, Minv, rhs, p, w, x_old, x_new, r, z, rz, rr, xbr, xr);
  rz = block_sum256(rz, s_l); rr = block_sum256(rr, s_l); xbr = block_sum256(xbr, s_l); xr = block_sum256(xr, s_l);
  if (threadIdx.x == 0) {
    double* o = partial + 4 * (size_t)blockIdx.x;
    o[0] = rz; o[1] = rr; o[2] = xbr; o[3] = xr;
  }
}

// one workgroup: sums of the partials, Q_k = -1/2 x.(rhs + r), the stopping rule (Q, then r, then the iteration
// limit), beta and the counter.  `it` is the iteration's index (the buffer that holds its x is (it + 1) & 1).
__global__ __launch_bounds__(256) void k_pcg_step(int nb, int it, const double* __restrict__ partial, PcgRule rule,
                                                  PcgState* __restrict__ st) {
  __shared__ double s_l[4];
  if (st->done) return;
  const double pw = st->pw, alpha = st->alpha;
  if (!(pw > 0.0 && alpha <= 1.7976931348623157e308 && alpha >= -1.7976931348623157e308)) {
    if (threadIdx.x == 0) { st->done = 1; st->term = PCD_PCG_BREAKDOWN; }
    return;
  }
  const double rz = block_sum_strided(partial, nb, 4, s_l);
  const double rr = block_sum_strided(partial + 1, nb, 4, s_l);
  const double xbr = block_sum_strided(partial + 2, nb, 4, s_l);
  const double xr = block_sum_strided(partial + 3, nb, 4, s_l);
  if (threadIdx.x != 0) return;
  const double q = -0.5 * xbr;
  const double lim = 1.7976931348623157e308;
  if (!(rz >= 0.0 && rz <= lim && rr <= lim && q >= -lim && q <= lim)) {   // the x of this iteration is not used
    st->done = 1; st->term = PCD_PCG_BREAKDOWN;
    return;
  }
  const int k = st->k + 1;
  const double zeta = (double)k * (q - st->q) / q;
  int done = 0, term = PCD_PCG_MAX_ITERATIONS;
  if (k >= rule.min_iterations && rule.q_tolerance >= 0.0 && zeta < rule.q_tolerance) { done = 1; term = PCD_PCG_Q_TOLERANCE; }
  else if (k >= rule.min_iterations && rule.r_tolerance >= 0.0 && sqrt(rr) <= rule.r_tolerance * st->bnorm) { done = 1; term = PCD_PCG_R_TOLERANCE; }
  else if (k >= rule.max_iterations) { done = 1; }
  st->beta = rz / st->rho; st->rho = rz; st->q = q; st->rn2 = rr; st->xr = xr;
  st->k = k; st->xsel = (it + 1) & 1; st->term = term; st->done = done;
}

// the selected x into the caller's dpose, the record into info (termination -1: still running)
__global__ __launch_bounds__(256) void k_pcg_finish(int ns, const PcgState* __restrict__ st, const double* __restrict__ x0,
                                                    const double* __restrict__ x1, double* __restrict__ dpose,
                                                    pcd_ba_pcg_info* __restrict__ info) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (dpose && t < 6 * ns) dpose[t] = (st->xsel ? x1 : x0)[t];
  if (t == 0 && info) {
    pcd_ba_pcg_info o;
    o.iterations = st->k; o.termination = st->done ? st->term : -1; o.precond_fallbacks = st->fallbacks;
    o.rhs_norm = st->bnorm; o.residual_norm = sqrt(st->rn2); o.q = st->q; o.step_dot_residual = st->xr;
    *info = o;
  }
}

// ---- the camera part of the bordered system -----------------------------------------------------------------------
// one wavefront per camera slot, the 12 x 12 diagonal block S_cam[r][r] in LDS.  SCHUR_JACOBI: its inverse through the
// Cholesky factor in the operation order of k_pcg_init's 6 x 6, with 12 for 6:
//   column j = 0..11:  d = A_jj - L_j0^2 - ... - L_j,j-1^2 (k ascending), L_jj = sqrt(d);
//                      L_aj = (A_aj - L_a0 L_j0 - ... - L_a,j-1 L_j,j-1) / L_jj for a > j (lane a);
//   M = L^-1, column j (lane j): M_jj = 1 / L_jj, M_aj = -(L_aj M_jj + ... + L_a,a-1 M_a-1,j) / L_aa (k ascending from j);
//   (M^T M)_ac = M_ka M_kc summed over k = max(a, c) .. 11 ascending from 0.0, every entry on its own (symmetric exactly).
// A pivot d that is not positive and finite: identity, counted.  An identity row / column of the block (inactive
// coordinate) gives an identity row / column of L, M and the inverse, exactly.  IDENTITY: I.
// Then x = 0, r = rhs_cam, z = M^-1 r (c ascending from 0.0), both directions 0 and the slot's partial
// [r.z, rhs.rhs, fallback, 0], each a sequential sum over the 12 coordinates from 0.0.
__global__ __launch_bounds__(64) void k_pcg_cam_init(PcgVec v, int precond, int nb, double* __restrict__ x0,
                                                     double* __restrict__ p0, double* __restrict__ p1) {
  __shared__ double s_a[kCamS * kCamS], s_l[kCamS * kCamS], s_m[kCamS * kCamS], s_r[kCamS], s_z[kCamS];
  const int r = blockIdx.x, lane = threadIdx.x, ncs = v.ncs;
  const double* A = v.Scam + ((size_t)r * ncs + r) * (kCamS * kCamS);
  for (int t = lane; t < kCamS * kCamS; t += 64) { s_a[t] = A[t]; s_l[t] = 0.0; s_m[t] = 0.0; }
  if (lane < kCamS) s_r[lane] = v.rhs_cam[kCamS * r + lane];
  __syncthreads();
  bool ok = true;
  if (precond != 0) {
    for (int j = 0; j < kCamS; ++j) {
      double d = s_a[(kCamS + 1) * j];
      for (int k = 0; k < j; ++k) d -= s_l[kCamS * j + k] * s_l[kCamS * j + k];
      ok = ok && d > 0.0 && d <= 1.7976931348623157e308;
      const double ljj = ok ? sqrt(d) : 1.0;
      if (lane == j) s_l[(kCamS + 1) * j] = ljj;
      if (lane > j && lane < kCamS) {
        double t = s_a[kCamS * lane + j];
        for (int k = 0; k < j; ++k) t -= s_l[kCamS * lane + k] * s_l[kCamS * j + k];
        s_l[kCamS * lane + j] = t / ljj;
      }
      __syncthreads();
    }
    if (ok && lane < kCamS) {
      const int j = lane;
      s_m[(kCamS + 1) * j] = 1.0 / s_l[(kCamS + 1) * j];
      for (int a = j + 1; a < kCamS; ++a) {
        double t = 0.0;
        for (int k = j; k < a; ++k) t += s_l[kCamS * a + k] * s_m[kCamS * k + j];
        s_m[kCamS * a + j] = -t / s_l[(kCamS + 1) * a];
      }
    }
    __syncthreads();
  }
  const bool inv = precond != 0 && ok;
  double* mo = v.Minv_cam + (size_t)r * (kCamS * kCamS);
  for (int t = lane; t < kCamS * kCamS; t += 64) {
    const int a = t / kCamS, c = t - kCamS * (t / kCamS);
    double e = a == c ? 1.0 : 0.0;
    if (inv) {
      e = 0.0;
      for (int k = a > c ? a : c; k < kCamS; ++k) e += s_m[kCamS * k + a] * s_m[kCamS * k + c];
    }
    s_a[t] = e; mo[t] = e;
  }
  __syncthreads();
  const size_t o = 6 * (size_t)v.ns + (size_t)kCamS * r + lane;
  if (lane < kCamS) {
    double z = 0.0;
    for (int c = 0; c < kCamS; ++c) z += s_a[kCamS * lane + c] * s_r[c];
    s_z[lane] = z;
    v.z[o] = z; v.r[o] = s_r[lane]; x0[o] = 0.0; p0[o] = 0.0; p1[o] = 0.0;
  }
  __syncthreads();
  if (lane == 0) {
    double rz = 0.0, bb = 0.0;
    for (int a = 0; a < kCamS; ++a) { rz += s_r[a] * s_z[a]; bb += s_r[a] * s_r[a]; }
    double* po = v.partial + 4 * ((size_t)nb + r);
    po[0] = rz; po[1] = bb; po[2] = (precond != 0 && !ok) ? 1.0 : 0.0; po[3] = 0.0;
  }
}

// k_pcg_spmv with the border.  One wavefront per pose slot i: the slot's row list as k_pcg_spmv sums it
// (pcg_row_product), then one read of B[i] ([12 ncs] rows of 6) serves both directions: lane t, t + 64 owns row t of
// B[i], stores camw[t][i] = B[i]_t . p_i (c ascending from 0.0; the slot's partial of w_cam) and adds B[i]_t p_cam[t] to
// six accumulators (t ascending), which the xor butterfly combines.  w_i = (row list sum) + (border sum): an add the
// plain kernel must not have, -0.0 + 0.0 flips a sign bit.
// p_cam = z_cam + beta p_cam_old is formed on the fly, as the partner directions are.
__global__ __launch_bounds__(256) void k_pcg_cam_spmv(PcgVec v, const uint32_t* __restrict__ row_start,
                                                      const uint32_t* __restrict__ row_blk,
                                                      const uint32_t* __restrict__ row_col, const double* __restrict__ Sdiag,
                                                      const double* __restrict__ Soff, const double* __restrict__ p_old,
                                                      double* __restrict__ p_new) {
  if (v.st->done) return;
  const int lane = threadIdx.x & 63, ns = v.ns;
  const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= ns) return;
  const double beta = v.st->beta;
  const double* z = v.z;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  pcg_row_product(ns, i, lane, beta, row_start, row_blk, row_col, Sdiag, Soff, z, p_old, acc);
  double pi[6], accb[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 6; ++k) pi[k] = z[6 * (size_t)i + k] + beta * p_old[6 * (size_t)i + k];
  const int nrow = kCamS * v.ncs;
  const size_t n0 = 6 * (size_t)ns;
  for (int t = lane; t < nrow; t += 64) {
    const double* brow = v.B + ((size_t)i * nrow + t) * 6;
    const double pc = z[n0 + t] + beta * p_old[n0 + t];
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double bc = brow[c];
      s += bc * pi[c];
      accb[c] += bc * pc;
    }
    v.camw[(size_t)t * ns + i] = s;
  }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      acc[a] += __shfl_xor(acc[a], off);
      accb[a] += __shfl_xor(accb[a], off);
    }
  if (lane == 0) {
    double pw = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const size_t o = 6 * (size_t)i + k;
      const double wk = acc[k] + accb[k];
      p_new[o] = pi[k]; v.w[o] = wk;
      pw += pi[k] * wk;
    }
    v.pw[i] = pw;
  }
}

// one wavefront per camera coordinate e = 12 r + a: w_e = (sum over the pose slots of camw[e][i], lane-strided, xor
// butterfly) + (S_cam row e . p_cam, lane-strided over the 12 ncs columns, xor butterfly).  Lane 0 stores the new
// direction p_e, w_e and p_e w_e behind the pose slots' partials of p.w.
__global__ __launch_bounds__(256) void k_pcg_cam_rows(PcgVec v, const double* __restrict__ p_old,
                                                      double* __restrict__ p_new) {
  if (v.st->done) return;
  const int lane = threadIdx.x & 63, ns = v.ns, nc = kCamS * v.ncs;
  const int e = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (e >= nc) return;
  const double beta = v.st->beta;
  const size_t n0 = 6 * (size_t)ns;
  const double* src = v.camw + (size_t)e * ns;
  double a = 0.0, c = 0.0;
  for (int i = lane; i < ns; i += 64) a += src[i];
  const int r = e / kCamS, ar = e - kCamS * (e / kCamS);
  for (int t = lane; t < nc; t += 64) {   // column t = 12 r' + b of S_cam [r][r'][a][b]
    const int rp = t / kCamS, b = t - kCamS * (t / kCamS);
    c += v.Scam[(((size_t)r * v.ncs + rp) * kCamS + ar) * kCamS + b] * (v.z[n0 + t] + beta * p_old[n0 + t]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); c += __shfl_xor(c, off); }
  if (lane == 0) {
    const double pe = v.z[n0 + e] + beta * p_old[n0 + e], we = a + c;
    p_new[n0 + e] = pe; v.w[n0 + e] = we;
    v.pw[ns + e] = pe * we;
  }
}

// k_pcg_update on the bordered vector.  Workgroups 0 .. nb - 1 are k_pcg_update's, thread = pose slot
// (pcg_slot_update); workgroup nb + r is camera slot r, thread a < 12 = its coordinate (z = M^-1 r through LDS, c
// ascending from 0.0).  p.w = the strided sum of k_pcg_update over [ns pose slot partials | 12 ncs camera coordinate
// products]; the camera slots' partials of r.z, r.r, x.(rhs + r), x.r follow the pose workgroups' in partial[][4].
__global__ __launch_bounds__(256) void k_pcg_cam_update(PcgVec v, int nb, PcgState* __restrict__ st,
                                                        const double* __restrict__ Minv, const double* __restrict__ rhs,
                                                        const double* __restrict__ p, const double* __restrict__ x_old,
                                                        double* __restrict__ x_new) {
  __shared__ double s_l[4], s_r[kCamS];
  if (st->done) return;
  const int ns = v.ns;
  const double pw = block_sum_strided(v.pw, ns + kCamS * v.ncs, 1, s_l);
  const double alpha = st->rho / pw;
  const bool good = pw > 0.0 && alpha <= 1.7976931348623157e308 && alpha >= -1.7976931348623157e308;
  if (blockIdx.x == 0 && threadIdx.x == 0) { st->pw = pw; st->alpha = alpha; }
  if (!good) return;
  double* r = v.r; double* z = v.z; const double* w = v.w;
  double rz = 0.0, rr = 0.0, xbr = 0.0, xr = 0.0;
  if ((int)blockIdx.x < nb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < ns) pcg_slot_update(i, alpha, Minv, rhs, p, w, x_old, x_new, r, z, rz, rr, xbr, xr);
  } else {
    const int cr = (int)blockIdx.x - nb, a = threadIdx.x;
    const size_t o = 6 * (size_t)ns + (size_t)kCamS * cr + a;
    double xa = 0.0, ra = 0.0;
    if (a < kCamS) {
      xa = x_old[o] + alpha * p[o];
      ra = r[o] - alpha * w[o];
      x_new[o] = xa; r[o] = ra; s_r[a] = ra;
    }
    __syncthreads();
    if (a < kCamS) {
      const double* mi = v.Minv_cam + (size_t)cr * (kCamS * kCamS) + kCamS * a;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < kCamS; ++c) s += mi[c] * s_r[c];
      z[o] = s;
      rz = ra * s; rr = ra * ra; xbr = xa * (v.rhs_cam[kCamS * cr + a] + ra); xr = xa * ra;
    }
  }
  rz = block_sum256(rz, s_l); rr = block_sum256(rr, s_l); xbr = block_sum256(xbr, s_l); xr = block_sum256(xr, s_l);
  if (threadIdx.x == 0) {
    double* o = v.partial + 4 * (size_t)blockIdx.x;
    o[0] = rz; o[1] = rr; o[2] = xbr; o[3] = xr;
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------
static unsigned pcg_pose_groups(int ns) { return std::max(1u, div_up((uint64_t)ns, 256)); }

void pcg_init(const PcgVec& v, int precond, const PcgRule& rule, hipStream_t s) {
  const unsigned nb = pcg_pose_groups(v.ns);
  hipLaunchKernelGGL(k_pcg_init, dim3(nb), dim3(256), 0, s, v.ns, precond, v.Sdiag, v.rhs, v.Minv, v.x0, v.r, v.z, v.p0,
                     v.p1, v.partial);
  if (v.ncs) hipLaunchKernelGGL(k_pcg_cam_init, dim3(v.ncs), dim3(64), 0, s, v, precond, (int)nb, v.x0, v.p0, v.p1);
  hipLaunchKernelGGL(k_pcg_begin, dim3(1), dim3(256), 0, s, (int)nb + v.ncs, v.partial, rule, v.st);
}

void pcg_iterate(const PcgVec& v, int it, const PcgRule& rule, hipStream_t s) {
  const int ns = v.ns;
  if (!ns && !v.ncs) return;
  const unsigned nb = pcg_pose_groups(ns);
  double* p_old = (it & 1) ? v.p1 : v.p0; double* p_new = (it & 1) ? v.p0 : v.p1;
  double* x_old = (it & 1) ? v.x1 : v.x0; double* x_new = (it & 1) ? v.x0 : v.x1;
  if (v.ncs) {
    if (ns)
      hipLaunchKernelGGL(k_pcg_cam_spmv, dim3(div_up((uint64_t)ns, 4)), dim3(256), 0, s, v, v.row_start, v.row_blk,
                         v.row_col, v.Sdiag, v.Soff, p_old, p_new);
    hipLaunchKernelGGL(k_pcg_cam_rows, dim3(div_up((uint64_t)kCamS * v.ncs, 4)), dim3(256), 0, s, v, p_old, p_new);
    hipLaunchKernelGGL(k_pcg_cam_update, dim3(nb + (unsigned)v.ncs), dim3(256), 0, s, v, (int)nb, v.st, v.Minv, v.rhs,
                       p_new, x_old, x_new);
  } else {
    hipLaunchKernelGGL(k_pcg_spmv, dim3(div_up((uint64_t)ns, 4)), dim3(256), 0, s, ns, v.st, v.row_start, v.row_blk,
                       v.row_col, v.Sdiag, v.Soff, v.z, p_old, p_new, v.w, v.pw);
    hipLaunchKernelGGL(k_pcg_update, dim3(nb), dim3(256), 0, s, ns, v.st, v.pw, v.Minv, v.rhs, p_new, v.w, x_old, x_new,
                       v.r, v.z, v.partial);
  }
  hipLaunchKernelGGL(k_pcg_step, dim3(1), dim3(256), 0, s, (int)nb + v.ncs, it, v.partial, rule, v.st);
}

// k_pcg_finish copies 6 slots' worth per slot, and the bordered vector is 6 (ns + 2 ncs) long
void pcg_finish(const PcgVec& v, double* d_delta, pcd_ba_pcg_info* d_info, hipStream_t s) {
  const int ns = v.ns + 2 * v.ncs;
  hipLaunchKernelGGL(k_pcg_finish, dim3(std::max(1u, div_up(6 * (uint64_t)ns, 256))), dim3(256), 0, s, ns, v.st, v.x0,
                     v.x1, d_delta, d_info);
}

}  // namespace pcd

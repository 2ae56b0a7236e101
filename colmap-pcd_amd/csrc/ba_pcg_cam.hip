// ba_pcg_cam.hip -- the bordered PCG of bundle adjustment with refined intrinsics (pcd_ba_schur_cam_solve_pcg*,
// DESIGN 4.3a): preconditioned conjugate gradients on the reduced system with camera rows,
//   S = [[S_pose, B^T], [B, S_cam]],  x = [dpose (6 ns) | dcam (12 ncs)],  b = [rhs | rhs_cam],
// from the blocks pcd_ba_schur_cam_device leaves in the handle (ba_solve_cam.hip).  No atomics, fp64, every sum in an
// order fixed by the structure: bitwise repeatable.  The launchers are ba_solve_cam.h's; the solver state, the batches
// and the entry points live in ba_solve.hip, as do the plain PCG's kernels that this solve shares.
#include "ba_solve_cam.h"

namespace pcd {

// The recurrence, the scalars and the done flag are the plain PCG's (ba_solve.hip); k_pcg_init, k_pcg_begin, k_pcg_step
// and k_pcg_finish run unchanged on the pose part and on partial lists that carry one more entry per camera slot.  An
// iteration is four launches: k_pcg_cam_spmv, k_pcg_cam_rows, k_pcg_cam_update, k_pcg_step.  The camera rows have a
// launch of their own because w_cam sums over every pose slot: folded into the prologue of k_pcg_cam_update, each of its
// workgroups would repeat that whole cross-slot reduction.

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
__global__ __launch_bounds__(64) void k_pcg_cam_init(PcgCamVec v, int precond, int nb, double* __restrict__ x0,
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

// k_pcg_spmv with the border.  One wavefront per pose slot i: the slot's row list exactly as k_pcg_spmv sums it, then
// one read of B[i] ([12 ncs] rows of 6) serves both directions: lane t, t + 64 owns row t of B[i], stores
// camw[t][i] = B[i]_t . p_i (c ascending from 0.0; the slot's partial of w_cam) and adds B[i]_t p_cam[t] to six
// accumulators (t ascending), which the xor butterfly combines.  w_i = (row list sum) + (border sum).
// p_cam = z_cam + beta p_cam_old is formed on the fly, as the partner directions are.
__global__ __launch_bounds__(256) void k_pcg_cam_spmv(PcgCamVec v, const uint32_t* __restrict__ row_start,
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
  for (uint32_t t = row_start[i] + lane; t < row_start[i + 1]; t += 64) {
    const uint32_t blk = row_blk[t], cj = row_col[t];
    const bool tr = cj & 1u;
    const size_t j = cj >> 1;
    const double* Bk = blk < (uint32_t)ns ? Sdiag + 36 * (size_t)blk : Soff + 36 * (size_t)(blk - (uint32_t)ns);
    double bv[36], pj[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) bv[k] = Bk[k];
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
__global__ __launch_bounds__(256) void k_pcg_cam_rows(PcgCamVec v, const double* __restrict__ p_old,
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

// k_pcg_update on the bordered vector.  Workgroups 0 .. nb - 1 are k_pcg_update's, thread = pose slot; workgroup
// nb + r is camera slot r, thread a < 12 = its coordinate (z = M^-1 r through LDS, c ascending from 0.0).
// p.w = the strided sum of k_pcg_update over [ns pose slot partials | 12 ncs camera coordinate products]; the camera
// slots' partials of r.z, r.r, x.(rhs + r), x.r follow the pose workgroups' in partial[][4].
__global__ __launch_bounds__(256) void k_pcg_cam_update(PcgCamVec v, int nb, PcgState* __restrict__ st,
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
    if (i < ns) {
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

void pcg_cam_init(const PcgCamVec& v, int precond, double* x0, double* p0, double* p1, hipStream_t s) {
  hipLaunchKernelGGL(k_pcg_cam_init, dim3(v.ncs), dim3(64), 0, s, v, precond, (int)pcg_pose_groups(v.ns), x0, p0, p1);
}

void pcg_cam_product(const PcgCamVec& v, const uint32_t* row_start, const uint32_t* row_blk, const uint32_t* row_col,
                     const double* Sdiag, const double* Soff, const double* p_old, double* p_new, hipStream_t s) {
  if (v.ns)
    hipLaunchKernelGGL(k_pcg_cam_spmv, dim3(div_up((uint64_t)v.ns, 4)), dim3(256), 0, s, v, row_start, row_blk, row_col,
                       Sdiag, Soff, p_old, p_new);
  hipLaunchKernelGGL(k_pcg_cam_rows, dim3(div_up((uint64_t)kCamS * v.ncs, 4)), dim3(256), 0, s, v, p_old, p_new);
}

void pcg_cam_update(const PcgCamVec& v, PcgState* st, const double* Minv, const double* rhs, const double* p,
                    const double* x_old, double* x_new, hipStream_t s) {
  const unsigned nb = pcg_pose_groups(v.ns);
  hipLaunchKernelGGL(k_pcg_cam_update, dim3(nb + (unsigned)v.ncs), dim3(256), 0, s, v, (int)nb, st, Minv, rhs, p, x_old,
                     x_new);
}

}  // namespace pcd

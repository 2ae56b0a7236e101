// ba_solve.hip -- the device solver of bundle adjustment: point elimination of the damped normal
// equations into the reduced camera system (k_schur_*), the manifold update (k_ba_plus), the batches of the
// block-sparse preconditioned CG on that system (kernels: ba_pcg.hip), the direct solve of it (the handle's blocks or
// the caller's dense S into the scratch of ba_chol.hip, which factors and solves) and the Levenberg-Marquardt loop
// around them (pcd_ba_solve).
//
// The blocks it eliminates come from ba.hip, which this unit reaches through two calls only: ba_normal_equations
// (ba_handle.h) for H, g, W and the cost, and pcd_ba_evaluate_device for the cost of a trial step.  No evaluation
// kernel is compiled here.
//
// Refined intrinsics ride beside all this, opt-in (pcd_ba_schur_cam*, pcd_ba_solve with refine_intrinsics): the camera rows
// of the reduced system are a dense border whose kernels live in ba_solve_cam.hip; the state and the entry points are
// here.  Every host path takes the number of camera slots, ncs: 0 is the plain system, and a _cam entry point on a handle
// without camera slots is its plain counterpart.
//
// Host side, behind the kernels: BaSchur, the solver state grouped by owner; schur_build, which has the co-visibility
// structure built on the device (ba_schur_structure.hip) on the stream of the call that needs it; the PCG batches;
// one internal function per operation, which the plain and the _cam entry point both call; pcd_ba_solve over
// lm_check_opts, lm_reserve, lm_enqueue_linear, lm_try_step, lm_decide.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>

#include "ba_chol.h"
#include "ba_handle.h"
#include "ba_pcg.h"
#include "ba_schur_structure.h"
#include "ba_solve_cam.h"
#include "common.h"

namespace pcd {

// ------------------------------------------------------------- Schur -------
// Point elimination of the damped normal equations (H + D) delta = -g, unknowns = pose tangents of the variable-pose
// images ("slots", ascending image index), then the points.  DESIGN 4.3a.  Observation data live in image-major
// positions e (the layout k_ba_images walks): W and Y = W V^-1 of the observations of an image are contiguous, so the
// entries of a pair block (a in image i, b in image j) gather from two short ranges.  No atomics anywhere: every sum
// runs in an order fixed by the structure, so results are bitwise reproducible run to run.
// kDiagMin / kDiagMax / damp_of: ba_solve_cam.h, shared with the camera rows.

// thread = point: V = H_pt + D through a 3x3 Cholesky -> V^-1, V^-1 g, D.  Constant points are not eliminated, points
// whose damped V is not numerically positive definite are skipped (V^-1 = 0: delta 0, no contribution) and counted.
// The pivot rule is scale-invariant: pivot k must exceed kPivotTol * V_kk, which is the k-th pivot of the Jacobi-scaled
// V (unit diagonal) exceeding kPivotTol.  A sign test would decide rank-deficient V (a point with one observation and
// no LiDAR term, or only LiDAR terms, at mu = 0) by the rounding error of the accumulation of H_pt; that error is a
// few ulp of V_kk, far below the threshold, while a 1e-4 Marquardt damping puts the scaled pivots of such points near
// 1e-4, far above it.
// tests/ba_schur_ref.point_inverse applies the same rule in the same operation order.
constexpr double kPivotTol = 1e-10;
__global__ __launch_bounds__(256) void k_schur_points(int P, const double* __restrict__ Hpt, const double* __restrict__ gpt,
                                                      const uint8_t* __restrict__ point_const, double mu, int mode,
                                                      double* __restrict__ Vinv, double* __restrict__ Vg,
                                                      double* __restrict__ Dpt, uint32_t* __restrict__ skip_partial) {
  __shared__ uint32_t s_n[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  uint32_t skipped = 0;
  if (p < P) {
    double vi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, d[3];
    double* dp = Dpt + 3 * (size_t)p;
    if (!(point_const && point_const[p])) {
      const double* h = Hpt + 9 * (size_t)p;
      d[0] = damp_of(mode, mu, h[0]); d[1] = damp_of(mode, mu, h[4]); d[2] = damp_of(mode, mu, h[8]);
      dp[0] = d[0]; dp[1] = d[1]; dp[2] = d[2];   // stored now: d is not live across the factorisation
      const double a00 = h[0] + d[0], a01 = h[1], a02 = h[2], a11 = h[4] + d[1], a12 = h[5], a22 = h[8] + d[2];
      bool ok = a00 > 0.0;   // false for NaN too; t <= V_kk, so a negative V_kk fails t > kPivotTol * V_kk as well
      double l00 = 0, l10 = 0, l20 = 0, l11 = 0, l21 = 0, l22 = 0;
      if (ok) { l00 = sqrt(a00); l10 = a01 / l00; l20 = a02 / l00; const double t = a11 - l10 * l10; ok = t > kPivotTol * a11; l11 = ok ? sqrt(t) : 0.0; }
      if (ok) { l21 = (a12 - l20 * l10) / l11; const double t = a22 - l20 * l20 - l21 * l21; ok = t > kPivotTol * a22; l22 = ok ? sqrt(t) : 0.0; }
      if (ok) {
        // M = L^-1 (lower), V^-1 = M^T M
        const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
        const double m10 = -(l10 * m00) * m11, m21 = -(l21 * m11) * m22, m20 = -(l20 * m00 + l21 * m10) * m22;
        vi[0] = m00 * m00 + m10 * m10 + m20 * m20; vi[1] = m10 * m11 + m20 * m21; vi[2] = m20 * m22;
        vi[4] = m11 * m11 + m21 * m21; vi[5] = m21 * m22; vi[8] = m22 * m22;
        vi[3] = vi[1]; vi[6] = vi[2]; vi[7] = vi[5];
      } else {
        skipped = 1;
      }
    } else {
      dp[0] = 0.0; dp[1] = 0.0; dp[2] = 0.0;
    }
    const double* g = gpt + 3 * (size_t)p;
    double* o = Vinv + 9 * (size_t)p;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = vi[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) Vg[3 * (size_t)p + r] = vi[3 * r] * g[0] + vi[3 * r + 1] * g[1] + vi[3 * r + 2] * g[2];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) skipped += __shfl_xor(skipped, off);
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = skipped;
  __syncthreads();
  if (threadIdx.x == 0) skip_partial[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}

// thread = image-major observation e: Y_e = W_e V_p^-1 (6x3)
__global__ __launch_bounds__(256) void k_schur_obs(uint64_t O, const int* __restrict__ img_pt, const double* __restrict__ Wim,
                                                   const double* __restrict__ Vinv, double* __restrict__ Y) {
  const uint64_t e = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (e >= O) return;
  const double* v = Vinv + 9 * (size_t)img_pt[e];
  const double* w = Wim + 18 * e;
  double vi[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) vi[k] = v[k];
  double* y = Y + 18 * e;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double w0 = w[3 * r], w1 = w[3 * r + 1], w2 = w[3 * r + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) y[3 * r + c] = w0 * vi[c] + w1 * vi[3 + c] + w2 * vi[6 + c];
  }
}

// Inputs of the block kernel (one struct keeps the launch readable)
struct SchurBlocks {
  int ns; uint32_t nblk;
  const uint32_t* blk_start;   // [nblk+1] entries of each block: the ns diagonal blocks, then the pair blocks
  const uint32_t* ent_a; const uint32_t* ent_b;   // image-major positions (a in image i, b in image j)
  const uint32_t* pair_ij;     // [npairs][2] slots i < j
  const int* slot_img;         // [ns]
  const uint32_t* img_obs_start; const int* img_pt;
  const double* Y; const double* Wim; const double* Vg;
  const double* Himg; const double* gimg;
  const uint8_t* image_const_tvec;
  double mu; int mode;
  double* Sdiag; double* Soff; double* rhs; double* Dimg;
};

// one wavefront per block: lane-strided entries, 36 accumulators, xor butterfly (every lane ends with the same
// bitwise value, the order of the adds depends on the entry count only).  Diagonal blocks add U_i + D_i and the
// right-hand side.  Constant-tvec coordinates become identity rows / columns with a zero right-hand side.
__global__ __launch_bounds__(256) void k_schur_blocks(SchurBlocks sb) {
  const int lane = threadIdx.x & 63;
  const uint32_t blk = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (blk >= sb.nblk) return;
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (uint32_t t = sb.blk_start[blk] + lane; t < sb.blk_start[blk + 1]; t += 64) {
    const double* y = sb.Y + 18 * (size_t)sb.ent_a[t];
    const double* w = sb.Wim + 18 * (size_t)sb.ent_b[t];
    double yv[18], wv[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) { yv[k] = y[k]; wv[k] = w[k]; }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int s = 0; s < 6; ++s)
        acc[6 * r + s] += yv[3 * r] * wv[3 * s] + yv[3 * r + 1] * wv[3 * s + 1] + yv[3 * r + 2] * wv[3 * s + 2];
  }
  double mine = 0.0;   // lane k < 36 keeps entry k (selects, no dynamic register indexing)
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    mine = lane == k ? v : mine;
  }
  const int r = lane / 6, s = lane - 6 * (lane / 6);
  if (blk < (uint32_t)sb.ns) {
    const int i = (int)blk, im = sb.slot_img[i];
    const unsigned tm = sb.image_const_tvec ? sb.image_const_tvec[im] : 0u;
    // rhs_i = -g_i + sum_{a in i} W_a V^-1 g_p(a), observations of the image in image-major order
    double q[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t e = sb.img_obs_start[im] + lane; e < sb.img_obs_start[im + 1]; e += 64) {
      const double* w = sb.Wim + 18 * (size_t)e;
      const double* vg = sb.Vg + 3 * (size_t)sb.img_pt[e];
      const double v0 = vg[0], v1 = vg[1], v2 = vg[2];
#pragma unroll
      for (int k = 0; k < 6; ++k) q[k] += w[3 * k] * v0 + w[3 * k + 1] * v1 + w[3 * k + 2] * v2;
    }
    double qm = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double v = q[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      qm = lane == k ? v : qm;
    }
    const double* H = sb.Himg + 36 * (size_t)im;
    if (lane < 36) {
      const bool ir = r >= 3 && ((tm >> (r - 3)) & 1u), is = s >= 3 && ((tm >> (s - 3)) & 1u);
      double v = H[6 * r + s] - mine;
      if (r == s) v += damp_of(sb.mode, sb.mu, H[7 * r]);
      if (ir || is) v = r == s ? 1.0 : 0.0;
      sb.Sdiag[36 * (size_t)i + lane] = v;
    }
    if (lane < 6) {
      const bool in = lane >= 3 && ((tm >> (lane - 3)) & 1u);
      sb.rhs[6 * (size_t)i + lane] = in ? 0.0 : qm - sb.gimg[6 * (size_t)im + lane];
      sb.Dimg[6 * (size_t)i + lane] = in ? 0.0 : damp_of(sb.mode, sb.mu, H[7 * lane]);
    }
  } else if (lane < 36) {
    const uint32_t pq = blk - (uint32_t)sb.ns;
    const int si = (int)sb.pair_ij[2 * (size_t)pq], sj = (int)sb.pair_ij[2 * (size_t)pq + 1];
    const unsigned ti = sb.image_const_tvec ? sb.image_const_tvec[sb.slot_img[si]] : 0u;
    const unsigned tj = sb.image_const_tvec ? sb.image_const_tvec[sb.slot_img[sj]] : 0u;
    const bool ir = r >= 3 && ((ti >> (r - 3)) & 1u), is = s >= 3 && ((tj >> (s - 3)) & 1u);
    sb.Soff[36 * (size_t)pq + lane] = (ir || is) ? 0.0 : 0.0 - mine;
  }
}

// the pose blocks, both triangles, into the dense S with leading dimension n (6 ns; 6 ns + 12 ncs with camera rows,
// whose entries are k_schur_cam_dense's); the caller zeroed it.  thread = (block, entry)
__global__ __launch_bounds__(256) void k_schur_dense(int ns, uint32_t nblk, const uint32_t* __restrict__ pair_ij,
                                                     const double* __restrict__ Sdiag, const double* __restrict__ Soff,
                                                     size_t n, double* __restrict__ S) {
  const uint64_t t = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (t >= (uint64_t)nblk * 36) return;
  const uint32_t blk = (uint32_t)(t / 36);
  const int k = (int)(t - 36 * (uint64_t)blk), r = k / 6, s = k - 6 * (k / 6);
  if (blk < (uint32_t)ns) {
    S[(6 * (size_t)blk + r) * n + 6 * (size_t)blk + s] = Sdiag[36 * (size_t)blk + k];
  } else {
    const uint32_t pq = blk - (uint32_t)ns;
    const size_t i = pair_ij[2 * (size_t)pq], j = pair_ij[2 * (size_t)pq + 1];
    const double v = Soff[36 * (size_t)pq + k];
    S[(6 * i + r) * n + 6 * j + s] = v;
    S[(6 * j + s) * n + 6 * i + r] = v;
  }
}

// The handle's blocks into the padded scratch of the direct solve (ba_chol.h; the caller zeroed it): lower triangle
// only -- a diagonal block's entries r >= s, a pair block (i < j) transposed into rows of j -- and the right-hand side
// row.  thread = (block, entry); the first 6 ns threads also carry the right-hand side.
__global__ __launch_bounds__(256) void k_chol_fill_blocks(int ns, uint32_t nblk, const uint32_t* __restrict__ pair_ij,
                                                          const double* __restrict__ Sdiag, const double* __restrict__ Soff,
                                                          const double* __restrict__ rhs, int np, double* __restrict__ A) {
  const uint64_t t = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (t >= (uint64_t)nblk * 36) return;
  const size_t ld = (size_t)np;
  if (t < 6 * (uint64_t)ns) A[ld * ld + t] = rhs[t];
  const uint32_t blk = (uint32_t)(t / 36);
  const int k = (int)(t - 36 * (uint64_t)blk), r = k / 6, s = k - 6 * (k / 6);
  if (blk < (uint32_t)ns) {
    if (r >= s) A[(6 * (size_t)blk + r) * ld + 6 * (size_t)blk + s] = Sdiag[36 * (size_t)blk + k];
  } else {
    const uint32_t pq = blk - (uint32_t)ns;
    const size_t i = pair_ij[2 * (size_t)pq], j = pair_ij[2 * (size_t)pq + 1];
    A[(6 * j + s) * ld + 6 * i + r] = Soff[36 * (size_t)pq + k];
  }
}

// thread = point: delta X_p = -V^-1 (g_p + sum_{a in p} W_a^T delta c_img(a)) and the partial of the model decrease
// over the points: schur_back_point (ba_solve_cam.h, shared with k_schur_cam_back) with no camera term
__global__ __launch_bounds__(256) void k_schur_back(int P, const uint32_t* __restrict__ pt_start,
                                                    const uint32_t* __restrict__ pt_list, const int* __restrict__ obs_image,
                                                    const uint32_t* __restrict__ obs_pos, const int* __restrict__ img_slot,
                                                    const double* __restrict__ Wim, const double* __restrict__ Vinv,
                                                    const double* __restrict__ gpt, const double* __restrict__ Dpt,
                                                    const double* __restrict__ dpose, double* __restrict__ dpoint,
                                                    double* __restrict__ md_partial) {
  schur_back_point(P, pt_start, pt_list, obs_image, obs_pos, img_slot, Wim, Vinv, gpt, Dpt, dpose, dpoint, md_partial,
                   [](int, double&, double&, double&) {});
}

// one workgroup: 1/2 (slot terms + point partials), strided per thread then a fixed tree
__global__ __launch_bounds__(256) void k_schur_model_decrease(int ns, const int* __restrict__ slot_img,
                                                              const uint8_t* __restrict__ image_const_tvec,
                                                              const double* __restrict__ gimg, const double* __restrict__ Dimg,
                                                              const double* __restrict__ dpose,
                                                              const double* __restrict__ md_partial, int nbp,
                                                              double* __restrict__ out) {
  __shared__ double s_c[256];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < ns; i += 256) {
    const int im = slot_img[i];
    const unsigned tm = image_const_tvec ? image_const_tvec[im] : 0u;
    const double* g = gimg + 6 * (size_t)im;
    const double* d = Dimg + 6 * (size_t)i;
    const double* x = dpose + 6 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const bool inactive = k >= 3 && ((tm >> (k - 3)) & 1u);   // delta 0 there, whatever the caller passed
      a += inactive ? 0.0 : -x[k] * g[k] + d[k] * x[k] * x[k];
    }
  }
  for (int i = threadIdx.x; i < nbp; i += 256) b += md_partial[i];
  s_c[threadIdx.x] = a + b;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_c[threadIdx.x] += s_c[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = 0.5 * s_c[0];
}

__global__ __launch_bounds__(256) void k_sum_u32(const uint32_t* __restrict__ partial, int n, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_c[256];
  unsigned long long a = 0;
  for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
  s_c[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_c[threadIdx.x] += s_c[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s_c[0];
}

// Ceres' QuaternionManifold::Plus (q <- [cos|d|, sin|d|/|d| d] * q) and t += dt on the variable coordinates;
// constant poses / tvec components / points are copied.  thread = image (t < I) or point.  In-place safe.
__global__ __launch_bounds__(256) void k_ba_plus(int I, int P, const int* __restrict__ img_slot,
                                                 const uint8_t* __restrict__ image_const_tvec,
                                                 const uint8_t* __restrict__ point_const, const double* poses,
                                                 const double* points, const double* __restrict__ dpose,
                                                 const double* __restrict__ dpoint, double* poses_out, double* points_out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < I) {
    const double* x = poses + 7 * (size_t)t;
    double y[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) y[k] = x[k];
    const int s = img_slot[t];
    if (s >= 0) {
      const double* d = dpose + 6 * (size_t)s;
      const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (nd != 0.0) {
        const double sd = sin(nd) / nd;
        const double a0 = cos(nd), a1 = sd * d[0], a2 = sd * d[1], a3 = sd * d[2];
        y[0] = a0 * x[0] - a1 * x[1] - a2 * x[2] - a3 * x[3];
        y[1] = a0 * x[1] + a1 * x[0] + a2 * x[3] - a3 * x[2];
        y[2] = a0 * x[2] - a1 * x[3] + a2 * x[0] + a3 * x[1];
        y[3] = a0 * x[3] + a1 * x[2] - a2 * x[1] + a3 * x[0];
      }
      const unsigned tm = image_const_tvec ? image_const_tvec[t] : 0u;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (!((tm >> k) & 1u)) y[4 + k] = x[4 + k] + d[3 + k];
    }
    double* o = poses_out + 7 * (size_t)t;
#pragma unroll
    for (int k = 0; k < 7; ++k) o[k] = y[k];
  } else if (t < I + P) {
    const int p = t - I;
    const double* x = points + 3 * (size_t)p;
    const double* d = dpoint + 3 * (size_t)p;
    const bool c = point_const && point_const[p];
    double* o = points_out + 3 * (size_t)p;
    const double y0 = c ? x[0] : x[0] + d[0], y1 = c ? x[1] : x[1] + d[1], y2 = c ? x[2] : x[2] + d[2];
    o[0] = y0; o[1] = y1; o[2] = y2;
  }
}

// max |g| over the active pose coordinates of the slots and the non-constant points: partial max per workgroup
// (a maximum does not depend on the order), grid-stride
__global__ __launch_bounds__(256) void k_ba_grad_max(int ns, const int* __restrict__ slot_img,
                                                     const uint8_t* __restrict__ image_const_tvec,
                                                     const double* __restrict__ gimg, int P,
                                                     const uint8_t* __restrict__ point_const,
                                                     const double* __restrict__ gpt, double* __restrict__ partial) {
  __shared__ double s_m[4];
  double m = 0.0;
  const int n = ns + P;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
    if (t < ns) {
      const int im = slot_img[t];
      const unsigned tm = image_const_tvec ? image_const_tvec[im] : 0u;
      const double* g = gimg + 6 * (size_t)im;
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (!(k >= 3 && ((tm >> (k - 3)) & 1u))) m = fmax(m, fabs(g[k]));
    } else {
      const int p = t - ns;
      if (!(point_const && point_const[p])) {
        const double* g = gpt + 3 * (size_t)p;
        m = fmax(m, fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2]))));
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
}

// what the LM loop of pcd_ba_solve reads per iteration, in one device-to-host copy
struct LmRecord {
  double cost, candidate_cost, model_decrease, gradient_max;
  unsigned long long num_skipped;
  pcd_ba_pcg_info pcg;
};
__global__ __launch_bounds__(256) void k_ba_lm_record(const double* __restrict__ cost, const double* __restrict__ cand,
                                                      const double* __restrict__ md, const double* __restrict__ gpart,
                                                      int ngp, const unsigned long long* __restrict__ skipped,
                                                      const pcd_ba_pcg_info* __restrict__ info, LmRecord* __restrict__ out) {
  __shared__ double s_m[4];
  double m = 0.0;
  for (int i = threadIdx.x; i < ngp; i += 256) m = fmax(m, gpart[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    LmRecord r;
    r.cost = cost[0]; r.candidate_cost = cand[0]; r.model_decrease = md[0];
    r.gradient_max = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
    r.num_skipped = skipped[0]; r.pcg = *info;
    *out = r;
  }
}

// the record of a direct solve in the form k_ba_lm_record reads: 0 iterations, termination = pcd_ba_chol_status
__global__ void k_chol_lm_info(const pcd_ba_chol_info* __restrict__ c, pcd_ba_pcg_info* __restrict__ out) {
  pcd_ba_pcg_info o;
  o.iterations = 0; o.termination = c->status; o.precond_fallbacks = 0;
  o.rhs_norm = 0.0; o.residual_norm = 0.0; o.q = 0.0; o.step_dot_residual = 0.0;
  *out = o;
}

// The solver state of a handle, one group per owner; the element counts are ba_handle.h's.  device_bytes()
// (pcd_ba_schur_stats) is the sum of the groups' bytes(): every DevBuf but the 8 bytes of num.skip_cnt.
struct BaSchur {
  using Structure = SchurStructure;   // ba_schur_structure.h: built on the device by the first Schur call, then read only
  Structure st;
  struct Numeric {   // the last Schur call (pcd_ba_schur_device)
    bool valid = false;   // it has filled the buffers below ...
    bool own_diag = false, own_off = false, own_rhs = false;   // ... and left S_diag / S_off / rhs in the handle
    DevBuf<double> Himg, gimg, Hpt, gpt, Wim, Y, Vinv, Vg, Dpt, Dimg, Sdiag, Soff, rhs, md_partial, md;
    DevBuf<uint32_t> skip_partial; DevBuf<unsigned long long> skip_cnt;
    DevBuf<double> cost, dense;   // dense: staging of the host form's S
    uint64_t bytes() const {
      return dev_bytes(Himg, gimg, Hpt, gpt, Wim, Y, Vinv, Vg, Dpt, Dimg, Sdiag, Soff, rhs, md_partial, md, skip_partial,
                       cost, dense);
    }
  } num;
  struct Pcg {   // pcd_ba_schur_solve_pcg*
    DevBuf<double> Minv, x0, x1, r, z, p0, p1, w, pw, partial, out;   // out: staging of the host form
    DevBuf<double> Minv_cam, camw;   // the bordered solve: the vectors above then carry the camera part behind the poses
    DevBuf<PcgState> state; DevBuf<pcd_ba_pcg_info> info; PinnedBuf<int> flag;
    int it = 0;   // iterations enqueued in the running solve (buffer parity)
    uint64_t bytes() const {
      return dev_bytes(Minv, x0, x1, r, z, p0, p1, w, pw, partial, out, Minv_cam, camw, state, info);
    }
  } cg;
  struct Lm {   // pcd_ba_solve: the step, the accepted parameters, the record of an iteration
    DevBuf<double> dpose, dpoint, poses, points, cam_params, cand_cost, gpart;   // dpose: dcam behind it with camera rows
    DevBuf<LmRecord> rec; PinnedBuf<LmRecord> host;
    uint64_t bytes() const { return dev_bytes(dpose, dpoint, poses, points, cam_params, cand_cost, gpart, rec); }
  } lm;
  struct Cam {   // pcd_ba_schur_cam*: the camera slots (uploaded once), the camera blocks and what is eliminated from them
    bool slots = false;   // cam_slot .. param_cam are on the device
    bool valid = false;   // the last Schur call was pcd_ba_schur_cam_device and has filled the buffers below
    DevBuf<int> cam_slot, slot_cam, param_cam; DevBuf<uint8_t> active;
    DevBuf<double> Hcam, gcam, Ecam, Wcam, Wc, Z, partial, B, Scam, rhs, D, dense, out;   // dense / out: host-form staging
    uint64_t bytes() const {
      return dev_bytes(cam_slot, slot_cam, param_cam, active, Hcam, gcam, Ecam, Wcam, Wc, Z, partial, B, Scam, rhs, D, dense, out);
    }
  } cam;
  struct Chol {   // pcd_ba_schur_solve_cholesky*: the padded dense scratch of ba_chol.h, allocated on first use
    DevBuf<double> A, S, rhs, out;   // S / rhs (freed after each call) / out: staging of the host form
    DevBuf<pcd_ba_chol_info> info, info_out;
    uint64_t bytes() const { return dev_bytes(A, S, rhs, out, info, info_out); }
  } chol;
  uint64_t device_bytes() const { return st.bytes() + num.bytes() + cg.bytes() + lm.bytes() + chol.bytes() + cam.bytes(); }
};

void BaSchurDelete::operator()(BaSchur* s) const { delete s; }
void ba_schur_invalidate(pcd_ba* b) { if (b->schur) b->schur->num.valid = b->schur->cam.valid = false; }
void ba_schur_drop_structure(pcd_ba* b) {
  if (!b->schur) return;
  b->schur->num.valid = b->schur->cam.valid = false;
  b->schur->st.built = false;   // the build assigns every member of the structure anew
}

}  // namespace pcd

using namespace pcd;

// ---- point elimination: guards and the co-visibility structure ----------------------------------------------
static int cam_slots(const pcd_ba* b) { return (int)b->h_slot_cam.size(); }

// Every Schur entry point, before anything is allocated or launched: no gfx950 device -> NO_DEVICE, no handle ->
// INVALID.  A plain call (cam false), and a _cam call on a handle without camera slots, which is its plain counterpart:
// refined intrinsics -> UNSUPPORTED (the reduced system would need the camera rows).  A _cam call: more camera slots
// than the bordered system carries -> UNSUPPORTED.  *ncs: the camera slots the call works with, 0 for the plain system.
static pcd_status schur_guard(pcd_ba* b, bool cam, int* ncs) {
  PCD_TRY(require_device(b ? b->device : 0));
  PCD_REQUIRE(b, "null handle");
  *ncs = cam ? cam_slots(b) : 0;
  if (*ncs > PCD_BA_MAX_CAMERA_SLOTS) {
    set_error("%d cameras have refined parameters; the reduced system carries at most PCD_BA_MAX_CAMERA_SLOTS = %d "
              "camera slots (cameras shared by many images)", *ncs, PCD_BA_MAX_CAMERA_SLOTS);
    return PCD_ERR_UNSUPPORTED;
  }
  if (!*ncs && b->refines_intrinsics) {
    set_error("point elimination with refined intrinsics (camera_refine) is not supported");
    return PCD_ERR_UNSUPPORTED;
  }
  return PCD_OK;
}
static pcd_status schur_guard(pcd_ba* b) { int ncs; return schur_guard(b, false, &ncs); }

// The co-visibility structure, if the handle has none (after pcd_ba_create, or after an edit dropped it): built on the
// device, on the stream of the call that needs it (ba_schur_structure.hip).  A capturing stream is refused before
// anything is allocated.  info (may be null): what the build did; build_ms 0 when there was nothing to build.
static pcd_status schur_build(pcd_ba* b, hipStream_t s, pcd_ba_schur_build_info* info = nullptr) {
  if (!b->schur || !b->schur->st.built) {
    PCD_TRY(refuse_capture(s, "pcd_ba_schur* (structure build)"));
    if (!b->schur) b->schur.reset(new BaSchur());
    PCD_HIP_TRY(hipSetDevice(b->device));
    int syncs = 0;
    PCD_TRY(schur_structure_build(b, b->schur->st, s, &syncs));
    if (info) { info->build_ms = b->schur->st.build_ms; info->num_syncs = syncs; }
  }
  const BaSchur::Structure& T = b->schur->st;
  if (info) { info->num_slots = T.ns; info->num_pairs = T.npairs; info->num_entries = T.nent; }
  return PCD_OK;
}

// ---- reduced solve: PCG and the LM loop -------------------------------------------------------------
// Iterations are enqueued in batches; between two batches the host reads the done flag (one 4-byte copy and a stream
// synchronisation).  8 covers the inexact steps of the LM loop (2-5 iterations at the defaults) in one batch at the
// price of a few returned-at-once launches; a tight solve grows the batch to 32.
static constexpr int kPcgFirstBatch = 8, kPcgMaxBatch = 32;

static pcd_status pcg_check_opts(const pcd_ba_pcg_opts* o) {
  PCD_REQUIRE(o, "null pointer");
  PCD_REQUIRE(o->preconditioner == PCD_PRECOND_IDENTITY || o->preconditioner == PCD_PRECOND_SCHUR_JACOBI, "preconditioner");
  PCD_REQUIRE(o->max_iterations >= 0 && o->min_iterations >= 0, "iteration limits must be >= 0");
  PCD_REQUIRE(o->q_tolerance == o->q_tolerance && o->r_tolerance == o->r_tolerance, "tolerance is not a number");
  return PCD_OK;
}

// Can a solver read the handle's own system?  The state of a Schur call (what the back-substitution reads), and with
// `blocks` its S_diag / S_off / rhs in the handle's buffers (what the PCG and the direct solve read).  With camera
// slots (ncs > 0), also that the last Schur call carried camera rows.
static pcd_status schur_state_guard(const pcd_ba* b, const char* fn, bool blocks, int ncs) {
  if (!b->schur || !b->schur->num.valid) {
    set_error("%s: no Schur state (call pcd_ba_schur[_device] first)", fn);
    return PCD_ERR_INVALID;
  }
  const BaSchur::Numeric& N = b->schur->num;
  if (blocks && !(N.own_diag && N.own_off && N.own_rhs)) {
    set_error("%s: the last Schur call sent %s%s%s to caller memory; the solver reads the handle's own copy "
              "(leave those outputs NULL)", fn, N.own_diag ? "" : "S_diag ", N.own_off ? "" : "S_off ",
              N.own_rhs ? "" : "rhs ");
    return PCD_ERR_INVALID;
  }
  if (ncs && !b->schur->cam.valid) {
    set_error("%s: no Schur state with camera rows (call pcd_ba_schur_cam[_device] first)", fn);
    return PCD_ERR_INVALID;
  }
  return PCD_OK;
}

static PcgRule pcg_rule(const pcd_ba_pcg_opts* o) {
  return PcgRule{o->max_iterations, o->min_iterations, o->q_tolerance, o->r_tolerance};
}

// a solve's view of the handle; ncs camera slots ride behind the poses (0: the plain system)
static PcgVec pcg_vec(pcd_ba* b, int ncs) {
  BaSchur& S = *b->schur; const BaSchur::Structure& T = S.st; BaSchur::Pcg& C = S.cg;
  PcgVec v{};
  v.ns = T.ns; v.ncs = ncs; v.st = C.state.p;
  v.row_start = T.row_start.p; v.row_blk = T.row_blk.p; v.row_col = T.row_col.p;
  v.Sdiag = S.num.Sdiag.p; v.Soff = S.num.Soff.p; v.rhs = S.num.rhs.p;
  v.B = S.cam.B.p; v.Scam = S.cam.Scam.p; v.rhs_cam = S.cam.rhs.p;
  v.Minv = C.Minv.p; v.Minv_cam = C.Minv_cam.p; v.x0 = C.x0.p; v.x1 = C.x1.p; v.p0 = C.p0.p; v.p1 = C.p1.p;
  v.z = C.z.p; v.r = C.r.p; v.w = C.w.p; v.camw = C.camw.p; v.pw = C.pw.p; v.partial = C.partial.p;
  return v;
}

// preconditioner, x = 0, r = rhs, the scalars of iteration 0.  With camera slots the vectors carry the 12 ncs camera
// coordinates behind the poses and the partial lists one entry per camera slot behind the workgroups
static pcd_status pcg_begin(pcd_ba* b, const pcd_ba_pcg_opts* o, int ncs, hipStream_t s) {
  BaSchur::Pcg& C = b->schur->cg;
  const int ns = b->schur->st.ns; const unsigned nb = std::max(1u, div_up((uint64_t)ns, 256));
  const size_t nc = (size_t)kCamS * ncs;
  PCD_TRY(C.Minv.reserve(at_least_1(blocks_6x6(ns))));
  for (DevBuf<double>* d : {&C.x0, &C.x1, &C.r, &C.z, &C.p0, &C.p1, &C.w}) PCD_TRY(d->reserve(at_least_1(slot_vec(ns) + nc)));
  PCD_TRY(C.pw.reserve(at_least_1(ns + nc))); PCD_TRY(C.partial.reserve(4 * ((size_t)nb + ncs)));
  PCD_TRY(C.state.reserve(1)); PCD_TRY(C.info.reserve(1)); PCD_TRY(C.flag.reserve(4));
  if (ncs) { PCD_TRY(C.Minv_cam.reserve(nc * kCamS)); PCD_TRY(C.camw.reserve(at_least_1(nc * ns))); }
  C.it = 0;
  pcg_init(pcg_vec(b, ncs), o->preconditioner, pcg_rule(o), s);
  return PCD_OK;
}

// `count` more iterations (all their launches return at once when the solve has ended)
static void pcg_enqueue(pcd_ba* b, const pcd_ba_pcg_opts* o, int ncs, int count, hipStream_t s) {
  const PcgVec v = pcg_vec(b, ncs); const PcgRule rule = pcg_rule(o); BaSchur::Pcg& C = b->schur->cg;
  if (!v.ns && !ncs) return;   // nothing was enqueued: the parity stays
  for (int c = 0; c < count; ++c, ++C.it) pcg_iterate(v, C.it, rule, s);
}

// batches until the device says done; `enqueued` iterations are already in the stream.  One flag copy per batch.
static pcd_status pcg_run(pcd_ba* b, const pcd_ba_pcg_opts* o, int ncs, int enqueued, hipStream_t s) {
  BaSchur::Pcg& C = b->schur->cg;
  int batch = kPcgFirstBatch;
  if (!enqueued) { pcg_enqueue(b, o, ncs, std::min(batch, o->max_iterations), s); enqueued = std::min(batch, o->max_iterations); }
  for (;;) {
    PCD_HIP_TRY(hipMemcpyAsync(C.flag.p, &C.state.p->done, sizeof(int), hipMemcpyDeviceToHost, s));
    PCD_HIP_TRY(hipStreamSynchronize(s));
    if (C.flag.p[0] || (!b->schur->st.ns && !ncs) || enqueued >= o->max_iterations) return PCD_OK;
    batch = std::min(2 * batch, kPcgMaxBatch);
    const int n = std::min(batch, o->max_iterations - enqueued);
    pcg_enqueue(b, o, ncs, n, s); enqueued += n;
  }
}

// Direct solve of the system [6 ns | 12 ncs]: scratch on first use, fill (the handle's blocks when d_S is null, else the
// caller's dense S, which only the plain system has: ncs = 0), factor and solve.  No synchronisation; the status record
// stays in chol.info.
static pcd_status chol_solve(pcd_ba* b, int ncs, const double* d_S, const double* d_rhs, double* d_delta,
                             pcd_ba_chol_info* d_info, hipStream_t s) {
  const BaSchur::Structure& T = b->schur->st; const BaSchur::Numeric& N = b->schur->num;
  BaSchur::Chol& K = b->schur->chol; const BaSchur::Cam& Cm = b->schur->cam;
  PCD_REQUIRE(!d_S || !ncs, "a caller's dense S has no camera rows");
  const int ns = T.ns, n = (int)slot_vec(ns) + kCamS * ncs;
  PCD_TRY(K.A.reserve(chol_scratch_doubles(n))); PCD_TRY(K.info.reserve(1));
  chol_begin(K.A.p, n, K.info.p, s);
  if (d_S) chol_fill_dense(K.A.p, n, d_S, d_rhs, s);
  else if (T.nblk())
    hipLaunchKernelGGL(k_chol_fill_blocks, dim3(div_up(blocks_6x6(T.nblk()), 256)), dim3(256), 0, s, ns, T.nblk(),
                       T.pair_ij.p, N.Sdiag.p, N.Soff.p, N.rhs.p, chol_padded(n), K.A.p);
  if (ncs) schur_cam_fill_chol(ns, ncs, Cm.B.p, Cm.Scam.p, Cm.rhs.p, chol_padded(n), K.A.p, s);
  chol_factor_solve(K.A.p, n, K.info.p, d_delta, d_info, s);
  return PCD_OK;
}

// the elimination proper: V^-1 per point and the skip count, Y per observation, the blocks of S and rhs
static void schur_eliminate(pcd_ba* b, const pcd_ba_schur_opts* opt, unsigned nbp, double* Sdiag, double* Soff,
                            double* rhs, unsigned long long* skipped, hipStream_t s) {
  const BaSchur::Structure& T = b->schur->st; BaSchur::Numeric& N = b->schur->num;
  const int P = b->P; const uint64_t O = b->O;
  hipLaunchKernelGGL(k_schur_points, dim3(nbp), dim3(256), 0, s, P, N.Hpt.p, N.gpt.p, b->const_points(), opt->mu,
                     opt->damping, N.Vinv.p, N.Vg.p, N.Dpt.p, N.skip_partial.p);
  hipLaunchKernelGGL(k_sum_u32, dim3(1), dim3(256), 0, s, N.skip_partial.p, (int)nbp, skipped);
  if (O) hipLaunchKernelGGL(k_schur_obs, dim3(div_up(O, 256)), dim3(256), 0, s, O, b->img_pt.p, N.Wim.p, N.Vinv.p, N.Y.p);
  SchurBlocks sb;
  sb.ns = T.ns; sb.nblk = T.nblk(); sb.blk_start = T.blk_start.p; sb.ent_a = T.ent_a.p; sb.ent_b = T.ent_b.p;
  sb.pair_ij = T.pair_ij.p; sb.slot_img = T.slot_img.p; sb.img_obs_start = b->img_obs_start.p; sb.img_pt = b->img_pt.p;
  sb.Y = N.Y.p; sb.Wim = N.Wim.p; sb.Vg = N.Vg.p; sb.Himg = N.Himg.p; sb.gimg = N.gimg.p;
  sb.image_const_tvec = b->const_tvec(); sb.mu = opt->mu; sb.mode = opt->damping;
  sb.Sdiag = Sdiag; sb.Soff = Soff; sb.rhs = rhs; sb.Dimg = N.Dimg.p;
  if (sb.nblk) hipLaunchKernelGGL(k_schur_blocks, dim3(div_up(sb.nblk, 4)), dim3(256), 0, s, sb);
}

static pcd_status lm_check_opts(const pcd_ba_solve_opts* o) {
  PCD_REQUIRE(o, "null pointer"); PCD_TRY(pcg_check_opts(&o->linear));
  PCD_REQUIRE(o->damping == PCD_DAMP_MARQUARDT || o->damping == PCD_DAMP_LEVENBERG, "damping");
  PCD_REQUIRE(o->max_num_iterations >= 0, "max_num_iterations must be >= 0");
  PCD_REQUIRE(o->initial_radius > 0.0 && o->max_radius > 0.0, "radius must be > 0");
  PCD_REQUIRE(o->linear_solver == PCD_LINEAR_PCG || o->linear_solver == PCD_LINEAR_CHOLESKY ||
              o->linear_solver == PCD_LINEAR_PCG_CAM, "linear_solver");
  return PCD_OK;
}

static pcd_status lm_reserve(pcd_ba* b, unsigned ngp, int ncs) {
  BaSchur::Lm& M = b->schur->lm;
  PCD_TRY(M.dpose.reserve(at_least_1(slot_vec(b->schur->st.ns) + (size_t)kCamS * ncs))); PCD_TRY(M.poses.reserve(7 * (size_t)b->I));
  if (ncs) PCD_TRY(M.cam_params.reserve(at_least_1(b->cam_params_len)));
  PCD_TRY(M.dpoint.reserve(point_vec(b->P))); PCD_TRY(M.points.reserve(point_vec(b->P)));
  PCD_TRY(M.cand_cost.reserve(1)); PCD_TRY(M.rec.reserve(1)); PCD_TRY(M.host.reserve(1));
  return M.gpart.reserve(ngp);
}

// poses and points of the handle's size from src to dst, on the device: the handle's own and lm.poses / lm.points
static pcd_status copy_parameters(const pcd_ba* b, double* dst_poses, double* dst_points, const double* src_poses,
                                  const double* src_points, hipStream_t s) {
  PCD_HIP_TRY(hipMemcpyAsync(dst_poses, src_poses, 7 * (size_t)b->I * sizeof(double), hipMemcpyDeviceToDevice, s));
  PCD_HIP_TRY(hipMemcpyAsync(dst_points, src_points, point_vec(b->P) * sizeof(double), hipMemcpyDeviceToDevice, s));
  return PCD_OK;
}
// the camera parameters beside them, when the loop moves them: save = the handle's into lm.cam_params, else back
static pcd_status copy_camera_parameters(pcd_ba* b, bool save, hipStream_t s) {
  double* kept = b->schur->lm.cam_params.p;
  if (b->cam_params_len)
    PCD_HIP_TRY(hipMemcpyAsync(save ? kept : b->cam_params.p, save ? b->cam_params.p : kept,
                               b->cam_params_len * sizeof(double), hipMemcpyDeviceToDevice, s));
  return PCD_OK;
}

// the internal forms of the entry points lm_try_step calls, below
static pcd_status back_substitute_device(pcd_ba* b, bool cam, const double* d_delta, double* d_dpoint,
                                         double* d_model_decrease, void* stream);
static pcd_status plus_device(pcd_ba* b, bool cam, const double* d_delta, const double* d_dpoint, double* d_poses_out,
                              double* d_points_out, double* d_cam_params_out, void* stream);

// The linear solve of an iteration into lm.dpose (dpose, then dcam) / cg.info: the direct solve (an exact step: nothing
// left to run, *enq = max_iterations), or pcg_begin and the first batch (*enq = its iterations)
static pcd_status lm_enqueue_linear(pcd_ba* b, const pcd_ba_solve_opts* o, int ncs, int* enq, hipStream_t s) {
  BaSchur& S = *b->schur;
  *enq = o->linear.max_iterations;
  if (o->linear_solver == PCD_LINEAR_CHOLESKY) {
    PCD_TRY(S.cg.info.reserve(1));
    if (S.st.ns || ncs) {
      ScopedKernelTimer t("ba_schur_cholesky", s);
      PCD_TRY(chol_solve(b, ncs, nullptr, nullptr, S.lm.dpose.p, nullptr, s));
      hipLaunchKernelGGL(k_chol_lm_info, dim3(1), dim3(1), 0, s, S.chol.info.p, S.cg.info.p);
    } else {
      PCD_HIP_TRY(hipMemsetAsync(S.cg.info.p, 0, sizeof(pcd_ba_pcg_info), s));   // 0 iterations, PCD_CHOL_OK
    }
  } else {
    PCD_TRY(pcg_begin(b, &o->linear, ncs, s));   // with camera slots: PCD_LINEAR_PCG_CAM, the bordered system
    *enq = std::min(kPcgFirstBatch, o->linear.max_iterations);
    pcg_enqueue(b, &o->linear, ncs, *enq, s);
  }
  return PCD_OK;
}

// Tail of an iteration up to the synchronised read-back of its record into lm.host.  It is enqueued behind the first
// batch without looking at the flag: at the defaults the PCG has ended by then and the iteration costs one copy.  If the
// step came from an unfinished solve, the accepted parameters go back, the batches go on and the tail runs once more.
static pcd_status lm_try_step(pcd_ba* b, const pcd_ba_solve_opts* o, int ncs, int enq, unsigned ngp, EventPair& ev,
                              double* linear_ms, hipStream_t s) {
  BaSchur& S = *b->schur; BaSchur::Lm& M = S.lm;
  const bool cam = ncs > 0;
  pcd_ba_out co{}; co.cost = M.cand_cost.p;
  for (;;) {
    if (o->linear_solver != PCD_LINEAR_CHOLESKY) pcg_finish(pcg_vec(b, ncs), M.dpose.p, S.cg.info.p, s);
    PCD_TRY(back_substitute_device(b, cam, M.dpose.p, M.dpoint.p, S.num.md.p, s));
    PCD_TRY(plus_device(b, cam, M.dpose.p, M.dpoint.p, b->poses.p, b->points.p, cam ? b->cam_params.p : nullptr, s));
    PCD_TRY(pcd_ba_evaluate_device(b, &co, s));
    hipLaunchKernelGGL(k_ba_lm_record, dim3(1), dim3(256), 0, s, S.num.cost.p, M.cand_cost.p, S.num.md.p, M.gpart.p,
                       (int)ngp, S.num.skip_cnt.p, S.cg.info.p, M.rec.p);
    PCD_HIP_TRY(hipMemcpyAsync(M.host.p, M.rec.p, sizeof(LmRecord), hipMemcpyDeviceToHost, s));
    PCD_HIP_TRY(hipStreamSynchronize(s));
    if (float ms = 0.f; ev.elapsed(&ms) == hipSuccess) *linear_ms += ms;
    if (M.host.p->pcg.termination >= 0 || enq >= o->linear.max_iterations) break;
    PCD_TRY(copy_parameters(b, b->poses.p, b->points.p, M.poses.p, M.points.p, s));
    if (cam) PCD_TRY(copy_camera_parameters(b, false, s));
    PCD_HIP_TRY(ev.start(s));
    PCD_TRY(pcg_run(b, &o->linear, ncs, enq, s)); enq = o->linear.max_iterations;
    PCD_HIP_TRY(ev.stop(s));
  }
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

// What a record means for the loop, host arithmetic only: the iteration as reported (radius: the new one), radius and
// shrink factor of the next, the termination that ends the loop or -1 (gradient tolerance: nothing is recorded).
struct LmDecision { pcd_ba_solve_iteration it; double radius, factor; int termination; };
static LmDecision lm_decide(const LmRecord& rec, const pcd_ba_solve_opts& o, double radius, double factor, bool direct) {
  LmDecision d{}; pcd_ba_solve_iteration& r = d.it;
  const bool restore_only = o.gradient_tolerance > 0.0 && rec.gradient_max <= o.gradient_tolerance;
  r.cost = rec.cost; r.candidate_cost = rec.candidate_cost; r.model_decrease = rec.model_decrease;
  r.gradient_max_norm = rec.gradient_max; r.num_skipped = rec.num_skipped;
  r.linear_iterations = rec.pcg.iterations; r.linear_termination = rec.pcg.termination;
  const bool solved = direct ? rec.pcg.termination == PCD_CHOL_OK : rec.pcg.termination != PCD_PCG_BREAKDOWN;
  const double rho = (solved && r.model_decrease > 0.0) ? (r.cost - r.candidate_cost) / r.model_decrease
                                                        : -std::numeric_limits<double>::infinity();
  r.relative_decrease = rho; r.accepted = !restore_only && rho > o.min_relative_decrease;
  d.termination = restore_only ? (int)PCD_SOLVE_GRADIENT_TOLERANCE : -1;
  if (r.accepted) {
    radius = std::min(o.max_radius, radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3.0)));
    factor = 2.0;
    if (o.function_tolerance > 0.0 && std::fabs(r.cost - r.candidate_cost) <= o.function_tolerance * r.cost)
      d.termination = PCD_SOLVE_FUNCTION_TOLERANCE;
  } else if (!restore_only) { radius /= factor; factor *= 2.0; }
  r.radius = d.radius = radius; d.factor = factor;
  return d;
}

// ---- one host path per operation: ncs = 0 is the plain call, ncs > 0 carries the camera rows (ba_solve_cam.h) ------

// the pose outputs of a pcd_ba_schur_cam* call in the plain call's form
static pcd_ba_schur_out pose_out(const pcd_ba_schur_cam_out& o) {
  pcd_ba_schur_out po{};
  po.cost = o.cost; po.S_diag = o.S_diag; po.S_off = o.S_off; po.rhs = o.rhs; po.S = o.S; po.num_skipped = o.num_skipped;
  return po;
}

// the camera slots on the device, once (the structure exists: schur_build ran)
static pcd_status cam_upload_slots(pcd_ba* b) {
  BaSchur::Cam& K = b->schur->cam;
  if (K.slots) return PCD_OK;
  PCD_HIP_TRY(hipSetDevice(b->device));
  PCD_TRY(upload(K.cam_slot, b->h_cam_slot.data(), b->h_cam_slot.size()));
  PCD_TRY(upload(K.slot_cam, b->h_slot_cam.data(), b->h_slot_cam.size()));
  PCD_TRY(upload(K.param_cam, b->h_param_cam.data(), b->h_param_cam.size()));
  PCD_TRY(upload(K.active, b->h_cam_active.data(), b->h_cam_active.size()));
  K.slots = true;
  return PCD_OK;
}

// The camera rows behind the pose elimination: the camera blocks of the evaluation (its own scopes: ba_cameras,
// ba_cam_w), then Wc, Z, S_cam, rhs_cam and the border B into the handle
static pcd_status schur_cam_rows(pcd_ba* b, int ncs, const pcd_ba_schur_opts* opt, hipStream_t s) {
  const BaSchur::Structure& T = b->schur->st; BaSchur::Numeric& N = b->schur->num; BaSchur::Cam& K = b->schur->cam;
  {
    pcd_ba_out co{};
    co.H_cam = K.Hcam.p; co.g_cam = K.gcam.p; co.E_cam = K.Ecam.p; co.W_cam = K.Wcam.p;
    PCD_TRY(pcd_ba_evaluate_device(b, &co, s));
  }
  SchurCamIn in{};
  in.P = b->P; in.I = b->I; in.ns = T.ns; in.ncs = ncs;
  in.shared = ncs == 1 && b->shared_cam >= 0 && b->h_cam_slot[b->shared_cam] == 0;
  in.cam_slot = K.cam_slot.p; in.slot_cam = K.slot_cam.p; in.active = K.active.p;
  in.image_cam = b->image_cam.p; in.obs_image = b->obs_image.p;
  in.pt_obs_start = b->pt_obs_start.p; in.pt_obs_list = b->pt_obs_list.p;
  in.img_obs_start = b->img_obs_start.p; in.img_pt = b->img_pt.p;
  in.slot_img = T.slot_img.p; in.image_const_tvec = b->const_tvec();
  in.Vinv = N.Vinv.p; in.gpt = N.gpt.p; in.Wim = N.Wim.p;
  in.Hcam = K.Hcam.p; in.gcam = K.gcam.p; in.Ecam = K.Ecam.p; in.Wcam = K.Wcam.p;
  in.mu = opt->mu; in.mode = opt->damping;
  const SchurCamOut out{K.Wc.p, K.Z.p, K.partial.p, K.B.p, K.Scam.p, K.rhs.p, K.D.p};
  {
    ScopedKernelTimer t("ba_schur_cam_eliminate", s);
    schur_cam_eliminate(in, out, s);
  }
  {
    ScopedKernelTimer t("ba_schur_cam_border", s);
    schur_cam_border(in, out, s);
  }
  return PCD_OK;
}

// pcd_ba_schur_device (ncs = 0, co null) and pcd_ba_schur_cam_device behind their handle guard.  o: the pose outputs and
// the dense S [n][n], n = 6 ns + 12 ncs; co: where B, S_cam and rhs_cam go beside the handle's own copy.
static pcd_status schur_device(pcd_ba* b, int ncs, const pcd_ba_schur_opts* opt, const pcd_ba_schur_out* o,
                               const pcd_ba_schur_cam_out* co, void* stream) {
  PCD_REQUIRE(opt && o, "null pointer");
  PCD_REQUIRE(opt->damping == PCD_DAMP_MARQUARDT || opt->damping == PCD_DAMP_LEVENBERG, "damping");
  PCD_REQUIRE(opt->mu >= 0.0, "mu must be >= 0");
  hipStream_t s = (hipStream_t)stream;
  PCD_TRY(refuse_capture(s, ncs ? "pcd_ba_schur_cam_device" : "pcd_ba_schur_device"));
  PCD_TRY(schur_build(b, s));
  if (ncs) PCD_TRY(cam_upload_slots(b));
  const BaSchur::Structure& T = b->schur->st; BaSchur::Numeric& N = b->schur->num; BaSchur::Cam& K = b->schur->cam;
  const int I = b->I, P = b->P, ns = T.ns;
  const size_t nc = (size_t)kCamS * ncs;
  const unsigned nbp = std::max(1u, div_up((uint64_t)P, 256));   // grid of k_schur_points = length of its partials
  N.valid = K.valid = false;
  if (ncs) {
    PCD_TRY(K.Hcam.reserve((size_t)kCamS * kCamS * b->C)); PCD_TRY(K.gcam.reserve((size_t)kCamS * b->C));
    PCD_TRY(K.Ecam.reserve(at_least_1((size_t)kCamS * 6 * I))); PCD_TRY(K.Wcam.reserve(at_least_1(36 * (size_t)b->O)));
    PCD_TRY(K.Wc.reserve(at_least_1(36 * (size_t)P * ncs))); PCD_TRY(K.Z.reserve(at_least_1(36 * (size_t)P * ncs)));
    PCD_TRY(K.partial.reserve(cam_pairs(ncs) * kCamEnt * cam_chunks(P)));
    PCD_TRY(K.B.reserve(at_least_1((size_t)ns * nc * 6))); PCD_TRY(K.Scam.reserve(nc * nc));
    PCD_TRY(K.rhs.reserve(nc)); PCD_TRY(K.D.reserve(nc));
  }
  PCD_TRY(N.Himg.reserve(blocks_6x6(I))); PCD_TRY(N.gimg.reserve(slot_vec(I)));
  PCD_TRY(N.Hpt.reserve(point_blocks(P))); PCD_TRY(N.gpt.reserve(point_vec(P)));
  PCD_TRY(N.Wim.reserve(at_least_1(obs_blocks(b->O)))); PCD_TRY(N.Y.reserve(at_least_1(obs_blocks(b->O))));
  PCD_TRY(N.Vinv.reserve(point_blocks(P))); PCD_TRY(N.Vg.reserve(point_vec(P))); PCD_TRY(N.Dpt.reserve(point_vec(P)));
  PCD_TRY(N.Dimg.reserve(at_least_1(slot_vec(ns)))); PCD_TRY(N.Sdiag.reserve(at_least_1(blocks_6x6(ns))));
  PCD_TRY(N.Soff.reserve(at_least_1(blocks_6x6(T.npairs)))); PCD_TRY(N.rhs.reserve(at_least_1(slot_vec(ns))));
  PCD_TRY(N.skip_partial.reserve(nbp)); PCD_TRY(N.skip_cnt.reserve(1));
  PCD_TRY(N.md_partial.reserve(nbp)); PCD_TRY(N.md.reserve(1)); PCD_TRY(N.cost.reserve(1));
  PCD_HIP_TRY(hipSetDevice(b->device));
  double* Sdiag = o->S_diag ? o->S_diag : N.Sdiag.p; double* Soff = o->S_off ? o->S_off : N.Soff.p;
  {
    ScopedKernelTimer t("ba_schur_normal", s);
    // iota as the W order: W lands in image-major order (k_ba_images' contiguous store path)
    PCD_TRY(ba_normal_equations(b, T.iota.p, N.Hpt.p, N.gpt.p, o->cost ? o->cost : N.cost.p, N.Himg.p, N.gimg.p,
                                N.Wim.p, s));
  }
  {
    ScopedKernelTimer t("ba_schur_eliminate", s);
    schur_eliminate(b, opt, nbp, Sdiag, Soff, o->rhs ? o->rhs : N.rhs.p,
                    o->num_skipped ? reinterpret_cast<unsigned long long*>(o->num_skipped) : N.skip_cnt.p, s);
  }
  if (ncs) PCD_TRY(schur_cam_rows(b, ncs, opt, s));
  if (o->S && (ns || ncs)) {   // test and debugging output; with camera rows one launch for the pose blocks, one for the rest
    ScopedKernelTimer t("ba_schur_dense", s);
    const size_t n = slot_vec(ns) + nc;
    PCD_HIP_TRY(hipMemsetAsync(o->S, 0, n * n * sizeof(double), s));
    if (T.nblk())
      hipLaunchKernelGGL(k_schur_dense, dim3(div_up(blocks_6x6(T.nblk()), 256)), dim3(256), 0, s, ns, T.nblk(),
                         T.pair_ij.p, Sdiag, Soff, n, o->S);
    if (ncs) schur_cam_dense(ns, ncs, K.B.p, K.Scam.p, o->S, s);
  }
  if (ncs) {
    const auto copy_out = [&](double* dst, const double* src, size_t n) -> pcd_status {
      if (dst && n) PCD_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, s));
      return PCD_OK;
    };
    PCD_TRY(copy_out(co->B, K.B.p, (size_t)ns * nc * 6)); PCD_TRY(copy_out(co->S_cam, K.Scam.p, nc * nc));
    PCD_TRY(copy_out(co->rhs_cam, K.rhs.p, nc));
  }
  PCD_HIP_TRY(hipGetLastError());
  N.valid = true; N.own_diag = !o->S_diag; N.own_off = !o->S_off; N.own_rhs = !o->rhs;
  K.valid = ncs > 0;
  return PCD_OK;
}

// the host forms pcd_ba_schur and pcd_ba_schur_cam behind their handle guard and null check: schur_device into the
// handle's own buffers and a staged dense S, then every requested output copied back
static pcd_status schur_host(pcd_ba* b, int ncs, const pcd_ba_schur_opts* opt, const pcd_ba_schur_out* o,
                             const pcd_ba_schur_cam_out* co) {
  PCD_TRY(schur_build(b, nullptr));
  const BaSchur::Structure& T = b->schur->st; BaSchur::Numeric& N = b->schur->num; BaSchur::Cam& K = b->schur->cam;
  const size_t n0 = slot_vec(T.ns), nc = (size_t)kCamS * ncs, n = n0 + nc;
  DevBuf<double>& dense = ncs ? K.dense : N.dense;
  pcd_ba_schur_out d{}; const pcd_ba_schur_cam_out dc{};
  if (o->S) { PCD_TRY(dense.reserve(at_least_1(n * n))); d.S = dense.p; }
  PCD_TRY(schur_device(b, ncs, opt, &d, &dc, nullptr));
  PCD_TRY(copy_back(o->cost, N.cost, 1)); PCD_TRY(copy_back(o->num_skipped, N.skip_cnt, 1));
  PCD_TRY(copy_back(o->S_diag, N.Sdiag, blocks_6x6(T.ns))); PCD_TRY(copy_back(o->S_off, N.Soff, blocks_6x6(T.npairs)));
  PCD_TRY(copy_back(o->rhs, N.rhs, n0));
  if (ncs) {
    PCD_TRY(copy_back(co->B, K.B, (size_t)T.ns * nc * 6)); PCD_TRY(copy_back(co->S_cam, K.Scam, nc * nc));
    PCD_TRY(copy_back(co->rhs_cam, K.rhs, nc));
  }
  PCD_TRY(copy_back(o->S, dense, n * n));
  PCD_HIP_TRY(hipDeviceSynchronize());
  return PCD_OK;
}

// pcd_ba_schur[_cam]_back_substitute_device.  d_delta: dpose [6 ns], then dcam [12 ncs]
static pcd_status back_substitute_device(pcd_ba* b, bool cam, const double* d_delta, double* d_dpoint,
                                         double* d_model_decrease, void* stream) {
  int ncs;
  PCD_TRY(schur_guard(b, cam, &ncs));
  const char* fn = ncs ? "pcd_ba_schur_cam_back_substitute_device" : "pcd_ba_schur_back_substitute_device";
  hipStream_t s = (hipStream_t)stream;
  PCD_TRY(refuse_capture(s, fn));
  PCD_TRY(schur_state_guard(b, fn, false, ncs));
  const BaSchur::Structure& T = b->schur->st; BaSchur::Numeric& N = b->schur->num; const BaSchur::Cam& K = b->schur->cam;
  // a zero-length array may be NULL (an empty torch tensor has data_ptr() 0): ns = 0 when every pose is constant
  PCD_REQUIRE((d_delta || (T.ns == 0 && !ncs)) && (d_dpoint || b->P == 0), "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  const int P = b->P; const unsigned nbp = std::max(1u, div_up((uint64_t)P, 256));
  const double* d_dcam = d_delta + slot_vec(T.ns);
  ScopedKernelTimer t("ba_schur_back", s);
  if (ncs) {
    const SchurCamBack kb{P, ncs, b->pt_obs_start.p, b->pt_obs_list.p, b->obs_image.p, T.obs_pos.p, T.img_slot.p,
                          N.Wim.p, N.Vinv.p, N.gpt.p, N.Dpt.p, K.Wc.p, K.active.p};
    schur_cam_back(kb, d_delta, d_dcam, d_dpoint, N.md_partial.p, s);
  } else {
    hipLaunchKernelGGL(k_schur_back, dim3(nbp), dim3(256), 0, s, P, b->pt_obs_start.p, b->pt_obs_list.p, b->obs_image.p,
                       T.obs_pos.p, T.img_slot.p, N.Wim.p, N.Vinv.p, N.gpt.p, N.Dpt.p, d_delta, d_dpoint, N.md_partial.p);
  }
  if (d_model_decrease) {
    hipLaunchKernelGGL(k_schur_model_decrease, dim3(1), dim3(256), 0, s, T.ns, T.slot_img.p, b->const_tvec(), N.gimg.p,
                       N.Dimg.p, d_delta, N.md_partial.p, (int)nbp, d_model_decrease);
    if (ncs) schur_cam_model_decrease(ncs, K.slot_cam.p, K.active.p, K.gcam.p, K.D.p, d_dcam, d_model_decrease, s);
  }
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

// pcd_ba_plus[_cam]_device.  d_cam_params_out (null from the plain call): the camera parameters with dcam added on the
// active ones; without camera slots a copy of the handle's, outside the ba_plus scope
static pcd_status plus_device(pcd_ba* b, bool cam, const double* d_delta, const double* d_dpoint, double* d_poses_out,
                              double* d_points_out, double* d_cam_params_out, void* stream) {
  int ncs;
  PCD_TRY(schur_guard(b, cam, &ncs));
  hipStream_t s = (hipStream_t)stream;
  PCD_TRY(refuse_capture(s, ncs ? "pcd_ba_plus_cam_device" : "pcd_ba_plus_device"));
  PCD_TRY(schur_build(b, s));
  if (ncs) PCD_TRY(cam_upload_slots(b));
  const BaSchur::Structure& T = b->schur->st; const BaSchur::Cam& K = b->schur->cam;
  // zero-length arrays may be NULL (ns = 0 when every pose is constant)
  PCD_REQUIRE((d_delta || (T.ns == 0 && !ncs)) && (d_dpoint || b->P == 0) && (d_poses_out || b->I == 0) &&
              (d_points_out || b->P == 0), "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  {
    ScopedKernelTimer t("ba_plus", s);
    hipLaunchKernelGGL(k_ba_plus, dim3(div_up((uint64_t)b->I + b->P, 256)), dim3(256), 0, s, b->I, b->P, T.img_slot.p,
                       b->const_tvec(), b->const_points(), b->poses.p, b->points.p, d_delta, d_dpoint, d_poses_out,
                       d_points_out);
    if (ncs && d_cam_params_out)
      ba_plus_cam(b->cam_params_len, K.param_cam.p, b->cam_off.p, K.cam_slot.p, K.active.p, b->cam_params.p,
                  d_delta + slot_vec(T.ns), d_cam_params_out, s);
    PCD_HIP_TRY(hipGetLastError());
  }
  if (!ncs && d_cam_params_out && d_cam_params_out != b->cam_params.p && b->cam_params_len)
    PCD_HIP_TRY(hipMemcpyAsync(d_cam_params_out, b->cam_params.p, b->cam_params_len * sizeof(double),
                               hipMemcpyDeviceToDevice, s));
  return PCD_OK;
}

// pcd_ba_schur[_cam]_solve_pcg_device.  d_delta [6 ns + 12 ncs]
static pcd_status solve_pcg_device(pcd_ba* b, bool cam, const pcd_ba_pcg_opts* opts, double* d_delta,
                                   pcd_ba_pcg_info* d_info, void* stream) {
  int ncs;
  PCD_TRY(schur_guard(b, cam, &ncs)); PCD_TRY(pcg_check_opts(opts));
  const char* fn = ncs ? "pcd_ba_schur_cam_solve_pcg_device" : "pcd_ba_schur_solve_pcg_device";
  hipStream_t s = (hipStream_t)stream;
  PCD_TRY(refuse_capture(s, fn));
  PCD_TRY(schur_state_guard(b, fn, true, ncs));
  PCD_REQUIRE(d_delta || (b->schur->st.ns == 0 && !ncs), "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  ScopedKernelTimer t("ba_schur_pcg", s);
  PCD_TRY(pcg_begin(b, opts, ncs, s));
  PCD_TRY(pcg_run(b, opts, ncs, 0, s));
  pcg_finish(pcg_vec(b, ncs), d_delta, d_info, s);
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

// pcd_ba_schur[_cam]_solve_pcg: the device form into the handle's staging, then copied back
static pcd_status solve_pcg_host(pcd_ba* b, bool cam, const pcd_ba_pcg_opts* opts, double* delta, pcd_ba_pcg_info* info) {
  int ncs;
  PCD_TRY(schur_guard(b, cam, &ncs)); PCD_TRY(pcg_check_opts(opts));
  PCD_TRY(schur_state_guard(b, ncs ? "pcd_ba_schur_cam_solve_pcg" : "pcd_ba_schur_solve_pcg", true, ncs));
  BaSchur::Pcg& C = b->schur->cg;
  const size_t n = slot_vec(b->schur->st.ns) + (size_t)kCamS * ncs;
  PCD_REQUIRE(delta || n == 0, "null pointer");
  PCD_TRY(C.out.reserve(at_least_1(n))); PCD_TRY(C.info.reserve(1));
  PCD_TRY(solve_pcg_device(b, cam, opts, C.out.p, C.info.p, nullptr));
  PCD_TRY(copy_back(delta, C.out, n)); PCD_TRY(copy_back(info, C.info, 1));
  PCD_HIP_TRY(hipDeviceSynchronize());
  return PCD_OK;
}

// pcd_ba_schur[_cam]_solve_cholesky_device.  The caller's dense system (d_S, d_rhs) is the plain call's alone
static pcd_status solve_cholesky_device(pcd_ba* b, bool cam, const double* d_S, const double* d_rhs, double* d_delta,
                                        pcd_ba_chol_info* d_info, void* stream) {
  int ncs;
  PCD_TRY(schur_guard(b, cam, &ncs));
  PCD_REQUIRE(!d_S == !d_rhs, "S and rhs: give both (caller's dense system) or neither (the handle's own blocks)");
  const char* fn = ncs ? "pcd_ba_schur_cam_solve_cholesky_device" : "pcd_ba_schur_solve_cholesky_device";
  hipStream_t s = (hipStream_t)stream;
  PCD_TRY(refuse_capture(s, fn));
  if (d_S) PCD_TRY(schur_build(b, s));
  else PCD_TRY(schur_state_guard(b, fn, true, ncs));
  const int ns = b->schur->st.ns;
  PCD_REQUIRE(d_delta || (ns == 0 && !ncs), "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  if (ns == 0 && !ncs) {   // nothing to solve, nothing launched
    if (d_info) {
      pcd_ba_chol_info o{}; o.status = PCD_CHOL_OK; o.failed_column = -1;
      PCD_HIP_TRY(hipMemcpyAsync(d_info, &o, sizeof o, hipMemcpyHostToDevice, s));
      PCD_HIP_TRY(hipStreamSynchronize(s));   // o leaves scope
    }
    return PCD_OK;
  }
  ScopedKernelTimer t("ba_schur_cholesky", s);
  PCD_TRY(chol_solve(b, ncs, d_S, d_rhs, d_delta, d_info, s));
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

extern "C" {

// ---- point elimination ------------------------------------------------------------------------------
pcd_status pcd_ba_schur_structure(pcd_ba* b, int32_t* image_slot, int32_t* num_slots, uint64_t* num_pairs,
                                  int32_t* pair_i, int32_t* pair_j) {
  return pcd::guard([&]() -> pcd_status {
    PCD_TRY(schur_guard(b)); PCD_TRY(schur_build(b, nullptr));
    const BaSchur::Structure& T = b->schur->st;
    PCD_HIP_TRY(hipDeviceSynchronize());   // the tail of a build is enqueued, not waited for
    PCD_TRY(copy_back(image_slot, T.img_slot, (size_t)b->I));
    if (num_slots) *num_slots = T.ns; if (num_pairs) *num_pairs = T.npairs;
    if ((pair_i || pair_j) && T.npairs) {   // on demand: the interleaved device list, split here
      std::vector<uint32_t> ij(2 * T.npairs);
      PCD_TRY(copy_back(ij.data(), T.pair_ij, ij.size()));
      for (uint64_t q = 0; q < T.npairs; ++q) {
        if (pair_i) pair_i[q] = (int32_t)ij[2 * q];
        if (pair_j) pair_j[q] = (int32_t)ij[2 * q + 1];
      }
    }
    return PCD_OK;
  });
}

pcd_status pcd_ba_schur_build_device(pcd_ba* b, void* stream, pcd_ba_schur_build_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    PCD_TRY(schur_guard(b));
    PCD_REFUSE_CAPTURE(stream);
    return schur_build(b, (hipStream_t)stream, info);
  });
}

pcd_status pcd_ba_schur_structure_lists(pcd_ba* b, const pcd_ba_schur_lists* o) {
  return pcd::guard([&]() -> pcd_status {
    PCD_TRY(schur_guard(b)); PCD_REQUIRE(o, "null pointer");
    PCD_TRY(schur_build(b, nullptr));
    const BaSchur::Structure& T = b->schur->st;
    const size_t ns = (size_t)T.ns, nrow = ns + 2 * T.npairs;
    PCD_HIP_TRY(hipDeviceSynchronize());   // a build on another stream may still be running
    PCD_TRY(copy_back(o->slot_image, T.slot_img, ns)); PCD_TRY(copy_back(o->obs_pos, T.obs_pos, b->O));
    PCD_TRY(copy_back(o->blk_start, T.blk_start, (size_t)T.nblk() + 1));
    PCD_TRY(copy_back(o->ent_a, T.ent_a, T.nent)); PCD_TRY(copy_back(o->ent_b, T.ent_b, T.nent));
    PCD_TRY(copy_back(o->pair_ij, T.pair_ij, 2 * T.npairs)); PCD_TRY(copy_back(o->row_start, T.row_start, ns + 1));
    PCD_TRY(copy_back(o->row_blk, T.row_blk, nrow)); PCD_TRY(copy_back(o->row_col, T.row_col, nrow));
    return PCD_OK;
  });
}

pcd_status pcd_ba_schur_stats(pcd_ba* b, pcd_ba_schur_info* info) {
  PCD_TRY(schur_guard(b)); PCD_REQUIRE(info, "null pointer");
  std::memset(info, 0, sizeof *info);
  if (!b->schur) return PCD_OK;
  info->scratch_bytes = b->schur->device_bytes();   // what the handle holds, built or not (an edit keeps the buffers)
  if (!b->schur->st.built) return PCD_OK;
  info->build_ms = b->schur->st.build_ms; info->num_entries = b->schur->st.nent;
  return PCD_OK;
}

pcd_status pcd_ba_schur_device(pcd_ba* b, const pcd_ba_schur_opts* opt, const pcd_ba_schur_out* o, void* stream) {
  return pcd::guard([&]() -> pcd_status {
    PCD_TRY(schur_guard(b));
    return schur_device(b, 0, opt, o, nullptr, stream);
  });
}

pcd_status pcd_ba_schur(pcd_ba* b, const pcd_ba_schur_opts* opt, const pcd_ba_schur_out* o) {
  return pcd::guard([&]() -> pcd_status {
    PCD_TRY(schur_guard(b)); PCD_REQUIRE(opt && o, "null pointer");
    return schur_host(b, 0, opt, o, nullptr);
  });
}

pcd_status pcd_ba_schur_back_substitute_device(pcd_ba* b, const double* d_dpose, double* d_dpoint,
                                               double* d_model_decrease, void* stream) {
  return back_substitute_device(b, false, d_dpose, d_dpoint, d_model_decrease, stream);
}

pcd_status pcd_ba_plus_device(pcd_ba* b, const double* d_dpose, const double* d_dpoint, double* d_poses_out,
                              double* d_points_out, void* stream) {
  return pcd::guard([&]() -> pcd_status {
    return plus_device(b, false, d_dpose, d_dpoint, d_poses_out, d_points_out, nullptr, stream);
  });
}

void pcd_ba_pcg_opts_default(pcd_ba_pcg_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->max_iterations = 100; o->min_iterations = 0; o->preconditioner = PCD_PRECOND_SCHUR_JACOBI;
  o->q_tolerance = 0.1; o->r_tolerance = -1.0;
}

pcd_status pcd_ba_schur_solve_pcg_device(pcd_ba* b, const pcd_ba_pcg_opts* opts, double* d_dpose,
                                         pcd_ba_pcg_info* d_info, void* stream) {
  return pcd::guard([&]() -> pcd_status { return solve_pcg_device(b, false, opts, d_dpose, d_info, stream); });
}

pcd_status pcd_ba_schur_solve_pcg(pcd_ba* b, const pcd_ba_pcg_opts* opts, double* dpose, pcd_ba_pcg_info* info) {
  return pcd::guard([&]() -> pcd_status { return solve_pcg_host(b, false, opts, dpose, info); });
}

pcd_status pcd_ba_schur_solve_cholesky_device(pcd_ba* b, const double* d_S, const double* d_rhs, double* d_dpose,
                                              pcd_ba_chol_info* d_info, void* stream) {
  return pcd::guard([&]() -> pcd_status { return solve_cholesky_device(b, false, d_S, d_rhs, d_dpose, d_info, stream); });
}

pcd_status pcd_ba_schur_solve_cholesky(pcd_ba* b, const double* Sh, const double* rhs, double* dpose,
                                       pcd_ba_chol_info* info) {
  return pcd::guard([&]() -> pcd_status {
    PCD_TRY(schur_guard(b));
    PCD_REQUIRE(!Sh == !rhs, "S and rhs: give both (caller's dense system) or neither (the handle's own blocks)");
    if (Sh) PCD_TRY(schur_build(b, nullptr));
    else PCD_TRY(schur_state_guard(b, "pcd_ba_schur_solve_cholesky", true, 0));
    BaSchur::Chol& K = b->schur->chol;
    const size_t n = slot_vec(b->schur->st.ns);
    PCD_REQUIRE(dpose || n == 0, "null pointer");
    PCD_TRY(K.out.reserve(at_least_1(n))); PCD_TRY(K.info_out.reserve(1));
    const double* d_S = nullptr; const double* d_rhs = nullptr;
    if (Sh && n) {
      PCD_TRY(K.S.reserve(n * n)); PCD_TRY(K.rhs.reserve(n));
      PCD_HIP_TRY(hipMemcpy(K.S.p, Sh, n * n * sizeof(double), hipMemcpyHostToDevice));
      PCD_HIP_TRY(hipMemcpy(K.rhs.p, rhs, n * sizeof(double), hipMemcpyHostToDevice));
      d_S = K.S.p; d_rhs = K.rhs.p;
    } else if (Sh) {   // an empty system given in caller memory: the device form only looks at the pointers
      d_S = K.out.p; d_rhs = K.out.p;
    }
    PCD_TRY(pcd_ba_schur_solve_cholesky_device(b, d_S, d_rhs, K.out.p, K.info_out.p, nullptr));
    PCD_TRY(copy_back(dpose, K.out, n)); PCD_TRY(copy_back(info, K.info_out, 1));
    PCD_HIP_TRY(hipDeviceSynchronize());
    K.S.release(); K.rhs.release();   // n^2 of staging: not kept beside the padded scratch
    return PCD_OK;
  });
}

// ---- refined intrinsics: camera rows in the reduced system -------------------------------------------
// On a handle without camera slots every call is its plain counterpart.
pcd_status pcd_ba_camera_slots(pcd_ba* b, int32_t* camera_slot, int32_t* num_slots, uint8_t* active) {
  PCD_TRY(require_device(b ? b->device : 0));
  PCD_REQUIRE(b, "null handle");
  if (camera_slot) std::copy(b->h_cam_slot.begin(), b->h_cam_slot.end(), camera_slot);
  if (num_slots) *num_slots = cam_slots(b);
  if (active) std::copy(b->h_cam_active.begin(), b->h_cam_active.end(), active);
  return PCD_OK;
}

pcd_status pcd_ba_schur_cam_device(pcd_ba* b, const pcd_ba_schur_opts* opt, const pcd_ba_schur_cam_out* o, void* stream) {
  return pcd::guard([&]() -> pcd_status {
    int ncs;
    PCD_TRY(schur_guard(b, true, &ncs)); PCD_REQUIRE(opt && o, "null pointer");
    const pcd_ba_schur_out po = pose_out(*o);
    return schur_device(b, ncs, opt, &po, o, stream);
  });
}

pcd_status pcd_ba_schur_cam(pcd_ba* b, const pcd_ba_schur_opts* opt, const pcd_ba_schur_cam_out* o) {
  return pcd::guard([&]() -> pcd_status {
    int ncs;
    PCD_TRY(schur_guard(b, true, &ncs)); PCD_REQUIRE(opt && o, "null pointer");
    const pcd_ba_schur_out po = pose_out(*o);
    return schur_host(b, ncs, opt, &po, o);
  });
}

pcd_status pcd_ba_schur_cam_solve_cholesky_device(pcd_ba* b, double* d_delta, pcd_ba_chol_info* d_info, void* stream) {
  return pcd::guard([&]() -> pcd_status { return solve_cholesky_device(b, true, nullptr, nullptr, d_delta, d_info, stream); });
}

pcd_status pcd_ba_schur_cam_solve_pcg_device(pcd_ba* b, const pcd_ba_pcg_opts* opts, double* d_delta,
                                             pcd_ba_pcg_info* d_info, void* stream) {
  return pcd::guard([&]() -> pcd_status { return solve_pcg_device(b, true, opts, d_delta, d_info, stream); });
}

pcd_status pcd_ba_schur_cam_solve_pcg(pcd_ba* b, const pcd_ba_pcg_opts* opts, double* delta, pcd_ba_pcg_info* info) {
  return pcd::guard([&]() -> pcd_status { return solve_pcg_host(b, true, opts, delta, info); });
}

pcd_status pcd_ba_schur_cam_back_substitute_device(pcd_ba* b, const double* d_delta, double* d_dpoint,
                                                   double* d_model_decrease, void* stream) {
  return back_substitute_device(b, true, d_delta, d_dpoint, d_model_decrease, stream);
}

pcd_status pcd_ba_plus_cam_device(pcd_ba* b, const double* d_delta, const double* d_dpoint, double* d_poses_out,
                                  double* d_points_out, double* d_cam_params_out, void* stream) {
  return pcd::guard([&]() -> pcd_status {
    return plus_device(b, true, d_delta, d_dpoint, d_poses_out, d_points_out, d_cam_params_out, stream);
  });
}

pcd_status pcd_ba_get_camera_parameters(pcd_ba* b, double* cam_params) {
  PCD_TRY(require_device(b ? b->device : 0));
  PCD_REQUIRE(b && cam_params, "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  if (b->cam_params_len)
    PCD_HIP_TRY(hipMemcpy(cam_params, b->cam_params.p, b->cam_params_len * sizeof(double), hipMemcpyDeviceToHost));
  return PCD_OK;
}

void pcd_ba_solve_opts_default(pcd_ba_solve_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->max_num_iterations = 10; o->damping = PCD_DAMP_MARQUARDT;
  o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32; o->min_relative_decrease = 1e-3;
  o->function_tolerance = 0.0; o->gradient_tolerance = 0.0;
  pcd_ba_pcg_opts_default(&o->linear);
}

pcd_status pcd_ba_solve(pcd_ba* b, const pcd_ba_solve_opts* opts, pcd_ba_solve_summary* summary,
                        pcd_ba_solve_iteration* iterations) {
  return pcd::guard([&]() -> pcd_status {
    // refine_intrinsics: the camera rows ride along (pcd_ba_schur_cam*); without camera slots the flag changes nothing
    int ncs;
    PCD_TRY(schur_guard(b, opts && opts->refine_intrinsics, &ncs)); PCD_TRY(lm_check_opts(opts));
    const bool cam = ncs > 0;
    if (cam && opts->linear_solver == PCD_LINEAR_PCG) {
      set_error("pcd_ba_solve: refine_intrinsics needs linear_solver = PCD_LINEAR_CHOLESKY or PCD_LINEAR_PCG_CAM "
                "(PCD_LINEAR_PCG is the PCG on the pose rows alone)");
      return PCD_ERR_UNSUPPORTED;
    }
    pcd_ba_solve_opts lo = *opts;   // without camera rows PCD_LINEAR_PCG_CAM is PCD_LINEAR_PCG
    if (!cam && lo.linear_solver == PCD_LINEAR_PCG_CAM) lo.linear_solver = PCD_LINEAR_PCG;
    opts = &lo;
    hipStream_t s = nullptr;
    PCD_REFUSE_CAPTURE(s);
    PCD_TRY(schur_build(b, s));
    if (cam) PCD_TRY(cam_upload_slots(b));
    BaSchur& S = *b->schur; BaSchur::Lm& M = S.lm;
    const auto t0 = std::chrono::steady_clock::now();
    const unsigned ngp = std::max(1u, std::min(1024u, div_up((uint64_t)S.st.ns + b->P, 256)));
    const unsigned ngr = ngp + (cam ? 1u : 0u);   // partials of the gradient norm: one more for g_cam
    PCD_TRY(lm_reserve(b, ngr, ncs));
    PCD_HIP_TRY(hipSetDevice(b->device));
    EventPair ev; PCD_TRY(ev.create());   // around the linear solve of an iteration
    // the accepted parameters: a rejected step copies them back into the handle
    PCD_TRY(copy_parameters(b, M.poses.p, M.points.p, b->poses.p, b->points.p, s));
    if (cam) PCD_TRY(copy_camera_parameters(b, true, s));
    pcd_ba_solve_summary sm{}; sm.termination = PCD_SOLVE_MAX_ITERATIONS;
    double radius = opts->initial_radius, factor = 2.0;
    for (int it = 0; it < opts->max_num_iterations; ++it) {
      if (radius < opts->min_radius) { sm.termination = PCD_SOLVE_MIN_RADIUS; break; }
      pcd_ba_schur_opts so{}; so.mu = 1.0 / radius; so.damping = opts->damping;
      const pcd_ba_schur_out none{}; const pcd_ba_schur_cam_out none_cam{};   // everything stays in the handle
      PCD_TRY(schur_device(b, ncs, &so, &none, &none_cam, s));
      hipLaunchKernelGGL(k_ba_grad_max, dim3(ngp), dim3(256), 0, s, S.st.ns, S.st.slot_img.p, b->const_tvec(), S.num.gimg.p,
                         b->P, b->const_points(), S.num.gpt.p, M.gpart.p);
      if (cam) ba_cam_grad_max(ncs, S.cam.slot_cam.p, S.cam.active.p, S.cam.gcam.p, M.gpart.p + ngp, s);
      int enq = 0;
      PCD_HIP_TRY(ev.start(s));
      PCD_TRY(lm_enqueue_linear(b, opts, ncs, &enq, s));
      PCD_HIP_TRY(ev.stop(s));
      PCD_TRY(lm_try_step(b, opts, ncs, enq, ngr, ev, &sm.linear_solver_ms, s));
      const LmRecord& rec = *M.host.p;
      if (it == 0) sm.initial_cost = sm.final_cost = rec.cost;
      const LmDecision d = lm_decide(rec, *opts, radius, factor, opts->linear_solver == PCD_LINEAR_CHOLESKY);
      if (d.it.accepted) PCD_TRY(copy_parameters(b, M.poses.p, M.points.p, b->poses.p, b->points.p, s));
      else PCD_TRY(copy_parameters(b, b->poses.p, b->points.p, M.poses.p, M.points.p, s));
      if (cam) PCD_TRY(copy_camera_parameters(b, d.it.accepted, s));
      if (d.termination == PCD_SOLVE_GRADIENT_TOLERANCE) { sm.termination = d.termination; break; }   // no iteration recorded
      radius = d.radius; factor = d.factor;
      if (iterations) iterations[it] = d.it;
      sm.num_iterations = it + 1;
      if (d.it.accepted) { sm.num_accepted++; sm.final_cost = d.it.candidate_cost; }
      if (d.termination >= 0) { sm.termination = d.termination; break; }
    }
    PCD_HIP_TRY(hipStreamSynchronize(s));
    if (cam && b->cam_params_len)   // the host mirror follows the accepted camera parameters (pcd_ba_project_lidar_device)
      PCD_HIP_TRY(hipMemcpy(b->h_cam_params.data(), b->cam_params.p, b->cam_params_len * sizeof(double),
                            hipMemcpyDeviceToHost));
    S.num.valid = S.cam.valid = false;   // the Schur state belongs to parameters the loop has moved on from
    sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (summary) *summary = sm;
    return PCD_OK;
  });
}

}  // extern "C"

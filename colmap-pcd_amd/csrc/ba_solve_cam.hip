// ba_solve_cam.hip -- camera rows of the reduced system of bundle adjustment (refined intrinsics):
//   Wc_p[r] = sum over the observations o of point p with cam(o) = r, ascending o, of W_cam[o]     (12 x 3)
//   Z_p[r]  = Wc_p[r] V_p^-1                                        (0 for constant and skipped points: V^-1 = 0 there)
//   S_cam[r][r'] = delta_rr' (H_cam[r] + D_r) - sum_p Z_p[r] Wc_p[r']^T
//   B[i][r]      = [cam(image of slot i) = r] E_cam[image] - sum over the observations e of the image of Z_pt(e)[r] W_e^T
//   rhs_cam[r]   = -g_cam[r] + sum_p Z_p[r] g_p
// in the idiom of k_schur_blocks (ba_solve.hip): no atomics, lane-strided entries with an xor butterfly or fixed trees,
// every sum in an order fixed by the structure, so results are bitwise repeatable run to run.  Inactive camera
// coordinates (constant parameters, entries at and above the model's K) are identity rows / columns with right-hand side
// 0, as constant-tvec coordinates are in the pose part.  The launchers are ba_solve_cam.h's; the state they work on and
// the entry points live in ba_solve.hip.
#include "ba_solve_cam.h"

namespace pcd {

// thread = (point, camera slot): the track's W_cam summed in the caller's observation order, then Z = Wc V^-1.
// SH: one slot and every image on its camera -- no camera test at all.
template <bool SH>
__global__ __launch_bounds__(256) void k_schur_cam_points(SchurCamIn in, double* __restrict__ Wc, double* __restrict__ Z) {
  const uint64_t t = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (t >= (uint64_t)in.P * in.ncs) return;
  const int p = (int)(t / in.ncs), r = (int)(t - (uint64_t)p * in.ncs);
  double w[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) w[k] = 0.0;
  for (uint32_t k = in.pt_obs_start[p]; k < in.pt_obs_start[p + 1]; ++k) {
    const uint32_t o = in.pt_obs_list[k];
    if (!SH && in.cam_slot[in.image_cam[in.obs_image[o]]] != r) continue;
    const double* s = in.Wcam + 36 * (size_t)o;
#pragma unroll
    for (int j = 0; j < 36; ++j) w[j] += s[j];
  }
  const double* v = in.Vinv + 9 * (size_t)p;
  double vi[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) vi[k] = v[k];
  double* wo = Wc + 36 * (size_t)t;
  double* zo = Z + 36 * (size_t)t;
#pragma unroll
  for (int a = 0; a < 12; ++a) {
    const double w0 = w[3 * a], w1 = w[3 * a + 1], w2 = w[3 * a + 2];
    wo[3 * a] = w0; wo[3 * a + 1] = w1; wo[3 * a + 2] = w2;
#pragma unroll
    for (int c = 0; c < 3; ++c) zo[3 * a + c] = w0 * vi[c] + w1 * vi[3 + c] + w2 * vi[6 + c];
  }
}

// slot pair q (r' <= r, row-major over the lower triangle) -> (r, r')
__device__ __forceinline__ void cam_pair(int q, int& r, int& rp) {
  r = 0;
  while (q > r) { q -= r + 1; ++r; }
  rp = q;
}

// one wavefront per (chunk of kCamChunk points, slot pair, quarter h of the 12 rows): rows 3h..3h+2 of Z_p[r] Wc_p[r']^T
// (36 accumulators, as k_schur_blocks) and, on a diagonal pair, of Z_p[r] g_p; lane-strided points, xor butterfly.
// partial [pair][entry][chunk]: the reduction below reads a chunk run contiguously.
__global__ __launch_bounds__(256) void k_schur_cam_partials(int P, int ncs, unsigned nchunk, unsigned nitems,
                                                            const double* __restrict__ Wc, const double* __restrict__ Z,
                                                            const double* __restrict__ gpt, double* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const uint32_t item = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= nitems) return;
  const int h = (int)(item & 3u);
  const uint32_t rest = item >> 2, npair = (uint32_t)(ncs * (ncs + 1) / 2);
  const uint32_t q = rest % npair, c = rest / npair;
  int r, rp;
  cam_pair((int)q, r, rp);
  const bool diag = r == rp;
  double acc[36], zg[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (int j = 0; j < kCamChunk / 64; ++j) {
    const int p = (int)c * kCamChunk + 64 * j + lane;
    if (p >= P) break;
    const double* z = Z + 36 * ((size_t)p * ncs + r) + 9 * h;
    const double* w = Wc + 36 * ((size_t)p * ncs + rp);
    double zv[9], wv[36];
#pragma unroll
    for (int k = 0; k < 9; ++k) zv[k] = z[k];
#pragma unroll
    for (int k = 0; k < 36; ++k) wv[k] = w[k];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 12; ++b)
        acc[12 * a + b] += zv[3 * a] * wv[3 * b] + zv[3 * a + 1] * wv[3 * b + 1] + zv[3 * a + 2] * wv[3 * b + 2];
    if (diag) {
      const double* g = gpt + 3 * (size_t)p;
      const double g0 = g[0], g1 = g[1], g2 = g[2];
#pragma unroll
      for (int a = 0; a < 3; ++a) zg[a] += zv[3 * a] * g0 + zv[3 * a + 1] * g1 + zv[3 * a + 2] * g2;
    }
  }
  double mine = 0.0;   // lane k < 36 keeps entry k of the quarter, lanes 36..38 the right-hand side rows
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    mine = lane == k ? v : mine;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = zg[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    mine = lane == 36 + k ? v : mine;
  }
  if (lane < 39) {
    const int e = lane < 36 ? 36 * h + lane : kCamS * kCamS + 3 * h + (lane - 36);
    partial[((size_t)q * kCamEnt + e) * nchunk + c] = mine;
  }
}

// one wavefront per (slot pair, entry): the chunk partials lane-strided, xor butterfly, then lane 0 finishes the entry:
// S_cam[r][r'] and its transpose (a diagonal block from its lower triangle, so S_cam is exactly symmetric), H_cam + D on
// the diagonal, rhs_cam, D; inactive coordinates become identity rows / columns with right-hand side 0.
__global__ __launch_bounds__(256) void k_schur_cam_reduce(SchurCamIn in, unsigned nchunk, unsigned nitems,
                                                          const double* __restrict__ partial, double* __restrict__ Scam,
                                                          double* __restrict__ rhs_cam, double* __restrict__ Dcam) {
  const int lane = threadIdx.x & 63;
  const uint32_t item = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= nitems) return;
  const uint32_t q = item / kCamEnt;
  const int e = (int)(item - q * kCamEnt), ncs = in.ncs;
  int r, rp;
  cam_pair((int)q, r, rp);
  const double* src = partial + (size_t)item * nchunk;
  double sum = 0.0;
  for (uint32_t c = lane; c < nchunk; c += 64) sum += src[c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane != 0) return;
  const uint8_t* act_r = in.active + kCamS * r;
  const uint8_t* act_p = in.active + kCamS * rp;
  if (e < kCamS * kCamS) {
    const int a = e / kCamS, b = e - kCamS * (e / kCamS);
    const bool dead = !act_r[a] || !act_p[b];
    double v;
    if (r != rp) {
      v = dead ? 0.0 : 0.0 - sum;
    } else {
      if (a < b) return;   // the mirror of (b, a)
      const double* H = in.Hcam + (size_t)kCamS * kCamS * in.slot_cam[r];
      v = H[kCamS * a + b] - sum;
      if (a == b) {
        const double d = damp_of(in.mode, in.mu, H[(kCamS + 1) * a]);
        v += d;
        Dcam[kCamS * r + a] = dead ? 0.0 : d;
      }
      if (dead) v = a == b ? 1.0 : 0.0;
    }
    Scam[(((size_t)r * ncs + rp) * kCamS + a) * kCamS + b] = v;
    Scam[(((size_t)rp * ncs + r) * kCamS + b) * kCamS + a] = v;
  } else if (r == rp) {
    const int a = e - kCamS * kCamS;
    rhs_cam[kCamS * r + a] = act_r[a] ? sum - in.gcam[(size_t)kCamS * in.slot_cam[r] + a] : 0.0;
  }
}

// one wavefront per (pose slot, camera slot, half h of the 12 rows): 36 accumulators, as k_schur_blocks -- a whole
// 12 x 6 block with its operands would not fit the register file.  Image-major over the image's observations: rows
// 6h..6h+5 of Z_pt(e)[r] W_e^T, lane-strided, xor butterfly; then E_cam of the image's own camera, constant-tvec
// columns and inactive rows zero.
__global__ __launch_bounds__(256) void k_schur_cam_border(SchurCamIn in, unsigned nitems, const double* __restrict__ Z,
                                                          double* __restrict__ B) {
  const int lane = threadIdx.x & 63;
  const uint32_t item = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= nitems) return;
  const int h = (int)(item & 1u), ncs = in.ncs;
  const uint32_t rest = item >> 1;
  const int r = (int)(rest % (uint32_t)ncs), i = (int)(rest / (uint32_t)ncs);
  const int im = in.slot_img[i];
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (uint32_t e = in.img_obs_start[im] + lane; e < in.img_obs_start[im + 1]; e += 64) {
    const double* z = Z + 36 * ((size_t)in.img_pt[e] * ncs + r) + 18 * h;
    const double* w = in.Wim + 18 * (size_t)e;
    double zv[18], wv[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) { zv[k] = z[k]; wv[k] = w[k]; }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = 0; c < 6; ++c)
        acc[6 * a + c] += zv[3 * a] * wv[3 * c] + zv[3 * a + 1] * wv[3 * c + 1] + zv[3 * a + 2] * wv[3 * c + 2];
  }
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    mine = lane == k ? v : mine;
  }
  if (lane < 36) {
    const int a = 6 * h + lane / 6, c = lane - 6 * (lane / 6);
    const unsigned tm = in.image_const_tvec ? in.image_const_tvec[im] : 0u;
    const bool own = in.cam_slot[in.image_cam[im]] == r;
    const double ecam = own ? in.Ecam[((size_t)im * kCamS + a) * 6 + c] : 0.0;
    const bool dead = (c >= 3 && ((tm >> (c - 3)) & 1u)) || !in.active[kCamS * r + a];
    B[(((size_t)i * ncs + r) * kCamS + a) * 6 + c] = dead ? 0.0 : ecam - mine;
  }
}

// thread = entry of B, then of the 12 ncs x 12 ncs camera part (lower triangle kept); the first entry of a camera row
// also carries its right-hand side
__global__ __launch_bounds__(256) void k_chol_fill_cam(int ns, int ncs, const double* __restrict__ B,
                                                       const double* __restrict__ Scam, const double* __restrict__ rhs_cam,
                                                       int np, double* __restrict__ A) {
  const uint64_t t = blockIdx.x * (uint64_t)256 + threadIdx.x;
  const uint64_t nB = (uint64_t)ns * ncs * (kCamS * 6), nc = (uint64_t)kCamS * ncs;
  const size_t ld = (size_t)np, n0 = 6 * (size_t)ns;
  if (t < nB) {
    const int c = (int)(t % 6), a = (int)((t / 6) % kCamS);
    const uint64_t ir = t / (6 * kCamS);
    const size_t r = ir % ncs, i = ir / ncs;
    A[(n0 + kCamS * r + a) * ld + 6 * i + c] = B[t];
  } else if (t < nB + nc * nc) {
    const uint64_t u = t - nB;
    const size_t row = u / nc, col = u - row * nc;
    if (col == 0) A[ld * ld + n0 + row] = rhs_cam[row];
    if (col <= row)
      A[(n0 + row) * ld + n0 + col] =
          Scam[(((row / kCamS) * ncs + col / kCamS) * kCamS + row % kCamS) * kCamS + col % kCamS];
  }
}

// thread = entry of B (written on both sides of the diagonal), then of the camera part; the pose blocks are
// k_schur_dense's (ba_solve.hip)
__global__ __launch_bounds__(256) void k_schur_cam_dense(int ns, int ncs, const double* __restrict__ B,
                                                         const double* __restrict__ Scam, double* __restrict__ S) {
  const uint64_t t = blockIdx.x * (uint64_t)256 + threadIdx.x;
  const uint64_t nB = (uint64_t)ns * ncs * (kCamS * 6), nc = (uint64_t)kCamS * ncs;
  const size_t n0 = 6 * (size_t)ns, n = n0 + nc;
  if (t < nB) {   // B [ns][ncs][12][6] = [ns][12 ncs][6]: entry (camera coordinate e, column c) of slot i
    const uint64_t q = t / 6;
    const size_t c = t - 6 * q, i = q / nc, e = q - i * nc;
    const double v = B[t];
    S[(n0 + e) * n + 6 * i + c] = v;
    S[(6 * i + c) * n + n0 + e] = v;
  } else if (t < nB + nc * nc) {
    const uint64_t u = t - nB;
    const size_t row = u / nc, col = u - row * nc;
    S[(n0 + row) * n + n0 + col] = Scam[(((row / kCamS) * ncs + col / kCamS) * kCamS + row % kCamS) * kCamS + col % kCamS];
  }
}

// thread = point: k_schur_back (schur_back_point) with the camera term sum_r Wc_p[r]^T dcam[r] behind the pose terms;
// inactive camera coordinates count as 0 whatever the caller passed
__global__ __launch_bounds__(256) void k_schur_cam_back(SchurCamBack kb, const double* __restrict__ dpose,
                                                        const double* __restrict__ dcam, double* __restrict__ dpoint,
                                                        double* __restrict__ md_partial) {
  schur_back_point(kb.P, kb.pt_obs_start, kb.pt_obs_list, kb.obs_image, kb.obs_pos, kb.img_slot, kb.Wim, kb.Vinv, kb.gpt,
                   kb.Dpt, dpose, dpoint, md_partial, [&](int p, double& r0, double& r1, double& r2) {
    for (int r = 0; r < kb.ncs; ++r) {
      const double* w = kb.Wc + 36 * ((size_t)p * kb.ncs + r);
#pragma unroll
      for (int a = 0; a < kCamS; ++a) {
        const double c = kb.active[kCamS * r + a] ? dcam[kCamS * r + a] : 0.0;
        r0 += w[3 * a] * c; r1 += w[3 * a + 1] * c; r2 += w[3 * a + 2] * c;
      }
    }
  });
}

// one wavefront: the camera term of the model decrease onto what k_schur_model_decrease wrote
__global__ __launch_bounds__(64) void k_schur_cam_model_decrease(int ncs, const int* __restrict__ slot_cam,
                                                                 const uint8_t* __restrict__ active,
                                                                 const double* __restrict__ gcam, const double* __restrict__ Dcam,
                                                                 const double* __restrict__ dcam, double* __restrict__ md) {
  double a = 0.0;
  for (int t = threadIdx.x; t < kCamS * ncs; t += 64) {
    const int r = t / kCamS, k = t - kCamS * (t / kCamS);
    const double x = dcam[t];
    a += active[t] ? -x * gcam[(size_t)kCamS * slot_cam[r] + k] + Dcam[t] * x * x : 0.0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
  if (threadIdx.x == 0) md[0] += 0.5 * a;
}

// thread = camera parameter: + dcam on an active parameter of a slot, a copy elsewhere.  In-place safe.
__global__ __launch_bounds__(256) void k_ba_plus_cam(uint64_t len, const int* __restrict__ param_cam,
                                                     const int* __restrict__ cam_off, const int* __restrict__ cam_slot,
                                                     const uint8_t* __restrict__ active, const double* params,
                                                     const double* __restrict__ dcam, double* out) {
  const uint64_t k = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (k >= len) return;
  const int c = param_cam[k];   // -1: the parameter belongs to no camera
  const int s = c >= 0 ? cam_slot[c] : -1, j = c >= 0 ? (int)k - cam_off[c] : 0;
  const double x = params[k];
  const bool moves = s >= 0 && j < kCamS && active[kCamS * s + j];
  out[k] = moves ? x + dcam[kCamS * s + j] : x;
}

// one wavefront: max |g_cam| over the active camera coordinates (a maximum does not depend on the order)
__global__ __launch_bounds__(64) void k_ba_cam_grad_max(int ncs, const int* __restrict__ slot_cam,
                                                        const uint8_t* __restrict__ active, const double* __restrict__ gcam,
                                                        double* __restrict__ partial) {
  double m = 0.0;
  for (int t = threadIdx.x; t < kCamS * ncs; t += 64) {
    const int r = t / kCamS, k = t - kCamS * (t / kCamS);
    if (active[t]) m = fmax(m, fabs(gcam[(size_t)kCamS * slot_cam[r] + k]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  if (threadIdx.x == 0) partial[0] = m;
}

// ---- launchers ----------------------------------------------------------------------------------------------------
void schur_cam_eliminate(const SchurCamIn& in, const SchurCamOut& out, hipStream_t s) {
  const int ncs = in.ncs;
  const unsigned nchunk = cam_chunks(in.P), npair = (unsigned)cam_pairs(ncs);
  const unsigned grid = std::max(1u, div_up((uint64_t)in.P * ncs, 256));
  if (in.shared) hipLaunchKernelGGL((k_schur_cam_points<true>), dim3(grid), dim3(256), 0, s, in, out.Wc, out.Z);
  else hipLaunchKernelGGL((k_schur_cam_points<false>), dim3(grid), dim3(256), 0, s, in, out.Wc, out.Z);
  const unsigned n1 = nchunk * npair * 4u;
  hipLaunchKernelGGL(k_schur_cam_partials, dim3(div_up(n1, 4)), dim3(256), 0, s, in.P, ncs, nchunk, n1, out.Wc, out.Z,
                     in.gpt, out.partial);
  const unsigned n2 = npair * (unsigned)kCamEnt;
  hipLaunchKernelGGL(k_schur_cam_reduce, dim3(div_up(n2, 4)), dim3(256), 0, s, in, nchunk, n2, out.partial, out.Scam,
                     out.rhs_cam, out.Dcam);
}

void schur_cam_border(const SchurCamIn& in, const SchurCamOut& out, hipStream_t s) {
  const unsigned n = (unsigned)in.ns * (unsigned)in.ncs * 2u;
  if (n) hipLaunchKernelGGL(k_schur_cam_border, dim3(div_up(n, 4)), dim3(256), 0, s, in, n, out.Z, out.B);
}

void schur_cam_fill_chol(int ns, int ncs, const double* B, const double* Scam, const double* rhs_cam, int np, double* A,
                         hipStream_t s) {
  const uint64_t n = (uint64_t)ns * ncs * (kCamS * 6) + (uint64_t)(kCamS * ncs) * (kCamS * ncs);
  hipLaunchKernelGGL(k_chol_fill_cam, dim3(div_up(n, 256)), dim3(256), 0, s, ns, ncs, B, Scam, rhs_cam, np, A);
}

void schur_cam_dense(int ns, int ncs, const double* B, const double* Scam, double* S, hipStream_t s) {
  const uint64_t n = (uint64_t)ns * ncs * (kCamS * 6) + (uint64_t)(kCamS * ncs) * (kCamS * ncs);
  hipLaunchKernelGGL(k_schur_cam_dense, dim3(div_up(n, 256)), dim3(256), 0, s, ns, ncs, B, Scam, S);
}

void schur_cam_back(const SchurCamBack& k, const double* dpose, const double* dcam, double* dpoint, double* md_partial,
                    hipStream_t s) {
  hipLaunchKernelGGL(k_schur_cam_back, dim3(std::max(1u, div_up((uint64_t)k.P, 256))), dim3(256), 0, s, k, dpose, dcam,
                     dpoint, md_partial);
}

void schur_cam_model_decrease(int ncs, const int* slot_cam, const uint8_t* active, const double* gcam, const double* Dcam,
                              const double* dcam, double* md, hipStream_t s) {
  hipLaunchKernelGGL(k_schur_cam_model_decrease, dim3(1), dim3(64), 0, s, ncs, slot_cam, active, gcam, Dcam, dcam, md);
}

void ba_plus_cam(uint64_t len, const int* param_cam, const int* cam_off, const int* cam_slot, const uint8_t* active,
                 const double* params, const double* dcam, double* out, hipStream_t s) {
  if (!len) return;
  hipLaunchKernelGGL(k_ba_plus_cam, dim3(div_up(len, 256)), dim3(256), 0, s, len, param_cam, cam_off, cam_slot, active,
                     params, dcam, out);
}

void ba_cam_grad_max(int ncs, const int* slot_cam, const uint8_t* active, const double* gcam, double* partial,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_ba_cam_grad_max, dim3(1), dim3(64), 0, s, ncs, slot_cam, active, gcam, partial);
}

}  // namespace pcd

// ba_pcg.h -- the PCG on the reduced camera system, plain (pcd_ba_schur_solve_pcg*) and bordered with the camera rows of
// refined intrinsics (pcd_ba_schur_cam_solve_pcg*), DESIGN 4.3a: what ba_solve.hip, which owns the solver state, the
// batches and the entry points, asks of the kernels in ba_pcg.hip.  Internal.
#pragma once
#include <cstdint>

#include "common.h"

namespace pcd {

// State and rule of a solve, plain or bordered
struct PcgState {
  double rho, alpha, beta, pw, q, rn2, bnorm, xr;
  int k, done, term, xsel;
  unsigned fallbacks; int pad;
};
struct PcgRule { int max_iterations, min_iterations; double q_tolerance, r_tolerance; };

// sum over the workgroup (256 threads), every thread gets the result; fixed order: wavefront butterfly, then the 4 waves
__device__ __forceinline__ double block_sum256(double v, double* lds4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();   // lds4 may still be read from the previous call
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}
// strided sum of partial[i * stride] (i < n) over one workgroup
__device__ __forceinline__ double block_sum_strided(const double* __restrict__ partial, int n, int stride, double* lds4) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += partial[(size_t)i * stride];
  return block_sum256(a, lds4);
}

// A solve's view of the handle; every pointer is device memory.  ncs = 0: the plain system, the camera members unused.
// With camera slots every vector is [6 ns pose | 12 ncs camera] in one buffer, so that the kernels that only sum
// partials (k_pcg_begin, k_pcg_step) and copy x (k_pcg_finish) serve both solves.
struct PcgVec {
  int ns, ncs;
  PcgState* st;
  const uint32_t* row_start; const uint32_t* row_blk; const uint32_t* row_col;   // the slot rows of the structure
  const double* Sdiag; const double* Soff; const double* rhs;   // the handle's pose blocks and right-hand side
  const double* B; const double* Scam; const double* rhs_cam;   // its border, camera block and right-hand side
  double* Minv;                     // [ns][6][6]
  double* Minv_cam;                 // [ncs][12][12]
  double* x0; double* x1;           // [6 ns + 12 ncs], double-buffered: iteration it reads buffer it & 1
  double* p0; double* p1;
  double* z; double* r; double* w;  // [6 ns + 12 ncs]
  double* camw;                     // [12 ncs][ns]: B[i] p_i of every pose slot, entry-major
  double* pw;                       // [ns + 12 ncs]: p_i . w_i of the pose slots, then p_e w_e of the camera coordinates
  double* partial;                  // [nb + ncs][4], nb = max(1, div_up(ns, 256)): pose workgroups, then camera slots
};

// Every launcher enqueues plain launches on s and nothing else; which kernels, plain or bordered, is decided by v.ncs
// here and nowhere else.
// preconditioner, x = 0, r = rhs, both directions 0, the scalars of iteration 0
void pcg_init(const PcgVec& v, int precond, const PcgRule& rule, hipStream_t s);
// iteration `it`: product, vector update, scalars (three launches; four with camera rows).  Nothing to do on an empty
// system (ns = ncs = 0)
void pcg_iterate(const PcgVec& v, int it, const PcgRule& rule, hipStream_t s);
// the selected x into d_delta [6 ns + 12 ncs], the record into d_info (either may be null)
void pcg_finish(const PcgVec& v, double* d_delta, pcd_ba_pcg_info* d_info, hipStream_t s);

}  // namespace pcd

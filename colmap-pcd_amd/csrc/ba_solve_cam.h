// ba_solve_cam.h -- the camera rows of the reduced system (refined intrinsics): what ba_solve.hip, which
// owns the solver state and the entry points, asks of the kernels in ba_solve_cam.hip.  Internal.
//
// Reduced unknowns [6 ns pose tangents | 12 ncs camera coordinates].  Camera slots are the cameras with a refined
// parameter, ascending camera index; a slot has PCD_CAM_JAC_STRIDE coordinates of which the refined ones are active and
// the others identity rows / columns.  Every launcher below enqueues plain launches on s and nothing else.
#pragma once
#include <cstdint>

#include "common.h"

namespace pcd {

constexpr int kCamS = PCD_CAM_JAC_STRIDE;   // coordinates of a camera slot
constexpr int kCamChunk = 256;              // points per partial of the point sums (one wavefront, four points a lane)
constexpr int kCamEnt = kCamS * kCamS + kCamS;   // entries of a partial: a 12 x 12 block and 12 of the right-hand side

// Ceres' LevenbergMarquardtStrategy min/max_diagonal and the two damping forms of pcd_ba_damping
constexpr double kDiagMin = 1e-6, kDiagMax = 1e32;
__device__ __forceinline__ double damp_of(int mode, double mu, double h) {
  return mode == 0 ? mu * fmin(fmax(h, kDiagMin), kDiagMax) : mu;
}

inline size_t cam_pairs(int ncs) { return (size_t)ncs * (ncs + 1) / 2; }   // slot pairs r' <= r
inline unsigned cam_chunks(int P) { return std::max(1u, div_up((uint64_t)P, kCamChunk)); }

// The camera slots of a handle and the arrays the kernels read; every pointer is device memory
struct SchurCamIn {
  int P, I, ns, ncs;
  bool shared;                      // every observation belongs to slot 0: no camera test in the point kernel
  const int* cam_slot;              // [C] slot of a camera, -1: none
  const int* slot_cam;              // [ncs]
  const uint8_t* active;            // [ncs][12]
  const int* image_cam; const int* obs_image;
  const uint32_t* pt_obs_start; const uint32_t* pt_obs_list;   // track CSR, the caller's observation order
  const uint32_t* img_obs_start; const int* img_pt;            // image-major
  const int* slot_img; const uint8_t* image_const_tvec;        // may be null
  const double* Vinv; const double* gpt; const double* Wim;    // of the pose elimination
  const double* Hcam; const double* gcam; const double* Ecam; const double* Wcam;   // pcd_ba_evaluate_device's blocks
  double mu; int mode;
};
struct SchurCamOut {
  double* Wc; double* Z;            // [P][ncs][12][3]
  double* partial;                  // [cam_pairs][kCamEnt][cam_chunks]
  double* B;                        // [ns][ncs][12][6]
  double* Scam;                     // [ncs][ncs][12][12], both triangles
  double* rhs_cam;                  // [ncs][12]
  double* Dcam;                     // [ncs][12] damping of the active coordinates, 0 elsewhere
};

// Wc_p[r], Z_p[r] = Wc_p[r] V_p^-1; the partials of Z Wc^T and Z g_p; S_cam, rhs_cam, D
void schur_cam_eliminate(const SchurCamIn& in, const SchurCamOut& out, hipStream_t s);
// the border B from Z, W and E_cam (after schur_cam_eliminate)
void schur_cam_border(const SchurCamIn& in, const SchurCamOut& out, hipStream_t s);
// B rows, the lower triangle of S_cam and the tail of the right-hand side into the padded scratch of ba_chol.h
// (leading dimension np); the pose part is k_chol_fill_blocks'
void schur_cam_fill_chol(int ns, int ncs, const double* B, const double* Scam, const double* rhs_cam, int np, double* A,
                         hipStream_t s);
// dense S [n][n], n = 6 ns + 12 ncs, both triangles, from the pose blocks and the camera blocks; the caller zeroed it
void schur_cam_dense(int ns, int ncs, uint32_t nblk, const uint32_t* pair_ij, const double* Sdiag, const double* Soff,
                     const double* B, const double* Scam, double* S, hipStream_t s);
// k_schur_back with the Wc_p^T dcam term: dpoint [P][3] and the point partials of the model decrease [div_up(P, 256)]
struct SchurCamBack {
  int P, ncs;
  const uint32_t* pt_obs_start; const uint32_t* pt_obs_list; const int* obs_image; const uint32_t* obs_pos;
  const int* img_slot; const double* Wim; const double* Vinv; const double* gpt; const double* Dpt;
  const double* Wc; const uint8_t* active;
};
void schur_cam_back(const SchurCamBack& k, const double* dpose, const double* dcam, double* dpoint, double* md_partial,
                    hipStream_t s);
// md[0] += 1/2 sum over the active camera coordinates of -dcam g_cam + D dcam^2
void schur_cam_model_decrease(int ncs, const int* slot_cam, const uint8_t* active, const double* gcam, const double* Dcam,
                              const double* dcam, double* md, hipStream_t s);
// out[k] = params[k] + dcam on the active parameters of the slots, a bitwise copy elsewhere (in-place safe)
void ba_plus_cam(uint64_t len, const int* param_cam, const int* cam_off, const int* cam_slot, const uint8_t* active,
                 const double* params, const double* dcam, double* out, hipStream_t s);
// partial[0] = max |g_cam| over the active camera coordinates
void ba_cam_grad_max(int ncs, const int* slot_cam, const uint8_t* active, const double* gcam, double* partial,
                     hipStream_t s);

// ---- the bordered PCG (pcd_ba_schur_cam_solve_pcg*) ---------------------------------------------------
// State and rule of a PCG solve, plain or bordered (the kernels of the plain one are ba_solve.hip's)
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

// Vectors of the bordered solve: [6 ns pose | 12 ncs camera] in one buffer each, so that the plain kernels that only sum
// partials (k_pcg_begin, k_pcg_step) and copy x (k_pcg_finish) serve both solves.
struct PcgCamVec {
  int ns, ncs;
  const PcgState* st;
  const double* B; const double* Scam; const double* rhs_cam;   // the handle's border, camera block and right-hand side
  double* Minv_cam;                 // [ncs][12][12]
  double* z; double* r; double* w;  // [6 ns + 12 ncs]
  double* camw;                     // [12 ncs][ns]: B[i] p_i of every pose slot, entry-major
  double* pw;                       // [ns + 12 ncs]: p_i . w_i of the pose slots, then p_e w_e of the camera coordinates
  double* partial;                  // [nb + ncs][4], nb = max(1, div_up(ns, 256)): pose workgroups, then camera slots
};
// camera part of k_pcg_init: 12 x 12 block-Jacobi inverses, x = 0, r = rhs_cam, z = M^-1 r, directions 0, partial[nb + r]
void pcg_cam_init(const PcgCamVec& v, int precond, double* x0, double* p0, double* p1, hipStream_t s);
// one iteration's product: pose rows with the border (B crosses memory once), then the camera rows
void pcg_cam_product(const PcgCamVec& v, const uint32_t* row_start, const uint32_t* row_blk, const uint32_t* row_col,
                     const double* Sdiag, const double* Soff, const double* p_old, double* p_new, hipStream_t s);
// k_pcg_update over both parts: pose workgroups, then one workgroup per camera slot
void pcg_cam_update(const PcgCamVec& v, PcgState* st, const double* Minv, const double* rhs, const double* p,
                    const double* x_old, double* x_new, hipStream_t s);

}  // namespace pcd

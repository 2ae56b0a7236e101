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
// B (on both sides of the diagonal) and S_cam into the dense S [n][n], n = 6 ns + 12 ncs; the pose blocks are
// k_schur_dense's (ba_solve.hip) with the leading dimension n
void schur_cam_dense(int ns, int ncs, const double* B, const double* Scam, double* S, hipStream_t s);
// The back-substitution of k_schur_back (ba_solve.hip) and k_schur_cam_back, thread = point:
//   delta X_p = -V^-1 (g_p + sum_{a in p} W_a^T dpose[slot(a)] + cam_term),
// the observations in ascending caller order; then the workgroup's partial of the model decrease
// -delta^T g + delta^T D delta over the points (fixed-order block sum).  cam_term(p, r0, r1, r2) adds the camera rows'
// share to the three sums, behind the pose terms; the plain kernel's adds nothing.
template <class CamTerm>
__device__ __forceinline__ void schur_back_point(int P, const uint32_t* pt_start, const uint32_t* pt_list,
                                                 const int* obs_image, const uint32_t* obs_pos, const int* img_slot,
                                                 const double* Wim, const double* Vinv, const double* gpt,
                                                 const double* Dpt, const double* dpose, double* dpoint,
                                                 double* md_partial, CamTerm cam_term) {
  __shared__ double s_m[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double md = 0.0;
  if (p < P) {
    const double* g = gpt + 3 * (size_t)p;
    double r0 = g[0], r1 = g[1], r2 = g[2];
    for (uint32_t k = pt_start[p]; k < pt_start[p + 1]; ++k) {
      const uint32_t o = pt_list[k];
      const int s = img_slot[obs_image[o]];
      if (s < 0) continue;
      const double* w = Wim + 18 * (size_t)obs_pos[o];
      const double* dc = dpose + 6 * (size_t)s;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double c = dc[a];
        r0 += w[3 * a] * c; r1 += w[3 * a + 1] * c; r2 += w[3 * a + 2] * c;
      }
    }
    cam_term(p, r0, r1, r2);
    const double* v = Vinv + 9 * (size_t)p;
    const double dx0 = -(v[0] * r0 + v[1] * r1 + v[2] * r2);
    const double dx1 = -(v[3] * r0 + v[4] * r1 + v[5] * r2);
    const double dx2 = -(v[6] * r0 + v[7] * r1 + v[8] * r2);
    dpoint[3 * (size_t)p] = dx0; dpoint[3 * (size_t)p + 1] = dx1; dpoint[3 * (size_t)p + 2] = dx2;
    const double* d = Dpt + 3 * (size_t)p;
    md = -(dx0 * g[0] + dx1 * g[1] + dx2 * g[2]) + (d[0] * dx0 * dx0 + d[1] * dx1 * dx1 + d[2] * dx2 * dx2);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) md += __shfl_xor(md, off);
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = md;
  __syncthreads();
  if (threadIdx.x == 0) md_partial[blockIdx.x] = (s_m[0] + s_m[1]) + (s_m[2] + s_m[3]);
}

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

}  // namespace pcd

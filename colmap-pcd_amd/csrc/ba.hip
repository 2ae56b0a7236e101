// ba.hip -- bundle-adjustment residual / Jacobian / normal-equation evaluation.
//
// Replaces the work ceres::Solve performs per iteration on the problem assembled by optim/bundle_adjustment.cc:694-1131
// (AddImageToProblem, AddImageInSphereToProblem, AddPointToProblem, AddLidarToProblem, ParameterizeCameras/Points):
// every residual block's CostFunction::Evaluate (base/cost_functions.h:49-141, :150-241, :256-370), the loss correction
// (optim/bundle_adjustment.cc:53-68) and the manifold projection (base/cost_functions.h:610-627), then J^T J / J^T r
// block accumulation.  This unit holds the evaluation kernels and the entry points that launch them (parameter access,
// pcd_ba_evaluate*, observation errors, track filters); the handle and the layouts they read are made in ba_build.hip
// (pcd_ba_create), sized from ba_handle.h.  The device solver on these blocks (point elimination, PCG, LM loop) is
// ba_solve.hip; it reaches this unit through pcd_ba_evaluate_device and ba_normal_equations (ba_handle.h) only.
//
// Kernels (all fp64, memory/latency-bound: ~300 flop per ~60-200 B per observation):
//   k_ba_points  thread = 3D point (track).  Tracks are processed in order of track length and their observations are
//                stored in a sliced-ELL layout (64 tracks per slice, observation j of lane l at slice_base + 64 j + l):
//                the lanes of a wavefront run the same number of iterations and every load instruction reads 64
//                consecutive records.  Accumulates the point's 3x3 block, gradient and the cost.  No atomics: point
//                blocks are complete inside one thread, the cost goes through a fixed-order two-stage sum.
//   k_ba_cost    thread = observation / LiDAR term: the cost alone (an LM trial step), same two-stage sum.
//   k_ba_images  workgroup = segment of an image; its observations are stored image-major (contiguous), strided
//                over 256 lanes; each lane recomputes the 2x6 pose-tangent Jacobian, the 21 + 6 unique entries of
//                [J | r]^T [J | r] are summed on the fp64 matrix pipe; fixed-order reduction -> deterministic 6x6
//                block + gradient.  Writes W (6x3 per observation) on request.
//   k_ba_cameras, k_ba_cam_w  the camera blocks of the normal equations when intrinsics are refined.
//   k_ba_raw*, k_ba_cam_jac, k_ba_lidar_raw  thread = observation / LiDAR term: the raw ambient blocks exactly as
//                CostFunction::Evaluate returns them, whole or as 64-byte records (the Ceres EvaluationCallback adapter).
//   k_ba_obs_errors, k_ba_filter_tracks, k_ba_negative_depth  the post-BA filters.
//   k_ba_proj_centers, k_ba_filter_tri_angle  the triangulation-angle filter on what k_ba_filter_tracks left.
// Jacobians are recomputed in each kernel instead of being staged through HBM (160 B/obs of traffic would cost more than
// the ~300 flops).  MODEL >= 0 compiles one camera model in (all cameras of the problem share it -- the usual case);
// MODEL = -1 switches per observation.
#include <algorithm>
#include <cmath>

#include "ba_cam_jac.h"
#include "ba_handle.h"
#include "ba_math.h"
#include "common.h"

namespace pcd {

// The camera of an evaluation: model id and parameters.
// SHARED: the handle has one camera for every image (BaDev::shared_cam >= 0).  The camera index is then a kernel
// argument: cam_off, cam_model and the parameters are read ONCE per thread, when the object is made at the top of the
// kernel, through wave-uniform addresses (scalar loads) -- not per observation through the three-deep per-lane gather
// chain image -> camera -> offset -> parameters behind the load of `im`.  The parameters are still read from cam_params
// at every launch (pcd_ba_set_camera_parameters and the device LM update them in place), and the arithmetic is the same
// expressions on the same values: the results are bit-identical to the per-image path.
template <int MODEL, bool SHARED>
struct BaCam {
  static constexpr int K = cam_num_params(MODEL >= 0 ? MODEL : 0);
  int model = MODEL;
  const double* p = nullptr;
  double v[K];   // SHARED with a compiled-in model: the parameters themselves
  __device__ __forceinline__ void resolve(const BaDev& d, int cm) {
    if (MODEL < 0) model = d.cam_model[cm];
    p = d.cam_params + d.cam_off[cm];
  }
  __device__ __forceinline__ explicit BaCam(const BaDev& d) {
    if (!SHARED) return;
    resolve(d, d.shared_cam);
    if (MODEL >= 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = p[k];   // uniform: held in SGPRs (copied to VGPRs they measured slower)
    }
  }
  // what reproj_eval / world_to_image_d2 read the parameters from
  __device__ __forceinline__ const double* params() const { return (SHARED && MODEL >= 0) ? v : p; }
  // per-image path: the camera of image im
  __device__ __forceinline__ void of_image(const BaDev& d, int im) {
    if (!SHARED) resolve(d, d.image_cam[im]);
  }
};

__device__ __forceinline__ void load_pose(const BaDev& d, int im, double pose[7]) {
#pragma unroll
  for (int k = 0; k < 7; ++k) pose[k] = d.poses[7 * (size_t)im + k];
}
// pose = the 7 doubles of the image, cam = its camera
template <int MODEL, bool SHARED>
__device__ __forceinline__ void eval_block_at(const BaCam<MODEL, SHARED>& cam, const double pose[7], const double X[3],
                                              double ox, double oy, ReprojBlock& b, double q[4]) {
  double t[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = pose[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = pose[4 + k];
  reproj_eval(cam.model, cam.params(), q, t, X, ox, oy, b);
}
// the per-image path in one call (the image and camera passes, whose image is workgroup-uniform anyway)
template <int MODEL>
__device__ __forceinline__ void eval_block(const BaDev& d, int im, const double X[3], double ox, double oy,
                                           ReprojBlock& b, double q[4]) {
  const double* pose = d.poses + 7 * (size_t)im;
  double t[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = pose[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = pose[4 + k];
  const int cm = d.image_cam[im];
  const int model = MODEL >= 0 ? MODEL : d.cam_model[cm];
  reproj_eval(model, d.cam_params + d.cam_off[cm], q, t, X, ox, oy, b);
}
// a double every lane of the wavefront holds the same value of, as the compiler sees it
__device__ __forceinline__ double wave_uniform(double v) {
  const long long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The same value, in its SGPR pair and opaque to the optimiser from here on: inside a loop it keeps arithmetic on
// wave-uniform doubles (VALU-only, so its results would sit in VGPRs) from being hoisted out and held across the loop.
__device__ __forceinline__ double sgpr_pin(double v) {
  asm volatile("" : "+s"(v));
  return v;
}

// A copy of a per-lane value made at this point of the program (not where the register allocator would put it)
template <typename T>
__device__ __forceinline__ T vgpr_pin(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

// How a write-once output leaves the chip.  Every byte of a store reaches memory either way; the policies differ in what
// the line does to the caches on its way:
//   plain          the line stays in the XCD's L2: right for what the next kernel, or a pinned-buffer copy, reads back
//   nt             non-temporal: a streamed line, first to go; for outputs nothing in the evaluation reads again
//   write_through  the sc1 form: written through, the line is dropped from L2 behind the write
enum class StorePolicy { plain, nt, write_through };
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 16 bytes of one lane under a policy the compiler sees and counts (no inline assembly: the waits of the loads around
// such a store are hipcc's own).  write_through has no flat form; it goes through wave_rows_rsrc below.
template <StorePolicy SP>
__device__ __forceinline__ void store_f64x2(f64x2* p, f64x2 v) {
  static_assert(SP != StorePolicy::write_through, "write-through stores take a buffer descriptor");
  if (SP == StorePolicy::nt) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// Buffer descriptor of `bytes` bytes at a wave-uniform address (raw buffer, no swizzle; dword 3 = DATA_FORMAT 32 bit).
// The base is the wavefront's own, so the 32-bit lane offsets stay small however large the array; the hardware drops a
// store at or past `bytes`.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_rows_rsrc(double* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
}
constexpr int kAuxSc1 = 16;   // aux bits of the raw buffer store builtins: sc1 (write-through)

// Coalesced store of one row of N doubles per lane, rows of consecutive lanes adjacent in memory
// (out[(row0 + lane) * N + k] = v[k] for lane < cnt): the rows are transposed through a per-wavefront LDS
// scratch of 64 * N doubles and leave as 16-B-per-lane stores of consecutive addresses (1 KiB per instruction)
// instead of N stores that each touch 64 different cache lines.  Every lane of the wavefront must call it.
// (lane = threadIdx.x & 63, handed in by a caller that wants the addresses derived from its own copy of it)
// SP: the store policy above; with write_through row0 and cnt must be wave-uniform for the compiler too.
template <int N, StorePolicy SP = StorePolicy::plain>
__device__ __forceinline__ void wave_store_rows(double* __restrict__ out, uint64_t row0, int cnt, const double (&v)[N],
                                                double* __restrict__ lds, int lane) {
  static_assert(N % 2 == 0, "rows are moved in 16-byte units");
#pragma unroll
  for (int k = 0; k < N; ++k) lds[lane * N + k] = v[k];
  // one wavefront: LDS operations complete in order; the fences keep the compiler from moving the reads up
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const f64x2* src = reinterpret_cast<const f64x2*>(lds);
  f64x2* dst = reinterpret_cast<f64x2*>(out + row0 * N);
  const int units = cnt * (N / 2);
  if (SP == StorePolicy::write_through) {
    const __amdgpu_buffer_rsrc_t rsrc = wave_rows_rsrc(out + row0 * N, units * 16);
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
      const int u = j * 64 + lane;
      if (u < units) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, src[u]), rsrc, u * 16, 0, kAuxSc1);
    }
  } else {
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
      const int u = j * 64 + lane;
      if (u < units) store_f64x2<SP == StorePolicy::nt ? StorePolicy::nt : StorePolicy::plain>(dst + u, src[u]);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();   // the scratch may be rewritten after this
}
template <int N, StorePolicy SP = StorePolicy::plain>
__device__ __forceinline__ void wave_store_rows(double* __restrict__ out, uint64_t row0, int cnt, const double (&v)[N],
                                                double* __restrict__ lds) {
  wave_store_rows<N, SP>(out, row0, cnt, v, lds, (int)(threadIdx.x & 63));
}

// The scattered twin: this lane's row alone, out[row * N + k] = v[k], for rows that are not adjacent in memory.  plain
// leaves the stores as the compiler forms them; nt sends the row as 16-byte units (the rows are 16-byte aligned, as
// wave_store_rows takes them to be).  A lane's own row has no wave-uniform base, so there is no write-through form.
template <int N, StorePolicy SP>
__device__ __forceinline__ void lane_store_row(double* __restrict__ out, uint64_t row, const double (&v)[N]) {
  static_assert(N % 2 == 0 && SP != StorePolicy::write_through, "16-byte units; plain or nt");
  double* dst = out + row * N;
  if (SP == StorePolicy::plain) {
#pragma unroll
    for (int k = 0; k < N; ++k) dst[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) store_f64x2<SP>(reinterpret_cast<f64x2*>(dst) + k, f64x2{v[2 * k], v[2 * k + 1]});
  }
}

// ------------------------------------------------------------- points ------
// One LiDAR term of a track into its sums (the cost, and with BLOCKS the 3x3 block and the gradient)
template <bool BLOCKS>
__device__ __forceinline__ void points_add_lidar(const BaDev& d, const double X[3], const double abcd[4], double w, bool cpt,
                                                 double& cost, double H[6], double g[3]) {
  double r, J[3];
  lidar_eval(X, abcd, w, 0, r, J);
  double rho0, rho1;
  loss_eval(d.loss_type, d.loss_scale, r * r, rho0, rho1);
  cost += 0.5 * rho0;
  if (BLOCKS && !cpt) {
    const double sr = sqrt(rho1);
    const double rc = sr * r;
    J[0] *= sr; J[1] *= sr; J[2] *= sr;
    H[0] += J[0] * J[0]; H[1] += J[0] * J[1]; H[2] += J[0] * J[2];
    H[3] += J[1] * J[1]; H[4] += J[1] * J[2]; H[5] += J[2] * J[2];
    g[0] += J[0] * rc; g[1] += J[1] * rc; g[2] += J[2] * rc;
  }
}

// number of LiDAR terms of track t, plane and weight of the first (half 0 takes the LiDAR terms; wave-uniform branch)
__device__ __forceinline__ void load_lidar_first(const BaDev& d, int half, int t, uint32_t& ln, double lf[5]) {
  if (half != 0 || !d.L) return;   // a handle without LiDAR terms has no such arrays
  const size_t ntr = 64 * (size_t)d.nslices;
  ln = d.pt_lidar_cnt[t];
#pragma unroll
  for (int k = 0; k < 5; ++k) lf[k] = d.pt_lidar_first[k * ntr + t];
}

// BLOCKS = false: residual-only pass (cost), what Ceres asks for when it evaluates a trial step
// Two threads per track (the even and the odd observations of its sliced-ELL column): the kernel is bound by the
// latency of each track's serial chain of observations, not by arithmetic or bytes, so halving the chain and doubling
// the wavefronts in flight took it from 0.18 to ~0.1 ms on the bench scene.  The halves live in different wavefronts
// of the workgroup (threads 0-63 / 64-127 = halves 0 / 1 of slice 2b, 128-255 of slice 2b + 1); half 1 hands its sums
// over through LDS and half 0 adds them in a fixed order and also takes the track's LiDAR terms.
//
// Load order.  The kernel is bound by the round trips a wavefront waits for one after the other, so every load is
// issued as soon as its address is known, next to the others of the same round trip:
//   trip 1   pt_order[t], the first row's sell_img and sell_xy, the number of LiDAR terms of the track and the first
//            of them (half 0; BaDev::pt_lidar_cnt / pt_lidar_first are stored in track order: the address needs only t)
//   trip 2   points[p], point_const[p], the first row's pose, the second row's sell_img
//   trip k   the pose and sell_xy of row k - 1, the sell_img of row k: the image of every row is read one row ahead
// (before: index, wait, pose, wait for every row, and three more dependent trips for the LiDAR term after the barrier).
// Indices past the end of the slice are replaced by slot 0, so no branch stands around the loads; what they return is
// not used.  Same values into the same arithmetic in the same order: the results are bit-identical.
template <int MODEL, bool BLOCKS, bool SHARED>
__global__ __launch_bounds__(256) void k_ba_points(BaDev d, double* __restrict__ Hpt, double* __restrict__ gpt,
                                                   double* __restrict__ cost_partial) {
  __shared__ double s_half[2][64][9];
  // slice and half are those of the wavefront: uniform for the compiler too (scalar loads of the slice bounds, scalar branches)
  const int sl = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7));
  const int half = __builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 6) & 1));
  const int lane = threadIdx.x & 63;
  const int slice = blockIdx.x * 2 + sl;
  const int t = slice * 64 + lane;
  double cost = 0.0;
  double H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  int p = -1;
  unsigned cpt_b = 1;                       // point_const[p] as loaded (converted where it is used: no wait behind the load)
  double X[3] = {0, 0, 0};
  uint32_t ln = 0;                          // LiDAR terms of the track (half 0)
  double lf[5] = {0, 0, 0, 0, 0};           // the first of them: plane and weight
  // Per-image cameras keep up to twelve more VGPRs per lane in the loop (OPENCV: 138 with the term held across it), so
  // there the term is read behind the loop instead: still one coalesced trip, in flight across the barrier.
  constexpr bool kLidarEarly = SHARED;
  BaCam<MODEL, SHARED> cam(d);
  if (slice < d.nslices) {
    const uint32_t s0 = d.slice_start[slice], s1 = d.slice_start[slice + 1];
    uint32_t sb = s0 + 64u * half;          // this wavefront's part of the row: lane l has slot sb + l; a slice holds whole rows
    // (the row goes out ahead of pt_order[t]: the wait for p then covers im on every path, LiDAR terms or none, and the
    // first row's pose loads stand behind no other wait)
    const uint32_t sc = sb < s1 ? sb + lane : 0u;
    int im = d.sell_img[sc];
    double ox = d.sell_xy[2 * (size_t)sc], oy = d.sell_xy[2 * (size_t)sc + 1];
    p = d.pt_order[t];
    if (kLidarEarly) load_lidar_first(d, half, t, ln, lf);
    if (p >= 0) {
      X[0] = d.points[3 * (size_t)p]; X[1] = d.points[3 * (size_t)p + 1]; X[2] = d.points[3 * (size_t)p + 2];
      cpt_b = d.point_const ? d.point_const[p] : 0u;
    }
    while (sb < s1) {
      const uint32_t sn = sb + 128;
      const int im_next = d.sell_img[sn < s1 ? sn + lane : 0u];
      if (im >= 0) {   // not the padding of a shorter track
        ReprojBlock b;
        double q[4], pose[7];
        cam.of_image(d, im);
        load_pose(d, im, pose);
        eval_block_at(cam, pose, X, ox, oy, b, q);
        double rho0, rho1;
        loss_eval(d.loss_type, d.loss_scale, b.r[0] * b.r[0] + b.r[1] * b.r[1], rho0, rho1);
        cost += 0.5 * rho0;
        cpt_b = vgpr_pin(cpt_b);   // tested here, in every row: ahead of the loop the test would wait for the byte
        if (BLOCKS && cpt_b == 0) {
          const double sr = sqrt(rho1);
          double J[6];
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
              J[3 * r + k] = sr * (b.M[3 * r] * b.D[k] + b.M[3 * r + 1] * b.D[3 + k] + b.M[3 * r + 2] * b.D[6 + k]);
          const double r0 = sr * b.r[0], r1 = sr * b.r[1];
          H[0] += J[0] * J[0] + J[3] * J[3]; H[1] += J[0] * J[1] + J[3] * J[4]; H[2] += J[0] * J[2] + J[3] * J[5];
          H[3] += J[1] * J[1] + J[4] * J[4]; H[4] += J[1] * J[2] + J[4] * J[5]; H[5] += J[2] * J[2] + J[5] * J[5];
          g[0] += J[0] * r0 + J[3] * r1; g[1] += J[1] * r0 + J[4] * r1; g[2] += J[2] * r0 + J[5] * r1;
        }
      }
      sb = sn;
      im = vgpr_pin(im_next);   // the copy is made here, not behind the load below
      if (sb < s1) {            // goes out with the row's pose loads
        ox = d.sell_xy[2 * ((size_t)sb + lane)];
        oy = d.sell_xy[2 * ((size_t)sb + lane) + 1];
      }
    }
    if (!kLidarEarly) load_lidar_first(d, half, t, ln, lf);
  }
  if (BLOCKS && half == 1) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_half[sl][lane][k] = H[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_half[sl][lane][6 + k] = g[k];
  }
  __syncthreads();
  if (half == 0 && slice < d.nslices) {
    if (BLOCKS) {
#pragma unroll
      for (int k = 0; k < 6; ++k) H[k] += s_half[sl][lane][k];
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] += s_half[sl][lane][6 + k];
    }
    if (p >= 0) {
      if (ln) {
        // colmap-pcd adds one plane per point: that one is in registers; any further term takes the list
        points_add_lidar<BLOCKS>(d, X, lf, lf[4], cpt_b != 0, cost, H, g);
        const uint32_t le = ln > 1 ? d.pt_lidar_start[p] : 0u;
        for (uint32_t e = le + 1; e < le + ln; ++e) {
          const uint32_t l = d.pt_lidar_list[e];
          const double abcd[4] = {d.lidar_abcd[4 * (size_t)l], d.lidar_abcd[4 * (size_t)l + 1],
                                  d.lidar_abcd[4 * (size_t)l + 2], d.lidar_abcd[4 * (size_t)l + 3]};
          points_add_lidar<BLOCKS>(d, X, abcd, d.lidar_w[l], cpt_b != 0, cost, H, g);
        }
      }
      if (BLOCKS && Hpt) {
        double* h = Hpt + 9 * (size_t)p;
        h[0] = H[0]; h[1] = H[1]; h[2] = H[2]; h[3] = H[1]; h[4] = H[3]; h[5] = H[4]; h[6] = H[2]; h[7] = H[4]; h[8] = H[5];
      }
      if (BLOCKS && gpt) { gpt[3 * (size_t)p] = g[0]; gpt[3 * (size_t)p + 1] = g[1]; gpt[3 * (size_t)p + 2] = g[2]; }
    }
  }
  __syncthreads();
  // fixed-order block sum of the cost
  __shared__ double s_c[256];
  s_c[threadIdx.x] = cost;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_c[threadIdx.x] += s_c[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) cost_partial[blockIdx.x] = s_c[0];
}

// Cost only (the LM trial-step evaluation): no per-point accumulation is needed, so the sum runs over
// observations and LiDAR terms in their given order, one thread each -- 5.9 M independent threads instead of
// 1 M tracks with serial inner loops.  Same fixed-order two-stage sum (bitwise reproducible run to run; the
// summation order, hence the last bits, differ from the cost the Jacobian pass reports).
template <int MODEL, bool SHARED>
__global__ __launch_bounds__(256) void k_ba_cost(BaDev d, double* __restrict__ cost_partial) {
  // one residual block per thread (a fixed grid of 2048 workgroups looping over them measured 0.109 ms against
  // 0.096 ms: fewer wavefronts in flight for a latency-bound gather); the loop form is kept for grids that are
  // capped.  The assignment of blocks to threads and the order of the sums depend on the problem size only.
  double cost = 0.0;
  BaCam<MODEL, SHARED> cam(d);
  for (uint64_t i = blockIdx.x * (uint64_t)256 + threadIdx.x; i < d.O + d.L; i += (uint64_t)gridDim.x * 256) {
    if (i < d.O) {
      const int im = d.obs_image[i], pt = d.obs_point[i];
      const double X[3] = {d.points[3 * (size_t)pt], d.points[3 * (size_t)pt + 1], d.points[3 * (size_t)pt + 2]};
      ReprojBlock b;
      double q[4];
      // In AddImageToProblem order an image owns thousands of consecutive observations, so nearly every wavefront sees
      // one image: its pose is then read once through a wave-uniform address (scalar loads) instead of four per-lane
      // gathers.  Same values into the same arithmetic.  wave_uniform keeps the two branches from being merged back into
      // one per-lane gather on a selected index.
      double pose[7];
      const int im0 = __builtin_amdgcn_readfirstlane(im);
      if (__all(im == im0)) {
#pragma unroll
        for (int k = 0; k < 7; ++k) pose[k] = wave_uniform(d.poses[7 * (size_t)im0 + k]);
      } else {
        load_pose(d, im, pose);
      }
      cam.of_image(d, im);
      eval_block_at(cam, pose, X, d.obs_xy[2 * i], d.obs_xy[2 * i + 1], b, q);
      double rho0, rho1;
      loss_eval(d.loss_type, d.loss_scale, b.r[0] * b.r[0] + b.r[1] * b.r[1], rho0, rho1);
      cost += 0.5 * rho0;
    } else {
      const uint64_t l = i - d.O;
      const int pt = d.lidar_point[l];
      const double X[3] = {d.points[3 * (size_t)pt], d.points[3 * (size_t)pt + 1], d.points[3 * (size_t)pt + 2]};
      const double abcd[4] = {d.lidar_abcd[4 * l], d.lidar_abcd[4 * l + 1], d.lidar_abcd[4 * l + 2], d.lidar_abcd[4 * l + 3]};
      double r, J[3];
      lidar_eval(X, abcd, d.lidar_w[l], 0, r, J);
      double rho0, rho1;
      loss_eval(d.loss_type, d.loss_scale, r * r, rho0, rho1);
      cost += 0.5 * rho0;
    }
  }
  __shared__ double s_c[256];
  s_c[threadIdx.x] = cost;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_c[threadIdx.x] += s_c[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) cost_partial[blockIdx.x] = s_c[0];
}

// One workgroup, bound by the latency of its loads: 1024 threads with eight independent accumulators each keep 8192
// loads in flight per sweep (the cost pass of the bench scene leaves ~23 k partials: three sweeps instead of 23 with 256
// threads x 4).  Which partial goes to which accumulator and the order of every addition depend on n only: the sum is
// bitwise reproducible run to run.
constexpr int kSumThreads = 1024;
__global__ __launch_bounds__(kSumThreads) void k_sum_partials(const double* __restrict__ partial, int n,
                                                              double* __restrict__ out) {
  constexpr int T = kSumThreads;
  __shared__ double s_c[T];
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int i = threadIdx.x;
  for (; i + 7 * T < n; i += 8 * T) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += partial[i + j * T];
  }
  for (; i < n; i += T) a[0] += partial[i];
  s_c[threadIdx.x] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  for (int off = T / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_c[threadIdx.x] += s_c[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s_c[0];
}

// ------------------------------------------------------------- images ------
// WANT_W: also write the pose-point coupling block W[o] = Jp^T JX (6x3, loss-corrected, manifold-projected) of
// every observation -- what a Schur complement needs next to H_img / H_pt -- from the Jacobians this pass has
// in registers anyway (no second sweep).  When the caller's observations are image-major (the order
// AddImageToProblem creates them in, optim/bundle_adjustment.cc:814-919) the 144-B blocks of consecutive
// lanes are adjacent in memory.
// Work item = one SEGMENT of <= kImgSeg (ba_handle.h) observations of an image (an image per workgroup left a quarter
// of the chip idle on a 1000-image scene and nearly all of it on a 25-image one); the 27 partial sums of a segment go
// to `partial` and k_ba_images_reduce adds the segments of an image in ascending order: still no atomics, still
// bitwise reproducible.
// The 27 sums of a segment are the upper triangle and the last column of A^T A, A = [J | r]: 7 columns and two rows
// per observation, a small-N GEMM.  They are summed on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64) instead of in
// 27 per-lane fp64 accumulators: a wavefront's sums live in one 4-double accumulator (8 VGPRs instead of 54, held
// across the whole Jacobian evaluation before), the 54 VALU FMAs per observation and the 27 x 6-step shuffle butterfly
// at the end of the segment go away, and the matrix pipe (otherwise idle here) runs beside the other wavefronts' VALU.
//
// Per iteration a wavefront has 128 rows (lane l: rows 2l and 2l+1) of 7 values.  They are staged COLUMN-major in the
// wavefront's LDS scratch -- column c, rows 2l..2l+1 as one 16-B write at c * kRowColStride + 16 l, so a write
// instruction covers 1 KiB of consecutive addresses -- and read back as MFMA operands.  The 16x16x4 instruction has
// room for two independent 7-column products: with the SAME register as both operands, lane l holding
// data[row(k = l >> 4, h = (l >> 3) & 1)][col = l & 7], the result is D[i][j] = sum_k op[k][i] op[k][j], whose
// top-left 8x8 block is the product over the rows with h = 0 and whose bottom-right 8x8 block is the product over the
// rows with h = 1 (the off-diagonal blocks mix the two and are not read).  So one step takes 8 rows and an
// iteration 16 steps; row of (step s, k, h) = 8 s + 2 k + h, which with the 1056-B column stride
// puts the 32 addresses of each half-wavefront read on 32 different bank pairs.  Column 7 is never staged: its lanes
// re-read column 0 and feed row/column 7 of D, which nobody reads.
// C/D map of the f64 instruction: register g of lane l is D[(l >> 4) + 4 g][l & 15].
constexpr int kRowColStride = 132;   // doubles between two staged columns: 128 rows + 32 B (bank spread, keeps 16-B alignment)
static_assert(7 * kRowColStride <= 64 * 18, "the staged rows share the W transpose scratch");
typedef double mfma_f64x4 __attribute__((ext_vector_type(4)));

// The camera of a workgroup-uniform image: model id and parameters, read once through wave-uniform addresses at the
// top of the kernel and held in SGPRs.  MODEL = -1 reads the slots its model does not have from slot 0 (never used).
template <int MODEL>
struct BaImageCam {
  static constexpr int K = MODEL >= 0 ? cam_num_params(MODEL >= 0 ? MODEL : 0) : PCD_CAM_JAC_STRIDE;
  int model = MODEL;
  double v[K];
  __device__ __forceinline__ BaImageCam(const BaDev& d, int im) {
    const int cm = d.image_cam[im];
    if (MODEL < 0) model = d.cam_model[cm];
    const double* p = d.cam_params + d.cam_off[cm];
    const int kn = MODEL >= 0 ? K : cam_num_params(model);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_uniform(p[k < kn ? k : 0]);
  }
};

// Where the constant-point flag of point pt is read from.  A handle without constant points (has_pc false, uniform)
// reads a byte of the point itself instead -- its line is being fetched anyway -- and ignores it: the load stands in
// the instruction stream unconditionally, and a branch around it would make every wait behind it a wait for all.
__device__ __forceinline__ const uint8_t* const_byte(const BaDev& d, bool has_pc, uint32_t pt) {
  return has_pc ? d.point_const + pt : reinterpret_cast<const uint8_t*>(d.points + 3 * (size_t)pt);
}

// Launch bound: the OPENCV instantiation with W (the one that was measured) fits 4 wavefronts per SIMD (<= 128 VGPRs)
// without scratch and is faster there; every other instantiation is left to the register allocator (with the pose and
// the camera in SGPRs the other compiled-in models with W come to 116-120 VGPRs on their own).
//
// Load order.  The image is fixed for the workgroup, so its pose and camera are read ONCE, ahead of the loop (scalar
// loads, SGPRs; inside the loop they would have to be vector loads of uniform addresses behind the W stores, a
// three-deep chain image -> camera -> offset -> parameters per iteration).  They are still read at every launch:
// pcd_ba_set_* and the device LM update them in place.  The observation indices of every iteration are known up front
// (e0 + threadIdx.x), so img_pt / img_xy / img_obs of iteration i + 1 are issued before the Jacobian arithmetic of
// iteration i, and the points[pt] / point_const[pt] gather of i + 1 before the row staging, the MFMA block and the W
// store of i.  Indices past the end of the segment are clamped to its last observation: no branch around the loads
// (a constant-pose image that only writes its zero W rows loads as well), and what the surplus lanes and the surplus
// last prefetch return is not used.  Same values into the same arithmetic.
//
// W leaves non-temporally (kWStore).  It is half of the pass's bytes (144 B per observation), written once and read by
// nothing in the evaluation; as plain stores its lines pass through L2 and the Infinity Cache between two gathers of a
// point's line, and the gathers of this pass and of k_ba_cost behind it miss more often.  Measured on the bench scene
// (profiles/ba_store_policy_bench_lines.txt): nt 0.248 -> 0.220 ms and k_ba_cost 0.098 -> 0.093 ms; write-through (sc1)
// stores 0.256 ms, slower than plain.  Same addresses, same values.
constexpr StorePolicy kWStore = StorePolicy::nt;
template <int MODEL, bool WANT_W>
__global__ __launch_bounds__(256, (MODEL == 4 && WANT_W) ? 4 : 1) void k_ba_images(BaDev d, double* __restrict__ partial,
                                                                       double* __restrict__ W_o) {
  __shared__ __attribute__((aligned(16))) double s_w[4][64 * 18];   // per wavefront: staged rows, then the W transpose
  __shared__ double s_a[4][2][27];
  const int im = (int)d.seg_img[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // uniform for the compiler
  // the two flag bytes of the image: read unconditionally (from the segment table when the handle has no such array,
  // and then ignored), so that they travel with the loads below instead of each behind a branch and a wait of its own
  const uint8_t* any_byte = reinterpret_cast<const uint8_t*>(d.seg_img + blockIdx.x);
  const unsigned cpose_b = *(d.image_const_pose ? d.image_const_pose + im : any_byte);
  const unsigned tmask_b = *(d.image_const_tvec ? d.image_const_tvec + im : any_byte);
  mfma_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  const uint32_t e_beg = d.seg_begin[blockIdx.x];
  const uint32_t e_end = min(d.seg_begin[blockIdx.x + 1], d.img_obs_start[im + 1]);   // segments never span images
  BaImageCam<MODEL> cam(d, im);
  double q[4], tv[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = wave_uniform(d.poses[7 * (size_t)im + k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) tv[k] = wave_uniform(d.poses[7 * (size_t)im + 4 + k]);
  // operand address of this lane: column l & 7 (7 -> 0), row 2 k + h of the step's 8
  const int op_k = lane >> 4, op_c = (lane & 7) == 7 ? 0 : (lane & 7);
  const double* op_src = s_w[wave] + op_c * kRowColStride + 2 * op_k + ((lane >> 3) & 1);
  const bool cpose = d.image_const_pose && cpose_b;
  const unsigned tmask = d.image_const_tvec ? tmask_b : 0u;
  if (!cpose || WANT_W) {
    const uint32_t e_last = e_end - 1;   // a segment holds at least one observation
    const bool has_pc = WANT_W && d.point_const;
    // the first iteration's loads
    // (indices and the point_const byte stay as loaded until their first use: converting them where they are loaded
    // would put a wait right behind the load)
    uint32_t pt = 0, o = 0, pc = 0;
    double ox = 0.0, oy = 0.0, X[3] = {0.0, 0.0, 0.0};
    {
      const uint32_t ec = min(e_beg + threadIdx.x, e_last);
      pt = (uint32_t)d.img_pt[ec]; ox = d.img_xy[2 * (size_t)ec]; oy = d.img_xy[2 * (size_t)ec + 1];
      if (WANT_W) o = d.img_obs[ec];
      X[0] = d.points[3 * (size_t)pt]; X[1] = d.points[3 * (size_t)pt + 1]; X[2] = d.points[3 * (size_t)pt + 2];
      if (WANT_W) pc = *const_byte(d, has_pc, pt);
    }
    // every lane runs every iteration (the row staging and the W store below are whole-wavefront operations)
    for (uint32_t e0 = e_beg; e0 < e_end; e0 += 256) {
      const uint32_t e = e0 + threadIdx.x;
      const bool active = e < e_end;
      // observations left for this wavefront (uniform): 0 for the wavefronts past the end in the last iteration
      const int cnt = (int)min(64u, e_end > e0 + wave * 64u ? e_end - (e0 + wave * 64u) : 0u);
      // Pose and parameters pass through sgpr_pin once per iteration: the uniform factors of the Jacobians (rotation
      // polynomial, doubled coefficients) are then recomputed per iteration, as before.  Hoisted out of the loop they
      // cost ~45 VGPRs and the fourth wavefront per SIMD.
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = sgpr_pin(q[k]);
#pragma unroll
      for (int k = 0; k < 3; ++k) tv[k] = sgpr_pin(tv[k]);
#pragma unroll
      for (int k = 0; k < BaImageCam<MODEL>::K; ++k) cam.v[k] = sgpr_pin(cam.v[k]);
      // the next iteration's indices
      const uint32_t en = (e_last >= 256u && e <= e_last - 256u) ? e + 256u : e_last;
      uint32_t pt_n = 0, o_n = 0;
      double ox_n = 0.0, oy_n = 0.0;
      pt_n = (uint32_t)d.img_pt[en]; ox_n = d.img_xy[2 * (size_t)en]; oy_n = d.img_xy[2 * (size_t)en + 1];
      if (WANT_W) o_n = d.img_obs[en];
      double w[18];
#pragma unroll
      for (int k = 0; k < 18; ++k) w[k] = 0.0;   // constant pose / constant point: the coupling is zero
      double J[12], r0 = 0.0, r1 = 0.0;          // 2 x 6 and the residual; zero rows for inactive lanes
#pragma unroll
      for (int k = 0; k < 12; ++k) J[k] = 0.0;
      if (active && !cpose) {
        ReprojBlock b;
        reproj_eval(cam.model, cam.v, q, tv, X, ox, oy, b);
        double rho0, rho1;
        loss_eval(d.loss_type, d.loss_scale, b.r[0] * b.r[0] + b.r[1] * b.r[1], rho0, rho1);
        const double sr = sqrt(rho1);
        double Jq[8], Jt[6], JX[6], Jqt[6];
        reproj_jacobians(b, Jq, Jt, JX);
        quat_tangent(q, Jq, Jqt);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            J[6 * r + k] = sr * Jqt[3 * r + k];
            J[6 * r + 3 + k] = ((tmask >> k) & 1u) ? 0.0 : sr * Jt[3 * r + k];
          }
        r0 = sr * b.r[0];
        r1 = sr * b.r[1];
        if (WANT_W && !(has_pc && pc != 0)) {
#pragma unroll
          for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) w[3 * a + c] = J[a] * (sr * JX[c]) + J[6 + a] * (sr * JX[3 + c]);
        }
      }
      // the next iteration's point: in flight under the staging, the MFMA block and the W store
      {
        X[0] = d.points[3 * (size_t)pt_n]; X[1] = d.points[3 * (size_t)pt_n + 1]; X[2] = d.points[3 * (size_t)pt_n + 2];
        if (WANT_W) pc = *const_byte(d, has_pc, pt_n);
        // the prefetched values move into the loop's registers HERE (vgpr_pin): left to the end of the iteration the
        // copies stand behind a wait for everything in flight, the W stores included
        ox = vgpr_pin(ox_n);
        oy = vgpr_pin(oy_n);
      }
      // the LDS addresses of the staging and of the W transpose are formed from this copy of the lane in every iteration
      // (held across the loop they are a dozen VGPRs)
      const int lane_i = vgpr_pin(lane);
      if (!cpose && cnt > 0) {   // uniform; a constant pose keeps its sums at exactly zero, an idle wavefront adds nothing
        double2* row_dst = reinterpret_cast<double2*>(s_w[wave]) + lane_i;
#pragma unroll
        for (int c = 0; c < 6; ++c) row_dst[c * (kRowColStride / 2)] = make_double2(J[c], J[6 + c]);
        row_dst[6 * (kRowColStride / 2)] = make_double2(r0, r1);
        // one wavefront: LDS operations complete in order; the fences keep the compiler from moving the reads up
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const double a = op_src[8 * s];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();   // the scratch may be rewritten after this
      }
      if (WANT_W) {
        // rows of this wavefront: observation indices in the caller's order
        const uint32_t oa = active ? o : 0u;
        o = vgpr_pin(o_n);
        const uint32_t o_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)oa);
        const bool contiguous = __all(!active || oa == o_first + (uint32_t)lane_i);
        if (contiguous) {
          wave_store_rows<18, kWStore>(W_o, o_first, cnt, w, s_w[wave], lane_i);
        } else if (active) {
          lane_store_row<18, kWStore>(W_o, oa, w);
        }
      }
    }
  }
  // the wavefront's two 7x7 products -> LDS in the packing of `partial` (upper triangle by rows, then the gradient):
  // lane (g = l >> 4, h, c) holds rows a = g and a = 4 + g of product h, column c
  {
    const int g = lane >> 4, h = (lane >> 3) & 1, c = lane & 7;
#pragma unroll
    for (int hi = 0; hi < 2; ++hi) {
      const int a = g + 4 * hi;
      const double v = h ? acc[2 + hi] : acc[hi];
      if (a < 6 && c >= a && c < 7) s_a[wave][h][c == 6 ? 21 + a : a * 6 - a * (a - 1) / 2 + (c - a)] = v;
    }
  }
  __syncthreads();
  // fixed order: the two products of a wavefront, then the wavefronts as (0 + 1) + (2 + 3)
  if (threadIdx.x < 27) {
    const int k = threadIdx.x;
    partial[27 * (size_t)blockIdx.x + k] = ((s_a[0][0][k] + s_a[0][1][k]) + (s_a[1][0][k] + s_a[1][1][k])) +
                                           ((s_a[2][0][k] + s_a[2][1][k]) + (s_a[3][0][k] + s_a[3][1][k]));
  }
}

// segments of an image added in ascending order -> 6x6 block (symmetric) + gradient
__global__ __launch_bounds__(64) void k_ba_images_reduce(BaDev d, const double* __restrict__ partial,
                                                         double* __restrict__ Himg, double* __restrict__ gimg) {
  const int im = blockIdx.x * 2 + (threadIdx.x >> 5), k = threadIdx.x & 31;
  if (im >= d.I || k >= 27) return;
  double v = 0.0;
  for (uint32_t sgm = d.img_seg_start[im]; sgm < d.img_seg_start[im + 1]; ++sgm) v += partial[27 * (size_t)sgm + k];
  if (k >= 21) {
    if (gimg) gimg[6 * (size_t)im + (k - 21)] = v;
  } else if (Himg) {
    int a = 0, kk = k;  // unpack the upper-triangle index
    while (kk >= 6 - a) { kk -= 6 - a; ++a; }
    const int c = a + kk;
    Himg[36 * (size_t)im + 6 * a + c] = v;
    Himg[36 * (size_t)im + 6 * c + a] = v;
  }
}

// ------------------------------------------------------------ cameras ------
// Camera blocks of the normal equations (refined intrinsics; ParameterizeCameras, optim/bundle_adjustment.cc:
// 1047-1100).  Per image the accumulation has NE = K(K+1)/2 + 6K + K entries -- upper triangle of Jc^T Jc,
// Jc^T Jp (K x 6), Jc^T r -- too many to keep per lane next to the Jacobians, so the four wavefronts of the
// workgroup each own a quarter of the entries and every wavefront sweeps all observations of the image
// (Jacobians recomputed four times; this pass only runs when intrinsics are refined, which the fork's defaults
// switch off).  Entry -> operand columns is resolved at compile time (K and the chunk are template constants).
// Fixed-order reductions, no atomics: bitwise reproducible.  k_ba_cameras_reduce then sums the images of a camera.
__host__ __device__ constexpr int cam_ne(int K) { return K * (K + 1) / 2 + 6 * K + K; }
// operand columns of entry e in A = [Jc (K) | Jp (6) | r (1)]
__host__ __device__ constexpr int cam_ent_l(int K, int e) {
  const int ncc = K * (K + 1) / 2;
  if (e < ncc) { int a = 0; while (e >= K - a) { e -= K - a; ++a; } return a; }
  e -= ncc;
  if (e < 6 * K) return e / 6;
  return e - 6 * K;
}
__host__ __device__ constexpr int cam_ent_r(int K, int e) {
  const int ncc = K * (K + 1) / 2;
  if (e < ncc) { int a = 0; while (e >= K - a) { e -= K - a; ++a; } return a + e; }
  e -= ncc;
  if (e < 6 * K) return K + e % 6;
  return K + 6;
}

template <int MODEL, int CH>
__device__ __forceinline__ void cam_accumulate(const BaDev& d, int im, double* __restrict__ partial) {
  constexpr int K = MODEL >= 0 ? cam_num_params(MODEL >= 0 ? MODEL : 0) : PCD_CAM_JAC_STRIDE;
  constexpr int NE = cam_ne(K), PER = (NE + 3) / 4, E0 = CH * PER, E1 = E0 + PER < NE ? E0 + PER : NE;
  constexpr int NA = K + 7;
  const int lane = threadIdx.x & 63;
  const bool cpose = d.image_const_pose && d.image_const_pose[im];
  const unsigned tmask = d.image_const_tvec ? d.image_const_tvec[im] : 0u;
  const int cm = d.image_cam[im];
  const double* cam = d.cam_params + d.cam_off[cm];
  const uint8_t* refine = d.cam_refine ? d.cam_refine + d.cam_off[cm] : nullptr;
  const int model = MODEL >= 0 ? MODEL : d.cam_model[cm];
  double acc[PER > 0 ? PER : 1];
#pragma unroll
  for (int t = 0; t < PER; ++t) acc[t] = 0.0;
  for (uint32_t e = d.img_obs_start[im] + lane; e < d.img_obs_start[im + 1]; e += 64) {
    const int pt = d.img_pt[e];
    const double X[3] = {d.points[3 * (size_t)pt], d.points[3 * (size_t)pt + 1], d.points[3 * (size_t)pt + 2]};
    ReprojBlock b;
    double q[4];
    eval_block<MODEL>(d, im, X, d.img_xy[2 * (size_t)e], d.img_xy[2 * (size_t)e + 1], b, q);
    double rho0, rho1;
    loss_eval(d.loss_type, d.loss_scale, b.r[0] * b.r[0] + b.r[1] * b.r[1], rho0, rho1);
    const double sr = sqrt(rho1);
    double A[2][NA];
    {  // camera columns: same normalised coordinates as reproj_eval
      double pose[7], P[3];
      load_pose(d, im, pose);
      pose_transform(pose, pose + 4, X, P);
      const double iz = 1.0 / P[2];
      double Jc[2 * K];
#pragma unroll
      for (int k = 0; k < 2 * K; ++k) Jc[k] = 0.0;
      if (MODEL >= 0) cam_param_jacobian<(MODEL >= 0 ? MODEL : 0)>(cam, P[0] * iz, P[1] * iz, Jc, K);
      else cam_param_jacobian_any(model, cam, P[0] * iz, P[1] * iz, Jc, K);
      const int kn = MODEL >= 0 ? K : cam_num_params(model);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const bool var = refine && k < kn && refine[k < kn ? k : 0];
        A[0][k] = var ? sr * Jc[k] : 0.0;
        A[1][k] = var ? sr * Jc[K + k] : 0.0;
      }
    }
    double Jq[8], Jt[6], JX[6], Jqt[6];
    reproj_jacobians(b, Jq, Jt, JX);
    quat_tangent(q, Jq, Jqt);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        A[r][K + k] = cpose ? 0.0 : sr * Jqt[3 * r + k];
        A[r][K + 3 + k] = (cpose || ((tmask >> k) & 1u)) ? 0.0 : sr * Jt[3 * r + k];
      }
      A[r][K + 6] = sr * b.r[r];
    }
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      if (E0 + t < E1) {
        const int l = cam_ent_l(K, E0 + t), r = cam_ent_r(K, E0 + t);
        acc[t] += A[0][l] * A[0][r] + A[1][l] * A[1][r];
      }
    }
  }
#pragma unroll
  for (int t = 0; t < PER; ++t) {
    if (E0 + t < E1) {
      double v = acc[t];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (lane == 0) partial[(size_t)im * cam_ne(PCD_CAM_JAC_STRIDE) + E0 + t] = v;
    }
  }
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_ba_cameras(BaDev d, double* __restrict__ partial) {
  const int im = blockIdx.x;
  switch (threadIdx.x >> 6) {
    case 0: cam_accumulate<MODEL, 0>(d, im, partial); break;
    case 1: cam_accumulate<MODEL, 1>(d, im, partial); break;
    case 2: cam_accumulate<MODEL, 2>(d, im, partial); break;
    default: cam_accumulate<MODEL, 3>(d, im, partial); break;
  }
}

// partial [I][NE(12)] (entries laid out for the image's own K) -> H_cam / g_cam per camera (images summed in
// ascending order) and E_cam per image
__global__ __launch_bounds__(256) void k_ba_cameras_reduce(BaDev d, const double* __restrict__ partial,
                                                           double* __restrict__ Hcam, double* __restrict__ gcam,
                                                           double* __restrict__ Ecam) {
  constexpr int S = PCD_CAM_JAC_STRIDE, NEMAX = cam_ne(S);
  const int c = blockIdx.x;
  const int model = d.cam_model[c];
  const int K = d.cam_k;
  (void)model;
  const int ncc = K * (K + 1) / 2, NE = ncc + 7 * K;
  for (int e = threadIdx.x; e < S * S + S; e += 256) {   // zero-fill, then the K x K / K part
    if (e < S * S) { if (Hcam) Hcam[(size_t)c * S * S + e] = 0.0; }
    else if (gcam) gcam[(size_t)c * S + (e - S * S)] = 0.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NE; e += 256) {
    if (e >= ncc && e < ncc + 6 * K) continue;   // coupling entries are per image
    double v = 0.0;
    for (uint32_t j = d.cam_img_start[c]; j < d.cam_img_start[c + 1]; ++j)
      v += partial[(size_t)d.cam_img_list[j] * NEMAX + e];
    if (e < ncc) {
      int a = 0, k = e;
      while (k >= K - a) { k -= K - a; ++a; }
      const int b = a + k;
      if (Hcam) { Hcam[(size_t)c * S * S + a * S + b] = v; Hcam[(size_t)c * S * S + b * S + a] = v; }
    } else if (gcam) {
      gcam[(size_t)c * S + (e - ncc - 6 * K)] = v;
    }
  }
  if (Ecam) {
    for (uint32_t j = d.cam_img_start[c]; j < d.cam_img_start[c + 1]; ++j) {
      const uint32_t im = d.cam_img_list[j];
      for (int e = threadIdx.x; e < S * 6; e += 256) {
        const int a = e / 6;
        Ecam[(size_t)im * S * 6 + e] = a < K ? partial[(size_t)im * NEMAX + ncc + e] : 0.0;
      }
    }
  }
}

// camera x point coupling of every observation: W_cam[o] = Jc^T JX (S x 3, loss-corrected, masks applied)
template <int MODEL>
__global__ __launch_bounds__(256) void k_ba_cam_w(BaDev d, double* __restrict__ Wc_o) {
  constexpr int S = PCD_CAM_JAC_STRIDE;
  __shared__ __attribute__((aligned(16))) double s_rows[4][64 * 3 * S];
  const int wave = threadIdx.x >> 6;
  const uint64_t o = blockIdx.x * (uint64_t)256 + threadIdx.x;
  const uint64_t o_wave = blockIdx.x * (uint64_t)256 + wave * 64;
  if (o_wave >= d.O) return;
  const int cnt = (int)min((uint64_t)64, d.O - o_wave);
  double Wc[3 * S];
#pragma unroll
  for (int k = 0; k < 3 * S; ++k) Wc[k] = 0.0;
  if (o < d.O) {
    const int im = d.obs_image[o], pt = d.obs_point[o];
    const bool cpt = d.point_const && d.point_const[pt];
    const int cm = d.image_cam[im];
    const uint8_t* refine = d.cam_refine ? d.cam_refine + d.cam_off[cm] : nullptr;
    if (!cpt && refine) {
      const double X[3] = {d.points[3 * (size_t)pt], d.points[3 * (size_t)pt + 1], d.points[3 * (size_t)pt + 2]};
      ReprojBlock b;
      double q[4];
      eval_block<MODEL>(d, im, X, d.obs_xy[2 * o], d.obs_xy[2 * o + 1], b, q);
      double rho0, rho1;
      loss_eval(d.loss_type, d.loss_scale, b.r[0] * b.r[0] + b.r[1] * b.r[1], rho0, rho1);
      double Jq[8], Jt[6], JX[6];
      reproj_jacobians(b, Jq, Jt, JX);
      double pose[7], P[3];
      load_pose(d, im, pose);
      pose_transform(pose, pose + 4, X, P);
      const double iz = 1.0 / P[2];
      const int model = MODEL >= 0 ? MODEL : d.cam_model[cm];
      double Jc[2 * S];
#pragma unroll
      for (int k = 0; k < 2 * S; ++k) Jc[k] = 0.0;
      if (MODEL >= 0) cam_param_jacobian<(MODEL >= 0 ? MODEL : 0)>(d.cam_params + d.cam_off[cm], P[0] * iz, P[1] * iz, Jc, S);
      else cam_param_jacobian_any(model, d.cam_params + d.cam_off[cm], P[0] * iz, P[1] * iz, Jc, S);
      const int kn = cam_num_params(model);
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const bool var = k < kn && refine[k < kn ? k : 0];
#pragma unroll
        for (int j = 0; j < 3; ++j)
          Wc[3 * k + j] = var ? rho1 * (Jc[k] * JX[j] + Jc[S + k] * JX[3 + j]) : 0.0;
      }
    }
  }
  wave_store_rows<3 * S>(Wc_o, o_wave, cnt, Wc, s_rows[wave]);
}

// ---------------------------------------------------------------- raw ------
// k_ba_raw / k_ba_raw_compact / k_ba_obs_errors take BaCam's SHARED flag as a template argument, like k_ba_points and
// k_ba_cost (own register allocation per instantiation, no branch inside).  k_ba_raw alone keeps its body in a device
// function: written into the kernel, the same statements compile to 116-142 VGPRs instead of 96-100 (compiled-in models).
template <int MODEL, bool SHARED>
__device__ __forceinline__ void ba_raw_body(const BaDev& d, double* __restrict__ residuals, double* __restrict__ Jq_o,
                                            double* __restrict__ Jt_o, double* __restrict__ JX_o,
                                            double* __restrict__ W_o, double (*s_rows)[64 * 18]) {
  // thread = observation in the caller's order: the blocks of a wavefront are adjacent in every output array,
  // so each array is written through wave_store_rows (coalesced 16-B stores)
  const int wave = threadIdx.x >> 6;
  const uint64_t o = blockIdx.x * (uint64_t)256 + threadIdx.x;
  const uint64_t o_wave = blockIdx.x * (uint64_t)256 + wave * 64;
  if (o_wave >= d.O) return;   // whole wavefront past the end
  const int cnt = (int)min((uint64_t)64, d.O - o_wave);
  const bool active = o < d.O;
  double res[2] = {0, 0}, Jq[8], Jt[6], JX[6], Wb[18];
#pragma unroll
  for (int k = 0; k < 8; ++k) Jq[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) { Jt[k] = 0.0; JX[k] = 0.0; }
#pragma unroll
  for (int k = 0; k < 18; ++k) Wb[k] = 0.0;
  if (active) {
    const int im = d.obs_image[o], pt = d.obs_point[o];
    const double X[3] = {d.points[3 * (size_t)pt], d.points[3 * (size_t)pt + 1], d.points[3 * (size_t)pt + 2]};
    ReprojBlock b;
    double q[4];
    double pose[7];
    BaCam<MODEL, SHARED> cam(d);
    cam.of_image(d, im);
    load_pose(d, im, pose);
    eval_block_at(cam, pose, X, d.obs_xy[2 * o], d.obs_xy[2 * o + 1], b, q);
    reproj_jacobians(b, Jq, Jt, JX);
    const bool cpose = d.image_const_pose && d.image_const_pose[im];
    res[0] = b.r[0]; res[1] = b.r[1];
    if (W_o) {
      double rho0, rho1;
      loss_eval(d.loss_type, d.loss_scale, b.r[0] * b.r[0] + b.r[1] * b.r[1], rho0, rho1);
      const double sr = sqrt(rho1);
      const unsigned tmask = d.image_const_tvec ? d.image_const_tvec[im] : 0u;
      const bool cpt = d.point_const && d.point_const[pt];
      double Jqt[6], J[12], Jx[6];
      quat_tangent(q, Jq, Jqt);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          J[6 * r + k] = cpose ? 0.0 : sr * Jqt[3 * r + k];
          J[6 * r + 3 + k] = (cpose || ((tmask >> k) & 1u)) ? 0.0 : sr * Jt[3 * r + k];
          Jx[3 * r + k] = cpt ? 0.0 : sr * JX[3 * r + k];
        }
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) Wb[3 * a + c] = J[a] * Jx[c] + J[6 + a] * Jx[3 + c];
    }
    if (cpose) {   // the constant-pose functor has no pose blocks: zero rows
#pragma unroll
      for (int k = 0; k < 8; ++k) Jq[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) Jt[k] = 0.0;
    }
  }
  if (residuals) wave_store_rows<2>(residuals, o_wave, cnt, res, s_rows[wave]);
  if (Jq_o) wave_store_rows<8>(Jq_o, o_wave, cnt, Jq, s_rows[wave]);
  if (Jt_o) wave_store_rows<6>(Jt_o, o_wave, cnt, Jt, s_rows[wave]);
  if (JX_o) wave_store_rows<6>(JX_o, o_wave, cnt, JX, s_rows[wave]);
  if (W_o) wave_store_rows<18>(W_o, o_wave, cnt, Wb, s_rows[wave]);
}
template <int MODEL, bool SHARED>
__global__ __launch_bounds__(256) void k_ba_raw(BaDev d, double* __restrict__ residuals, double* __restrict__ Jq_o,
                                                double* __restrict__ Jt_o, double* __restrict__ JX_o,
                                                double* __restrict__ W_o) {
  __shared__ __attribute__((aligned(16))) double s_rows[4][64 * 18];
  ba_raw_body<MODEL, SHARED>(d, residuals, Jq_o, Jt_o, JX_o, W_o, s_rows);
}

// Camera-parameter block of every reprojection residual (2 x K, row stride PCD_CAM_JAC_STRIDE).
template <int MODEL>
__global__ __launch_bounds__(256) void k_ba_cam_jac(BaDev d, double* __restrict__ Jc_o) {
  const uint64_t o = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (o >= d.O) return;
  const int im = d.obs_image[o], pt = d.obs_point[o];
  const double* pose = d.poses + 7 * (size_t)im;
  const double* Xp = d.points + 3 * (size_t)pt;
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  double P[3];
  pose_transform(pose, pose + 4, X, P);
  const double iz = 1.0 / P[2];
  const int cm = d.image_cam[im];
  double J[2 * PCD_CAM_JAC_STRIDE];
#pragma unroll
  for (int k = 0; k < 2 * PCD_CAM_JAC_STRIDE; ++k) J[k] = 0.0;
  if (MODEL >= 0) cam_param_jacobian<(MODEL >= 0 ? MODEL : 0)>(d.cam_params + d.cam_off[cm], P[0] * iz, P[1] * iz, J, PCD_CAM_JAC_STRIDE);
  else cam_param_jacobian_any(d.cam_model[cm], d.cam_params + d.cam_off[cm], P[0] * iz, P[1] * iz, J, PCD_CAM_JAC_STRIDE);
  double* out = Jc_o + 2 * PCD_CAM_JAC_STRIDE * o;
#pragma unroll
  for (int k = 0; k < 2 * PCD_CAM_JAC_STRIDE; ++k) out[k] = J[k];
}

// Compact Ceres route (pcd_ba_evaluate_blocks_compact): one record {r0, r1, M row-major 2x3} per observation, M = dr/dP.
// Every Jacobian block of the observation is M times a factor of the evaluation point alone (jac_t = M, jac_X = M D(q),
// jac_q = M dPdq(q, X)), which the host rebuilds (shim/ceres_compact.h): 64 B cross PCIe instead of 176 B.  r and M are
// the values eval_block gives k_ba_raw, bit for bit; D and dPdq are never read here, so the compiler drops them
// (tests/test_ceres_compact_isa.py holds the register count against k_ba_raw's).  A constant-pose observation keeps
// its true M: its jac_X needs it.
template <int MODEL, bool SHARED>
__global__ __launch_bounds__(256) void k_ba_raw_compact(BaDev d, double* __restrict__ rec_o) {
  __shared__ __attribute__((aligned(16))) double s_rows[4][64 * 8];
  const int wave = threadIdx.x >> 6;
  const uint64_t o = blockIdx.x * (uint64_t)256 + threadIdx.x;
  const uint64_t o_wave = blockIdx.x * (uint64_t)256 + wave * 64;
  if (o_wave >= d.O) return;   // whole wavefront past the end
  const int cnt = (int)min((uint64_t)64, d.O - o_wave);
  double rec[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) rec[k] = 0.0;
  if (o < d.O) {
    const int im = d.obs_image[o], pt = d.obs_point[o];
    const double X[3] = {d.points[3 * (size_t)pt], d.points[3 * (size_t)pt + 1], d.points[3 * (size_t)pt + 2]};
    ReprojBlock b;
    double q[4];
    double pose[7];
    BaCam<MODEL, SHARED> cam(d);
    cam.of_image(d, im);
    load_pose(d, im, pose);
    eval_block_at(cam, pose, X, d.obs_xy[2 * o], d.obs_xy[2 * o + 1], b, q);
    rec[0] = b.r[0]; rec[1] = b.r[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) rec[2 + k] = b.M[k];
  }
  wave_store_rows<8>(rec_o, o_wave, cnt, rec, s_rows[wave]);   // 4 KiB of consecutive addresses per wavefront
}

// Camera blocks for the compact route: [O][2][PCD_CAM_JAC_STRIDE] -> [O][2][cs], cs = the widest camera of the handle
// (columns >= K of a narrower camera are the zeros k_ba_cam_jac wrote).  thread = output double: consecutive lanes
// write consecutive addresses and read runs of cs doubles.
__global__ __launch_bounds__(256) void k_ba_pack_cam_jac(const double* __restrict__ in, uint64_t nrows, int cs,
                                                         double* __restrict__ out) {
  const uint64_t u = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (u >= nrows * (uint64_t)cs) return;
  const uint64_t r = u / (uint64_t)cs;
  const int k = (int)(u - r * (uint64_t)cs);
  out[u] = in[r * PCD_CAM_JAC_STRIDE + k];
}

// Inputs of the post-BA filters, per observation:
//   sq_err = CalculateSquaredReprojectionError (base/projection.cc:104-117; quaternion normalised first as
//            base/pose.cc QuaternionRotatePoint does; DBL_MAX when the point is not in front of the camera)
//   depth  = P.z (FilterObservationsWithNegativeDepth, base/reconstruction.cc:837-855, tests it against eps)
template <int MODEL, bool SHARED>
__global__ __launch_bounds__(256) void k_ba_obs_errors(BaDev d, double* __restrict__ sq_err, double* __restrict__ depth) {
  const uint64_t o = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (o >= d.O) return;
  const int im = d.obs_image[o], pt = d.obs_point[o];
  const double* pose = d.poses + 7 * (size_t)im;
  double q[4] = {pose[0], pose[1], pose[2], pose[3]};
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n == 0.0) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; }
  else { q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; }
  const double X[3] = {d.points[3 * (size_t)pt], d.points[3 * (size_t)pt + 1], d.points[3 * (size_t)pt + 2]};
  double P[3];
  pose_transform(q, pose + 4, X, P);
  if (depth) depth[o] = P[2];
  if (!sq_err) return;
  if (P[2] < 2.220446049250313e-16) { sq_err[o] = 1.7976931348623157e308; return; }
  BaCam<MODEL, SHARED> cam(d);
  cam.of_image(d, im);
  D2 x, y;
  world_to_image_d2(cam.model, cam.params(), P[0] / P[2], P[1] / P[2], x, y);
  const double dx = x.a - d.obs_xy[2 * o], dy = y.a - d.obs_xy[2 * o + 1];
  sq_err[o] = dx * dx + dy * dy;
}

__global__ __launch_bounds__(256) void k_ba_lidar_raw(BaDev d, double* __restrict__ residuals, double* __restrict__ JL) {
  const uint64_t l = blockIdx.x * (uint64_t)256 + threadIdx.x;
  if (l >= d.L) return;
  const int p = d.lidar_point[l];
  const double X[3] = {d.points[3 * (size_t)p], d.points[3 * (size_t)p + 1], d.points[3 * (size_t)p + 2]};
  const double abcd[4] = {d.lidar_abcd[4 * l], d.lidar_abcd[4 * l + 1], d.lidar_abcd[4 * l + 2], d.lidar_abcd[4 * l + 3]};
  double r, J[3];
  lidar_eval(X, abcd, d.lidar_w[l], 0, r, J);
  if (residuals) residuals[2 * d.O + l] = r;
  if (JL) { JL[3 * l] = J[0]; JL[3 * l + 1] = J[1]; JL[3 * l + 2] = J[2]; }
}

// ---- post-BA filters, reduced per track (base/reconstruction.cc:1662-1712, :837-855, :906-921) -----------------
// thread = point; its observations in ascending observation index (pt_obs_list)
__global__ __launch_bounds__(256) void k_ba_filter_tracks(int P, const uint32_t* __restrict__ pt_start,
                                                          const uint32_t* __restrict__ pt_list,
                                                          const double* __restrict__ sq_err, double max_sq,
                                                          uint8_t* __restrict__ obs_erase, uint8_t* __restrict__ point_delete,
                                                          double* __restrict__ point_error, double* __restrict__ partial) {
  __shared__ double s_f[4], s_e[4], s_n[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double filtered = 0.0, esum = 0.0, valid = 0.0;
  if (p < P) {
    const uint32_t b = pt_start[p], len = pt_start[p + 1] - b;
    uint32_t ndel = 0;
    double sum = 0.0;
    for (uint32_t j = 0; j < len; ++j) {
      const double e = sq_err[pt_list[b + j]];
      if (e > max_sq) ++ndel; else sum += sqrt(e);
    }
    // reconstruction.cc:1677-1681 (length < 2) and :1700-1702 (at most one element survives): DeletePoint3D
    const bool del = len < 2 || ndel + 1 >= len;
    if (obs_erase)
      for (uint32_t j = 0; j < len; ++j) {
        const uint32_t o = pt_list[b + j];
        obs_erase[o] = (del || sq_err[o] > max_sq) ? 1 : 0;
      }
    filtered = del ? (double)len : (double)ndel;
    const double err = del ? -1.0 : sum / (double)(len - ndel);   // Track().Length() after the deletions (:1708)
    if (point_delete) point_delete[p] = del ? 1 : 0;
    if (point_error) point_error[p] = err;
    if (!del) { esum = err; valid = 1.0; }
  }
  // fixed-order reduction: lanes by butterfly, the 4 wavefronts in order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    filtered += __shfl_xor(filtered, off); esum += __shfl_xor(esum, off); valid += __shfl_xor(valid, off);
  }
  if (lane == 0) { s_f[wave] = filtered; s_e[wave] = esum; s_n[wave] = valid; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[3 * (size_t)blockIdx.x] = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
    partial[3 * (size_t)blockIdx.x + 1] = (s_e[0] + s_e[1]) + (s_e[2] + s_e[3]);
    partial[3 * (size_t)blockIdx.x + 2] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
  }
}
__global__ __launch_bounds__(256) void k_ba_negative_depth(uint64_t O, const double* __restrict__ depth,
                                                           uint8_t* __restrict__ flag, double* __restrict__ partial) {
  __shared__ double s_c[4];
  const uint64_t o = blockIdx.x * (uint64_t)256 + threadIdx.x;
  const bool neg = o < O && depth[o] < 2.220446049250313e-16;   // !HasPointPositiveDepth (base/projection.cc:191-195)
  if (o < O && flag) flag[o] = neg ? 1 : 0;
  double c = neg ? 1.0 : 0.0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}
// one workgroup: partials added in block order (strided per thread, then the threads in order)
__global__ __launch_bounds__(256) void k_ba_filter_summary(const double* __restrict__ part3, int nb3,
                                                           const double* __restrict__ part1, int nb1,
                                                           double* __restrict__ summary) {
  __shared__ double s_v[4][256];
  double a[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < nb3; b += 256) { a[0] += part3[3 * (size_t)b]; a[1] += part3[3 * (size_t)b + 1]; a[2] += part3[3 * (size_t)b + 2]; }
  for (int b = threadIdx.x; b < nb1; b += 256) a[3] += part1[b];
  for (int k = 0; k < 4; ++k) s_v[k][threadIdx.x] = a[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[4] = {0, 0, 0, 0};
    for (int i = 0; i < 256; ++i) for (int k = 0; k < 4; ++k) t[k] += s_v[k][i];
    summary[0] = t[0];
    summary[1] = t[2] > 0.0 ? t[1] / t[2] : 0.0;   // ComputeMeanReprojectionError: 0 when no point has an error
    summary[2] = t[2];
    summary[3] = t[3];
  }
}

// ---- the triangulation-angle filter (base/reconstruction.cc:1600-1660), stage 2 of pcd_ba_filter_points --------
// thread = image: ProjectionCenterFromPose (base/pose.cc:164-171), the normalised quaternion conjugated and applied to
// -tvec; a zero quaternion counts as the identity, as in k_ba_obs_errors
__global__ __launch_bounds__(256) void k_ba_proj_centers(int I, const double* __restrict__ poses,
                                                         double* __restrict__ centers) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= I) return;
  double c[3];
  proj_center(poses + 7 * (size_t)i, c);
  centers[3 * (size_t)i] = c[0]; centers[3 * (size_t)i + 1] = c[1]; centers[3 * (size_t)i + 2] = c[2];
}

// thread = point, on what stage 1 (k_ba_filter_tracks) left in obs_erase / point_delete / point_error, all three
// required here.  A point stage 1 kept is kept as soon as one pair (i1, i2 < i1) of its SURVIVING elements, in ascending
// observation index, reaches min_angle; the centre of element i1 is loaded once, those of i2 come from the [I][3] table
// (24 KB at 1000 images: cache hits).  A point that no pair keeps is deleted: point_delete = 1, every obs_erase = 1,
// point_error = -1.  The three summary partials of the workgroup are written anew from the final state (elements stage 1
// filtered, plus ONE per point deleted here; the error of every point still alive), by k_ba_filter_tracks' fixed-order
// reduction, so k_ba_filter_summary serves both filters.
// Cost of the pair loop: quadratic in the survivors, but only for a point that ends deleted -- a kept point leaves at its
// first sufficient pair, for a triangulated point usually the first.  The longest track of workload M has 30 elements:
// 435 pairs of ~60 fp64 operations, one sqrt, one division and one acos, ~0.2 M cycles (~0.1 ms) for the one thread if
// every pair fails; its wavefront's other lanes have left by then.  Such a point needs 30 cameras within 1.5 degrees of
// each other as seen from it; the kernel has no wavefront-per-track path for it.  Measured at workload M with the stage
// on all 979 k tracks, 36 k of them deleted after all their pairs: 0.18 ms for the stage (profiles/ba_filter_probe.txt).
__global__ __launch_bounds__(256) void k_ba_filter_tri_angle(int P, const uint32_t* __restrict__ pt_start,
                                                             const uint32_t* __restrict__ pt_list,
                                                             const int* __restrict__ obs_image,
                                                             const double* __restrict__ centers,
                                                             const double* __restrict__ points, double min_angle,
                                                             uint8_t* __restrict__ obs_erase, uint8_t* __restrict__ point_delete,
                                                             double* __restrict__ point_error, double* __restrict__ partial) {
  __shared__ double s_f[4], s_e[4], s_n[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double filtered = 0.0, esum = 0.0, valid = 0.0;
  if (p < P) {
    const uint32_t b = pt_start[p], len = pt_start[p + 1] - b;
    if (point_delete[p]) {
      filtered = (double)len;
    } else {
      const double X[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
      uint32_t ndel = 0;
      bool keep = false;
      for (uint32_t j1 = 0; j1 < len; ++j1) {
        const uint32_t o1 = pt_list[b + j1];
        if (obs_erase[o1]) { ++ndel; continue; }
        if (keep) continue;   // only the count of stage 1's erasures is still wanted
        const double* cp1 = centers + 3 * (size_t)obs_image[o1];
        const double c1[3] = {cp1[0], cp1[1], cp1[2]};
        for (uint32_t j2 = 0; j2 < j1 && !keep; ++j2) {
          const uint32_t o2 = pt_list[b + j2];
          if (obs_erase[o2]) continue;
          const double* cp2 = centers + 3 * (size_t)obs_image[o2];
          const double c2[3] = {cp2[0], cp2[1], cp2[2]};
          keep = tri_angle(c1, c2, X) >= min_angle;
        }
      }
      if (keep) {
        filtered = (double)ndel; esum = point_error[p]; valid = 1.0;
      } else {
        filtered = (double)ndel + 1.0;   // the reference counts points here, not elements
        point_delete[p] = 1;
        point_error[p] = -1.0;
        for (uint32_t j = 0; j < len; ++j) obs_erase[pt_list[b + j]] = 1;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    filtered += __shfl_xor(filtered, off); esum += __shfl_xor(esum, off); valid += __shfl_xor(valid, off);
  }
  if (lane == 0) { s_f[wave] = filtered; s_e[wave] = esum; s_n[wave] = valid; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[3 * (size_t)blockIdx.x] = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
    partial[3 * (size_t)blockIdx.x + 1] = (s_e[0] + s_e[1]) + (s_e[2] + s_e[3]);
    partial[3 * (size_t)blockIdx.x + 2] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
  }
}

// rows of the variable-pose observations, packed: thread = 16-byte unit of an output row
template <int N>   // doubles per row
__global__ void k_pack_rows(const double* __restrict__ in, const uint32_t* __restrict__ vobs, uint64_t nrows,
                            double* __restrict__ out) {
  const uint64_t u = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  constexpr int UPR = N / 2;
  if (u >= nrows * UPR) return;
  const uint64_t r = u / UPR;
  const int k = (int)(u - r * UPR);
  reinterpret_cast<double2*>(out)[u] = reinterpret_cast<const double2*>(in + (size_t)vobs[r] * N)[k];
}

}  // namespace pcd

using namespace pcd;

// kernel dispatch on the (uniform) camera model; the five common models are compiled in
#define PCD_BA_DISPATCH(MODELVAR, ...)                            \
  switch (MODELVAR) {                                             \
    case 0: { constexpr int M = 0; __VA_ARGS__; } break;          \
    case 1: { constexpr int M = 1; __VA_ARGS__; } break;          \
    case 2: { constexpr int M = 2; __VA_ARGS__; } break;          \
    case 3: { constexpr int M = 3; __VA_ARGS__; } break;          \
    case 4: { constexpr int M = 4; __VA_ARGS__; } break;          \
    default: { constexpr int M = -1; __VA_ARGS__; } break;        \
  }

// the same with the shared-camera flag of the handle as a second template argument SH
#define PCD_BA_DISPATCH_CAM(MODELVAR, SHAREDVAR, ...)                                  \
  if (SHAREDVAR) { constexpr bool SH = true; PCD_BA_DISPATCH(MODELVAR, __VA_ARGS__) }  \
  else { constexpr bool SH = false; PCD_BA_DISPATCH(MODELVAR, __VA_ARGS__) }

// One block of a blocks route's pinned result: n doubles from src to the cursor h, which moves past them; slot points
// at the copy (nullptr when the block is empty)
static hipError_t down(double*& h, hipStream_t s, uint64_t& bytes_d2h, const double*& slot, const double* src, size_t n) {
  slot = n ? h : nullptr;
  const hipError_t e = n ? hipMemcpyAsync(h, src, n * sizeof(double), hipMemcpyDeviceToHost, s) : hipSuccess;
  h += n;
  bytes_d2h += n * sizeof(double);
  return e;
}

// The launches pcd_ba_evaluate_device and ba_normal_equations share.  Point pass: cost_blocks(b, true) cost partials
static void launch_points(const pcd_ba* b, const BaDev& d, double* Hpt, double* gpt, hipStream_t s) {
  PCD_BA_DISPATCH_CAM(b->uniform_model, d.shared_cam >= 0,
                      hipLaunchKernelGGL((k_ba_points<M, true, SH>), dim3(cost_blocks(b, true)), dim3(256), 0, s, d, Hpt, gpt,
                                         b->cost_partial.p));
}
// Image pass and its reduction; W (non-null) rides on the image pass, in the order d.img_obs gives.  img_partial is reserved.
static void launch_images(const pcd_ba* b, const BaDev& d, double* Himg, double* gimg, double* W, hipStream_t s) {
  if (b->nseg) {
    PCD_BA_DISPATCH(b->uniform_model,
                    if (W) hipLaunchKernelGGL((k_ba_images<M, true>), dim3(b->nseg), dim3(256), 0, s, d, b->img_partial.p, W);
                    else hipLaunchKernelGGL((k_ba_images<M, false>), dim3(b->nseg), dim3(256), 0, s, d, b->img_partial.p, W));
  }
  hipLaunchKernelGGL(k_ba_images_reduce, dim3(div_up(b->I, 2)), dim3(64), 0, s, d, b->img_partial.p, Himg, gimg);
}

pcd_status pcd::ba_normal_equations(pcd_ba* b, const uint32_t* w_order, double* Hpt, double* gpt, double* cost,
                                    double* Himg, double* gimg, double* W, hipStream_t s) {
  PCD_TRY(b->img_partial.reserve(27 * (size_t)std::max(b->nseg, 1u)));
  BaDev d = b->dev();
  launch_points(b, d, Hpt, gpt, s);
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kSumThreads), 0, s, b->cost_partial.p, (int)cost_blocks(b, true), cost);
  if (w_order) d.img_obs = w_order;   // only the image pass reads it
  launch_images(b, d, Himg, gimg, W, s);
  return PCD_OK;
}

extern "C" {

pcd_status pcd_ba_set_parameters(pcd_ba* b, const double* poses, const double* points) {
  PCD_REQUIRE(b, "null handle");
  PCD_HIP_TRY(hipSetDevice(b->device));
  if (poses) PCD_HIP_TRY(hipMemcpy(b->poses.p, poses, 7 * (size_t)b->I * sizeof(double), hipMemcpyHostToDevice));
  if (points) PCD_HIP_TRY(hipMemcpy(b->points.p, points, 3 * (size_t)b->P * sizeof(double), hipMemcpyHostToDevice));
  return PCD_OK;
}

pcd_status pcd_ba_set_parameters_device(pcd_ba* b, const double* d_poses, const double* d_points, void* stream) {
  PCD_TRY(require_device(b ? b->device : 0));
  PCD_REQUIRE(b, "null handle");
  PCD_REFUSE_CAPTURE(stream);
  PCD_HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  if (d_poses && d_poses != b->poses.p)
    PCD_HIP_TRY(hipMemcpyAsync(b->poses.p, d_poses, 7 * (size_t)b->I * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (d_points && d_points != b->points.p)
    PCD_HIP_TRY(hipMemcpyAsync(b->points.p, d_points, 3 * (size_t)b->P * sizeof(double), hipMemcpyDeviceToDevice, s));
  return PCD_OK;
}

pcd_status pcd_ba_get_parameters(pcd_ba* b, double* poses, double* points) {
  PCD_TRY(require_device(b ? b->device : 0));
  PCD_REQUIRE(b, "null handle");
  PCD_HIP_TRY(hipSetDevice(b->device));
  if (poses) PCD_HIP_TRY(hipMemcpy(poses, b->poses.p, 7 * (size_t)b->I * sizeof(double), hipMemcpyDeviceToHost));
  if (points) PCD_HIP_TRY(hipMemcpy(points, b->points.p, 3 * (size_t)b->P * sizeof(double), hipMemcpyDeviceToHost));
  return PCD_OK;
}

pcd_status pcd_ba_set_camera_parameters(pcd_ba* b, const double* cam_params) {
  PCD_REQUIRE(b && cam_params, "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  PCD_HIP_TRY(hipMemcpy(b->cam_params.p, cam_params, b->cam_params_len * sizeof(double), hipMemcpyHostToDevice));
  b->h_cam_params.assign(cam_params, cam_params + b->cam_params_len);   // pcd_ba_project_lidar_device reads the mirror
  return PCD_OK;
}

pcd_status pcd_ba_device_parameters(pcd_ba* b, double** d_poses, double** d_points) {
  PCD_REQUIRE(b, "null handle");
  if (d_poses) *d_poses = b->poses.p;
  if (d_points) *d_points = b->points.p;
  return PCD_OK;
}

pcd_status pcd_ba_evaluate_device(pcd_ba* b, const pcd_ba_out* o, void* stream) {
  PCD_REQUIRE(b && o, "null pointer");
  PCD_REFUSE_CAPTURE(stream);
  PCD_HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const BaDev d = b->dev();
  const int model = b->uniform_model;
  if (o->cost || o->H_pt || o->g_pt) {
    const bool want_blocks = o->H_pt || o->g_pt;
    const unsigned blocks = cost_blocks(b, want_blocks);
    {
      ScopedKernelTimer t(want_blocks ? "ba_points" : "ba_points_cost", s);
      if (want_blocks) {
        launch_points(b, d, o->H_pt, o->g_pt, s);
      } else {
        PCD_BA_DISPATCH_CAM(model, d.shared_cam >= 0,
                            hipLaunchKernelGGL((k_ba_cost<M, SH>), dim3(blocks), dim3(256), 0, s, d, b->cost_partial.p));
      }
    }
    if (o->cost) hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kSumThreads), 0, s, b->cost_partial.p, (int)blocks, o->cost);
  }
  // W rides on the image pass when that runs anyway (normal-equation mode); otherwise the raw kernel fills it
  const bool w_fused = o->W && (o->H_img || o->g_img) && b->O;
  if (o->H_img || o->g_img) {
    PCD_TRY(b->img_partial.reserve(27 * (size_t)std::max(b->nseg, 1u)));
    ScopedKernelTimer t(w_fused ? "ba_images_w" : "ba_images", s);
    launch_images(b, d, o->H_img, o->g_img, w_fused ? o->W : nullptr, s);
  }
  double* const W_raw = w_fused ? nullptr : o->W;
  if ((o->residuals || o->jac_q || o->jac_t || o->jac_X || W_raw) && b->O) {
    ScopedKernelTimer t("ba_raw", s);
    PCD_BA_DISPATCH_CAM(model, d.shared_cam >= 0,
                        hipLaunchKernelGGL((k_ba_raw<M, SH>), dim3(div_up(b->O, 256)), dim3(256), 0, s, d, o->residuals,
                                           o->jac_q, o->jac_t, o->jac_X, W_raw));
  }
  if (o->jac_cam && b->O) {
    ScopedKernelTimer t("ba_cam_jac", s);
    PCD_BA_DISPATCH(model, hipLaunchKernelGGL((k_ba_cam_jac<M>), dim3(div_up(b->O, 256)), dim3(256), 0, s, d, o->jac_cam));
  }
  if (o->H_cam || o->g_cam || o->E_cam) {
    PCD_TRY(b->cam_partial.reserve((size_t)b->I * cam_ne(PCD_CAM_JAC_STRIDE)));
    ScopedKernelTimer t("ba_cameras", s);
    PCD_BA_DISPATCH(model, hipLaunchKernelGGL((k_ba_cameras<M>), dim3(b->I), dim3(256), 0, s, d, b->cam_partial.p));
    hipLaunchKernelGGL(k_ba_cameras_reduce, dim3(b->C), dim3(256), 0, s, d, b->cam_partial.p, o->H_cam, o->g_cam,
                       o->E_cam);
  }
  if (o->W_cam && b->O) {
    ScopedKernelTimer t("ba_cam_w", s);
    PCD_BA_DISPATCH(model, hipLaunchKernelGGL((k_ba_cam_w<M>), dim3(div_up(b->O, 256)), dim3(256), 0, s, d, o->W_cam));
  }
  if ((o->residuals || o->jac_lidar) && b->L) {
    ScopedKernelTimer t("ba_lidar_raw", s);
    hipLaunchKernelGGL(k_ba_lidar_raw, dim3(div_up(b->L, 256)), dim3(256), 0, s, d, o->residuals, o->jac_lidar);
  }
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

pcd_status pcd_ba_observation_errors_device(pcd_ba* b, double* d_sq_err, double* d_depth, void* stream) {
  PCD_REQUIRE(b, "null handle");
  PCD_REFUSE_CAPTURE(stream);
  if (!b->O || (!d_sq_err && !d_depth)) return PCD_OK;
  PCD_HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const BaDev d = b->dev();
  ScopedKernelTimer t("ba_obs_errors", s);
  PCD_BA_DISPATCH_CAM(b->uniform_model, d.shared_cam >= 0,
                      hipLaunchKernelGGL((k_ba_obs_errors<M, SH>), dim3(div_up(b->O, 256)), dim3(256), 0, s, d, d_sq_err,
                                         d_depth));
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

pcd_status pcd_ba_observation_errors(pcd_ba* b, double* sq_err, double* depth) {
  PCD_REQUIRE(b, "null handle");
  if (!b->O) return PCD_OK;
  PCD_HIP_TRY(hipSetDevice(b->device));
  PCD_TRY(b->f_sq.reserve(b->O)); PCD_TRY(b->f_depth.reserve(b->O));
  PCD_TRY(pcd_ba_observation_errors_device(b, sq_err ? b->f_sq.p : nullptr, depth ? b->f_depth.p : nullptr, nullptr));
  if (sq_err) PCD_HIP_TRY(hipMemcpy(sq_err, b->f_sq.p, b->O * sizeof(double), hipMemcpyDeviceToHost));
  if (depth) PCD_HIP_TRY(hipMemcpy(depth, b->f_depth.p, b->O * sizeof(double), hipMemcpyDeviceToHost));
  return PCD_OK;
}

pcd_status pcd_ba_filter_tracks_device(pcd_ba* b, double max_reproj_error, const pcd_ba_filter_out* o, void* stream) {
  PCD_REQUIRE(b && o, "null pointer");
  PCD_REFUSE_CAPTURE(stream);
  PCD_HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const uint64_t O = b->O;
  const int nbp = (int)div_up((uint64_t)b->P, 256), nbo = (int)div_up(std::max<uint64_t>(O, 1), 256);
  PCD_TRY(b->f_sq.reserve(std::max<uint64_t>(O, 1))); PCD_TRY(b->f_depth.reserve(std::max<uint64_t>(O, 1)));
  PCD_TRY(b->f_part.reserve(3 * (size_t)nbp + nbo + 4));
  if (O) PCD_TRY(pcd_ba_observation_errors_device(b, b->f_sq.p, b->f_depth.p, s));
  ScopedKernelTimer t("ba_filter_tracks", s);
  double* part3 = b->f_part.p, *part1 = b->f_part.p + 3 * (size_t)nbp;
  hipLaunchKernelGGL(k_ba_filter_tracks, dim3(nbp), dim3(256), 0, s, b->P, b->pt_obs_start.p, b->pt_obs_list.p, b->f_sq.p,
                     max_reproj_error * max_reproj_error, o->obs_erase, o->point_delete, o->point_error, part3);
  hipLaunchKernelGGL(k_ba_negative_depth, dim3(nbo), dim3(256), 0, s, O, b->f_depth.p, o->obs_negative_depth, part1);
  if (o->summary) hipLaunchKernelGGL(k_ba_filter_summary, dim3(1), dim3(256), 0, s, part3, nbp, part1, nbo, o->summary);
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

pcd_status pcd_ba_filter_tracks(pcd_ba* b, double max_reproj_error, const pcd_ba_filter_out* o) {
  PCD_REQUIRE(b && o, "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  const size_t O = b->O, P = (size_t)b->P;
  PCD_TRY(b->f_u8.reserve(2 * O + P + 1)); PCD_TRY(b->f_summary.reserve(P + 4));
  pcd_ba_filter_out d{};
  d.obs_erase = o->obs_erase ? b->f_u8.p : nullptr;
  d.obs_negative_depth = o->obs_negative_depth ? b->f_u8.p + O : nullptr;
  d.point_delete = o->point_delete ? b->f_u8.p + 2 * O : nullptr;
  d.point_error = o->point_error ? b->f_summary.p + 4 : nullptr;
  d.summary = o->summary ? b->f_summary.p : nullptr;
  PCD_TRY(pcd_ba_filter_tracks_device(b, max_reproj_error, &d, nullptr));
  if (o->obs_erase && O) PCD_HIP_TRY(hipMemcpy(o->obs_erase, d.obs_erase, O, hipMemcpyDeviceToHost));
  if (o->obs_negative_depth && O) PCD_HIP_TRY(hipMemcpy(o->obs_negative_depth, d.obs_negative_depth, O, hipMemcpyDeviceToHost));
  if (o->point_delete) PCD_HIP_TRY(hipMemcpy(o->point_delete, d.point_delete, P, hipMemcpyDeviceToHost));
  if (o->point_error) PCD_HIP_TRY(hipMemcpy(o->point_error, d.point_error, P * sizeof(double), hipMemcpyDeviceToHost));
  if (o->summary) PCD_HIP_TRY(hipMemcpy(o->summary, d.summary, 4 * sizeof(double), hipMemcpyDeviceToHost));
  PCD_HIP_TRY(hipDeviceSynchronize());
  return PCD_OK;
}

void pcd_ba_filter_opts_default(pcd_ba_filter_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->max_reproj_error = 8.0;
  o->min_tri_angle_deg = 1.5;
}

pcd_status pcd_ba_filter_points_device(pcd_ba* b, const pcd_ba_filter_opts* opts, const pcd_ba_filter_out* o, void* stream) {
  PCD_REQUIRE(b && opts && o, "null pointer");
  PCD_REFUSE_CAPTURE(stream);
  if (!(opts->min_tri_angle_deg > 0.0)) return pcd_ba_filter_tracks_device(b, opts->max_reproj_error, o, stream);
  PCD_HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t O = b->O, P = (size_t)b->P;
  // stage 2 reads and rewrites all three per-track outputs of stage 1: those the caller left NULL go to scratch
  pcd_ba_filter_out d = *o;
  d.summary = nullptr;
  if (!d.obs_erase || !d.point_delete) {
    PCD_TRY(b->f_tri_u8.reserve(O + P + 1));
    if (!d.obs_erase) d.obs_erase = b->f_tri_u8.p;
    if (!d.point_delete) d.point_delete = b->f_tri_u8.p + O;
  }
  if (!d.point_error) { PCD_TRY(b->f_tri_err.reserve(at_least_1(P))); d.point_error = b->f_tri_err.p; }
  PCD_TRY(b->f_centers.reserve(3 * at_least_1((size_t)b->I)));
  PCD_TRY(pcd_ba_filter_tracks_device(b, opts->max_reproj_error, &d, stream));
  ScopedKernelTimer t("ba_filter_tri_angle", s);
  const int nbp = (int)div_up((uint64_t)b->P, 256), nbo = (int)div_up(std::max<uint64_t>(O, 1), 256);
  double* part3 = b->f_part.p, *part1 = b->f_part.p + 3 * (size_t)nbp;   // as stage 1 laid them out
  const double min_angle = opts->min_tri_angle_deg * 0.0174532925199432954743716805978692718781530857086181640625;   // DegToRad
  hipLaunchKernelGGL(k_ba_proj_centers, dim3(div_up((uint64_t)b->I, 256)), dim3(256), 0, s, b->I, b->poses.p, b->f_centers.p);
  hipLaunchKernelGGL(k_ba_filter_tri_angle, dim3(nbp), dim3(256), 0, s, b->P, b->pt_obs_start.p, b->pt_obs_list.p,
                     b->obs_image.p, b->f_centers.p, b->points.p, min_angle, d.obs_erase, d.point_delete, d.point_error, part3);
  if (o->summary) hipLaunchKernelGGL(k_ba_filter_summary, dim3(1), dim3(256), 0, s, part3, nbp, part1, nbo, o->summary);
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

pcd_status pcd_ba_filter_points(pcd_ba* b, const pcd_ba_filter_opts* opts, const pcd_ba_filter_out* o) {
  PCD_REQUIRE(b && opts && o, "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  const size_t O = b->O, P = (size_t)b->P;
  PCD_TRY(b->f_u8.reserve(2 * O + P + 1)); PCD_TRY(b->f_summary.reserve(P + 4));
  pcd_ba_filter_out d{};
  d.obs_erase = o->obs_erase ? b->f_u8.p : nullptr;
  d.obs_negative_depth = o->obs_negative_depth ? b->f_u8.p + O : nullptr;
  d.point_delete = o->point_delete ? b->f_u8.p + 2 * O : nullptr;
  d.point_error = o->point_error ? b->f_summary.p + 4 : nullptr;
  d.summary = o->summary ? b->f_summary.p : nullptr;
  PCD_TRY(pcd_ba_filter_points_device(b, opts, &d, nullptr));
  if (o->obs_erase && O) PCD_HIP_TRY(hipMemcpy(o->obs_erase, d.obs_erase, O, hipMemcpyDeviceToHost));
  if (o->obs_negative_depth && O) PCD_HIP_TRY(hipMemcpy(o->obs_negative_depth, d.obs_negative_depth, O, hipMemcpyDeviceToHost));
  if (o->point_delete) PCD_HIP_TRY(hipMemcpy(o->point_delete, d.point_delete, P, hipMemcpyDeviceToHost));
  if (o->point_error) PCD_HIP_TRY(hipMemcpy(o->point_error, d.point_error, P * sizeof(double), hipMemcpyDeviceToHost));
  if (o->summary) PCD_HIP_TRY(hipMemcpy(o->summary, d.summary, 4 * sizeof(double), hipMemcpyDeviceToHost));
  PCD_HIP_TRY(hipDeviceSynchronize());
  return PCD_OK;
}

// h_pose_row after pcd_ba_remove_observations_device: the walk of build_pose_rows (ba_build.hip) over the device's
// obs_image, read back once.  The blocking copy below is on the null stream while the removal wrote obs_image on the
// caller's: it reads finished data only because the removal synchronises that stream (after k_edit_compact_obs) before
// it returns.  A removal without that synchronisation would have to order this copy behind its stream.
static pcd_status ba_refresh_pose_rows(pcd_ba* b) {
  if (!b->pose_row_stale) return PCD_OK;
  const size_t O = b->O;
  std::vector<int> img(O);
  std::vector<uint8_t> cpose((size_t)b->I, 0);
  if (O) PCD_HIP_TRY(hipMemcpy(img.data(), b->obs_image.p, O * sizeof(int), hipMemcpyDeviceToHost));
  if (b->has_cpose) PCD_HIP_TRY(hipMemcpy(cpose.data(), b->image_const_pose.p, (size_t)b->I, hipMemcpyDeviceToHost));
  b->h_pose_row.assign(O, 0xFFFFFFFFu);
  uint32_t row = 0;
  for (size_t o = 0; o < O; ++o)
    if (!cpose[img[o]]) b->h_pose_row[o] = row++;
  b->pose_row_stale = false;
  return PCD_OK;
}

pcd_status pcd_ba_evaluate_blocks(pcd_ba* b, int want_jacobians, int want_jac_cam, pcd_ba_blocks* out) {
  PCD_REQUIRE(b && out, "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  std::memset(out, 0, sizeof *out);
  PCD_TRY(ba_refresh_pose_rows(b));
  const uint64_t O = b->O, L = b->L, V = b->n_pose_rows;
  const bool packed = V != O;
  const size_t n_res = 2 * O + L, n_jq = want_jacobians ? 8 * V : 0, n_jt = want_jacobians ? 6 * V : 0,
               n_jx = want_jacobians ? 6 * O : 0, n_jl = want_jacobians ? 3 * L : 0,
               n_jc = (want_jacobians && want_jac_cam) ? 2 * (size_t)PCD_CAM_JAC_STRIDE * O : 0;
  PCD_TRY(b->h_blocks.reserve(n_res + n_jq + n_jt + n_jx + n_jl + n_jc + 2));
  PCD_TRY(b->o_res.reserve(std::max<size_t>(n_res, 1)));
  pcd_ba_out d{};
  d.residuals = b->o_res.p;
  if (want_jacobians) {
    PCD_TRY(b->o_jq.reserve(std::max<size_t>(8 * O, 1))); PCD_TRY(b->o_jt.reserve(std::max<size_t>(6 * O, 1)));
    PCD_TRY(b->o_jx.reserve(std::max<size_t>(6 * O, 1))); PCD_TRY(b->o_jl.reserve(std::max<size_t>(3 * L, 1)));
    d.jac_q = b->o_jq.p; d.jac_t = b->o_jt.p; d.jac_X = b->o_jx.p; d.jac_lidar = b->o_jl.p;
    if (n_jc) { PCD_TRY(b->o_jc.reserve(n_jc)); d.jac_cam = b->o_jc.p; }
    if (packed) { PCD_TRY(b->p_jq.reserve(std::max<size_t>(8 * V, 1))); PCD_TRY(b->p_jt.reserve(std::max<size_t>(6 * V, 1))); }
  }
  hipStream_t s = nullptr;
  PCD_TRY(pcd_ba_evaluate_device(b, &d, s));
  const double *src_jq = b->o_jq.p, *src_jt = b->o_jt.p;
  if (want_jacobians && packed && V) {
    hipLaunchKernelGGL(k_pack_rows<8>, dim3(div_up(V * 4, 256)), dim3(256), 0, s, b->o_jq.p, b->vobs.p, V, b->p_jq.p);
    hipLaunchKernelGGL(k_pack_rows<6>, dim3(div_up(V * 3, 256)), dim3(256), 0, s, b->o_jt.p, b->vobs.p, V, b->p_jt.p);
    src_jq = b->p_jq.p; src_jt = b->p_jt.p;
  }
  double* h = b->h_blocks.p;
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->residuals, b->o_res.p, n_res));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->jac_q, src_jq, n_jq));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->jac_t, src_jt, n_jt));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->jac_X, b->o_jx.p, n_jx));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->jac_lidar, b->o_jl.p, n_jl));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->jac_cam, b->o_jc.p, n_jc));
  PCD_HIP_TRY(hipStreamSynchronize(s));
  out->pose_row = b->h_pose_row.data();
  out->num_pose_rows = V;
  return PCD_OK;
}

pcd_status pcd_ba_evaluate_blocks_compact(pcd_ba* b, int want_jacobians, int want_jac_cam, pcd_ba_blocks_compact* out) {
  PCD_TRY(require_device(b ? b->device : 0));
  PCD_REQUIRE(b && out, "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  std::memset(out, 0, sizeof *out);
  const uint64_t O = b->O, L = b->L;
  const int cs = b->cam_stride;
  out->cam_stride = cs;
  const size_t n_res = want_jacobians ? 0 : 2 * O, n_rec = want_jacobians ? 8 * O : 0, n_jl = want_jacobians ? 3 * L : 0,
               n_jc = (want_jacobians && want_jac_cam) ? 2 * (size_t)cs * O : 0;
  PCD_TRY(b->h_blocks.reserve(n_res + n_rec + L + n_jl + n_jc + 2));
  PCD_TRY(b->o_res.reserve(std::max<size_t>(2 * O + L, 1)));   // the LiDAR residuals sit behind the 2 O reprojection slots
  hipStream_t s = nullptr;
  if (want_jacobians) {
    PCD_TRY(b->o_rec.reserve(std::max<size_t>(n_rec, 1))); PCD_TRY(b->o_jl.reserve(std::max<size_t>(n_jl, 1)));
    const BaDev d = b->dev();
    if (O) {
      ScopedKernelTimer t("ba_raw_compact", s);
      PCD_BA_DISPATCH_CAM(b->uniform_model, d.shared_cam >= 0,
                          hipLaunchKernelGGL((k_ba_raw_compact<M, SH>), dim3(div_up(O, 256)), dim3(256), 0, s, d, b->o_rec.p));
    }
    if (L) {
      ScopedKernelTimer t("ba_lidar_raw", s);
      hipLaunchKernelGGL(k_ba_lidar_raw, dim3(div_up(L, 256)), dim3(256), 0, s, d, b->o_res.p, b->o_jl.p);
    }
    PCD_HIP_TRY(hipGetLastError());
    if (n_jc) {
      PCD_TRY(b->o_jc.reserve(2 * (size_t)PCD_CAM_JAC_STRIDE * O)); PCD_TRY(b->p_jc.reserve(n_jc));
      pcd_ba_out dc{};
      dc.jac_cam = b->o_jc.p;
      PCD_TRY(pcd_ba_evaluate_device(b, &dc, s));   // k_ba_cam_jac alone
      ScopedKernelTimer t("ba_pack_cam_jac", s);
      hipLaunchKernelGGL(k_ba_pack_cam_jac, dim3(div_up(n_jc, 256)), dim3(256), 0, s, b->o_jc.p, 2 * O, cs, b->p_jc.p);
      PCD_HIP_TRY(hipGetLastError());
    }
  } else {   // a trial step: the residual rows of k_ba_raw and k_ba_lidar_raw, nothing else
    pcd_ba_out dr{};
    dr.residuals = b->o_res.p;
    PCD_TRY(pcd_ba_evaluate_device(b, &dr, s));
  }
  double* h = b->h_blocks.p;
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->residuals, b->o_res.p, n_res));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->records, b->o_rec.p, n_rec));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->lidar_residuals, b->o_res.p + 2 * O, L));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->jac_lidar, b->o_jl.p, n_jl));
  PCD_HIP_TRY(down(h, s, out->bytes_d2h, out->jac_cam, b->p_jc.p, n_jc));
  PCD_HIP_TRY(hipStreamSynchronize(s));
  return PCD_OK;
}

pcd_status pcd_ba_evaluate(pcd_ba* b, const pcd_ba_out* o) {
  PCD_REQUIRE(b && o, "null pointer");
  PCD_HIP_TRY(hipSetDevice(b->device));
  pcd_ba_out d{};
  struct Item { double* host; DevBuf<double>* buf; size_t n; double** slot; };
  Item items[] = {
      {o->cost, &b->cost, 1, &d.cost},
      {o->residuals, &b->o_res, 2 * b->O + b->L, &d.residuals},
      {o->jac_q, &b->o_jq, 8 * b->O, &d.jac_q},
      {o->jac_t, &b->o_jt, 6 * b->O, &d.jac_t},
      {o->jac_X, &b->o_jx, 6 * b->O, &d.jac_X},
      {o->jac_lidar, &b->o_jl, 3 * b->L, &d.jac_lidar},
      {o->H_img, &b->o_himg, 36 * (size_t)b->I, &d.H_img},
      {o->g_img, &b->o_gimg, 6 * (size_t)b->I, &d.g_img},
      {o->H_pt, &b->o_hpt, 9 * (size_t)b->P, &d.H_pt},
      {o->g_pt, &b->o_gpt, 3 * (size_t)b->P, &d.g_pt},
      {o->W, &b->o_w, 18 * b->O, &d.W},
      {o->jac_cam, &b->o_jc, 2 * PCD_CAM_JAC_STRIDE * b->O, &d.jac_cam},
      {o->H_cam, &b->o_hcam, (size_t)PCD_CAM_JAC_STRIDE * PCD_CAM_JAC_STRIDE * b->C, &d.H_cam},
      {o->g_cam, &b->o_gcam, (size_t)PCD_CAM_JAC_STRIDE * b->C, &d.g_cam},
      {o->E_cam, &b->o_ecam, (size_t)PCD_CAM_JAC_STRIDE * 6 * b->I, &d.E_cam},
      {o->W_cam, &b->o_wcam, (size_t)PCD_CAM_JAC_STRIDE * 3 * b->O, &d.W_cam},
  };
  for (auto& it : items)
    if (it.host) {
      PCD_TRY(it.buf->reserve(std::max<size_t>(it.n, 1)));
      *it.slot = it.buf->p;
    }
  PCD_TRY(pcd_ba_evaluate_device(b, &d, nullptr));
  for (auto& it : items)
    if (it.host && it.n) PCD_HIP_TRY(hipMemcpy(it.host, it.buf->p, it.n * sizeof(double), hipMemcpyDeviceToHost));
  PCD_HIP_TRY(hipDeviceSynchronize());
  return PCD_OK;
}

}  // extern "C"

// ba_lidar.hip -- the LiDAR terms of a BA handle rebuilt on the device: pcd_ba_set_lidar_device,
// pcd_ba_get_lidar / pcd_ba_lidar_device, pcd_ba_associate_lidar_device, pcd_ba_project_lidar_device.
// What build_lidar_layout (ba_build.hip) makes on the host from the caller's term list is made here from Q device rows,
// byte for byte: the terms (rows that pass the type / NaN rule, in ascending row order), the CSR point -> terms
// (ascending term number) and the first term of every track in the thread order of k_ba_points.  The passes:
//   k_lidar_flag     row -> kept?, and one record per workgroup: invalid rows, selected rows, terms of each type, and
//                    the first / last point and the order of the workgroup's kept rows
//   exclusive_sum    kept -> term number
//   k_lidar_status   the workgroup records merged in workgroup order -> one record; read back with the term count (the
//                    ONE synchronisation: the count sizes the buffers and grids below)
//   k_lidar_compact  kept rows -> terms
//   sort_pairs       (point, term), stable, only when the terms' points are not already non-decreasing
//   k_lidar_bounds   CSR bounds of every point by bisection of the sorted points
//   k_lidar_tracks   thread of k_ba_points -> number of terms and the first of them, component-major
// No atomics; every order is that of the rows: nothing depends on the launch geometry.  The new terms are a BaTerms
// (ba_handle.h) built in pcd_ba::lidar_next and swapped in at the end, group by group; a refusal returns before the swap.
// pcd_ba_project_lidar_device makes its rows here too, in front of the same rebuild: the projector (proj.h)
// writes found / lidar6 per observation, k_lidar_proj_pick picks per track, k_lidar_proj_merge folds the Proj rows into the
// association's, k_lidar_proj_count* sum the counts of the info record.
#include <cmath>

#include "ba_handle.h"
#include "cloud.h"
#include "prim.h"
#include "proj.h"

namespace pcd {

constexpr uint32_t kNoPoint = 0xFFFFFFFFu;
// per workgroup of k_lidar_flag, and their merge in row order
struct LidarPart {
  uint32_t bad, selected, ntype[3];   // invalid rows; selected rows; kept rows of type 1, 2, 3
  uint32_t first_pt, last_pt;         // point of the first / last kept row, kNoPoint: none
  uint32_t unsorted;                  // some kept row's point is below that of the kept row before it
};
constexpr int kPartWords = sizeof(LidarPart) / sizeof(uint32_t);
// the record the host reads: the merged LidarPart, then the number of terms
constexpr int kStatusWords = kPartWords + 1;

__device__ __forceinline__ LidarPart part_empty() {
  LidarPart p;
  p.bad = p.selected = p.ntype[0] = p.ntype[1] = p.ntype[2] = 0;
  p.first_pt = p.last_pt = kNoPoint;
  p.unsorted = 0;
  return p;
}
// a: rows before those of b
__device__ __forceinline__ LidarPart part_merge(const LidarPart& a, const LidarPart& b) {
  LidarPart p;
  p.bad = a.bad + b.bad;
  p.selected = a.selected + b.selected;
  for (int k = 0; k < 3; ++k) p.ntype[k] = a.ntype[k] + b.ntype[k];
  p.first_pt = a.first_pt != kNoPoint ? a.first_pt : b.first_pt;
  p.last_pt = b.last_pt != kNoPoint ? b.last_pt : a.last_pt;
  p.unsorted = a.unsorted | b.unsorted | ((a.last_pt != kNoPoint && b.first_pt != kNoPoint && a.last_pt > b.first_pt) ? 1u : 0u);
  return p;
}

// One row: its record as a LidarPart of one row, and whether it is kept.  A point outside [0, P) or a type above 3 is
// invalid in any row; an unselected row counts as type 0 behind that test.
__global__ __launch_bounds__(256) void k_lidar_flag(uint32_t Q, int P, const int32_t* __restrict__ point,
                                                    const uint8_t* __restrict__ type, const double* __restrict__ abcd,
                                                    const uint8_t* __restrict__ select, uint32_t* __restrict__ flag,
                                                    LidarPart* __restrict__ part) {
  __shared__ LidarPart s_row[256];
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  LidarPart r = part_empty();
  if (q < Q) {
    const int p = point ? point[q] : (int)q;
    uint32_t t = type[q];
    r.bad = (p < 0 || p >= P || t > 3u) ? 1u : 0u;
    const bool sel = !select || select[q] != 0;
    r.selected = sel ? 1u : 0u;
    if (!sel) t = 0;
    bool keep = t != 0 && !r.bad;
    if (keep) {
      const double* v = abcd + 4 * (size_t)q;   // the caller's rows: no alignment beyond a double's is assumed
      keep = !(isnan(v[0]) || isnan(v[1]) || isnan(v[2]) || isnan(v[3]));   // optim/bundle_adjustment.cc:1005-1009
    }
    if (keep) {
      r.ntype[t - 1] = 1;
      r.first_pt = r.last_pt = (uint32_t)p;
    }
    flag[q] = keep ? 1u : 0u;
  }
  s_row[threadIdx.x] = r;
  __syncthreads();
  // merge in row order: a tree over adjacent ranges keeps the order (part_merge is associative)
  for (int w = 1; w < 256; w <<= 1) {
    LidarPart m = r;
    const bool on = (threadIdx.x & (2 * w - 1)) == 0;
    if (on) m = part_merge(s_row[threadIdx.x], s_row[threadIdx.x + w]);
    __syncthreads();
    if (on) s_row[threadIdx.x] = m;
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = s_row[0];
}

// the nb workgroup records -> status[0 .. kPartWords), and the term count behind them.  One workgroup: thread t merges a
// contiguous run of records in order, then the 256 runs are merged in order.
__global__ __launch_bounds__(256) void k_lidar_status(uint32_t nb, const LidarPart* __restrict__ part, uint32_t Q,
                                                      const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                      uint32_t* __restrict__ status) {
  __shared__ LidarPart s_run[256];
  const uint32_t per = (nb + 255u) / 256u;
  LidarPart r = part_empty();
  for (uint32_t k = 0; k < per; ++k) {
    const uint32_t i = threadIdx.x * per + k;
    if (i < nb) r = part_merge(r, part[i]);
  }
  s_run[threadIdx.x] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    LidarPart m = s_run[0];
    for (int t = 1; t < 256; ++t) m = part_merge(m, s_run[t]);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&m);
    for (int k = 0; k < kPartWords; ++k) status[k] = w[k];
    status[kPartWords] = Q ? pos[Q - 1] + flag[Q - 1] : 0u;
  }
}

struct LidarWeights { double w[4]; };

// kept row q -> term pos[q].  ident[t] = t, the value array of the sort or, when the points are
// already in order, the term list itself.
__global__ __launch_bounds__(256) void k_lidar_compact(uint32_t Q, const uint32_t* __restrict__ flag,
                                                       const uint32_t* __restrict__ pos, const int32_t* __restrict__ point,
                                                       const uint8_t* __restrict__ type, const double* __restrict__ abcd,
                                                       const double* __restrict__ xyz, LidarWeights wt,
                                                       int* __restrict__ o_point, double* __restrict__ o_abcd,
                                                       double* __restrict__ o_w, uint8_t* __restrict__ o_type,
                                                       double* __restrict__ o_xyz, uint32_t* __restrict__ ident) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= Q || !flag[q]) return;
  const uint32_t t = pos[q];
  const uint8_t ty = type[q];
  o_point[t] = point ? point[q] : (int)q;
  for (int k = 0; k < 4; ++k) o_abcd[4 * (size_t)t + k] = abcd[4 * (size_t)q + k];
  o_w[t] = wt.w[ty & 3];
  o_type[t] = ty;
  for (int k = 0; k < 3; ++k) o_xyz[3 * (size_t)t + k] = xyz ? xyz[3 * (size_t)q + k] : 0.0;
  ident[t] = t;
}

// start[p] = number of terms whose point is below p, p = 0 .. P: bisection of the L sorted points
__global__ __launch_bounds__(256) void k_lidar_bounds(int P, uint32_t L, const uint32_t* __restrict__ sorted_pt,
                                                      uint32_t* __restrict__ start) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p > (uint32_t)P) return;
  uint32_t lo = 0, hi = L;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (sorted_pt[mid] < p) lo = mid + 1; else hi = mid;
  }
  start[p] = lo;
}

// thread t of k_ba_points (track order[t], -1: padding): how many terms its track has, and the first of them
__global__ __launch_bounds__(256) void k_lidar_tracks(uint32_t ntr, const int* __restrict__ order,
                                                      const uint32_t* __restrict__ start, const uint32_t* __restrict__ list,
                                                      const double* __restrict__ abcd, const double* __restrict__ w,
                                                      uint32_t* __restrict__ cnt, double* __restrict__ first) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= ntr) return;
  const int p = order[t];
  uint32_t n = 0;
  double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (p >= 0) {
    const uint32_t b = start[p];
    n = start[p + 1] - b;
    if (n) {
      const uint32_t l = list[b];
      const double4 v = *reinterpret_cast<const double4*>(abcd + 4 * (size_t)l);
      f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; f[4] = w[l];
    }
  }
  cnt[t] = n;
  for (int k = 0; k < 5; ++k) first[(size_t)k * ntr + t] = f[k];
}
void launch_lidar_tracks(const BaLayout& y, int nslices, const BaTerms& rows, BaTerms& next, hipStream_t s) {
  const uint32_t ntr = (uint32_t)nslices * 64u;
  hipLaunchKernelGGL(k_lidar_tracks, dim3(div_up(ntr, 256)), dim3(256), 0, s, ntr, y.pt_order.p, next.pt_lidar_start.p,
                     rows.pt_lidar_list.p, rows.lidar_abcd.p, rows.lidar_w.p, next.pt_lidar_cnt.p, next.pt_lidar_first.p);
}

// ---- pcd_ba_project_lidar_device ------------------------------------------------------------------------
// BundleAdjustmentConfig::MatchVariablePoint2LidarPoint (optim/bundle_adjustment.cc:288-350) for every track at once: one
// thread per point walks its observations in ascending observation index (the track CSR).  The projector wrote found /
// l6 in the CALLER's observation order (its read-out scatters through img_obs), so the walk reads the 48-byte candidate
// of observation o at l6 + 6 o: one hop from pt_obs_list, not o -> image-major position -> row.  An observation of an
// image that was not projected has found = 0.  Of several found observations of the point in ONE image only the first
// counts (std::map::insert, pcd_projection.cc:79): a candidate is skipped when an earlier found observation of the track
// has its image.  Double arithmetic in the order of shim/lidar_hip.h:326-346, no FMA (the unit is built without
// contraction); strict < from 360, so ties stay with the lowest observation and a NaN never wins.  No atomics.
__global__ __launch_bounds__(64) void k_lidar_proj_pick(int P, const uint32_t* __restrict__ pt_obs_start,
                                                        const uint32_t* __restrict__ pt_obs_list,
                                                        const int* __restrict__ obs_image, const uint8_t* __restrict__ found,
                                                        const double* __restrict__ l6, const double* __restrict__ points,
                                                        const uint8_t* __restrict__ mode, uint8_t* __restrict__ o_type,
                                                        double* __restrict__ o_abcd, double* __restrict__ o_xyz) {
  const uint32_t p = blockIdx.x * 64u + threadIdx.x;
  if (p >= (uint32_t)P) return;
  uint8_t ty = 0;
  double abcd[4] = {0.0, 0.0, 0.0, 0.0}, xyz[3] = {0.0, 0.0, 0.0};
  if (!mode || mode[p] == 1) {
    const double X[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
    const uint32_t kb = pt_obs_start[p], ke = pt_obs_start[p + 1];
    double angle = 360;
    double best[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = kb; k < ke; ++k) {
      const uint32_t o = pt_obs_list[k];
      if (!found[o]) continue;
      const int img = obs_image[o];
      bool dup = false;
      for (uint32_t k2 = kb; k2 < k && !dup; ++k2) {
        const uint32_t o2 = pt_obs_list[k2];
        dup = found[o2] && obs_image[o2] == img;
      }
      if (dup) continue;
      // the handle's own scratch: a 48-byte row is 16-byte aligned, three 16-byte loads
      const double2* row = reinterpret_cast<const double2*>(l6 + 6 * (size_t)o);
      const double2 r0 = row[0], r1 = row[1], r2 = row[2];
      const double c[6] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y};
      const double v[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
      const double dot = v[0] * c[3] + v[1] * c[4] + v[2] * c[5];
      const double nn = sqrt(c[3] * c[3] + c[4] * c[4] + c[5] * c[5]);
      const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      const double a = fabs(dot / (nn * vn));
      if (a < angle) {
        angle = a;
        for (int j = 0; j < 6; ++j) best[j] = c[j];
      }
    }
    if (angle != 360) {   // lidar_point.cc:39-50: the plane normalised, d from the LiDAR point
      ty = PCD_LIDAR_PROJ;
      for (int j = 0; j < 3; ++j) xyz[j] = best[j];
      const double norm = sqrt(best[3] * best[3] + best[4] * best[4] + best[5] * best[5]);
      abcd[0] = best[3] / norm; abcd[1] = best[4] / norm; abcd[2] = best[5] / norm;
      abcd[3] = 0 - abcd[0] * xyz[0] - abcd[1] * xyz[1] - abcd[2] * xyz[2];
    }
  }
  o_type[p] = ty;
  for (int j = 0; j < 4; ++j) o_abcd[4 * (size_t)p + j] = abcd[j];
  for (int j = 0; j < 3; ++j) o_xyz[3 * (size_t)p + j] = xyz[j];
}

// The rows of the two routes into one: a_* hold the association of ALL points; a point of mode 1 takes its Proj row, a
// point of mode 0 gets no term, a point of mode 2 keeps its association.  A mode above 2 becomes a type above 3, which
// the rebuild's validation record counts: the refusal needs no read-back of its own.
__global__ __launch_bounds__(256) void k_lidar_proj_merge(int P, const uint8_t* __restrict__ mode,
                                                          const uint8_t* __restrict__ p_type, const double* __restrict__ p_abcd,
                                                          const double* __restrict__ p_xyz, uint8_t* __restrict__ a_type,
                                                          double* __restrict__ a_abcd, double* __restrict__ a_xyz) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= (uint32_t)P) return;
  const uint8_t m = mode[p];
  if (m == 2) return;
  if (m == 1) {
    a_type[p] = p_type[p];
    for (int j = 0; j < 4; ++j) a_abcd[4 * (size_t)p + j] = p_abcd[4 * (size_t)p + j];
    for (int j = 0; j < 3; ++j) a_xyz[3 * (size_t)p + j] = p_xyz[3 * (size_t)p + j];
  } else {
    a_type[p] = m == 0 ? 0 : 0xFF;
  }
}

// The counts of pcd_ba_proj_info, without atomics: found observations per workgroup (kCountPer each), then one workgroup
// sums those and, over the images, the selected ones and their observations -> count[0..3) = images, features, found
constexpr uint32_t kCountPer = 4096;
__device__ __forceinline__ uint64_t block_sum_256(uint64_t v, uint64_t* s_v) {
  s_v[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s_v[threadIdx.x] += s_v[threadIdx.x + w];
    __syncthreads();
  }
  const uint64_t r = s_v[0];
  __syncthreads();
  return r;
}
__global__ __launch_bounds__(256) void k_lidar_proj_count_found(uint64_t O, const uint8_t* __restrict__ found,
                                                                uint64_t* __restrict__ part) {
  __shared__ uint64_t s_v[256];
  const uint64_t base = (uint64_t)blockIdx.x * kCountPer;
  uint64_t n = 0;
  for (uint32_t k = threadIdx.x; k < kCountPer; k += 256)
    if (base + k < O) n += found[base + k] ? 1u : 0u;
  n = block_sum_256(n, s_v);
  if (threadIdx.x == 0) part[blockIdx.x] = n;
}
__global__ __launch_bounds__(256) void k_lidar_proj_count(uint32_t nb, const uint64_t* __restrict__ part, int I,
                                                          const uint8_t* __restrict__ select,
                                                          const uint32_t* __restrict__ img_obs_start,
                                                          uint64_t* __restrict__ count) {
  __shared__ uint64_t s_v[256];
  uint64_t f = 0, ni = 0, nf = 0;
  for (uint32_t k = threadIdx.x; k < nb; k += 256) f += part[k];
  for (int i = threadIdx.x; i < I; i += 256)
    if (!select || select[i]) { ni += 1; nf += img_obs_start[i + 1] - img_obs_start[i]; }
  f = block_sum_256(f, s_v);
  ni = block_sum_256(ni, s_v);
  nf = block_sum_256(nf, s_v);
  if (threadIdx.x == 0) { count[0] = ni; count[1] = nf; count[2] = f; }
}

// what the host reads back
struct LidarStatus {
  LidarPart part;
  uint32_t L;
};
static_assert(sizeof(LidarStatus) == kStatusWords * sizeof(uint32_t), "status record");

// Argument checks shared by the entry points, in the documented order: arguments (INVALID), device (NO_DEVICE), capture
// (UNSUPPORTED) -- nothing allocated before them
static pcd_status lidar_guards(pcd_ba* b, void* stream, const char* fn) {
  PCD_REQUIRE(b, "null handle");
  PCD_TRY(require_device(b->device));
  PCD_TRY(refuse_capture((hipStream_t)stream, fn));
  return PCD_OK;
}

// The rebuild.  Rows as documented for pcd_ba_set_lidar_device, plus d_select (unselected rows count as type 0).
// Synchronises s once.  st (may be null) receives the record.
static pcd_status lidar_rebuild(pcd_ba* b, uint64_t Q, const int32_t* d_point, const uint8_t* d_type, const double* d_abcd,
                                const double* d_xyz, const uint8_t* d_select, const double weight[4], hipStream_t s,
                                LidarStatus* st) {
  BaLidarScratch& N = b->lidar_next;
  const int P = b->P;
  const uint32_t q32 = (uint32_t)Q;
  const uint32_t nb = div_up(Q, 256);
  LidarStatus hs{};
  if (Q) {
    PCD_TRY(N.flag.reserve(Q)); PCD_TRY(N.pos.reserve(Q));
    PCD_TRY(N.part.reserve((size_t)nb * kPartWords)); PCD_TRY(N.status.reserve(kStatusWords));
    PCD_TRY(N.h_status.reserve(kStatusWords));
    LidarPart* part = reinterpret_cast<LidarPart*>(N.part.p);
    {
      ScopedKernelTimer t("ba_lidar_flag", s);
      hipLaunchKernelGGL(k_lidar_flag, dim3(nb), dim3(256), 0, s, q32, P, d_point, d_type, d_abcd, d_select, N.flag.p, part);
      PCD_TRY(exclusive_sum(N.prim, N.flag.p, N.pos.p, 0u, (size_t)Q, s));
      hipLaunchKernelGGL(k_lidar_status, dim3(1), dim3(256), 0, s, nb, part, q32, N.flag.p, N.pos.p, N.status.p);
    }
    PCD_HIP_TRY(hipMemcpyAsync(N.h_status.p, N.status.p, sizeof(LidarStatus), hipMemcpyDeviceToHost, s));
    PCD_HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(&hs, N.h_status.p, sizeof hs);
  }
  if (st) *st = hs;   // a caller that is refused below can still say what was wrong with ITS rows
  if (hs.part.bad) {
    set_error("pcd_ba_set_lidar_device: %u row(s) with a point outside [0, %d) or a type above 3; the handle is unchanged",
              hs.part.bad, P);
    return PCD_ERR_INVALID;
  }
  for (int k = 0; k < 3; ++k)
    if (hs.part.ntype[k] && !std::isfinite(weight[k + 1])) {
      set_error("pcd_ba_set_lidar_device: the weight of type %d, which %u term(s) have, is not finite; the handle is unchanged",
                k + 1, hs.part.ntype[k]);
      return PCD_ERR_INVALID;
    }
  const uint32_t L = hs.L;
  // what this call builds: the rows with their meta and the index, sized as pcd_ba_create sizes the live ones; the
  // per-track copies only when there are terms
  BaTerms& T = N.terms;
  const unsigned built = kTermRows | kTermMeta | kTermIndex | (L ? kTermTracks : 0u);
  PCD_TRY(T.reserve_terms(built, L, (size_t)P, (size_t)b->nslices * 64));
  const bool sorted = !hs.part.unsorted;
  if (L && !sorted) { PCD_TRY(N.keys.reserve(L)); PCD_TRY(N.iota.reserve(L)); }
  PCD_TRY(reserve_cost_partial(b, (size_t)b->nslices, b->O, L));   // the sweep's grid follows O + L
  {
    ScopedKernelTimer t("ba_lidar_rebuild", s);
    LidarWeights wt;
    for (int k = 0; k < 4; ++k) wt.w[k] = weight[k];
    if (L)
      hipLaunchKernelGGL(k_lidar_compact, dim3(nb), dim3(256), 0, s, q32, N.flag.p, N.pos.p, d_point, d_type, d_abcd, d_xyz,
                         wt, T.lidar_point.p, T.lidar_abcd.p, T.lidar_w.p, T.lidar_type.p, T.lidar_xyz.p,
                         sorted ? T.pt_lidar_list.p : N.iota.p);
    const uint32_t* sorted_pt = reinterpret_cast<const uint32_t*>(T.lidar_point.p);
    if (L && !sorted) {   // points are at most P - 1
      PCD_TRY(sort_pairs(N.prim, reinterpret_cast<uint32_t*>(T.lidar_point.p), N.keys.p, N.iota.p, T.pt_lidar_list.p, (size_t)L,
                         0u, key_bits((uint64_t)P - 1), s));
      sorted_pt = N.keys.p;
    }
    hipLaunchKernelGGL(k_lidar_bounds, dim3(div_up((uint64_t)P + 1, 256)), dim3(256), 0, s, P, L, sorted_pt, T.pt_lidar_start.p);
    if (L) launch_lidar_tracks(*b, b->nslices, T, T, s);
    PCD_HIP_TRY(hipGetLastError());
  }
  // success: what was built becomes the handle's; the retired buffers are the next call's
  b->swap_terms(T, built);
  b->L = L;
  b->has_lidar_meta = true;
  ba_schur_invalidate(b);
  return PCD_OK;
}

// type / lidar_xyz of terms that came from pcd_ba_create: zeros, made when first asked for
static pcd_status lidar_meta(pcd_ba* b) {
  if (b->has_lidar_meta) return PCD_OK;
  const size_t L = b->L;
  PCD_TRY(b->reserve_terms(kTermMeta, L, 0, 0));
  PCD_HIP_TRY(hipMemset(b->lidar_type.p, 0, std::max<size_t>(L, 1)));
  PCD_HIP_TRY(hipMemset(b->lidar_xyz.p, 0, std::max<size_t>(3 * L, 1) * sizeof(double)));
  b->has_lidar_meta = true;
  return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" {

pcd_status pcd_ba_set_lidar_device(pcd_ba* b, uint64_t Q, const int32_t* d_point, const uint8_t* d_type,
                                   const double* d_abcd, const double* d_lidar_xyz, const double weight[4], void* stream,
                                   uint64_t* num_terms) {
  return pcd::guard([&]() -> pcd_status {
    PCD_REQUIRE(b, "null handle");
    PCD_REQUIRE(weight, "null weight");
    PCD_REQUIRE(Q == 0 || (d_type && d_abcd), "null rows");
    PCD_REQUIRE(Q < 0xFFFFFFF0ull, "too many rows");
    PCD_REQUIRE(d_point || Q == (uint64_t)b->P, "without d_point row q is point q: Q must equal the number of points");
    PCD_TRY(lidar_guards(b, stream, "pcd_ba_set_lidar_device"));
    PCD_HIP_TRY(hipSetDevice(b->device));
    LidarStatus st{};
    PCD_TRY(lidar_rebuild(b, Q, d_point, d_type, d_abcd, d_lidar_xyz, nullptr, weight, (hipStream_t)stream, &st));
    if (num_terms) *num_terms = st.L;
    return PCD_OK;
  });
}

pcd_status pcd_ba_get_lidar(pcd_ba* b, uint64_t* num_terms, int32_t* point, double* abcd, double* weight, uint8_t* type,
                            double* lidar_xyz) {
  PCD_REQUIRE(b, "null handle");
  PCD_TRY(require_device(b->device));
  PCD_HIP_TRY(hipSetDevice(b->device));
  const size_t L = b->L;
  if (num_terms) *num_terms = L;
  if (!L) return PCD_OK;
  if (type || lidar_xyz) PCD_TRY(lidar_meta(b));
  if (point) PCD_HIP_TRY(hipMemcpy(point, b->lidar_point.p, L * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (abcd) PCD_HIP_TRY(hipMemcpy(abcd, b->lidar_abcd.p, 4 * L * sizeof(double), hipMemcpyDeviceToHost));
  if (weight) PCD_HIP_TRY(hipMemcpy(weight, b->lidar_w.p, L * sizeof(double), hipMemcpyDeviceToHost));
  if (type) PCD_HIP_TRY(hipMemcpy(type, b->lidar_type.p, L, hipMemcpyDeviceToHost));
  if (lidar_xyz) PCD_HIP_TRY(hipMemcpy(lidar_xyz, b->lidar_xyz.p, 3 * L * sizeof(double), hipMemcpyDeviceToHost));
  return PCD_OK;
}

pcd_status pcd_ba_lidar_device(pcd_ba* b, uint64_t* num_terms, const int32_t** d_point, const double** d_abcd,
                               const double** d_weight, const uint8_t** d_type, const double** d_lidar_xyz) {
  PCD_REQUIRE(b, "null handle");
  PCD_TRY(require_device(b->device));
  PCD_HIP_TRY(hipSetDevice(b->device));
  if (d_type || d_lidar_xyz) PCD_TRY(lidar_meta(b));
  if (num_terms) *num_terms = b->L;
  if (d_point) *d_point = b->lidar_point.p;
  if (d_abcd) *d_abcd = b->lidar_abcd.p;
  if (d_weight) *d_weight = b->lidar_w.p;
  if (d_type) *d_type = b->lidar_type.p;
  if (d_lidar_xyz) *d_lidar_xyz = b->lidar_xyz.p;
  return PCD_OK;
}

void pcd_ba_assoc_opts_default(pcd_ba_assoc_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->gate_mode = PCD_GATE_MAPPER_GLOBAL;
  o->icp_weight = 100.0;
  o->icp_ground_weight = 1000.0;
}

pcd_status pcd_ba_associate_lidar_device(pcd_ba* b, pcd_cloud* c, const pcd_ba_assoc_opts* opts, void* stream,
                                         pcd_ba_assoc_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    PCD_REQUIRE(opts, "null options");
    const int mode = opts->gate_mode & ~PCD_GATE_BOUNDED_SEARCH;
    PCD_REQUIRE(mode >= 0 && mode <= 2, "gate_mode");
    PCD_REQUIRE(b, "null handle");
    PCD_REQUIRE(c, "null cloud");
    const uint64_t P = (uint64_t)b->P;
    PCD_REQUIRE(mode == PCD_GATE_CONTROLLER ||
                (opts->d_max_range && (opts->max_range_count == 1 || opts->max_range_count == P)),
                "max_range must have 1 or num_points entries");
    PCD_REQUIRE(b->device == c->device, "the BA handle and the cloud live on different devices");
    PCD_TRY(lidar_guards(b, stream, "pcd_ba_associate_lidar_device"));
    if (c->row_index.p || c->g2l.p || c->index_stride != 1 || c->index_base != 0) {
      set_error("pcd_ba_associate_lidar_device needs ONE handle holding the whole cloud, not a shard or a strided handle "
                "(pcd_cloud_create_sharded, index_stride / index_base)");
      return PCD_ERR_UNSUPPORTED;
    }
    if (P == 0) return PCD_OK;
    PCD_HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BaLidarScratch& N = b->lidar_next;
    PCD_TRY(N.a_xyz.reserve(3 * P)); PCD_TRY(N.a_abcd.reserve(4 * P)); PCD_TRY(N.a_type.reserve(P));
    EventPair ea, er;
    if (info) { PCD_TRY(ea.create()); PCD_TRY(er.create()); (void)ea.start(s); }
    pcd_assoc_out ao{};
    ao.lidar_xyz = N.a_xyz.p; ao.abcd = N.a_abcd.p; ao.type = N.a_type.p;
    PCD_TRY(pcd_associate_device(c, b->points.p, P, opts->d_max_range, opts->max_range_count, opts->gate_mode, nullptr,
                                 &ao, stream));
    if (info) { (void)ea.stop(s); (void)er.start(s); }
    const double weight[4] = {0.0, opts->icp_weight, opts->icp_ground_weight, 0.0};
    LidarStatus st{};
    PCD_TRY(lidar_rebuild(b, P, nullptr, N.a_type.p, N.a_abcd.p, N.a_xyz.p, opts->d_select, weight, s, &st));
    if (info) {
      float ms = 0.f;
      PCD_HIP_TRY(er.stop_and_wait(s, &ms));
      info->rebuild_ms = ms;
      PCD_HIP_TRY(ea.elapsed(&ms));
      info->assoc_ms = ms;
      info->num_queries = st.part.selected;
      info->num_terms = st.L;
      info->num_icp = st.part.ntype[0];
      info->num_icp_ground = st.part.ntype[1];
    }
    return PCD_OK;
  });
}

void pcd_ba_proj_opts_default(pcd_ba_proj_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->gate_mode = PCD_GATE_MAPPER_LOCAL;
  o->proj_weight = 1.0;
  o->icp_weight = 100.0;
  o->icp_ground_weight = 1000.0;
}

pcd_status pcd_ba_project_lidar_device(pcd_ba* b, pcd_proj* proj, const pcd_ba_proj_opts* opts, void* stream,
                                       pcd_ba_proj_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    PCD_REQUIRE(opts, "null options");
    PCD_REQUIRE(opts->cam_width && opts->cam_height, "null cam_width / cam_height");
    PCD_REQUIRE(b, "null handle");
    PCD_REQUIRE(proj, "null projector");
    const bool mixed = opts->d_point_mode != nullptr;   // some point may take the nearest-neighbour route
    const uint64_t P = (uint64_t)b->P;
    const int mode = opts->gate_mode & ~PCD_GATE_BOUNDED_SEARCH;
    if (mixed) {
      PCD_REQUIRE(mode >= 0 && mode <= 2, "gate_mode");
      PCD_REQUIRE(mode == PCD_GATE_CONTROLLER ||
                  (opts->d_max_range && (opts->max_range_count == 1 || opts->max_range_count == P)),
                  "max_range must have 1 or num_points entries");
    }
    pcd_cloud* c = proj_cloud(proj);
    PCD_REQUIRE(b->device == c->device, "the BA handle and the projector live on different devices");
    if (mixed && (c->row_index.p || c->g2l.p || c->index_stride != 1 || c->index_base != 0)) {
      set_error("pcd_ba_project_lidar_device needs ONE handle holding the whole cloud, not a shard or a strided handle");
      return PCD_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < b->C; ++k) {   // pcd_proj_set_new_images' check, on the host mirror: params[0], params[1] of an OPENCV camera
      const double* cp = b->h_cam_params.data() + b->h_cam_off[k];
      const int K = cam_num_params(b->h_cam_model[k]);
      PCD_REQUIRE(cp[0] != 0 && (K > 1 ? cp[1] : 0.0) != 0, "focal length");
    }
    PCD_TRY(lidar_guards(b, stream, "pcd_ba_project_lidar_device"));
    if (P == 0) return PCD_OK;
    PCD_HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    BaLidarScratch& N = b->lidar_next;
    const uint64_t O = b->O;
    const int I = b->I;
    PCD_TRY(N.a_xyz.reserve(3 * P)); PCD_TRY(N.a_abcd.reserve(4 * P)); PCD_TRY(N.a_type.reserve(P));
    PCD_TRY(N.p_found.reserve(at_least_1(O))); PCD_TRY(N.p_l6.reserve(at_least_1(6 * O)));
    if (mixed) { PCD_TRY(N.p_xyz.reserve(3 * P)); PCD_TRY(N.p_abcd.reserve(4 * P)); PCD_TRY(N.p_type.reserve(P)); }
    const uint32_t nbf = div_up(O, kCountPer);
    if (info) {
      PCD_TRY(N.p_count_part.reserve(at_least_1(nbf))); PCD_TRY(N.p_count.reserve(3)); PCD_TRY(N.h_count.reserve(3));
    }
    EventPair ep, ea, er;
    if (info) { PCD_TRY(ep.create()); PCD_TRY(ea.create()); PCD_TRY(er.create()); (void)ep.start(s); }
    // the images: sizes and parameter counts by camera, from the mirrors; poses and parameters stay where they are
    std::vector<uint64_t> width((size_t)I), height((size_t)I);
    std::vector<int> nprm((size_t)I);
    for (int i = 0; i < I; ++i) {
      const int cam = b->h_image_cam[i];
      width[i] = opts->cam_width[cam];
      height[i] = opts->cam_height[cam];
      nprm[i] = cam_num_params(b->h_cam_model[cam]);
    }
    ProjDeviceImages im;
    im.n = (uint64_t)I;
    im.width = width.data(); im.height = height.data(); im.num_params = nprm.data();
    im.feat_start = b->h_img_obs_start.data();
    {
      const int cam0 = b->h_image_cam[0];
      const double* cp = b->h_cam_params.data() + b->h_cam_off[cam0];
      im.latch_fx = cp[0];
      im.latch_fy = cam_num_params(b->h_cam_model[cam0]) > 1 ? cp[1] : 0.0;
    }
    im.d_poses = b->poses.p; im.d_image_cam = b->image_cam.p; im.d_cam_off = b->cam_off.p;
    im.d_cam_params = b->cam_params.p; im.d_select = opts->d_image_select;
    // from here to the rebuild's synchronisation the projector's pinned scratch is in flight: a refusal waits for s
    auto fail = [&](pcd_status st) { (void)hipStreamSynchronize(s); return st; };
    pcd_status st = proj_project_device_images(proj, im, O, b->img_xy.p, b->img_obs.p, N.p_found.p, N.p_l6.p, s);
    if (st != PCD_OK) return fail(st);
    {
      ScopedKernelTimer t("ba_lidar_proj_pick", s);
      hipLaunchKernelGGL(k_lidar_proj_pick, dim3(div_up(P, 64)), dim3(64), 0, s, b->P, b->pt_obs_start.p, b->pt_obs_list.p,
                         b->obs_image.p, N.p_found.p, N.p_l6.p, b->points.p, opts->d_point_mode,
                         mixed ? N.p_type.p : N.a_type.p, mixed ? N.p_abcd.p : N.a_abcd.p, mixed ? N.p_xyz.p : N.a_xyz.p);
    }
    if (info) {
      hipLaunchKernelGGL(k_lidar_proj_count_found, dim3(std::max(nbf, 1u)), dim3(256), 0, s, O, N.p_found.p, N.p_count_part.p);
      hipLaunchKernelGGL(k_lidar_proj_count, dim3(1), dim3(256), 0, s, O ? nbf : 0u, N.p_count_part.p, I, opts->d_image_select,
                         b->img_obs_start.p, N.p_count.p);
      PCD_HIP_TRY(hipMemcpyAsync(N.h_count.p, N.p_count.p, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      (void)ep.stop(s); (void)ea.start(s);
    }
    if (mixed) {
      pcd_assoc_out ao{};
      ao.lidar_xyz = N.a_xyz.p; ao.abcd = N.a_abcd.p; ao.type = N.a_type.p;
      st = pcd_associate_device(c, b->points.p, P, opts->d_max_range, opts->max_range_count, opts->gate_mode, nullptr, &ao,
                                stream);
      if (st != PCD_OK) return fail(st);
      hipLaunchKernelGGL(k_lidar_proj_merge, dim3(div_up(P, 256)), dim3(256), 0, s, b->P, opts->d_point_mode, N.p_type.p,
                         N.p_abcd.p, N.p_xyz.p, N.a_type.p, N.a_abcd.p, N.a_xyz.p);
    }
    if (info) { (void)ea.stop(s); (void)er.start(s); }
    const double weight[4] = {0.0, opts->icp_weight, opts->icp_ground_weight, opts->proj_weight};
    LidarStatus ls{};
    st = lidar_rebuild(b, P, nullptr, N.a_type.p, N.a_abcd.p, N.a_xyz.p, nullptr, weight, s, &ls);   // synchronises s
    if (st != PCD_OK) (void)hipStreamSynchronize(s);   // a rebuild that failed ahead of its synchronisation
    const uint64_t pairs = proj_collect_pairs(proj);
    if (st == PCD_ERR_INVALID && ls.part.bad)
      set_error("pcd_ba_project_lidar_device: %u point_mode value(s) above 2; the handle is unchanged", ls.part.bad);
    PCD_TRY(st);
    if (info) {
      float ms = 0.f;
      PCD_HIP_TRY(er.stop_and_wait(s, &ms));
      info->rebuild_ms = ms;
      PCD_HIP_TRY(ea.elapsed(&ms));
      info->assoc_ms = ms;
      PCD_HIP_TRY(ep.elapsed(&ms));
      info->proj_ms = ms;
      info->num_images = N.h_count.p[0]; info->num_features = N.h_count.p[1]; info->num_found = N.h_count.p[2];
      info->num_terms = ls.L;
      info->num_icp = ls.part.ntype[0]; info->num_icp_ground = ls.part.ntype[1]; info->num_proj = ls.part.ntype[2];
      info->pairs = pairs;
    }
    return PCD_OK;
  });
}

}  // extern "C"

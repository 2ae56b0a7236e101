// ba_local.hip -- the start of the local round on a live handle: pcd_ba_local_bundle_device restates
// IncrementalMapper::FindLocalBundle (sfm/incremental_mapper.cc:1747-1914), pcd_ba_local_window_create_device derives
// the sub-problem of AdjustLocalBundle (:1004-1213) as a second handle.  The arithmetic of both is written out in
// pcdhip.h.  The bundle's passes, all on `stream`, no wait:
//   k_lb_mult      thread = point: mult[p] = its rows on `image` (the track CSR)
//   k_lb_shared    wavefront = image j: shared[j] = the sum of mult over its image-major rows; the sort key ~shared
//   sort_pairs     stable by the key: shared descending, ties by image index ascending; images without a shared row last
//   k_lb_head      one workgroup: the number of candidates, n, num_eff, the short case
//   k_lb_angles    workgroup = rank: n angles, then the exact k-th smallest by a radix select over their 64-bit patterns
//                  (8-bit digits, an LDS histogram per digit, scanned by wavefront shuffles).  The first kLbCache angles
//                  live in LDS; the rest are computed again in every digit pass, so any n works and nothing spills
//   k_lb_select    one workgroup: the eight passes and the fill-up.  Whether a candidate qualifies in a pass does not
//                  depend on the others, only the cap does: a pass is a ballot and a prefix count over 256 ranks at a time
// The window: k_win_images (ba_window.hip) with the caller's set, k_lwin_points (thread = point: V, kept, point_const'),
// k_lwin_rows / k_lwin_terms (the erase masks of the compaction), then window_derive's sequence, shared with the sphere
// window.  No floating-point atomics; nothing depends on the launch geometry.
#include <cmath>

#include "ba_handle.h"
#include "ba_math.h"
#include "prim.h"

namespace pcd {

enum { kLbCand = 0, kLbRows, kLbEff, kLbShort, kLbHeadWords };
constexpr uint32_t kLbCache = 2048;       // angles kept in LDS: 16 KB of the workgroup's 64 KB
constexpr uint32_t kNoShare = 0xFFFFFFFFu;   // the sort key of an image that shares no row: behind every candidate
__constant__ double kLbDiv[8] = {1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0};
__constant__ double kLbFrac[8] = {0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1};

__global__ __launch_bounds__(256) void k_lb_mult(uint32_t P, const uint32_t* __restrict__ pt_start,
                                                 const uint32_t* __restrict__ pt_list, const int* __restrict__ obs_image,
                                                 int image, uint32_t* __restrict__ mult) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= P) return;
  uint32_t m = 0;
  for (uint32_t k = pt_start[p], e = pt_start[p + 1]; k < e; ++k) m += obs_image[pt_list[k]] == image ? 1u : 0u;
  mult[p] = m;
}

// four images per workgroup, one wavefront each (an integer sum: any order)
__global__ __launch_bounds__(256) void k_lb_shared(uint32_t I, int image, const uint32_t* __restrict__ img_start,
                                                   const int* __restrict__ img_pt, const uint32_t* __restrict__ mult,
                                                   uint32_t* __restrict__ key, uint32_t* __restrict__ iota,
                                                   uint32_t* __restrict__ shared) {
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (j >= I) return;
  uint32_t sum = 0;
  for (uint32_t e = img_start[j] + lane, end = img_start[j + 1]; e < end; e += 64u) sum += mult[img_pt[e]];
  for (int off = 32; off > 0; off >>= 1) sum += (uint32_t)__shfl_xor((int)sum, off);
  if (j == (uint32_t)image) sum = 0;
  if (lane == 0) {
    key[j] = ~sum;
    iota[j] = j;
    if (shared) shared[j] = sum;
  }
}

__global__ __launch_bounds__(256) void k_lb_head(uint32_t I, int image, int num_images, const uint32_t* __restrict__ key_sorted,
                                                 const uint32_t* __restrict__ img_start, uint32_t* __restrict__ head) {
  __shared__ uint32_t s_n[256];
  uint32_t c = 0;
  for (uint32_t r = threadIdx.x; r < I; r += 256) c += key_sorted[r] != kNoShare ? 1u : 0u;
  s_n[threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s_n[threadIdx.x] += s_n[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t nc = s_n[0], eff = min((uint32_t)(num_images - 1), nc);
    head[kLbCand] = nc;
    head[kLbRows] = img_start[image + 1] - img_start[image];
    head[kLbEff] = eff;
    head[kLbShort] = nc == eff ? 1u : 0u;
  }
}

// an angle is never negative: its bit pattern orders as it does.  A NaN goes behind every number
__device__ __forceinline__ uint64_t lb_key(double a) { return a != a ? ~0ull : (uint64_t)__double_as_longlong(a); }

__global__ __launch_bounds__(256) void k_lb_angles(int image, const uint32_t* __restrict__ head,
                                                   const uint32_t* __restrict__ key_sorted, const uint32_t* __restrict__ img_sorted,
                                                   const uint32_t* __restrict__ img_start, const int* __restrict__ img_pt,
                                                   const double* __restrict__ poses, const double* __restrict__ points,
                                                   double* __restrict__ tri, double* __restrict__ tri_of_image) {
  __shared__ double s_ang[kLbCache];
  __shared__ uint32_t s_hist[256], s_wsum[4], s_sel[2];
  const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t j = img_sorted[r], n = head[kLbRows];
  // the loosest pass's bound: below it no pass looks at an angle
  const bool wanted = r < head[kLbCand] && !head[kLbShort] && (double)(~key_sorted[r]) >= 0.1 * (double)n;
  if (!wanted) {   // the same for every thread of the workgroup
    if (tid == 0) {
      tri[r] = -1.0;
      if (tri_of_image) tri_of_image[j] = -1.0;
    }
    return;
  }
  double c1[3], c2[3];
  proj_center(poses + 7 * (size_t)image, c1);
  proj_center(poses + 7 * (size_t)j, c2);
  const int* pt = img_pt + img_start[image];
  auto angle = [&](uint32_t e) {
    const double* x = points + 3 * (size_t)pt[e];
    const double X[3] = {x[0], x[1], x[2]};
    return tri_angle(c1, c2, X);
  };
  for (uint32_t e = tid; e < min(n, kLbCache); e += 256) s_ang[e] = angle(e);
  // Percentile: idx = (int)std::round(p / 100 * (n - 1)), halves away from zero, clamped
  uint32_t k = min((uint32_t)round(0.75 * (double)(n - 1u)), n - 1u);
  uint64_t prefix = 0;
  for (int d = 7; d >= 0; --d) {
    s_hist[tid] = 0;
    __syncthreads();
    for (uint32_t e = tid; e < n; e += 256) {
      const uint64_t key = lb_key(e < kLbCache ? s_ang[e] : angle(e));
      if (d == 7 || (key >> (8 * (d + 1))) == prefix) atomicAdd(&s_hist[(uint32_t)(key >> (8 * d)) & 255u], 1u);
    }
    __syncthreads();
    // inclusive scan of the 256 counters: each wavefront scans its 64 by shuffles, the three sums in front come from LDS
    const uint32_t v = s_hist[tid];
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = __shfl_up(incl, off);
      if ((int)lane >= off) incl += t;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) incl += s_wsum[w];
    const uint32_t excl = incl - v;
    if (excl <= k && k < incl) { s_sel[0] = tid; s_sel[1] = k - excl; }   // one thread: the digit of the k-th smallest
    __syncthreads();
    prefix = (prefix << 8) | s_sel[0];
    k = s_sel[1];
  }
  if (tid == 0) {
    const double a = prefix == ~0ull ? __longlong_as_double(0x7FF8000000000000ll) : __longlong_as_double((long long)prefix);
    tri[r] = a;
    if (tri_of_image) tri_of_image[j] = a;
  }
}

// position of a flagged thread among the flagged threads of the workgroup, in thread order; total = their number
__device__ __forceinline__ uint32_t lb_rank(bool q, uint32_t* s_w, uint32_t& total) {
  const uint64_t b = __ballot(q);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t pos = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (uint32_t w = 0; w < 4; ++w) {
    if (w < wave) before += s_w[w];
    total += s_w[w];
  }
  __syncthreads();
  return before + pos;
}

// rank r is handled by thread r % 256 in every pass: used[r] is read and written by that thread alone
__global__ __launch_bounds__(256) void k_lb_select(uint32_t I, int image, int num_images, double m,
                                                   const uint32_t* __restrict__ head, const uint32_t* __restrict__ key_sorted,
                                                   const uint32_t* __restrict__ img_sorted, const double* __restrict__ tri,
                                                   uint8_t* __restrict__ used, int32_t* bundle, int32_t* __restrict__ num,
                                                   uint8_t* set) {
  __shared__ uint32_t s_w[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t nc = head[kLbCand], eff = head[kLbEff];
  const double fn = (double)head[kLbRows];
  for (uint32_t k = tid; k < (uint32_t)(num_images - 1); k += 256) bundle[k] = -1;
  for (uint32_t i = tid; i < I; i += 256) { set[i] = i == (uint32_t)image ? 1 : 0; used[i] = 0; }
  __syncthreads();
  uint32_t count = 0;   // the same in every thread
  if (head[kLbShort]) {
    for (uint32_t r = tid; r < nc; r += 256) bundle[r] = (int32_t)img_sorted[r];
    count = nc;
  } else {
    for (int pass = 0; pass < 8 && count < eff; ++pass) {
      const double min_angle = m / kLbDiv[pass], min_shared = kLbFrac[pass] * fn;
      for (uint32_t base = 0; base < nc && count < eff; base += 256) {
        const uint32_t r = base + tid;
        const bool over = r < nc && (double)(~key_sorted[r]) >= min_shared;   // a prefix of the order
        const bool q = over && !used[r] && tri[r] >= min_angle;
        uint32_t total;
        const uint32_t pos = lb_rank(q, s_w, total), left = eff - count;
        if (q && pos < left) { bundle[count + pos] = (int32_t)img_sorted[r]; used[r] = 1; }
        count += min(total, left);
        if (__syncthreads_or(!over)) break;   // the first candidate below the bound ends the pass
      }
    }
    for (uint32_t base = 0; base < nc && count < eff; base += 256) {   // the fill-up
      const uint32_t r = base + tid;
      const bool q = r < nc && !used[r];
      uint32_t total;
      const uint32_t pos = lb_rank(q, s_w, total), left = eff - count;
      if (q && pos < left) { bundle[count + pos] = (int32_t)img_sorted[r]; used[r] = 1; }
      count += min(total, left);
    }
  }
  __syncthreads();
  for (uint32_t k = tid; k < count; k += 256) set[bundle[k]] = 1;
  if (tid == 0) num[0] = (int32_t)count;
}

static pcd_status local_bundle(pcd_ba* b, const pcd_ba_local_bundle_opts* o, int32_t* d_bundle, int32_t* d_num,
                               uint8_t* d_set, uint32_t* d_shared, double* d_tri, hipStream_t s) {
  BaLocalScratch& N = b->local_next;
  const uint32_t I = (uint32_t)b->I, P = (uint32_t)b->P;
  PCD_TRY(N.mult.reserve(at_least_1(P)));
  for (DevBuf<uint32_t>* d : {&N.key, &N.key_sorted, &N.iota, &N.img_sorted}) PCD_TRY(d->reserve(I));
  PCD_TRY(N.head.reserve(kLbHeadWords)); PCD_TRY(N.tri.reserve(I)); PCD_TRY(N.used.reserve(I));
  size_t need = 0;
  PCD_TRY(prim_storage_u32({}, {{I, 32u}}, need));
  PCD_TRY(N.prim.reserve(need));
  ScopedKernelTimer t("ba_local_bundle", s);
  if (P)
    hipLaunchKernelGGL(k_lb_mult, dim3(div_up(P, 256)), dim3(256), 0, s, P, b->pt_obs_start.p, b->pt_obs_list.p,
                       b->obs_image.p, (int)o->image, N.mult.p);
  hipLaunchKernelGGL(k_lb_shared, dim3(div_up(I, 4)), dim3(256), 0, s, I, (int)o->image, b->img_obs_start.p, b->img_pt.p,
                     N.mult.p, N.key.p, N.iota.p, d_shared);
  PCD_TRY(sort_pairs(N.prim, N.key.p, N.key_sorted.p, N.iota.p, N.img_sorted.p, (size_t)I, 0u, 32u, s));
  hipLaunchKernelGGL(k_lb_head, dim3(1), dim3(256), 0, s, I, (int)o->image, (int)o->num_images, N.key_sorted.p,
                     b->img_obs_start.p, N.head.p);
  hipLaunchKernelGGL(k_lb_angles, dim3(I), dim3(256), 0, s, (int)o->image, N.head.p, N.key_sorted.p, N.img_sorted.p,
                     b->img_obs_start.p, b->img_pt.p, b->poses.p, b->points.p, N.tri.p, d_tri);
  const double m = o->min_tri_angle_deg * 0.0174532925199432954743716805978692718781530857086181640625;   // DegToRad
  hipLaunchKernelGGL(k_lb_select, dim3(1), dim3(256), 0, s, I, (int)o->image, (int)o->num_images, m, N.head.p,
                     N.key_sorted.p, N.img_sorted.p, N.tri.p, N.used.p, d_bundle, d_num, d_set);
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

static pcd_status check_bundle_opts(const pcd_ba* b, const pcd_ba_local_bundle_opts* o) {
  PCD_REQUIRE(o->image >= 0 && o->image < b->I, "image out of range");
  PCD_REQUIRE(o->num_images >= 2, "num_images below 2");
  PCD_REQUIRE(o->min_tri_angle_deg >= 0.0, "min_tri_angle_deg negative or NaN");   // NaN fails the comparison
  return PCD_OK;
}

// ---- the local window ----------------------------------------------------------------------------------------------
enum { kLwinImagesIn = kRecWords, kLwinVariable, kLwinFixed, kLwinWords };

// thread = point.  V[p]: the caller's flag, or (observed by `image` and track length <= max_len).  kept = the rows that
// stay (all of a variable point, else those on "in" images); pconst[p] = src's || 0 < kept < length.
// part_v / part_f [workgroup] = its variable points / the points the rule made constant
__global__ __launch_bounds__(256) void k_lwin_points(uint32_t P, const uint32_t* __restrict__ pt_start,
                                                     const uint32_t* __restrict__ pt_list, const int* __restrict__ obs_image,
                                                     const uint8_t* __restrict__ in, const uint8_t* __restrict__ variable,
                                                     int image, uint32_t max_len, const uint8_t* __restrict__ src_const,
                                                     uint8_t* __restrict__ V, uint8_t* __restrict__ pconst,
                                                     uint32_t* __restrict__ part_v, uint32_t* __restrict__ part_f) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  bool v = false, fixed = false;
  if (p < P) {
    const uint32_t b = pt_start[p], len = pt_start[p + 1] - b;
    uint32_t inside = 0;
    bool seen = false;
    for (uint32_t k = 0; k < len; ++k) {
      const int i = obs_image[pt_list[b + k]];
      inside += in[i] ? 1u : 0u;
      seen = seen || i == image;
    }
    v = variable ? variable[p] != 0 : (seen && len <= max_len);
    const uint32_t kept = v ? len : inside;
    const bool part = kept > 0 && kept < len, held = src_const && src_const[p];
    fixed = part && !held;
    V[p] = v ? 1 : 0;
    pconst[p] = (held || part) ? 1 : 0;
  }
  const int nv = __syncthreads_count(v), nf = __syncthreads_count(fixed);
  if (threadIdx.x == 0) { part_v[blockIdx.x] = (uint32_t)nv; part_f[blockIdx.x] = (uint32_t)nf; }
}
__global__ __launch_bounds__(256) void k_lwin_rows(uint32_t O, const int* __restrict__ obs_image,
                                                   const int* __restrict__ obs_point, const uint8_t* __restrict__ in,
                                                   const uint8_t* __restrict__ V, uint8_t* __restrict__ erase) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o >= O) return;
  erase[o] = (in[obs_image[o]] || V[obs_point[o]]) ? 0 : 1;
}
__global__ __launch_bounds__(256) void k_lwin_terms(uint32_t L, const int* __restrict__ lidar_point,
                                                    const uint8_t* __restrict__ V, uint8_t* __restrict__ erase) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= L) return;
  erase[l] = V[lidar_point[l]] ? 0 : 1;
}
// one workgroup: the three counts from the per-workgroup counts (nbi of k_win_images, then 2 x nbp of k_lwin_points)
__global__ __launch_bounds__(256) void k_lwin_record(uint32_t nbi, uint32_t nbp, const uint32_t* __restrict__ part,
                                                     uint32_t* __restrict__ rec) {
  __shared__ uint32_t s_n[3][256];
  uint32_t n[3] = {0, 0, 0};
  for (uint32_t k = threadIdx.x; k < nbi; k += 256) n[0] += part[k];
  for (uint32_t k = threadIdx.x; k < nbp; k += 256) { n[1] += part[nbi + k]; n[2] += part[nbi + nbp + k]; }
  for (int c = 0; c < 3; ++c) s_n[c][threadIdx.x] = n[c];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int c = 0; c < 3; ++c) s_n[c][threadIdx.x] += s_n[c][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) { rec[kLwinImagesIn] = s_n[0][0]; rec[kLwinVariable] = s_n[1][0]; rec[kLwinFixed] = s_n[2][0]; }
}

struct LocalSelection : WindowSelection {
  const pcd_ba_local_window_opts* o;
  uint8_t* d_var;
  DevBuf<uint8_t> in, var_own, erase, term_erase;
  DevBuf<uint32_t> part;
  uint32_t nbi = 0, nbp = 0;   // the workgroups of k_win_images / k_lwin_points
  LocalSelection(const pcd_ba_local_window_opts* opts, uint8_t* d_variable_out) : o(opts), d_var(d_variable_out) {
    words = kLwinWords;
  }
  pcd_status reserve(const pcd_ba* src, pcd_ba* w) override {
    const size_t I = (size_t)src->I, P = (size_t)src->P;
    PCD_TRY(in.reserve(I));
    if (!d_var) { PCD_TRY(var_own.reserve(at_least_1(P))); d_var = var_own.p; }
    PCD_TRY(erase.reserve(at_least_1(src->O))); PCD_TRY(term_erase.reserve(at_least_1(src->L)));
    PCD_TRY(w->point_const.reserve(at_least_1(P)));   // always an array on a local window
    nbi = div_up(I, 256); nbp = div_up(P, 256);
    return part.reserve(at_least_1((size_t)nbi + 2 * (size_t)nbp));
  }
  pcd_status select(const pcd_ba* src, pcd_ba* w, hipStream_t s, WindowMasks* m) override {
    const uint32_t P = (uint32_t)src->P, O = (uint32_t)src->O, L = (uint32_t)src->L;
    launch_win_images(src, -1, 0.0, o->d_image_set, o->d_extra_const_pose, in.p, w->image_const_pose.p, part.p, s);
    if (P)
      hipLaunchKernelGGL(k_lwin_points, dim3(nbp), dim3(256), 0, s, P, src->pt_obs_start.p, src->pt_obs_list.p,
                         src->obs_image.p, in.p, o->d_point_variable, (int)o->image, o->max_track_length,
                         src->const_points(), d_var, w->point_const.p, part.p + nbi, part.p + nbi + nbp);
    if (O)
      hipLaunchKernelGGL(k_lwin_rows, dim3(div_up(O, 256)), dim3(256), 0, s, O, src->obs_image.p, src->obs_point.p, in.p,
                         d_var, erase.p);
    if (L)
      hipLaunchKernelGGL(k_lwin_terms, dim3(div_up(L, 256)), dim3(256), 0, s, L, src->lidar_point.p, d_var, term_erase.p);
    w->has_cpt = true;
    m->obs_erase = erase.p;
    m->term_erase = term_erase.p;
    return PCD_OK;
  }
  pcd_status record(pcd_ba* w, hipStream_t s) override {
    hipLaunchKernelGGL(k_lwin_record, dim3(1), dim3(256), 0, s, nbi, nbp, part.p, w->edit_next.record.p);
    return PCD_OK;
  }
};

}  // namespace pcd

using namespace pcd;

extern "C" void pcd_ba_local_bundle_opts_default(pcd_ba_local_bundle_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->image = -1;
  o->num_images = 6;
  o->min_tri_angle_deg = 6.0;
}

extern "C" pcd_status pcd_ba_local_bundle_device(pcd_ba* b, const pcd_ba_local_bundle_opts* opts, int32_t* d_bundle,
                                                 int32_t* d_num, uint8_t* d_image_set, uint32_t* d_shared,
                                                 double* d_tri_angle, void* stream) {
  return pcd::guard([&]() -> pcd_status {
    PCD_REQUIRE(b && opts && d_bundle && d_num && d_image_set, "null pointer");
    PCD_TRY(require_device(b->device));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_ba_local_bundle_device"));
    PCD_TRY(check_bundle_opts(b, opts));
    PCD_HIP_TRY(hipSetDevice(b->device));
    return local_bundle(b, opts, d_bundle, d_num, d_image_set, d_shared, d_tri_angle, (hipStream_t)stream);
  });
}

extern "C" pcd_status pcd_ba_local_bundle(pcd_ba* b, const pcd_ba_local_bundle_opts* opts, int32_t* bundle, int32_t* num,
                                          uint32_t* shared, double* tri_angle) {
  return pcd::guard([&]() -> pcd_status {
    PCD_REQUIRE(b && opts && bundle && num, "null pointer");
    PCD_TRY(require_device(b->device));
    PCD_TRY(check_bundle_opts(b, opts));
    PCD_HIP_TRY(hipSetDevice(b->device));
    const size_t I = (size_t)b->I, cap = (size_t)opts->num_images - 1;
    DevBuf<int32_t> d_bundle, d_num;
    DevBuf<uint8_t> d_set;
    DevBuf<uint32_t> d_shared;
    DevBuf<double> d_tri;
    PCD_TRY(d_bundle.reserve(cap)); PCD_TRY(d_num.reserve(1)); PCD_TRY(d_set.reserve(I));
    if (shared) PCD_TRY(d_shared.reserve(I));
    if (tri_angle) PCD_TRY(d_tri.reserve(I));
    PCD_TRY(pcd_ba_local_bundle_device(b, opts, d_bundle.p, d_num.p, d_set.p, shared ? d_shared.p : nullptr,
                                       tri_angle ? d_tri.p : nullptr, nullptr));
    PCD_HIP_TRY(hipStreamSynchronize(nullptr));
    PCD_TRY(copy_back(bundle, d_bundle, cap)); PCD_TRY(copy_back(num, d_num, 1));
    PCD_TRY(copy_back(shared, d_shared, I)); PCD_TRY(copy_back(tri_angle, d_tri, I));
    return PCD_OK;
  });
}

extern "C" void pcd_ba_local_window_opts_default(pcd_ba_local_window_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->image = -1;
  o->max_track_length = 1000;
}

extern "C" pcd_status pcd_ba_local_window_create_device(pcd_ba* src, const pcd_ba_local_window_opts* opts,
                                                        uint8_t* d_point_variable_out, uint32_t* d_obs_map, void* stream,
                                                        pcd_ba** window, pcd_ba_local_window_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    if (window) *window = nullptr;
    PCD_REQUIRE(src && opts && window, "null pointer");
    PCD_TRY(require_device(src->device));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_ba_local_window_create_device"));
    PCD_REQUIRE(opts->d_image_set, "d_image_set is required");
    PCD_REQUIRE((opts->image >= 0) != (opts->d_point_variable != nullptr),
                "exactly one of image >= 0 and d_point_variable names the variable points");
    PCD_REQUIRE(opts->d_point_variable || opts->image < src->I, "image out of range");
    PCD_HIP_TRY(hipSetDevice(src->device));
    LocalSelection sel(opts, d_point_variable_out);
    float ms = 0.f;
    PCD_TRY(window_derive(src, sel, d_obs_map, (hipStream_t)stream, window, info ? &ms : nullptr));
    if (info) {
      const pcd_ba* w = *window;
      const uint32_t* rec = w->edit_next.h_record.p;
      info->num_images_in = rec[kLwinImagesIn]; info->num_points_variable = rec[kLwinVariable];
      info->num_points_fixed = rec[kLwinFixed];
      info->num_obs = w->O; info->num_lidar = w->L; info->num_pose_rows = w->n_pose_rows;
      info->build_ms = ms;
    }
    return PCD_OK;
  });
}

// ba_window.hip -- the sphere window of a global round as a second handle, derived on the device from a live one
// (DESIGN 4.3f): pcd_ba_window_create_device, pcd_ba_window_commit_device.  The selection is the reference's
// (sfm/incremental_mapper.cc:1347-1408): images within `radius` of the centre image's projection centre are "in", a
// point is active iff one of its observations lies on an "in" image, an active point keeps all its rows and terms, every
// image that is not "in" gets a constant pose.  The passes, all on `stream`:
//   ba_clone_problem (ba_build.hip)   cameras, masks, the parameters as they are now: device-to-device copies
//   k_win_images        image -> in? (the reference's centre arithmetic, or the caller's set) and the window's pose mask
//   k_win_points        point -> active?  An OR over the rows of its track (the track CSR): one thread per point writes
//                       one byte, no scattered same-address stores.  Its complement is the removal's point_delete
//   edit_compact (ba_edit.hip)        the removal's passes with that mask: row, term and list flags, the pose-row flags
//                       taken with the WINDOW's mask, scans, compaction of both CSRs, length sort, slices, segments,
//                       the sliced-ELL and per-track LiDAR fills, the record
//   k_win_record        the two counts of the selection, summed from the per-workgroup counts the two kernels above
//                       leave, behind the removal's in the same record
//   edit_read_record    the ONE synchronisation; the image-major fill follows it
// The removal builds in the handle's own scratch and swaps; here the scratch is the NEW handle's (its edit_next), and the
// swap makes the result that handle's layout and terms.  The source is only read.  No atomics; nothing depends on the
// launch geometry.  The sequence itself is window_derive (declared in ba_handle.h): the sphere's selection here and the
// local round's (ba_local.hip) are the two WindowSelections it runs.
#include "ba_handle.h"

namespace pcd {

enum { kWinImagesIn = kRecWords, kWinPointsActive, kWinWords };

// c = -R(q)^T t with Eigen's Quaterniond(w, x, y, z).toRotationMatrix() on the stored, unnormalised quaternion
__device__ __forceinline__ void win_center(const double* __restrict__ pose, double* __restrict__ c) {
  const double w = pose[0], x = pose[1], y = pose[2], z = pose[3];
  const double t0 = pose[4], t1 = pose[5], t2 = pose[6];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double R00 = 1.0 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy;
  const double R10 = txy + twz, R11 = 1.0 - (txx + tzz), R12 = tyz - twx;
  const double R20 = txz - twy, R21 = tyz + twx, R22 = 1.0 - (txx + tyy);
  c[0] = -((R00 * t0 + R10 * t1) + R20 * t2);
  c[1] = -((R01 * t0 + R11 * t1) + R21 * t2);
  c[2] = -((R02 * t0 + R12 * t1) + R22 * t2);
}

// in[i] and the window's pose mask cpose[i] = src's | !in | extra.  set != null: the caller's flags; else the sphere
// around image `center` (every thread recomputes that centre: 40 flops against a second launch).
// part[workgroup] = its images that are in, summed by k_win_record
__global__ __launch_bounds__(256) void k_win_images(uint32_t I, const double* __restrict__ poses, int center, double radius,
                                                    const uint8_t* __restrict__ set, const uint8_t* __restrict__ src_cpose,
                                                    const uint8_t* __restrict__ extra, uint8_t* __restrict__ in,
                                                    uint8_t* __restrict__ cpose, uint32_t* __restrict__ part) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool inside = false;
  if (i < I) {
    if (set) {
      inside = set[i] != 0;
    } else {
      double c[3], cc[3];
      win_center(poses + 7 * (size_t)i, c);
      win_center(poses + 7 * (size_t)center, cc);
      const double dx = cc[0] - c[0], dy = cc[1] - c[1], dz = cc[2] - c[2];
      inside = sqrt((dx * dx + dy * dy) + dz * dz) <= radius;
    }
    in[i] = inside ? 1 : 0;
    cpose[i] = ((src_cpose && src_cpose[i]) || !inside || (extra && extra[i])) ? 1 : 0;
  }
  const int n = __syncthreads_count(inside);
  if (threadIdx.x == 0) part[blockIdx.x] = (uint32_t)n;
}

// active[p] = some row of track p is on an "in" image; pdel[p] = !active[p]; part[workgroup] = its active points
__global__ __launch_bounds__(256) void k_win_points(uint32_t P, const uint32_t* __restrict__ pt_start,
                                                    const uint32_t* __restrict__ pt_list, const int* __restrict__ obs_image,
                                                    const uint8_t* __restrict__ in, uint8_t* __restrict__ active,
                                                    uint8_t* __restrict__ pdel, uint32_t* __restrict__ part) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  bool a = false;
  if (p < P) {
    for (uint32_t k = pt_start[p], e = pt_start[p + 1]; k < e && !a; ++k) a = in[obs_image[pt_list[k]]] != 0;
    if (active) active[p] = a ? 1 : 0;
    pdel[p] = a ? 0 : 1;
  }
  const int n = __syncthreads_count(a);
  if (threadIdx.x == 0) part[blockIdx.x] = (uint32_t)n;
}

// one workgroup: the images that are in and the points that are active, from the counts of the nbi + nbp workgroups of
// the two kernels above (integer sums: any order)
__global__ __launch_bounds__(256) void k_win_record(uint32_t nbi, uint32_t nbp, const uint32_t* __restrict__ part,
                                                    uint32_t* __restrict__ rec) {
  __shared__ uint32_t s_i[256], s_p[256];
  uint32_t ni = 0, np = 0;
  for (uint32_t k = threadIdx.x; k < nbi; k += 256) ni += part[k];
  for (uint32_t k = threadIdx.x; k < nbp; k += 256) np += part[nbi + k];
  s_i[threadIdx.x] = ni; s_p[threadIdx.x] = np;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { s_i[threadIdx.x] += s_i[threadIdx.x + w]; s_p[threadIdx.x] += s_p[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { rec[kWinImagesIn] = s_i[0]; rec[kWinPointsActive] = s_p[0]; }
}

void launch_win_images(const pcd_ba* src, int center, double radius, const uint8_t* set, const uint8_t* extra, uint8_t* in,
                       uint8_t* cpose, uint32_t* part, hipStream_t s) {
  const uint32_t I = (uint32_t)src->I;
  hipLaunchKernelGGL(k_win_images, dim3(div_up(I, 256)), dim3(256), 0, s, I, src->poses.p, center, radius, set,
                     src->const_poses(), extra, in, cpose, part);
}

pcd_status window_derive(const pcd_ba* src, WindowSelection& sel, uint32_t* d_map, hipStream_t s, pcd_ba** out,
                         float* build_ms) {
  struct Destroy { void operator()(pcd_ba* p) const { pcd_ba_destroy(p); } };
  std::unique_ptr<pcd_ba, Destroy> owner(new pcd_ba());   // destroys the window on every failing return below
  pcd_ba* w = owner.get();
  BaEditScratch& N = w->edit_next;
  const uint32_t I = (uint32_t)src->I, P = (uint32_t)src->P, L = (uint32_t)src->L;
  const bool meta = src->has_lidar_meta;
  const unsigned terms = L ? kTermRows | (meta ? kTermMeta : 0u) | kTermIndex | kTermTracks : 0u;
  // every buffer before the first launch: the selection's flags, the new handle's own arrays, the layout and the terms
  PCD_TRY(sel.reserve(src, w));
  PCD_TRY(edit_reserve(src, N, terms, /*pose_rows=*/true, sel.words));
  if (!L) {   // no terms to compact: what pcd_ba_create makes of an empty list (the meta when src has it)
    PCD_TRY(w->reserve_terms(kTermRows | (meta ? kTermMeta : 0u) | kTermIndex, 0, P, 0));
  }
  PCD_TRY(reserve_cost_partial(w, (size_t)src->nslices, src->O, src->L));
  PCD_TRY(w->cost.reserve(1));
  EventPair ev;
  if (build_ms) { PCD_TRY(ev.create()); (void)ev.start(s); }
  PCD_TRY(ba_clone_problem(src, w, s));
  WindowMasks m;
  {
    ScopedKernelTimer t("ba_window_select", s);
    PCD_TRY(sel.select(src, w, s, &m));
    PCD_HIP_TRY(hipGetLastError());
  }
  if (!L) PCD_HIP_TRY(hipMemsetAsync(w->pt_lidar_start.p, 0, ((size_t)P + 1) * sizeof(uint32_t), s));
  PCD_TRY(edit_compact(src, N, m.obs_erase, m.point_delete, m.term_erase, w->image_const_pose.p, d_map, s));
  PCD_TRY(sel.record(w, s));
  PCD_HIP_TRY(hipGetLastError());
  PCD_TRY(edit_read_record(N, sel.words, I, build_ms ? &ev : nullptr, s));
  const uint32_t* rec = N.h_record.p;
  // behind the synchronisation: the fill that needs the count, then what was built becomes the window's
  launch_fill_image_major(N.layout, rec[kRecObs], s);
  PCD_HIP_TRY(hipGetLastError());
  w->swap_layout(N.layout, /*pose_rows=*/true);
  w->swap_terms(N.terms, terms);
  w->O = rec[kRecObs]; w->L = rec[kRecTerms]; w->nslices = src->nslices;
  w->nseg = rec[kRecSegs]; w->n_pose_rows = rec[kRecPoseRows];
  w->has_lidar_meta = meta;
  w->h_img_obs_start.assign(rec + sel.words, rec + sel.words + I + 1);
  w->pose_row_stale = true;   // h_pose_row: refreshed by the first pcd_ba_evaluate_blocks, as after a removal
  // The work buffers of N, sized by the source, stay with the window until it is closed (they are the scratch of its own
  // edits).  Freeing them here was measured: ~20 hipFree add 1.3 - 2.9 ms to the call's 3.4 - 4.9 ms at workload M and
  // slow the allocations of the structure build that follows.
  if (build_ms) PCD_HIP_TRY(ev.elapsed(build_ms));
  *out = owner.release();
  return PCD_OK;
}

// The sphere's selection: the images in, the active points; an inactive point is deleted with its rows and terms
struct SphereSelection : WindowSelection {
  const pcd_ba_window_opts* o;
  uint8_t* d_in;
  uint8_t* d_active;
  DevBuf<uint8_t> in_own, pdel;
  DevBuf<uint32_t> part;
  uint32_t nbi = 0, nbp = 0;   // the workgroups of k_win_images / k_win_points
  SphereSelection(const pcd_ba_window_opts* opts, uint8_t* in, uint8_t* active) : o(opts), d_in(in), d_active(active) {
    words = kWinWords;
  }
  pcd_status reserve(const pcd_ba* src, pcd_ba*) override {
    const uint32_t I = (uint32_t)src->I, P = (uint32_t)src->P;
    if (!d_in) { PCD_TRY(in_own.reserve(I)); d_in = in_own.p; }
    PCD_TRY(pdel.reserve(P));
    nbi = div_up(I, 256); nbp = div_up(P, 256);
    return part.reserve((size_t)nbi + nbp);
  }
  pcd_status select(const pcd_ba* src, pcd_ba* w, hipStream_t s, WindowMasks* m) override {
    launch_win_images(src, (int)o->center_image, o->radius, o->d_image_set, o->d_extra_const_pose, d_in,
                      w->image_const_pose.p, part.p, s);
    hipLaunchKernelGGL(k_win_points, dim3(nbp), dim3(256), 0, s, (uint32_t)src->P, src->pt_obs_start.p, src->pt_obs_list.p,
                       src->obs_image.p, d_in, d_active, pdel.p, part.p + nbi);
    m->point_delete = pdel.p;
    return PCD_OK;
  }
  pcd_status record(pcd_ba* w, hipStream_t s) override {
    hipLaunchKernelGGL(k_win_record, dim3(1), dim3(256), 0, s, nbi, nbp, part.p, w->edit_next.record.p);
    return PCD_OK;
  }
};

static pcd_status window_create(const pcd_ba* src, const pcd_ba_window_opts* o, uint8_t* d_in, uint8_t* d_active,
                                uint32_t* d_map, hipStream_t s, pcd_ba** out, pcd_ba_window_info* info) {
  SphereSelection sel(o, d_in, d_active);
  float ms = 0.f;
  PCD_TRY(window_derive(src, sel, d_map, s, out, info ? &ms : nullptr));
  if (info) {
    const pcd_ba* w = *out;
    const uint32_t* rec = w->edit_next.h_record.p;
    info->num_images_in = rec[kWinImagesIn]; info->num_points_active = rec[kWinPointsActive];
    info->num_obs = w->O; info->num_lidar = w->L; info->num_pose_rows = w->n_pose_rows;
    info->build_ms = ms;
  }
  return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" void pcd_ba_window_opts_default(pcd_ba_window_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->center_image = -1;
  o->radius = 40.0;
}

extern "C" pcd_status pcd_ba_window_create_device(pcd_ba* src, const pcd_ba_window_opts* opts, uint8_t* d_image_in,
                                                  uint8_t* d_point_active, uint32_t* d_obs_map, void* stream,
                                                  pcd_ba** window, pcd_ba_window_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    if (window) *window = nullptr;
    PCD_REQUIRE(src && opts && window, "null pointer");
    PCD_TRY(require_device(src->device));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_ba_window_create_device"));
    PCD_REQUIRE((opts->center_image >= 0) != (opts->d_image_set != nullptr),
                "exactly one of center_image >= 0 and d_image_set selects the window");
    PCD_REQUIRE(opts->d_image_set || opts->center_image < src->I, "center_image out of range");
    PCD_REQUIRE(opts->d_image_set || opts->radius >= 0.0, "radius negative or NaN");   // NaN fails the comparison
    PCD_HIP_TRY(hipSetDevice(src->device));
    return window_create(src, opts, d_image_in, d_point_active, d_obs_map, (hipStream_t)stream, window, info);
  });
}

extern "C" pcd_status pcd_ba_window_commit_device(pcd_ba* w, pcd_ba* src, void* stream) {
  return pcd::guard([&]() -> pcd_status {
    PCD_REQUIRE(w && src && w != src, "null handle");
    PCD_TRY(require_device(src->device));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_ba_window_commit_device"));
    PCD_REQUIRE(w->device == src->device, "the window and the source live on different devices");
    PCD_REQUIRE(w->I == src->I && w->P == src->P && w->cam_params_len == src->cam_params_len,
                "the window and the source differ in I, P or cam_params_len");
    PCD_HIP_TRY(hipSetDevice(src->device));
    hipStream_t s = (hipStream_t)stream;
    PCD_HIP_TRY(hipMemcpyAsync(src->poses.p, w->poses.p, 7 * (size_t)w->I * sizeof(double), hipMemcpyDeviceToDevice, s));
    PCD_HIP_TRY(hipMemcpyAsync(src->points.p, w->points.p, 3 * (size_t)w->P * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (w->refines_intrinsics && w->cam_params_len) {   // what pcd_ba_set_camera_parameters does: the device copy and the mirror
      PCD_HIP_TRY(hipMemcpyAsync(src->cam_params.p, w->cam_params.p, (size_t)w->cam_params_len * sizeof(double),
                                 hipMemcpyDeviceToDevice, s));
      src->h_cam_params.resize((size_t)w->cam_params_len);
      PCD_HIP_TRY(hipMemcpyAsync(src->h_cam_params.data(), w->cam_params.p, (size_t)w->cam_params_len * sizeof(double),
                                 hipMemcpyDeviceToHost, s));
      PCD_HIP_TRY(hipStreamSynchronize(s));   // the mirror is host memory: complete when the call returns
    }
    ba_schur_invalidate(src);   // the numeric state of the last Schur call belongs to the old parameters
    return PCD_OK;
  });
}

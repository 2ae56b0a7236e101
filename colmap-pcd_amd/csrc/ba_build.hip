// ba_build.hip -- pcd_ba_create / pcd_ba_destroy: the bundle-adjustment handle and its derived layouts.
// pcd_ba_create uploads the caller's arrays once and builds what the evaluation kernels of ba.hip read (BaDev,
// ba_handle.h), one stage per layout.  The host only sorts indices (counting sorts); the 16-byte observation payloads
// never make a second trip over PCIe and are never gathered by a host loop: two fill kernels gather them on the device
// from the uploaded arrays, on the null stream behind the synchronous uploads; pcd_ba_create waits for them once.
// The stages upload into the handle's own BaLayout / BaTerms (ba_handle.h); ba_edit.hip uses the two fill launchers too.
#include "ba_handle.h"

namespace pcd {

// sliced ELL: thread = (slice, lane): track p = order[slice*64 + lane], its j-th observation goes to slot
// slice_start[slice] + 64 j + lane
__global__ void k_ba_fill_sell(const int* __restrict__ order, const uint32_t* __restrict__ slice_start,
                               const uint32_t* __restrict__ pt_start, const uint32_t* __restrict__ pt_list,
                               const int* __restrict__ obs_image, const double* __restrict__ obs_xy, int nslices,
                               int* __restrict__ sell_img, double* __restrict__ sell_xy) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int slice = t >> 6, lane = t & 63;
  if (slice >= nslices) return;
  const uint32_t s0 = slice_start[slice], width = (slice_start[slice + 1] - s0) >> 6;
  const int p = order[t];
  const uint32_t b = p >= 0 ? pt_start[p] : 0u, len = p >= 0 ? pt_start[p + 1] - b : 0u;
  for (uint32_t j = 0; j < width; ++j) {
    const size_t slot = (size_t)s0 + 64 * (size_t)j + lane;
    if (j < len) {
      const uint32_t o = pt_list[b + j];
      sell_img[slot] = obs_image[o];
      const double2 xy = *reinterpret_cast<const double2*>(obs_xy + 2 * (size_t)o);
      *reinterpret_cast<double2*>(sell_xy + 2 * slot) = xy;
    } else {
      sell_img[slot] = -1;   // padding of a shorter track
      *reinterpret_cast<double2*>(sell_xy + 2 * slot) = make_double2(0.0, 0.0);
    }
  }
}
void launch_fill_sell(const BaLayout& y, int nslices, hipStream_t s) {
  hipLaunchKernelGGL(k_ba_fill_sell, dim3(div_up((size_t)nslices * 64, 256)), dim3(256), 0, s, y.pt_order.p, y.slice_start.p,
                     y.pt_obs_start.p, y.pt_obs_list.p, y.obs_image.p, y.obs_xy.p, nslices, y.sell_img.p, y.sell_xy.p);
}
// image-major copies: e-th observation of the image-major order = observation img_obs[e] of the caller's order
__global__ void k_ba_fill_image_major(const uint32_t* __restrict__ img_obs, const int* __restrict__ obs_point,
                                      const double* __restrict__ obs_xy, uint64_t O, int* __restrict__ img_pt,
                                      double* __restrict__ img_xy) {
  const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (e >= O) return;
  const uint32_t o = img_obs[e];
  img_pt[e] = obs_point[o];
  *reinterpret_cast<double2*>(img_xy + 2 * e) = *reinterpret_cast<const double2*>(obs_xy + 2 * (size_t)o);
}

void launch_fill_image_major(const BaLayout& y, uint64_t O, hipStream_t s) {
  if (!O) return;
  hipLaunchKernelGGL(k_ba_fill_image_major, dim3(div_up(O, 256)), dim3(256), 0, s, y.img_obs.p, y.obs_point.p, y.obs_xy.p, O,
                     y.img_pt.p, y.img_xy.p);
}

// What upload_problem and build_image_layout make of the description, taken from a handle that has it already: no
// payload goes through the host.  The rows, the terms and everything derived from them are the caller's to build.
// Every buffer is reserved before the first copy is enqueued.
pcd_status ba_clone_problem(const pcd_ba* a, pcd_ba* b, hipStream_t s) {
  b->device = a->device;
  b->C = a->C; b->I = a->I; b->P = a->P;
  b->loss_type = a->loss_type; b->loss_scale = a->loss_scale;
  b->cam_params_len = a->cam_params_len; b->cam_stride = a->cam_stride;
  b->uniform_model = a->uniform_model; b->shared_cam = a->shared_cam;
  b->h_cam_params = a->h_cam_params; b->h_cam_model = a->h_cam_model; b->h_cam_off = a->h_cam_off;
  b->h_image_cam = a->h_image_cam;
  b->refines_intrinsics = a->refines_intrinsics;
  b->h_cam_slot = a->h_cam_slot; b->h_slot_cam = a->h_slot_cam; b->h_param_cam = a->h_param_cam;
  b->h_cam_active = a->h_cam_active;
  b->has_cpose = true; b->has_ctvec = a->has_ctvec; b->has_cpt = a->has_cpt; b->has_refine = a->has_refine;
  struct Copy { void* dst; const void* src; size_t bytes; };
  std::vector<Copy> copies;
  auto plan = [&](auto& dst, const auto& src, size_t n) -> pcd_status {   // n elements of a's buffer into b's
    PCD_TRY(dst.reserve(at_least_1(n)));
    if (n) copies.push_back(Copy{dst.p, src.p, n * sizeof(*dst.p)});
    return PCD_OK;
  };
  const size_t C = (size_t)a->C, I = (size_t)a->I, P = (size_t)a->P, K = (size_t)a->cam_params_len;
  PCD_TRY(plan(b->cam_model, a->cam_model, C)); PCD_TRY(plan(b->cam_off, a->cam_off, C));
  PCD_TRY(plan(b->cam_params, a->cam_params, K));
  PCD_TRY(plan(b->poses, a->poses, 7 * I)); PCD_TRY(plan(b->image_cam, a->image_cam, I));
  PCD_TRY(plan(b->points, a->points, 3 * P));
  PCD_TRY(plan(b->cam_img_start, a->cam_img_start, C + 1)); PCD_TRY(plan(b->cam_img_list, a->cam_img_list, I));
  PCD_TRY(b->image_const_pose.reserve(at_least_1(I)));
  if (a->has_ctvec) PCD_TRY(plan(b->image_const_tvec, a->image_const_tvec, I));
  if (a->has_cpt) PCD_TRY(plan(b->point_const, a->point_const, P));
  if (a->has_refine) PCD_TRY(plan(b->cam_refine, a->cam_refine, K));
  for (const Copy& c : copies) PCD_HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, s));
  return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

// stable counting sort of element ids by key -> CSR (start[nkeys+1], list[n])
static void build_csr(const int32_t* key, uint64_t n, int nkeys, std::vector<uint32_t>& start,
                      std::vector<uint32_t>& list) {
  start.assign((size_t)nkeys + 1, 0);
  for (uint64_t i = 0; i < n; ++i) start[(size_t)key[i] + 1]++;
  for (int k = 0; k < nkeys; ++k) start[k + 1] += start[k];
  list.resize(n);
  std::vector<uint32_t> cur(start.begin(), start.end() - 1);
  for (uint64_t i = 0; i < n; ++i) list[cur[key[i]]++] = (uint32_t)i;
}

#define UP(buf, src, n) PCD_TRY(upload(b->buf, src, (size_t)(n)))

// ---- the stages of pcd_ba_create, in the order it runs them ---------------------------------------------------
// the description alone, before any device is touched
static pcd_status check_desc(const pcd_ba_desc* d) {
  PCD_REQUIRE(d->num_cameras > 0 && d->cam_model && d->cam_param_offset && d->cam_params, "cameras");
  PCD_REQUIRE(d->num_images > 0 && d->poses && d->image_camera, "images");
  PCD_REQUIRE(d->num_points > 0 && d->points, "points");
  PCD_REQUIRE(d->num_obs == 0 || (d->obs_image && d->obs_point && d->obs_xy), "observations");
  PCD_REQUIRE(d->num_lidar == 0 || (d->lidar_point && d->lidar_abcd && d->lidar_weight), "lidar terms");
  PCD_REQUIRE(d->loss_type >= 0 && d->loss_type <= 2, "loss_type");
  PCD_REQUIRE(d->loss_type == PCD_LOSS_TRIVIAL || d->loss_scale > 0, "loss_scale");
  PCD_REQUIRE(d->num_obs < 0xFFFFFFF0ull && d->num_lidar < 0xFFFFFFF0ull, "too many residual blocks");
  for (int c = 0; c < d->num_cameras; ++c) {
    const int k = pcd_camera_num_params(d->cam_model[c]);
    PCD_REQUIRE(k > 0, "unknown camera model id");  // reference: std::domain_error, camera_models.h:140
    PCD_REQUIRE(d->cam_param_offset[c] >= 0 && (uint64_t)d->cam_param_offset[c] + k <= d->cam_params_len,
                "camera parameter offsets");
  }
  for (int i = 0; i < d->num_images; ++i)
    PCD_REQUIRE(d->image_camera[i] >= 0 && d->image_camera[i] < d->num_cameras, "image_camera out of range");
  for (uint64_t o = 0; o < d->num_obs; ++o) {
    PCD_REQUIRE(d->obs_image[o] >= 0 && d->obs_image[o] < d->num_images, "obs_image out of range");
    PCD_REQUIRE(d->obs_point[o] >= 0 && d->obs_point[o] < d->num_points, "obs_point out of range");
  }
  for (uint64_t l = 0; l < d->num_lidar; ++l)
    PCD_REQUIRE(d->lidar_point[l] >= 0 && d->lidar_point[l] < d->num_points, "lidar_point out of range");
  return PCD_OK;
}

// sizes, loss, what the cameras have in common (uniform_model, shared_cam, cam_stride); then the caller's arrays and
// the constness / refine flags, as given
static pcd_status upload_problem(const pcd_ba_desc* d, pcd_ba* b) {
  b->device = d->device;
  b->C = d->num_cameras; b->I = d->num_images; b->P = d->num_points; b->O = d->num_obs; b->L = d->num_lidar;
  b->loss_type = d->loss_type; b->loss_scale = d->loss_scale;
  b->cam_params_len = d->cam_params_len;
  for (int c = 0; c < d->num_cameras; ++c) b->cam_stride = std::max(b->cam_stride, cam_num_params(d->cam_model[c]));
  b->uniform_model = d->cam_model[0];
  for (int c = 1; c < d->num_cameras; ++c)
    if (d->cam_model[c] != b->uniform_model) b->uniform_model = -1;
  b->shared_cam = d->image_camera[0];
  for (int i = 1; i < d->num_images; ++i)
    if (d->image_camera[i] != b->shared_cam) b->shared_cam = -1;
  UP(cam_model, d->cam_model, b->C); UP(cam_off, d->cam_param_offset, b->C); UP(cam_params, d->cam_params, d->cam_params_len);
  b->h_cam_model.assign(d->cam_model, d->cam_model + b->C); b->h_cam_off.assign(d->cam_param_offset, d->cam_param_offset + b->C);
  b->h_cam_params.assign(d->cam_params, d->cam_params + d->cam_params_len);
  b->h_image_cam.assign(d->image_camera, d->image_camera + b->I);
  UP(poses, d->poses, 7 * (size_t)b->I); UP(image_cam, d->image_camera, b->I);
  UP(points, d->points, 3 * (size_t)b->P);
  UP(obs_image, d->obs_image, b->O); UP(obs_point, d->obs_point, b->O); UP(obs_xy, d->obs_xy, 2 * b->O);
  UP(lidar_point, d->lidar_point, b->L); UP(lidar_abcd, d->lidar_abcd, 4 * b->L); UP(lidar_w, d->lidar_weight, b->L);
  if (d->image_const_pose) { b->has_cpose = true; UP(image_const_pose, d->image_const_pose, b->I); }
  if (d->image_const_tvec) { b->has_ctvec = true; UP(image_const_tvec, d->image_const_tvec, b->I); }
  if (d->point_const) { b->has_cpt = true; UP(point_const, d->point_const, b->P); }
  if (d->camera_refine) { b->has_refine = true; UP(cam_refine, d->camera_refine, d->cam_params_len); }
  for (uint64_t k = 0; d->camera_refine && k < d->cam_params_len; ++k) b->refines_intrinsics |= d->camera_refine[k] != 0;
  // camera slots of the reduced system with refined intrinsics (pcd_ba_schur_cam*)
  b->h_cam_slot.assign(b->C, -1); b->h_param_cam.assign(d->cam_params_len, -1);
  for (int c = 0; c < b->C; ++c) {
    const int K = cam_num_params(d->cam_model[c]);
    uint8_t act[PCD_CAM_JAC_STRIDE] = {};
    bool any = false;
    for (int j = 0; j < K && (uint64_t)d->cam_param_offset[c] + j < d->cam_params_len; ++j) {
      b->h_param_cam[d->cam_param_offset[c] + j] = c;
      act[j] = d->camera_refine && d->camera_refine[d->cam_param_offset[c] + j] != 0;
      any |= act[j] != 0;
    }
    if (!any) continue;
    b->h_cam_slot[c] = (int)b->h_slot_cam.size();
    b->h_slot_cam.push_back(c);
    b->h_cam_active.insert(b->h_cam_active.end(), act, act + PCD_CAM_JAC_STRIDE);
  }
  return PCD_OK;
}

// The track CSR (pt_obs_start / pt_obs_list) and the per-track sliced ELL in order of track length (nslices, pt_order,
// slice_start, sell_img / sell_xy: k_ba_fill_sell, enqueued).  order = thread of k_ba_points -> point (-1: padding).
static pcd_status build_track_layout(const pcd_ba_desc* d, pcd_ba* b, std::vector<int>& order) {
  std::vector<uint32_t> st, li;
  build_csr(d->obs_point, b->O, b->P, st, li);
  // tracks in ascending order of length, ties in ascending point id: a counting sort (lengths are small numbers)
  uint32_t maxlen = 0;
  for (int p = 0; p < b->P; ++p) maxlen = std::max(maxlen, st[p + 1] - st[p]);
  std::vector<uint32_t> bucket((size_t)maxlen + 2, 0);
  for (int p = 0; p < b->P; ++p) bucket[(size_t)(st[p + 1] - st[p]) + 1]++;
  for (size_t k = 1; k < bucket.size(); ++k) bucket[k] += bucket[k - 1];
  const int nslices = (b->P + 63) / 64;
  b->nslices = nslices;
  order.assign((size_t)nslices * 64, -1);
  for (int p = 0; p < b->P; ++p) order[bucket[st[p + 1] - st[p]]++] = p;
  std::vector<uint32_t> slice_start(nslices + 1, 0);
  for (int s = 0; s < nslices; ++s) {
    // ascending lengths: the longest track of a slice is its last real one
    uint32_t mx = 0;
    for (int l = 63; l >= 0; --l) {
      const int p = order[(size_t)s * 64 + l];
      if (p >= 0) { mx = st[p + 1] - st[p]; break; }
    }
    slice_start[s + 1] = slice_start[s] + mx * 64;
  }
  const size_t nslots = slice_start[nslices];
  UP(pt_order, order.data(), order.size());
  UP(slice_start, slice_start.data(), slice_start.size());
  UP(pt_obs_start, st.data(), st.size()); UP(pt_obs_list, li.data(), li.size());
  PCD_TRY(b->reserve_sell(nslots));
  if (nslots) launch_fill_sell(*b, nslices, nullptr);
  return PCD_OK;
}

// The LiDAR CSR (pt_lidar_start / pt_lidar_list) and, when the handle has terms, those of every track in thread
// order: how many, and the first (BaDev::pt_lidar_cnt, pt_lidar_first)
static pcd_status build_lidar_layout(const pcd_ba_desc* d, pcd_ba* b, const std::vector<int>& order) {
  std::vector<uint32_t> st, li;
  build_csr(d->lidar_point, b->L, b->P, st, li);
  UP(pt_lidar_start, st.data(), st.size()); UP(pt_lidar_list, li.data(), li.size());
  if (!b->L) return PCD_OK;
  const size_t ntr = order.size();
  std::vector<double> first(5 * ntr, 0.0);
  std::vector<uint32_t> cnt(ntr, 0);
  for (size_t t = 0; t < ntr; ++t) {
    const int p = order[t];
    if (p < 0 || st[p] == st[p + 1]) continue;
    cnt[t] = st[p + 1] - st[p];
    const uint32_t l = li[st[p]];
    for (int k = 0; k < 4; ++k) first[k * ntr + t] = d->lidar_abcd[4 * (size_t)l + k];
    first[4 * ntr + t] = d->lidar_weight[l];
  }
  UP(pt_lidar_first, first.data(), first.size());
  UP(pt_lidar_cnt, cnt.data(), cnt.size());
  return PCD_OK;
}

// The image-major order (img_obs_start, img_obs), its segments (nseg, seg_img, seg_begin, img_seg_start), the images
// of each camera (cam_img_start / cam_img_list) and the image-major copies (img_pt / img_xy: k_ba_fill_image_major, enqueued)
static pcd_status build_image_layout(const pcd_ba_desc* d, pcd_ba* b) {
  std::vector<uint32_t> st, li;
  build_csr(d->obs_image, b->O, b->I, st, li);
  UP(img_obs_start, st.data(), st.size());
  b->h_img_obs_start = st;
  // segments of <= kImgSeg observations, never spanning two images (an image without observations has none)
  std::vector<uint32_t> seg_img, seg_begin, img_seg_start(b->I + 1, 0);
  for (int i = 0; i < b->I; ++i) {
    img_seg_start[i] = (uint32_t)seg_img.size();
    for (uint32_t e = st[i]; e < st[i + 1]; e += kImgSeg) { seg_img.push_back((uint32_t)i); seg_begin.push_back(e); }
  }
  img_seg_start[b->I] = (uint32_t)seg_img.size();
  b->nseg = (uint32_t)seg_img.size();
  seg_begin.push_back((uint32_t)b->O);
  UP(seg_img, seg_img.data(), seg_img.size());
  UP(seg_begin, seg_begin.data(), seg_begin.size());
  UP(img_seg_start, img_seg_start.data(), img_seg_start.size());
  std::vector<uint32_t> cst, cli;   // images of each camera, ascending
  build_csr(d->image_camera, (uint64_t)b->I, b->C, cst, cli);
  UP(cam_img_start, cst.data(), cst.size());
  UP(cam_img_list, cli.data(), cli.size());
  UP(img_obs, li.data(), li.size());
  PCD_TRY(b->img_pt.reserve(std::max<size_t>(b->O, 1)));
  PCD_TRY(b->img_xy.reserve(std::max<size_t>(2 * b->O, 2)));
  launch_fill_image_major(*b, b->O, nullptr);
  return PCD_OK;
}

// rows of the packed pose Jacobians (pcd_ba_evaluate_blocks): h_pose_row, n_pose_rows, vobs
static pcd_status build_pose_rows(const pcd_ba_desc* d, pcd_ba* b) {
  b->h_pose_row.assign(b->O, 0xFFFFFFFFu);
  std::vector<uint32_t> vobs;
  vobs.reserve(b->O);
  for (uint64_t o = 0; o < b->O; ++o)
    if (!(d->image_const_pose && d->image_const_pose[d->obs_image[o]])) {
      b->h_pose_row[o] = (uint32_t)vobs.size();
      vobs.push_back((uint32_t)o);
    }
  b->n_pose_rows = vobs.size();
  if (b->n_pose_rows != b->O) UP(vobs, vobs.data(), vobs.size());
  return PCD_OK;
}
#undef UP

extern "C" {

pcd_status pcd_ba_create(const pcd_ba_desc* d, pcd_ba** out) {
  return pcd::guard([&]() -> pcd_status {
  PCD_REQUIRE(d && out, "null pointer");
  *out = nullptr;
  PCD_TRY(check_desc(d));
  PCD_TRY(require_device(d->device));
  struct Destroy { void operator()(pcd_ba* p) const { pcd_ba_destroy(p); } };
  std::unique_ptr<pcd_ba, Destroy> owner(new pcd_ba());   // destroys the handle on every failing return below
  pcd_ba* b = owner.get();
  std::vector<int> order;   // thread of k_ba_points -> point: the track stage makes it, the LiDAR stage follows it
  PCD_TRY(upload_problem(d, b));
  PCD_TRY(build_track_layout(d, b, order));
  PCD_TRY(build_lidar_layout(d, b, order));
  PCD_TRY(build_image_layout(d, b));
  PCD_TRY(build_pose_rows(d, b));
  // one cost partial per workgroup of whichever of the two cost-producing kernels has the larger grid (cost_blocks)
  PCD_TRY(reserve_cost_partial(b, (size_t)b->nslices, b->O, b->L));
  PCD_TRY(b->cost.reserve(1));
  // the two fill kernels ran on the null stream behind the synchronous uploads: one wait, one check
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) {
    set_error("pcd_ba_create: filling the derived layouts (per-track sliced ELL, image-major copies) failed");
    return PCD_ERR_HIP;
  }
  *out = owner.release();
  return PCD_OK;
  });
}

void pcd_ba_destroy(pcd_ba* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

}  // extern "C"

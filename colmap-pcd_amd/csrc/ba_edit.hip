// ba_edit.hip -- observations and points dropped from a live BA handle on the device:
// pcd_ba_remove_observations_device.  What pcd_ba_create (ba_build.hip) derives on the host from the caller's
// observation and term lists is derived here from the handle's own device arrays and two flag arrays, byte for byte.
// Dropping rows keeps the order of the rest, so every list of the old handle, read through one scan of its keep flags,
// is the list of the new one; only the order of the tracks by length is sorted anew.  The passes, all on `stream`:
//   k_edit_obs_flag / k_edit_term_flag   row -> kept?  (n + 1 flags, the last 0: the scan's last value is the count)
//   k_edit_list_flag                     the same flags in the order of a CSR's list (track, image, point -> terms)
//   k_edit_vobs_flag                     kept and of a variable pose (only with constant poses)
//   exclusive_sum                        flags -> new index; one per order
//   k_edit_compact_obs / _terms / _list  kept rows and list entries to their new places, renumbered; obs_map
//   k_edit_starts                        new CSR bounds: the scan value at the old bound
//   k_edit_lengths, sort_pairs           track lengths; point ids stably by length = pcd_ba_create's counting sort
//   k_edit_slice_width, exclusive_sum    64 x the longest track of every slice -> slice_start
//   k_edit_seg_count, exclusive_sum, k_edit_segs   segments of <= kImgSeg observations per image
//   k_ba_fill_sell, k_ba_fill_image_major, k_lidar_tracks   the fills pcd_ba_create and ba_lidar.hip use
//   k_edit_record                        the counts the host reads (the ONE synchronisation), with img_obs_start
// No atomics; nothing depends on the launch geometry.  The new state is a BaLayout and a BaTerms (ba_handle.h) built in
// pcd_ba::edit_next, every buffer of it reserved before the first launch, and swapped in at the end.  Both edits go through
// edit_reserve_shared, edit_derive, edit_read_record (the synchronisation) and edit_commit (the tail behind it).  The
// removal's passes up to the record are edit_reserve / edit_compact (declared in ba_handle.h): they only read the handle
// and take the scratch to build in, so the window derivation (ba_window.hip) runs the same passes into a new handle.
//
// pcd_ba_add_observations_device is the growing edit: rows and points appended.  Its passes:
//   k_add_keys, sort_pairs               the new rows' keys (clamped, with the verdict on their range) sorted stably, once
//                                        by point and once by image
//   k_add_lower, k_add_starts            new rows in front of every key (a lower bound per key) -> the new CSR bounds
//   k_add_move_old / k_add_place_new     old list entries shifted, new ones behind them in input order
//   k_add_vflag, exclusive_sum, k_add_vobs   the packed pose rows, the new ones appended
//   edit_derive                          the tail both edits share: lengths, length sort, slices, segments, k_lidar_tracks
//   k_add_record                         verdict and counts (the ONE synchronisation); the two fills follow it (edit_commit)
#include "ba_handle.h"
#include "prim.h"

namespace pcd {

constexpr uint32_t kDropped = 0xFFFFFFFFu;

// flag[o] = 1: observation o stays.  Thread O writes the closing 0.
__global__ __launch_bounds__(256) void k_edit_obs_flag(uint32_t O, const uint8_t* __restrict__ erase,
                                                       const uint8_t* __restrict__ pdel, const int* __restrict__ obs_point,
                                                       uint32_t* __restrict__ flag) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o > O) return;
  flag[o] = (o < O && !(erase && erase[o]) && !(pdel && pdel[obs_point[o]])) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_edit_term_flag(uint32_t L, const uint8_t* __restrict__ erase,
                                                        const uint8_t* __restrict__ pdel,
                                                        const int* __restrict__ lidar_point, uint32_t* __restrict__ flag) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l > L) return;
  flag[l] = (l < L && !(erase && erase[l]) && !(pdel && pdel[lidar_point[l]])) ? 1u : 0u;
}
// out[k] = flag[list[k]], out[n] = 0
__global__ __launch_bounds__(256) void k_edit_list_flag(uint32_t n, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ flag, uint32_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > n) return;
  out[k] = k < n ? flag[list[k]] : 0u;
}
__global__ __launch_bounds__(256) void k_edit_vobs_flag(uint32_t O, const uint32_t* __restrict__ flag,
                                                        const int* __restrict__ obs_image, const uint8_t* __restrict__ cpose,
                                                        uint32_t* __restrict__ out) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o > O) return;
  out[o] = (o < O && flag[o] && !cpose[obs_image[o]]) ? 1u : 0u;
}

// kept observation o -> row pos[o]; obs_map (may be null) for every old observation; the packed pose rows (v_flag null:
// no constant pose, no vobs)
__global__ __launch_bounds__(256) void k_edit_compact_obs(uint32_t O, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ pos, const int* __restrict__ obs_image,
                                                          const int* __restrict__ obs_point, const double* __restrict__ obs_xy,
                                                          const uint32_t* __restrict__ v_flag, const uint32_t* __restrict__ v_pos,
                                                          int* __restrict__ n_image, int* __restrict__ n_point,
                                                          double* __restrict__ n_xy, uint32_t* __restrict__ vobs,
                                                          uint32_t* __restrict__ obs_map) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o >= O) return;
  const bool keep = flag[o] != 0;
  const uint32_t t = pos[o];
  if (obs_map) obs_map[o] = keep ? t : kDropped;
  if (!keep) return;
  n_image[t] = obs_image[o];
  n_point[t] = obs_point[o];
  *reinterpret_cast<double2*>(n_xy + 2 * (size_t)t) = *reinterpret_cast<const double2*>(obs_xy + 2 * (size_t)o);
  if (v_flag && v_flag[o]) vobs[v_pos[o]] = t;
}
// type / xyz (the meta of pcd_ba_set_lidar_device) only when the handle has them
__global__ __launch_bounds__(256) void k_edit_compact_terms(uint32_t L, const uint32_t* __restrict__ flag,
                                                            const uint32_t* __restrict__ pos, const int* __restrict__ point,
                                                            const double* __restrict__ abcd, const double* __restrict__ w,
                                                            const uint8_t* __restrict__ type, const double* __restrict__ xyz,
                                                            int* __restrict__ n_point, double* __restrict__ n_abcd,
                                                            double* __restrict__ n_w, uint8_t* __restrict__ n_type,
                                                            double* __restrict__ n_xyz) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= L || !flag[l]) return;
  const uint32_t t = pos[l];
  n_point[t] = point[l];
  for (int k = 0; k < 4; ++k) n_abcd[4 * (size_t)t + k] = abcd[4 * (size_t)l + k];
  n_w[t] = w[l];
  if (type) {
    n_type[t] = type[l];
    for (int k = 0; k < 3; ++k) n_xyz[3 * (size_t)t + k] = xyz[3 * (size_t)l + k];
  }
}
// kept entry k of a CSR's list -> entry l_pos[k], holding the new index of its row
__global__ __launch_bounds__(256) void k_edit_compact_list(uint32_t n, const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ l_flag, const uint32_t* __restrict__ l_pos,
                                                           const uint32_t* __restrict__ pos, uint32_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n || !l_flag[k]) return;
  out[l_pos[k]] = pos[list[k]];
}
// start[key] for key = 0 .. nkeys: the kept entries in front of the old bound (l_pos has the list's n + 1 scan values)
__global__ __launch_bounds__(256) void k_edit_starts(uint32_t nkeys, const uint32_t* __restrict__ old_start,
                                                     const uint32_t* __restrict__ l_pos, uint32_t* __restrict__ start) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > nkeys) return;
  start[k] = l_pos[old_start[k]];
}
__global__ __launch_bounds__(256) void k_edit_lengths(uint32_t P, const uint32_t* __restrict__ start,
                                                      uint32_t* __restrict__ len, uint32_t* __restrict__ iota) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= P) return;
  len[p] = start[p + 1] - start[p];
  iota[p] = p;
}
// threads behind the P tracks are padding (-1); width[s] = 64 x the length of the last real track of slice s (ascending
// lengths: its longest), width[nslices] = 0 closes the scan
__global__ __launch_bounds__(256) void k_edit_slice_width(uint32_t P, uint32_t nslices, const uint32_t* __restrict__ len_sorted,
                                                          int* __restrict__ order, uint32_t* __restrict__ width) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= P && t < nslices * 64u) order[t] = -1;
  if (t > nslices) return;
  uint32_t w = 0;
  if (t < nslices) {
    const uint32_t last = min(t * 64u + 63u, P - 1u);
    w = len_sorted[last] * 64u;
  }
  width[t] = w;
}
__global__ __launch_bounds__(256) void k_edit_seg_count(uint32_t I, const uint32_t* __restrict__ img_start,
                                                        uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > I) return;
  cnt[i] = i < I ? (img_start[i + 1] - img_start[i] + kImgSeg - 1u) / kImgSeg : 0u;
}
// thread = image: its segments; thread I closes seg_begin with the number of observations
__global__ __launch_bounds__(256) void k_edit_segs(uint32_t I, const uint32_t* __restrict__ img_start,
                                                   const uint32_t* __restrict__ img_seg_start, uint32_t* __restrict__ seg_img,
                                                   uint32_t* __restrict__ seg_begin) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > I) return;
  if (i == I) { seg_begin[img_seg_start[I]] = img_start[I]; return; }
  uint32_t j = img_seg_start[i];
  for (uint32_t e = img_start[i]; e < img_start[i + 1]; e += kImgSeg, ++j) { seg_img[j] = i; seg_begin[j] = e; }
}
// one workgroup: the counts; emptied = points that had observations and have none now (an integer sum: any order)
__global__ __launch_bounds__(256) void k_edit_record(uint32_t O, uint32_t L, uint32_t I, uint32_t P,
                                                     const uint32_t* __restrict__ pos, const uint32_t* __restrict__ l_pos,
                                                     const uint32_t* __restrict__ img_seg_start, const uint32_t* __restrict__ v_pos,
                                                     const uint32_t* __restrict__ old_start, const uint32_t* __restrict__ start,
                                                     uint32_t* __restrict__ rec) {
  __shared__ uint32_t s_n[256];
  uint32_t n = 0;
  for (uint32_t p = threadIdx.x; p < P; p += 256)
    n += (old_start[p + 1] != old_start[p] && start[p + 1] == start[p]) ? 1u : 0u;
  s_n[threadIdx.x] = n;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s_n[threadIdx.x] += s_n[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    rec[kRecObs] = pos[O];
    rec[kRecTerms] = l_pos ? l_pos[L] : 0u;
    rec[kRecSegs] = img_seg_start[I];
    rec[kRecPoseRows] = v_pos ? v_pos[O] : pos[O];
    rec[kRecEmptied] = s_n[0];
  }
}

static dim3 grid(uint64_t n) { return dim3(div_up(n, 256)); }   // of 256 threads
static pcd_status scan_flags(BaEditScratch& N, const uint32_t* flag, uint32_t* pos, size_t n, hipStream_t s) {
  return exclusive_sum(N.prim, flag, pos, 0u, n, s);
}

// What both edits derive from the new CSRs in N.layout (pt_obs_start / pt_obs_list, img_obs_start) and the new rows
// (obs_image, obs_xy): the tracks in order of length (pt_order, slice_start), the sliced-ELL copies (fill_sell: when they
// are reserved already), the segments of the images and the per-track copies of N.terms in the new thread order, from
// N.terms' own pt_lidar_start and the list, planes and weights of `rows` (null: the handle has no terms).  P, nslices and
// O are those of the new layout; O only bounds a track's length.
static pcd_status edit_derive(BaEditScratch& N, uint32_t P, uint32_t I, uint32_t nslices, uint64_t O, bool fill_sell,
                              const BaTerms* rows, hipStream_t s) {
  BaLayout& Y = N.layout;
  const uint32_t ntr = nslices * 64u;
  // tracks in ascending order of length, ties in ascending point id; a length is at most O
  hipLaunchKernelGGL(k_edit_lengths, grid(P), dim3(256), 0, s, P, Y.pt_obs_start.p, N.len.p, N.iota.p);
  PCD_TRY(sort_pairs(N.prim, N.len.p, N.len_sorted.p, N.iota.p, reinterpret_cast<uint32_t*>(Y.pt_order.p), (size_t)P, 0u,
                     key_bits(O), s));
  hipLaunchKernelGGL(k_edit_slice_width, grid(std::max<uint64_t>(ntr, (uint64_t)nslices + 1)), dim3(256), 0, s, P, nslices,
                     N.len_sorted.p, Y.pt_order.p, N.width.p);
  PCD_TRY(scan_flags(N, N.width.p, Y.slice_start.p, (size_t)nslices + 1, s));
  if (fill_sell) launch_fill_sell(Y, (int)nslices, s);
  // segments of the images
  hipLaunchKernelGGL(k_edit_seg_count, grid((uint64_t)I + 1), dim3(256), 0, s, I, Y.img_obs_start.p, N.seg_cnt.p);
  PCD_TRY(scan_flags(N, N.seg_cnt.p, Y.img_seg_start.p, (size_t)I + 1, s));
  hipLaunchKernelGGL(k_edit_segs, grid((uint64_t)I + 1), dim3(256), 0, s, I, Y.img_obs_start.p, Y.img_seg_start.p,
                     Y.seg_img.p, Y.seg_begin.p);
  if (rows) launch_lidar_tracks(Y, (int)nslices, *rows, N.terms, s);
  return PCD_OK;
}

// What both edits reserve ahead of their first launch: the layout under construction at the sizes z, the work buffers
// of edit_derive, the record (`words` counts, then img_obs_start)
static pcd_status edit_reserve_shared(BaEditScratch& N, const BaLayoutSizes& z, size_t words) {
  PCD_TRY(N.layout.reserve_layout(z));
  PCD_TRY(N.len.reserve(z.P)); PCD_TRY(N.len_sorted.reserve(z.P)); PCD_TRY(N.iota.reserve(z.P));
  PCD_TRY(N.width.reserve(z.nslices + 1)); PCD_TRY(N.seg_cnt.reserve(z.I + 1));
  PCD_TRY(N.record.reserve(words)); PCD_TRY(N.h_record.reserve(words + z.I + 1));
  return PCD_OK;
}

// The one synchronisation of an edit: the record and the image bounds (O(I) bytes) arrive in N.h_record.  rebuild_ms ends
// here: the wait completes the event, no second one is needed.
pcd_status edit_read_record(BaEditScratch& N, size_t words, uint32_t I, EventPair* ev, hipStream_t s) {
  PCD_HIP_TRY(hipMemcpyAsync(N.h_record.p, N.record.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipMemcpyAsync(N.h_record.p + words, N.layout.img_obs_start.p, ((size_t)I + 1) * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, s));
  if (ev) (void)ev->stop(s);
  PCD_HIP_TRY(hipStreamSynchronize(s));
  return PCD_OK;
}

// The tail of both edits behind that synchronisation: the fills that need a count of the record, then success -- what was
// built (the layout, the groups `terms` of the terms, the grown points when P grows) becomes the handle's with the counts c
// and the record's image bounds; the retired buffers are the next edit's.  nslots null: the sliced-ELL copies are filled.
struct EditCounts { uint32_t O, L, P, nslices, nseg, n_pose_rows; };
static pcd_status edit_commit(pcd_ba* b, const EditCounts& c, const uint32_t* nslots, unsigned terms, size_t words,
                              EventPair* ev, float* rebuild_ms, hipStream_t s) {
  BaEditScratch& N = b->edit_next;
  if (nslots) {
    PCD_TRY(N.layout.reserve_sell(*nslots));
    if (*nslots) launch_fill_sell(N.layout, (int)c.nslices, s);
  }
  launch_fill_image_major(N.layout, c.O, s);
  PCD_HIP_TRY(hipGetLastError());
  b->swap_layout(N.layout, b->has_cpose);
  b->swap_terms(N.terms, terms);
  if (c.P != (uint32_t)b->P) { b->points.swap(N.points); if (b->has_cpt) b->point_const.swap(N.point_const); }
  b->O = c.O; b->L = c.L; b->P = (int)c.P; b->nslices = (int)c.nslices;
  b->nseg = c.nseg; b->n_pose_rows = c.n_pose_rows;
  b->h_img_obs_start.assign(N.h_record.p + words, N.h_record.p + words + b->I + 1);
  b->pose_row_stale = true;
  ba_schur_drop_structure(b);
  if (ev) PCD_HIP_TRY(ev->elapsed(rebuild_ms));
  return PCD_OK;
}

// Every buffer the compaction writes, at the sizes of the handle as it is: nothing grows when rows are dropped, so nothing
// is allocated after the first launch
pcd_status edit_reserve(const pcd_ba* b, BaEditScratch& N, unsigned terms, bool pose_rows, size_t words) {
  const size_t O = b->O, L = b->L, P = (size_t)b->P, I = (size_t)b->I, ns = (size_t)b->nslices;
  // slices only get narrower: the sliced-ELL copies at the live capacity
  PCD_TRY(edit_reserve_shared(N, BaLayoutSizes{O, P, I, ns, b->nseg, pose_rows, b->sell_img.n, b->sell_xy.n}, words));
  if (pose_rows) { PCD_TRY(N.v_flag.reserve(O + 1)); PCD_TRY(N.v_pos.reserve(O + 1)); }
  for (DevBuf<uint32_t>* d : {&N.flag, &N.pos, &N.t_flag, &N.t_pos, &N.i_flag, &N.i_pos}) PCD_TRY(d->reserve(O + 1));
  PCD_TRY(N.terms.reserve_terms(terms, L, P, ns * 64));
  if (L) for (DevBuf<uint32_t>* d : {&N.lf, &N.lp, &N.lt_flag, &N.lt_pos}) PCD_TRY(d->reserve(L + 1));
  size_t need = 0;
  PCD_TRY(prim_storage_u32({O + 1, L + 1, ns + 1, I + 1}, {{P, key_bits(O)}}, need));
  return N.prim.reserve(need);
}

pcd_status edit_compact(const pcd_ba* b, BaEditScratch& N, const uint8_t* d_erase, const uint8_t* d_pdel,
                        const uint8_t* d_term_erase, const uint8_t* cpose, uint32_t* d_map, hipStream_t s) {
  BaLayout& Y = N.layout;
  BaTerms& T = N.terms;
  const uint32_t O = (uint32_t)b->O, L = (uint32_t)b->L, P = (uint32_t)b->P, I = (uint32_t)b->I;
  const uint32_t nslices = (uint32_t)b->nslices;
  const bool vrows = cpose != nullptr, meta = b->has_lidar_meta;
  {
    ScopedKernelTimer t("ba_edit_scan", s);
    hipLaunchKernelGGL(k_edit_obs_flag, grid((uint64_t)O + 1), dim3(256), 0, s, O, d_erase, d_pdel, b->obs_point.p, N.flag.p);
    PCD_TRY(scan_flags(N, N.flag.p, N.pos.p, (size_t)O + 1, s));
    hipLaunchKernelGGL(k_edit_list_flag, grid((uint64_t)O + 1), dim3(256), 0, s, O, b->pt_obs_list.p, N.flag.p, N.t_flag.p);
    PCD_TRY(scan_flags(N, N.t_flag.p, N.t_pos.p, (size_t)O + 1, s));
    hipLaunchKernelGGL(k_edit_list_flag, grid((uint64_t)O + 1), dim3(256), 0, s, O, b->img_obs.p, N.flag.p, N.i_flag.p);
    PCD_TRY(scan_flags(N, N.i_flag.p, N.i_pos.p, (size_t)O + 1, s));
    if (vrows) {
      hipLaunchKernelGGL(k_edit_vobs_flag, grid((uint64_t)O + 1), dim3(256), 0, s, O, N.flag.p, b->obs_image.p, cpose, N.v_flag.p);
      PCD_TRY(scan_flags(N, N.v_flag.p, N.v_pos.p, (size_t)O + 1, s));
    }
    if (L) {
      hipLaunchKernelGGL(k_edit_term_flag, grid((uint64_t)L + 1), dim3(256), 0, s, L, d_term_erase, d_pdel, b->lidar_point.p,
                         N.lf.p);
      PCD_TRY(scan_flags(N, N.lf.p, N.lp.p, (size_t)L + 1, s));
      hipLaunchKernelGGL(k_edit_list_flag, grid((uint64_t)L + 1), dim3(256), 0, s, L, b->pt_lidar_list.p, N.lf.p, N.lt_flag.p);
      PCD_TRY(scan_flags(N, N.lt_flag.p, N.lt_pos.p, (size_t)L + 1, s));
    }
  }
  {
    ScopedKernelTimer t("ba_edit_rebuild", s);
    // the observations, the track CSR and the image CSR
    if (O) {
      hipLaunchKernelGGL(k_edit_compact_obs, grid(O), dim3(256), 0, s, O, N.flag.p, N.pos.p, b->obs_image.p, b->obs_point.p,
                         b->obs_xy.p, vrows ? N.v_flag.p : nullptr, N.v_pos.p, Y.obs_image.p, Y.obs_point.p, Y.obs_xy.p,
                         Y.vobs.p, d_map);
      hipLaunchKernelGGL(k_edit_compact_list, grid(O), dim3(256), 0, s, O, b->pt_obs_list.p, N.t_flag.p, N.t_pos.p, N.pos.p,
                         Y.pt_obs_list.p);
      hipLaunchKernelGGL(k_edit_compact_list, grid(O), dim3(256), 0, s, O, b->img_obs.p, N.i_flag.p, N.i_pos.p, N.pos.p,
                         Y.img_obs.p);
    }
    hipLaunchKernelGGL(k_edit_starts, grid((uint64_t)P + 1), dim3(256), 0, s, P, b->pt_obs_start.p, N.t_pos.p, Y.pt_obs_start.p);
    hipLaunchKernelGGL(k_edit_starts, grid((uint64_t)I + 1), dim3(256), 0, s, I, b->img_obs_start.p, N.i_pos.p, Y.img_obs_start.p);
    // the terms and their CSR
    if (L) {
      hipLaunchKernelGGL(k_edit_compact_terms, grid(L), dim3(256), 0, s, L, N.lf.p, N.lp.p, b->lidar_point.p, b->lidar_abcd.p,
                         b->lidar_w.p, meta ? b->lidar_type.p : nullptr, meta ? b->lidar_xyz.p : nullptr, T.lidar_point.p,
                         T.lidar_abcd.p, T.lidar_w.p, T.lidar_type.p, T.lidar_xyz.p);
      hipLaunchKernelGGL(k_edit_compact_list, grid(L), dim3(256), 0, s, L, b->pt_lidar_list.p, N.lt_flag.p, N.lt_pos.p, N.lp.p,
                         T.pt_lidar_list.p);
      hipLaunchKernelGGL(k_edit_starts, grid((uint64_t)P + 1), dim3(256), 0, s, P, b->pt_lidar_start.p, N.lt_pos.p,
                         T.pt_lidar_start.p);
    }
    PCD_TRY(edit_derive(N, P, I, nslices, O, /*fill_sell=*/true, L ? &T : nullptr, s));
    hipLaunchKernelGGL(k_edit_record, dim3(1), dim3(256), 0, s, O, L, I, P, N.pos.p, L ? N.lp.p : nullptr, Y.img_seg_start.p,
                       vrows ? N.v_pos.p : nullptr, b->pt_obs_start.p, Y.pt_obs_start.p, N.record.p);
    PCD_HIP_TRY(hipGetLastError());
  }
  return PCD_OK;
}

static pcd_status edit_rebuild(pcd_ba* b, const uint8_t* d_erase, const uint8_t* d_pdel, uint32_t* d_map, hipStream_t s,
                               pcd_ba_remove_info* info) {
  BaEditScratch& N = b->edit_next;
  const uint32_t O = (uint32_t)b->O, L = (uint32_t)b->L, P = (uint32_t)b->P, I = (uint32_t)b->I;
  const uint32_t nslices = (uint32_t)b->nslices;
  // the terms this call builds: every group when the handle has terms (the meta when it has that), none otherwise
  const unsigned terms = L ? kTermRows | (b->has_lidar_meta ? kTermMeta : 0u) | kTermIndex | kTermTracks : 0u;
  PCD_TRY(edit_reserve(b, N, terms, b->has_cpose, kRecWords));
  EventPair ev;
  if (info) { PCD_TRY(ev.create()); (void)ev.start(s); }
  PCD_TRY(edit_compact(b, N, d_erase, d_pdel, nullptr, b->const_poses(), d_map, s));
  PCD_TRY(edit_read_record(N, kRecWords, I, info ? &ev : nullptr, s));
  const uint32_t* rec = N.h_record.p;
  const uint32_t nO = rec[kRecObs], nL = rec[kRecTerms];
  float ms = 0.f;
  PCD_TRY(edit_commit(b, EditCounts{nO, nL, P, nslices, rec[kRecSegs], rec[kRecPoseRows]}, nullptr, terms, kRecWords,
                      info ? &ev : nullptr, &ms, s));
  if (info) {
    info->num_obs = nO; info->num_obs_removed = O - nO;
    info->num_lidar = nL; info->num_lidar_removed = L - nL;
    info->num_points_emptied = rec[kRecEmptied];
    info->rebuild_ms = ms;
  }
  return PCD_OK;
}

// ---- the addition ------------------------------------------------------------------------------------
// In the concatenated order every new row has a larger index than every old row, so in the stable counting sort
// pcd_ba_create does (build_csr) the old entries of a key keep their order and the new entries of the key follow them in
// input order.  With the new rows sorted stably by key and add[k] = the new rows of keys below k:
//   start'[k] = start[k] + add[k]                    (the old bound of a new key is O)
//   old entry e of key k          -> e + add[k]
//   sorted new row of rank r, key k -> start'[k] + oldlen[k] + (r - add[k]) = oldend[k] + r, and holds O + row
enum { kAddBad = 0, kAddSegs, kAddPoseRows, kAddSlots, kAddWords };

// key[r] of new row r, clamped into [0, nkeys): every later pass stays in bounds whatever the row holds.
// bad[workgroup] = its rows out of range: the verdict, summed by k_add_record
__global__ __launch_bounds__(256) void k_add_keys(uint32_t A, const int* __restrict__ in, uint32_t nkeys,
                                                  uint32_t* __restrict__ key, uint32_t* __restrict__ iota,
                                                  uint32_t* __restrict__ bad) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  int out = 0;
  if (r < A) {
    const int k = in[r];
    out = (k < 0 || (uint32_t)k >= nkeys) ? 1 : 0;
    key[r] = out ? 0u : (uint32_t)k;
    iota[r] = r;
  }
  const int n = __syncthreads_count(out);
  if (threadIdx.x == 0) bad[blockIdx.x] = (uint32_t)n;
}
// add[k] for k = 0 .. nkeys: the first sorted new row whose key is not below k (a lower bound: no histogram, no atomics)
__global__ __launch_bounds__(256) void k_add_lower(uint32_t nkeys, uint32_t A, const uint32_t* __restrict__ sorted,
                                                   uint32_t* __restrict__ add) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > nkeys) return;
  uint32_t lo = 0, hi = A;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < k) lo = mid + 1; else hi = mid;
  }
  add[k] = lo;
}
// start'[k] for k = 0 .. nnew; the old CSR has nold keys and n entries (its bound from nold on)
__global__ __launch_bounds__(256) void k_add_starts(uint32_t nold, uint32_t nnew, uint32_t n, const uint32_t* __restrict__ old_start,
                                                    const uint32_t* __restrict__ add, uint32_t* __restrict__ start) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > nnew) return;
  start[k] = (k <= nold ? old_start[k] : n) + add[k];
}
__global__ __launch_bounds__(256) void k_add_move_old(uint32_t O, const uint32_t* __restrict__ list, const int* __restrict__ key_of,
                                                      const uint32_t* __restrict__ add, uint32_t* __restrict__ out) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= O) return;
  const uint32_t o = list[e];
  out[e + add[key_of[o]]] = o;
}
__global__ __launch_bounds__(256) void k_add_place_new(uint32_t A, const uint32_t* __restrict__ sorted_key,
                                                       const uint32_t* __restrict__ sorted_row, uint32_t nold,
                                                       const uint32_t* __restrict__ old_start, uint32_t O,
                                                       uint32_t* __restrict__ out) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= A) return;
  const uint32_t k = sorted_key[r];
  const uint32_t end = k < nold ? old_start[k + 1] : O;
  out[end + r] = O + sorted_row[r];
}
// flag[r] = 1: new row r is on a variable-pose image (a row out of range counts as none: the call is refused anyway)
__global__ __launch_bounds__(256) void k_add_vflag(uint32_t A, const int* __restrict__ obs_image, uint32_t I,
                                                   const uint8_t* __restrict__ cpose, uint32_t* __restrict__ flag) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r > A) return;
  uint32_t f = 0;
  if (r < A) {
    const int i = obs_image[r];
    f = (i >= 0 && (uint32_t)i < I && !cpose[i]) ? 1u : 0u;
  }
  flag[r] = f;
}
// the packed pose rows: the old ones as they are (old null: every old observation had one, the identity), then the
// flagged new rows
__global__ __launch_bounds__(256) void k_add_vobs(uint32_t V, uint32_t A, uint32_t O, const uint32_t* __restrict__ old,
                                                  const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                  uint32_t* __restrict__ vobs) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < V) { vobs[t] = old ? old[t] : t; return; }
  const uint32_t r = t - V;
  if (r < A && flag[r]) vobs[V + pos[r]] = O + r;
}
__global__ __launch_bounds__(256) void k_add_extend(uint32_t nold, uint32_t nnew, uint32_t n, const uint32_t* __restrict__ old_start,
                                                    uint32_t* __restrict__ start) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > nnew) return;
  start[k] = k <= nold ? old_start[k] : n;
}
// one workgroup: the verdict and the counts (integer sums: any order)
__global__ __launch_bounds__(256) void k_add_record(uint32_t nbad, const uint32_t* __restrict__ bad, uint32_t I,
                                                    const uint32_t* __restrict__ img_seg_start, uint32_t A, uint32_t V,
                                                    const uint32_t* __restrict__ v_pos, uint32_t nslices,
                                                    const uint32_t* __restrict__ slice_start, uint32_t* __restrict__ rec) {
  uint32_t n = 0;
  for (uint32_t k = threadIdx.x; k < nbad; k += 256) n += bad[k];
  const int any = __syncthreads_or(n != 0);
  if (threadIdx.x == 0) {
    rec[kAddBad] = any ? 1u : 0u;
    rec[kAddSegs] = img_seg_start[I];
    rec[kAddPoseRows] = v_pos ? V + v_pos[A] : V + A;
    rec[kAddSlots] = slice_start[nslices];
  }
}

// One CSR of the grown handle (start [nnew + 1], list [O + A]) from the old one (nold keys) and the new rows' keys
static pcd_status add_merge_csr(BaEditScratch& N, const int* d_key, uint32_t A, uint32_t nold, uint32_t nnew, uint32_t O,
                                const uint32_t* old_start, const uint32_t* old_list, const int* old_key_of_obs,
                                uint32_t* bad, uint32_t* start, uint32_t* list, hipStream_t s) {
  if (A) {
    hipLaunchKernelGGL(k_add_keys, grid(A), dim3(256), 0, s, A, d_key, nnew, N.a_key.p, N.a_iota.p, bad);
    PCD_TRY(sort_pairs(N.prim, N.a_key.p, N.a_key_sorted.p, N.a_iota.p, N.a_row.p, (size_t)A, 0u, key_bits(nnew), s));
  }
  hipLaunchKernelGGL(k_add_lower, grid((uint64_t)nnew + 1), dim3(256), 0, s, nnew, A, N.a_key_sorted.p, N.a_add.p);
  hipLaunchKernelGGL(k_add_starts, grid((uint64_t)nnew + 1), dim3(256), 0, s, nold, nnew, O, old_start, N.a_add.p, start);
  if (O) hipLaunchKernelGGL(k_add_move_old, grid(O), dim3(256), 0, s, O, old_list, old_key_of_obs, N.a_add.p, list);
  if (A) hipLaunchKernelGGL(k_add_place_new, grid(A), dim3(256), 0, s, A, N.a_key_sorted.p, N.a_row.p, nold, old_start, O, list);
  return PCD_OK;
}

// Every buffer whose size follows from the counts, before the first launch.  Buffers grow here, unlike in edit_reserve;
// the sliced-ELL copies wait for their size
static pcd_status add_reserve(pcd_ba* b, size_t A, size_t Pn, unsigned terms) {
  BaEditScratch& N = b->edit_next;
  const size_t O2 = b->O + A, P2 = (size_t)b->P + Pn, I = (size_t)b->I, L = b->L;
  const size_t ns2 = (P2 + 63) / 64, nb = div_up(A, 256);
  // segments of the grown handle at most: an image that gains a > 0 rows gains at most 1 + a / kImgSeg segments
  const size_t nseg = (size_t)b->nseg + (size_t)std::min<uint64_t>(A, (uint64_t)b->I) + (size_t)(A / kImgSeg);
  PCD_TRY(edit_reserve_shared(N, BaLayoutSizes{O2, P2, I, ns2, nseg, b->has_cpose, 0, 0}, kAddWords));
  if (b->has_cpose) { PCD_TRY(N.v_flag.reserve(A + 1)); PCD_TRY(N.v_pos.reserve(A + 1)); }
  PCD_TRY(N.terms.reserve_terms(terms, L, P2, ns2 * 64));
  if (Pn) {
    PCD_TRY(N.points.reserve(3 * P2));
    if (b->has_cpt) PCD_TRY(N.point_const.reserve(P2));
  }
  for (DevBuf<uint32_t>* d : {&N.a_key, &N.a_key_sorted, &N.a_iota, &N.a_row}) PCD_TRY(d->reserve(at_least_1(A)));
  PCD_TRY(N.a_add.reserve(std::max(P2, I) + 1)); PCD_TRY(N.a_bad.reserve(at_least_1(2 * nb)));
  PCD_TRY(reserve_cost_partial(b, ns2, O2, L));   // the cost partials of the grown handle
  size_t need = 0;   // the track lengths; the new rows by point and by image (not sorted when there are none)
  PCD_TRY(prim_storage_u32({A + 1, ns2 + 1, I + 1}, {{P2, key_bits(O2)}, {A, key_bits(P2)}, {A, key_bits(I)}}, need));
  return N.prim.reserve(need);
}

static pcd_status add_rebuild(pcd_ba* b, const double* d_points, uint64_t Pn64, const int* d_image, const int* d_point,
                              const double* d_xy, uint64_t A64, hipStream_t s, pcd_ba_add_info* info) {
  BaEditScratch& N = b->edit_next;
  BaLayout& Y = N.layout;
  const uint32_t O = (uint32_t)b->O, A = (uint32_t)A64, O2 = O + A, L = (uint32_t)b->L, I = (uint32_t)b->I;
  const uint32_t P = (uint32_t)b->P, Pn = (uint32_t)Pn64, P2 = P + Pn, ns2 = (P2 + 63u) / 64u, V = (uint32_t)b->n_pose_rows;
  const uint32_t nb = div_up(A, 256);
  const bool vrows = b->has_cpose;
  // the terms this call builds: the index's start (the new points have none) and the per-track copies in the new order
  const unsigned terms = kTermStart | (L ? kTermTracks : 0u);
  PCD_TRY(add_reserve(b, A, Pn, terms));
  EventPair ev;
  if (info) { PCD_TRY(ev.create()); (void)ev.start(s); }
  {
    ScopedKernelTimer t("ba_add_merge", s);
    // the rows and the points: the old ones, then the new ones
    if (O) {
      PCD_HIP_TRY(hipMemcpyAsync(Y.obs_image.p, b->obs_image.p, (size_t)O * sizeof(int), hipMemcpyDeviceToDevice, s));
      PCD_HIP_TRY(hipMemcpyAsync(Y.obs_point.p, b->obs_point.p, (size_t)O * sizeof(int), hipMemcpyDeviceToDevice, s));
      PCD_HIP_TRY(hipMemcpyAsync(Y.obs_xy.p, b->obs_xy.p, 2 * (size_t)O * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (A) {
      PCD_HIP_TRY(hipMemcpyAsync(Y.obs_image.p + O, d_image, (size_t)A * sizeof(int), hipMemcpyDeviceToDevice, s));
      PCD_HIP_TRY(hipMemcpyAsync(Y.obs_point.p + O, d_point, (size_t)A * sizeof(int), hipMemcpyDeviceToDevice, s));
      PCD_HIP_TRY(hipMemcpyAsync(Y.obs_xy.p + 2 * (size_t)O, d_xy, 2 * (size_t)A * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (Pn) {
      PCD_HIP_TRY(hipMemcpyAsync(N.points.p, b->points.p, 3 * (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, s));
      PCD_HIP_TRY(hipMemcpyAsync(N.points.p + 3 * (size_t)P, d_points, 3 * (size_t)Pn * sizeof(double), hipMemcpyDeviceToDevice, s));
      if (b->has_cpt) {
        PCD_HIP_TRY(hipMemcpyAsync(N.point_const.p, b->point_const.p, (size_t)P, hipMemcpyDeviceToDevice, s));
        PCD_HIP_TRY(hipMemsetAsync(N.point_const.p + P, 0, (size_t)Pn, s));
      }
    }
    // the track CSR over P2 points and the image CSR
    PCD_TRY(add_merge_csr(N, d_point, A, P, P2, O, b->pt_obs_start.p, b->pt_obs_list.p, b->obs_point.p, N.a_bad.p,
                          Y.pt_obs_start.p, Y.pt_obs_list.p, s));
    PCD_TRY(add_merge_csr(N, d_image, A, I, I, O, b->img_obs_start.p, b->img_obs.p, b->obs_image.p, N.a_bad.p + nb,
                          Y.img_obs_start.p, Y.img_obs.p, s));
    if (vrows) {
      hipLaunchKernelGGL(k_add_vflag, grid((uint64_t)A + 1), dim3(256), 0, s, A, d_image, I, b->image_const_pose.p, N.v_flag.p);
      PCD_TRY(scan_flags(N, N.v_flag.p, N.v_pos.p, (size_t)A + 1, s));
      if (V + A)
        hipLaunchKernelGGL(k_add_vobs, grid((uint64_t)V + A), dim3(256), 0, s, V, A, O, V == O ? nullptr : b->vobs.p,
                           N.v_flag.p, N.v_pos.p, Y.vobs.p);
    }
    hipLaunchKernelGGL(k_add_extend, grid((uint64_t)P2 + 1), dim3(256), 0, s, P, P2, L, b->pt_lidar_start.p,
                       N.terms.pt_lidar_start.p);
  }
  {
    ScopedKernelTimer t("ba_add_rebuild", s);
    // the sliced-ELL copies wait for their size: the number of slots is in the record.  The per-track copies read the
    // live rows and list.
    PCD_TRY(edit_derive(N, P2, I, ns2, O2, /*fill_sell=*/false, L ? b : nullptr, s));
    hipLaunchKernelGGL(k_add_record, dim3(1), dim3(256), 0, s, 2 * nb, N.a_bad.p, I, Y.img_seg_start.p, A, V,
                       vrows ? N.v_pos.p : nullptr, ns2, Y.slice_start.p, N.record.p);
    PCD_HIP_TRY(hipGetLastError());
  }
  PCD_TRY(edit_read_record(N, kAddWords, I, info ? &ev : nullptr, s));
  const uint32_t* rec = N.h_record.p;
  PCD_REQUIRE(!rec[kAddBad], "obs_image / obs_point of a new row out of range");   // nothing swapped, no slot reserved
  float ms = 0.f;
  PCD_TRY(edit_commit(b, EditCounts{O2, L, P2, ns2, rec[kAddSegs], rec[kAddPoseRows]}, rec + kAddSlots, terms, kAddWords,
                      info ? &ev : nullptr, &ms, s));
  if (info) {
    info->num_obs = O2; info->num_points = P2; info->num_pose_rows = b->n_pose_rows;
    info->rebuild_ms = ms;
  }
  return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" pcd_status pcd_ba_remove_observations_device(pcd_ba* b, const uint8_t* d_obs_erase, const uint8_t* d_point_delete,
                                                        uint32_t* d_obs_map, void* stream, pcd_ba_remove_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    PCD_REQUIRE(b, "null handle");
    PCD_TRY(require_device(b->device));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_ba_remove_observations_device"));
    if (info) { info->num_obs = b->O; info->num_lidar = b->L; }
    if (!d_obs_erase && !d_point_delete) return PCD_OK;   // nothing flagged: nothing changes, nothing is invalidated
    PCD_HIP_TRY(hipSetDevice(b->device));
    return edit_rebuild(b, d_obs_erase, d_point_delete, d_obs_map, (hipStream_t)stream, info);
  });
}

extern "C" pcd_status pcd_ba_add_observations_device(pcd_ba* b, const double* d_new_points, uint64_t num_new_points,
                                                     const int32_t* d_obs_image, const int32_t* d_obs_point,
                                                     const double* d_obs_xy, uint64_t num_new_obs, void* stream,
                                                     pcd_ba_add_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    PCD_REQUIRE(b, "null handle");
    PCD_TRY(require_device(b->device));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_ba_add_observations_device"));
    if (info) { info->num_obs = b->O; info->num_points = (uint64_t)b->P; info->num_pose_rows = b->n_pose_rows; }
    PCD_REQUIRE(num_new_points == 0 || d_new_points, "new points");
    PCD_REQUIRE(num_new_obs == 0 || (d_obs_image && d_obs_point && d_obs_xy), "new observations");
    PCD_REQUIRE(num_new_obs < 0xFFFFFFF0ull && b->O + num_new_obs < 0xFFFFFFF0ull, "too many residual blocks");
    PCD_REQUIRE(num_new_points <= (uint64_t)INT32_MAX && (uint64_t)b->P + num_new_points <= (uint64_t)INT32_MAX, "too many points");
    if (!num_new_obs && !num_new_points) return PCD_OK;   // nothing to add: nothing changes, nothing is invalidated
    PCD_HIP_TRY(hipSetDevice(b->device));
    PCD_TRY(add_rebuild(b, d_new_points, num_new_points, d_obs_image, d_obs_point, d_obs_xy, num_new_obs, (hipStream_t)stream, info));
    if (info) { info->num_obs_added = num_new_obs; info->num_points_added = num_new_points; }
    return PCD_OK;
  });
}

extern "C" pcd_status pcd_ba_add_observations(pcd_ba* b, const double* new_points, uint64_t num_new_points,
                                              const int32_t* obs_image, const int32_t* obs_point, const double* obs_xy,
                                              uint64_t num_new_obs, pcd_ba_add_info* info) {
  return pcd::guard([&]() -> pcd_status {
    if (info) std::memset(info, 0, sizeof *info);
    PCD_REQUIRE(b, "null handle");
    PCD_TRY(require_device(b->device));
    PCD_REQUIRE(num_new_points == 0 || new_points, "new points");
    PCD_REQUIRE(num_new_obs == 0 || (obs_image && obs_point && obs_xy), "new observations");
    PCD_REQUIRE(num_new_obs < 0xFFFFFFF0ull && num_new_points <= (uint64_t)INT32_MAX, "too many rows");
    PCD_HIP_TRY(hipSetDevice(b->device));
    DevBuf<double> d_points, d_xy;
    DevBuf<int> d_image, d_point;
    PCD_TRY(upload(d_points, new_points, 3 * (size_t)num_new_points));
    PCD_TRY(upload(d_image, obs_image, (size_t)num_new_obs)); PCD_TRY(upload(d_point, obs_point, (size_t)num_new_obs));
    PCD_TRY(upload(d_xy, obs_xy, 2 * (size_t)num_new_obs));
    // the device form waits for the null stream before it returns; the fills it enqueues behind that wait read the
    // handle's own copies, so the staging can go when this scope ends
    return pcd_ba_add_observations_device(b, d_points.p, num_new_points, d_image.p, d_point.p, d_xy.p, num_new_obs, nullptr, info);
  });
}

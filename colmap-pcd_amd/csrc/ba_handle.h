// ba_handle.h -- the bundle-adjustment handle as every BA unit sees it, and the sizes builder and launchers must agree
// on (kImgSeg, kCostBlocks, cost_blocks, the element counts of the block form).  Internal; no kernel is defined or declared
// here.  What the handle derives from its observations and LiDAR terms is named once, as BaLayout and BaTerms (below).
//   ba_build.hip  makes and destroys it: pcd_ba_create uploads the problem and builds the derived layouts below
//   ba.hip        evaluates on it: the kernels that read BaDev, and every pcd_ba_evaluate* / filter entry point
//   ba_solve.hip  point elimination, PCG, LM loop (its own state hangs off pcd_ba::schur)
//   ba_schur_structure.hip  the co-visibility structure of the elimination, built on the device (ba_schur_structure.h)
//   ba_lidar.hip  replaces the LiDAR terms of a live handle: pcd_ba_set_lidar_device / pcd_ba_associate_lidar_device
//   ba_edit.hip   drops observations and points from a live handle, and adds them: pcd_ba_remove_observations_device,
//                 pcd_ba_add_observations_device
//   ba_window.hip derives a second handle, the sphere window of a global round, from a live one and carries its
//                 parameters back: pcd_ba_window_create_device, pcd_ba_window_commit_device
//   ba_local.hip  the local round's start: FindLocalBundle on the handle and the local sub-problem as a second handle:
//                 pcd_ba_local_bundle_device, pcd_ba_local_window_create_device
#pragma once
#include <memory>

#include "ba_cam_jac.h"
#include "common.h"

namespace pcd {

constexpr uint32_t kImgSeg = 1024;           // observations per segment of an image: the work item of k_ba_images
constexpr unsigned kCostBlocks = 1u << 20;   // cap of the cost pass's grid (256 M residual blocks in one sweep)

struct BaDev {
  // problem (device)
  const int* cam_model; const int* cam_off; const double* cam_params;
  const double* poses; const int* image_cam; const uint8_t* image_const_pose; const uint8_t* image_const_tvec;
  const double* points; const uint8_t* point_const;
  const int* obs_image; const int* obs_point; const double* obs_xy;
  const int* lidar_point; const double* lidar_abcd; const double* lidar_w;
  // the derived layouts: BaLayout and BaTerms below say what each array holds
  const int* pt_order; const uint32_t* slice_start; const int* sell_img; const double* sell_xy;
  const uint32_t* pt_lidar_start; const uint32_t* pt_lidar_list;
  const uint32_t* pt_lidar_cnt; const double* pt_lidar_first;   // both nullptr when L == 0
  const uint32_t* img_obs_start; const int* img_pt; const uint32_t* img_obs;
  const uint32_t* seg_img; const uint32_t* seg_begin; const uint32_t* img_seg_start;
  const uint8_t* cam_refine;      // [cam_params_len] 1 = parameter optimised (nullptr: all constant)
  const uint32_t* cam_img_start;  // [C+1] images of each camera (CSR, ascending image index)
  const uint32_t* cam_img_list;
  int C;
  int cam_k;                      // K of the camera accumulation: the model's when one of the compiled-in models is
                                  // used by every camera, PCD_CAM_JAC_STRIDE for the generic (per-observation switch) path
  const double* img_xy;           // [O][2]
  int I, P, nslices; uint64_t O, L;
  int loss_type; double loss_scale;
  int shared_cam;                 // >= 0: every image maps to this camera (one physical camera, the usual dataset); -1: per image
};

// ---- the derived state of a handle -------------------------------------------------------------------------------
// It is derived in three places, byte for byte the same -- on creation (ba_build.hip, host counting sorts), when the terms
// change (ba_lidar.hip), when observations are dropped or added (ba_edit.hip); WHAT is derived is listed here alone.  pcd_ba
// is a BaLayout and a BaTerms; a rebuild of a live handle reserves and writes a second one and swaps it in on success, so
// the buffers a call retires are the next call's scratch.
// The swap invariant: a live buffer is never exchanged for one that the call did not both reserve and write.  A rebuild
// therefore names the groups it builds once, for its reserve and its swap alike.  With L == 0 no per-track copies are built
// (the kernels get nullptr) and an edit builds no term group at all: the at_least_1 buffers of pcd_ba_create stay.
inline size_t at_least_1(size_t n) { return std::max<size_t>(n, 1); }   // for a buffer a kernel is handed even when its count is 0

// The sizes of a BaLayout: pcd_ba's counts (nseg: an upper bound will do), whether some pose is constant (vobs exists) and
// the capacity of the sliced-ELL copies (0: reserved later, when the slot count is known: reserve_sell)
struct BaLayoutSizes { size_t O, P, I, nslices, nseg; bool pose_rows; size_t sell_img, sell_xy; };
// What follows from the observation rows
struct BaLayout {
  DevBuf<int> obs_image, obs_point;   // [O] the rows, in the caller's order
  DevBuf<double> obs_xy;              // [O][2]
  // the track CSR (point -> its observations, ascending): the sliced-ELL fill and pcd_ba_filter_tracks read it
  DevBuf<uint32_t> pt_obs_start, pt_obs_list;
  // per-track copies of the observations: sliced ELL, the tracks in ascending order of length (ties: ascending point id)
  DevBuf<int> pt_order;               // [nslices*64]  thread of k_ba_points -> point id (-1 = padding)
  DevBuf<uint32_t> slice_start;       // [nslices+1]   first slot of each 64-track slice
  DevBuf<int> sell_img;               // [nslots]      image of the observation, -1 = padding
  DevBuf<double> sell_xy;             // [nslots][2]
  // per-image copies: the image-major order, contiguous
  DevBuf<uint32_t> img_obs_start;     // [I+1]
  DevBuf<uint32_t> img_obs;           // [O] index of the e-th image-major observation in the caller's order (W is written there)
  DevBuf<int> img_pt;                 // [O] its point
  DevBuf<double> img_xy;              // [O][2]
  DevBuf<uint32_t> seg_img;           // [nseg] image of each segment of <= kImgSeg observations (image-major order)
  DevBuf<uint32_t> seg_begin;         // [nseg+1] first observation (image-major position) of each segment
  DevBuf<uint32_t> img_seg_start;     // [I+1] segments of each image
  DevBuf<uint32_t> vobs;              // [n_pose_rows] observation of every packed pose row (only when some pose is constant)

  pcd_status reserve_layout(const BaLayoutSizes& z) {
    const size_t O1 = at_least_1(z.O);
    PCD_TRY(obs_image.reserve(O1)); PCD_TRY(obs_point.reserve(O1)); PCD_TRY(obs_xy.reserve(at_least_1(2 * z.O)));
    PCD_TRY(pt_obs_start.reserve(z.P + 1)); PCD_TRY(pt_obs_list.reserve(O1));
    PCD_TRY(pt_order.reserve(at_least_1(z.nslices * 64))); PCD_TRY(slice_start.reserve(z.nslices + 1));
    PCD_TRY(sell_img.reserve(z.sell_img)); PCD_TRY(sell_xy.reserve(z.sell_xy));
    PCD_TRY(img_obs_start.reserve(z.I + 1)); PCD_TRY(img_obs.reserve(O1));
    PCD_TRY(img_pt.reserve(O1)); PCD_TRY(img_xy.reserve(std::max<size_t>(2 * z.O, 2)));
    PCD_TRY(seg_img.reserve(at_least_1(z.nseg))); PCD_TRY(seg_begin.reserve(z.nseg + 1)); PCD_TRY(img_seg_start.reserve(z.I + 1));
    if (z.pose_rows) PCD_TRY(vobs.reserve(O1));
    return PCD_OK;
  }
  pcd_status reserve_sell(size_t nslots) {
    PCD_TRY(sell_img.reserve(at_least_1(nslots)));
    return sell_xy.reserve(std::max<size_t>(2 * nslots, 2));
  }
  // every buffer; vobs only when the call built it (pose_rows as it reserved)
  void swap_layout(BaLayout& o, bool pose_rows) {
    obs_image.swap(o.obs_image); obs_point.swap(o.obs_point); obs_xy.swap(o.obs_xy);
    pt_obs_start.swap(o.pt_obs_start); pt_obs_list.swap(o.pt_obs_list);
    pt_order.swap(o.pt_order); slice_start.swap(o.slice_start); sell_img.swap(o.sell_img); sell_xy.swap(o.sell_xy);
    img_obs_start.swap(o.img_obs_start); img_obs.swap(o.img_obs); img_pt.swap(o.img_pt); img_xy.swap(o.img_xy);
    seg_img.swap(o.seg_img); seg_begin.swap(o.seg_begin); img_seg_start.swap(o.img_seg_start);
    if (pose_rows) vobs.swap(o.vobs);
  }
};

// The LiDAR terms and what follows from them, in the three groups the rebuilds replace (the rows' meta and the index's
// list are parts a rebuild may leave out):
//   removal (L > 0)   rows (meta when the handle has it), index, per-track copies
//   addition          the index's start alone (the terms stay, the new points have none); per-track copies when L > 0
//   the terms change  rows with meta, index; per-track copies when the new L > 0
enum : unsigned { kTermRows = 1, kTermMeta = 2, kTermStart = 4, kTermList = 8, kTermTracks = 16, kTermIndex = kTermStart | kTermList };
struct BaTerms {
  // the rows: point, plane (a, b, c, d) and weight of each of the L terms; its pcd_lidar_type and LiDAR point, for the
  // outlier filter.  pcd_ba_create knows neither: the two do not exist until pcd_ba_lidar_device asks for them (zeros)
  // or pcd_ba_set_lidar_device installs them (pcd_ba::has_lidar_meta).
  DevBuf<int> lidar_point; DevBuf<double> lidar_abcd, lidar_w;
  DevBuf<uint8_t> lidar_type; DevBuf<double> lidar_xyz;
  // the index: CSR point -> its terms, ascending term number
  DevBuf<uint32_t> pt_lidar_start, pt_lidar_list;
  // The terms in the order of k_ba_points' threads (not built when L == 0).  The terms and the thread order change only
  // as a whole, never between the launches of one evaluation, so the kernel reads its one plane per point coalesced and
  // ahead of everything else, not through point -> list -> term; only a second or third term of a point goes through
  // the lists.
  DevBuf<uint32_t> pt_lidar_cnt;      // [nslices*64] number of LiDAR terms of the track of thread t
  DevBuf<double> pt_lidar_first;      // [5][nslices*64] plane (a, b, c, d) and weight of the first of them, component-major

  // L terms over P points and ntr = nslices*64 threads
  pcd_status reserve_terms(unsigned groups, size_t L, size_t P, size_t ntr) {
    const size_t L1 = at_least_1(L);
    if (groups & kTermRows) { PCD_TRY(lidar_point.reserve(L1)); PCD_TRY(lidar_abcd.reserve(at_least_1(4 * L))); PCD_TRY(lidar_w.reserve(L1)); }
    if (groups & kTermMeta) { PCD_TRY(lidar_type.reserve(L1)); PCD_TRY(lidar_xyz.reserve(at_least_1(3 * L))); }
    if (groups & kTermStart) PCD_TRY(pt_lidar_start.reserve(P + 1));
    if (groups & kTermList) PCD_TRY(pt_lidar_list.reserve(L1));
    if (groups & kTermTracks) { PCD_TRY(pt_lidar_cnt.reserve(at_least_1(ntr))); PCD_TRY(pt_lidar_first.reserve(at_least_1(5 * ntr))); }
    return PCD_OK;
  }
  // groups: those the call reserved with and wrote in full
  void swap_terms(BaTerms& o, unsigned groups) {
    if (groups & kTermRows) { lidar_point.swap(o.lidar_point); lidar_abcd.swap(o.lidar_abcd); lidar_w.swap(o.lidar_w); }
    if (groups & kTermMeta) { lidar_type.swap(o.lidar_type); lidar_xyz.swap(o.lidar_xyz); }
    if (groups & kTermStart) pt_lidar_start.swap(o.pt_lidar_start);
    if (groups & kTermList) pt_lidar_list.swap(o.pt_lidar_list);
    if (groups & kTermTracks) { pt_lidar_cnt.swap(o.pt_lidar_cnt); pt_lidar_first.swap(o.pt_lidar_first); }
  }
};

// Scratch of the device rebuild of the LiDAR terms (ba_lidar.hip): the terms under construction, then the work buffers
struct BaLidarScratch {
  BaTerms terms;
  DevBuf<uint32_t> flag, pos, part, status, keys, iota;   // per row: kept / position; per workgroup and total: the record
  DevBuf<char> prim;                                      // rocPRIM temporary storage (scan, sort)
  PinnedBuf<uint32_t> h_status;
  DevBuf<double> a_xyz, a_abcd; DevBuf<uint8_t> a_type;   // association rows of pcd_ba_associate_lidar_device, [P]
  // pcd_ba_project_lidar_device: per observation (the caller's order) whether its feature found a winner and the winner's
  // x y z nx ny nz; the Proj rows [P] when they are merged with association rows; the counts of the info record
  DevBuf<uint8_t> p_found, p_type; DevBuf<double> p_l6, p_xyz, p_abcd;
  DevBuf<uint64_t> p_count_part, p_count;
  PinnedBuf<uint64_t> h_count;
};

// Scratch of the two edits (ba_edit.hip): the layout and the terms under construction, then the work buffers
struct BaEditScratch {
  BaLayout layout;
  BaTerms terms;
  // keep flags and their scans (n + 1 entries each: the last scan value is the count): observations in the caller's order,
  // through the track lists, through the image lists, the variable-pose ones; terms in term order, through the point lists
  DevBuf<uint32_t> flag, pos, t_flag, t_pos, i_flag, i_pos, v_flag, v_pos, lf, lp, lt_flag, lt_pos;
  DevBuf<uint32_t> len, len_sorted, iota, width, seg_cnt, record;
  // the addition alone: the grown points and their constness; the new rows' keys (clamped into range), their stable sort
  // (keys, rows), the new entries in front of every key [max(P', I) + 1], the bad rows of every workgroup
  DevBuf<double> points; DevBuf<uint8_t> point_const;
  DevBuf<uint32_t> a_key, a_key_sorted, a_iota, a_row, a_add, a_bad;
  DevBuf<char> prim;                                      // rocPRIM temporary storage (scan, sort)
  PinnedBuf<uint32_t> h_record;                           // the counts, then img_obs_start [I+1]
};

// Scratch of pcd_ba_local_bundle_device (ba_local.hip): rows of `image` per point [P]; per image the sort key
// (~shared) and the image, before and after the stable sort [I]; the percentile of every rank [I]; the ranks taken [I];
// the head (candidates, rows of `image`, num_eff, short case)
struct BaLocalScratch {
  DevBuf<uint32_t> mult, key, key_sorted, iota, img_sorted, head;
  DevBuf<double> tri;
  DevBuf<uint8_t> used;
  DevBuf<char> prim;
};

// The point-elimination state is complete in ba_solve.hip only.  The deleter is defined there, so a pcd_ba can be
// made and destroyed where BaSchur is an incomplete type (the default deleter would need the complete one).
struct BaSchur;
struct BaSchurDelete { void operator()(BaSchur* s) const; };

// Element counts of the block form, each written once: a vector over n images or slots, n 6x6 blocks (per image; the
// reduced system's diagonal or pair blocks), the 6x3 blocks W / Y of O observations, the 3x3 blocks of P points and a
// vector over them.
inline size_t slot_vec(uint64_t n) { return 6 * (size_t)n; }
inline size_t blocks_6x6(uint64_t n) { return 36 * (size_t)n; }
inline size_t obs_blocks(uint64_t O) { return 18 * (size_t)O; }
inline size_t point_blocks(uint64_t P) { return 9 * (size_t)P; }
inline size_t point_vec(uint64_t P) { return 3 * (size_t)P; }

template <typename T>
static pcd_status upload(DevBuf<T>& b, const T* src, size_t n) {
  PCD_TRY(b.reserve(at_least_1(n)));
  if (n) PCD_HIP_TRY(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return PCD_OK;
}
// its counterpart for a host form's copy-backs: n elements of a buffer, if the caller wants them and there are any
template <typename T>
static pcd_status copy_back(void* dst, const DevBuf<T>& src, size_t n) {
  if (dst && n) PCD_HIP_TRY(hipMemcpy(dst, src.p, n * sizeof(T), hipMemcpyDeviceToHost));
  return PCD_OK;
}
template <typename... B>
static uint64_t dev_bytes(const B&... b) { return (uint64_t(0) + ... + (b.n * sizeof(*b.p))); }   // capacity held

// The normal equations at the handle's parameters (ba.hip): point blocks and the cost (k_ba_points, k_sum_partials),
// then image blocks with W riding on the image pass (k_ba_images, k_ba_images_reduce), on stream s.  w_order[e] is
// the row of W that image-major observation e writes; nullptr = the caller's observation order (BaDev::img_obs).
// Every output is device memory and required.  Opens no profiling scope, sets no device.
pcd_status ba_normal_equations(pcd_ba* b, const uint32_t* w_order, double* Hpt, double* gpt, double* cost, double* Himg,
                               double* gimg, double* W, hipStream_t s);
// Drops the numeric state of the last Schur call (ba_solve.hip): pcd_ba_schur_solve_* and the back-substitution report
// "no Schur state" until the next one.  The co-visibility structure and every scratch buffer stay.
void ba_schur_invalidate(pcd_ba* b);
// The same, and the co-visibility structure with it: the next Schur call builds it as the first call on a fresh handle
// does (ba_edit.hip, when the observations change).  Scratch buffers stay.
void ba_schur_drop_structure(pcd_ba* b);

// The fills the derivations share, each launched in one place, beside its kernel.  ba_build.hip: the sliced-ELL copies of y
// and its image-major copies (no launch when O == 0).  ba_lidar.hip: the per-track copies of `next` in the thread order of
// y, from next's own pt_lidar_start and the list, planes and weights of `rows` (the addition: the live ones; else next).
void launch_fill_sell(const BaLayout& y, int nslices, hipStream_t s);
void launch_fill_image_major(const BaLayout& y, uint64_t O, hipStream_t s);
void launch_lidar_tracks(const BaLayout& y, int nslices, const BaTerms& rows, BaTerms& next, hipStream_t s);

}  // namespace pcd

struct pcd_ba;

namespace pcd {

// The compaction of a handle's rows (ba_edit.hip), shared by the removal, which swaps the result into the handle it
// read, and the window derivation (ba_window.hip), which makes it a new handle's.  `src` is only read; N is the scratch
// the new BaLayout / BaTerms are built in (the removal: src's own edit_next; the window: the new handle's).
//   edit_reserve      every buffer edit_compact writes, at the sizes of src: nothing is allocated after the first launch.
//                     terms: the groups to build (0: src has no terms); pose_rows: vobs is built; words: the record's length
//   edit_compact      observation o stays iff !d_erase[o] && !d_pdel[obs_point[o]], term l iff !d_term_erase[l] &&
//                     !d_pdel[lidar_point[l]] (each may be null).  cpose (null: no packed pose rows) is the constness mask the pose rows are
//                     taken with.  Flags, scans, compaction of rows and both CSRs, the derived layouts, the sliced-ELL and
//                     per-track fills; the counts go to N.record[0 .. kRecWords).  Enqueued on s, no wait.
//   edit_read_record  the ONE synchronisation: `words` of the record and the new image bounds arrive in N.h_record;
//                     ev (may be null) is stopped in front of the wait
enum { kRecObs = 0, kRecTerms, kRecSegs, kRecPoseRows, kRecEmptied, kRecWords };
pcd_status edit_reserve(const pcd_ba* src, BaEditScratch& N, unsigned terms, bool pose_rows, size_t words);
pcd_status edit_compact(const pcd_ba* src, BaEditScratch& N, const uint8_t* d_erase, const uint8_t* d_pdel,
                        const uint8_t* d_term_erase, const uint8_t* cpose, uint32_t* d_map, hipStream_t s);
pcd_status edit_read_record(BaEditScratch& N, size_t words, uint32_t I, EventPair* ev, hipStream_t s);
// ba_build.hip: what a handle holds besides its rows and terms, copied from a live one on the device (the window
// derivation): counts that do not change (C, I, P), cameras with their host mirrors, camera slots and refine state,
// image_cam and the cam_img CSR, the parameters as they are on the device now, image_const_tvec / point_const /
// cam_refine.  image_const_pose is reserved [I] and left to the caller, has_cpose is set.  Copies are enqueued on s.
pcd_status ba_clone_problem(const pcd_ba* src, pcd_ba* dst, hipStream_t s);

// ba_window.hip: the derivation both windows share.  A selection names what it adds to the sequence
//   reserve (its own buffers, before the first launch), ba_clone_problem, select (its kernels: the window's pose mask in
//   w->image_const_pose, and the masks the compaction takes), edit_compact into the window's edit_next, record (its
//   counts behind the removal's, record words kRecWords .. words), edit_read_record (the ONE synchronisation), the
//   image-major fill, the swaps.
// On success *out is the window and its edit_next.h_record holds the `words` counts; build_ms (may be null) is the device
// time up to the synchronisation.
struct WindowMasks { const uint8_t* obs_erase = nullptr; const uint8_t* point_delete = nullptr; const uint8_t* term_erase = nullptr; };
struct WindowSelection {
  size_t words = kRecWords;
  virtual ~WindowSelection() = default;
  virtual pcd_status reserve(const pcd_ba* src, pcd_ba* w) = 0;
  virtual pcd_status select(const pcd_ba* src, pcd_ba* w, hipStream_t s, WindowMasks* m) = 0;
  virtual pcd_status record(pcd_ba* w, hipStream_t s) = 0;
};
pcd_status window_derive(const pcd_ba* src, WindowSelection& sel, uint32_t* d_map, hipStream_t s, pcd_ba** out, float* build_ms);
// k_win_images of ba_window.hip: in[i] (the caller's set, or the sphere around `center`), the window's pose mask
// cpose[i] = src's | !in | extra, and part[workgroup of 256 images] = its images that are in
void launch_win_images(const pcd_ba* src, int center, double radius, const uint8_t* set, const uint8_t* extra, uint8_t* in,
                       uint8_t* cpose, uint32_t* part, hipStream_t s);

}  // namespace pcd

struct pcd_ba : pcd::BaLayout, pcd::BaTerms {
  int device = 0;
  int C = 0, I = 0, P = 0, nslices = 0;
  uint64_t O = 0, L = 0, cam_params_len = 0;
  int loss_type = 0;
  double loss_scale = 1.0;
  int uniform_model = -1;  // >= 0: every camera has this model
  int shared_cam = -1;     // >= 0: every image maps to this camera (BaDev::shared_cam)
  pcd::DevBuf<int> cam_model, cam_off, image_cam;
  pcd::DevBuf<double> cam_params, poses, points;
  pcd::DevBuf<uint8_t> image_const_pose, image_const_tvec, point_const;
  bool has_cpose = false, has_ctvec = false, has_cpt = false;
  // host mirrors of what pcd_ba_project_lidar_device decides on the host (focal lengths, the coefficient latch, the
  // sizes of the depth images, the feature ranges): cam_params follows pcd_ba_set_camera_parameters, the rest is fixed
  std::vector<double> h_cam_params;
  std::vector<int> h_cam_model, h_cam_off, h_image_cam;
  std::vector<uint32_t> h_img_obs_start;
  bool has_lidar_meta = false;   // lidar_type / lidar_xyz exist (BaTerms)
  pcd::BaLidarScratch lidar_next;
  pcd::BaEditScratch edit_next;
  pcd::BaLocalScratch local_next;
  pcd::DevBuf<uint32_t> cam_img_start, cam_img_list;
  uint32_t nseg = 0;
  pcd::DevBuf<double> img_partial;
  pcd::DevBuf<uint8_t> cam_refine;
  bool has_refine = false;
  pcd::DevBuf<double> cam_partial;
  pcd::DevBuf<double> cost_partial, cost;
  // host-API staging
  pcd::DevBuf<double> o_res, o_jq, o_jt, o_jx, o_jl, o_himg, o_gimg, o_hpt, o_gpt, o_w, o_jc, o_hcam, o_gcam, o_ecam, o_wcam;
  // pcd_ba_evaluate_blocks: rows of the variable-pose observations, packed pose Jacobians, pinned results
  // [O] row of observation o in the packed jac_q / jac_t (0xFFFFFFFF: constant pose).  O(O) on the host and read only by
  // pcd_ba_evaluate_blocks: pcd_ba_remove_observations_device marks it stale instead of rebuilding it, and the first
  // pcd_ba_evaluate_blocks afterwards refreshes it from the device's obs_image (ba_refresh_pose_rows, ba.hip)
  std::vector<uint32_t> h_pose_row;
  bool pose_row_stale = false;
  uint64_t n_pose_rows = 0;
  pcd::DevBuf<double> p_jq, p_jt;        // packed pose Jacobians (only when some pose is constant)
  pcd::PinnedBuf<double> h_blocks;       // residuals | jac_q | jac_t | jac_X | jac_lidar | jac_cam
  // pcd_ba_evaluate_blocks_compact: records and packed camera blocks (h_blocks is shared with the full route)
  int cam_stride = 0;                    // largest pcd_camera_num_params over the cameras
  pcd::DevBuf<double> o_rec, p_jc;
  // filter scratch; f_sq / f_depth also stage pcd_ba_observation_errors
  pcd::DevBuf<double> f_sq, f_depth, f_part, f_summary;
  pcd::DevBuf<uint8_t> f_u8;
  // pcd_ba_filter_points_device: projection centres [I][3]; the stage-1 outputs the caller did not ask for
  pcd::DevBuf<double> f_centers, f_tri_err;
  pcd::DevBuf<uint8_t> f_tri_u8;
  // point elimination (pcd_ba_schur*): built on the first call, so pcd_ba_create costs existing users nothing
  bool refines_intrinsics = false;   // some camera_refine byte is set: the reduced system would need camera rows
  // the camera slots of pcd_ba_schur_cam* (fixed at pcd_ba_create): the cameras with a refined parameter below their
  // model's K, ascending camera index.  h_cam_slot [C] (-1: none), h_slot_cam [ncs], h_cam_active [ncs][12] (1 = refined),
  // h_param_cam [cam_params_len] camera of every packed parameter.  Not limited here: the _cam calls refuse more than
  // PCD_BA_MAX_CAMERA_SLOTS.
  std::vector<int> h_cam_slot, h_slot_cam, h_param_cam;
  std::vector<uint8_t> h_cam_active;
  std::unique_ptr<pcd::BaSchur, pcd::BaSchurDelete> schur;
  // the optional constant masks as the kernels take them: nullptr when the problem gave none
  const uint8_t* const_poses() const { return has_cpose ? image_const_pose.p : nullptr; }
  const uint8_t* const_tvec() const { return has_ctvec ? image_const_tvec.p : nullptr; }
  const uint8_t* const_points() const { return has_cpt ? point_const.p : nullptr; }
  pcd::BaDev dev() const {
    pcd::BaDev d;
    d.cam_model = cam_model.p; d.cam_off = cam_off.p; d.cam_params = cam_params.p;
    d.poses = poses.p; d.image_cam = image_cam.p;
    d.image_const_pose = const_poses(); d.image_const_tvec = const_tvec();
    d.points = points.p; d.point_const = const_points();
    d.obs_image = obs_image.p; d.obs_point = obs_point.p; d.obs_xy = obs_xy.p;
    d.lidar_point = lidar_point.p; d.lidar_abcd = lidar_abcd.p; d.lidar_w = lidar_w.p;
    d.pt_order = pt_order.p; d.slice_start = slice_start.p; d.sell_img = sell_img.p; d.sell_xy = sell_xy.p;
    d.pt_lidar_start = pt_lidar_start.p; d.pt_lidar_list = pt_lidar_list.p;
    d.pt_lidar_first = L ? pt_lidar_first.p : nullptr; d.pt_lidar_cnt = L ? pt_lidar_cnt.p : nullptr;
    d.img_obs_start = img_obs_start.p; d.img_pt = img_pt.p; d.img_xy = img_xy.p; d.img_obs = img_obs.p;
    d.seg_img = seg_img.p; d.seg_begin = seg_begin.p; d.img_seg_start = img_seg_start.p;
    d.cam_refine = has_refine ? cam_refine.p : nullptr; d.cam_img_start = cam_img_start.p; d.cam_img_list = cam_img_list.p;
    d.C = C; d.shared_cam = shared_cam; d.cam_k = (uniform_model >= 0 && uniform_model <= 4) ? pcd::cam_num_params(uniform_model) : PCD_CAM_JAC_STRIDE;
    d.I = I; d.P = P; d.nslices = nslices; d.O = O; d.L = L; d.loss_type = loss_type; d.loss_scale = loss_scale;
    return d;
  }
};

namespace pcd {

// Grid of the kernel that writes cost_partial[blockIdx.x]: k_ba_points takes two 64-track slices per workgroup,
// k_ba_cost sweeps the residual blocks with a capped grid.
inline unsigned cost_point_blocks(size_t nslices) { return std::max(1u, div_up(nslices, 2)); }
inline unsigned cost_sweep_blocks(uint64_t O, uint64_t L) { return std::max(1u, std::min(kCostBlocks, div_up(O + L, 256))); }
inline unsigned cost_blocks(const pcd_ba* b, bool want_blocks) {
  return want_blocks ? cost_point_blocks((size_t)b->nslices) : cost_sweep_blocks(b->O, b->L);
}
// cost_partial from the SAME functions: one partial per workgroup of the larger of the two grids, for counts the handle
// may not have yet (a rebuild sizes it before its swap)
inline pcd_status reserve_cost_partial(pcd_ba* b, size_t nslices, uint64_t O, uint64_t L) {
  return b->cost_partial.reserve((size_t)std::max(cost_point_blocks(nslices), cost_sweep_blocks(O, L)) + 1);
}

}  // namespace pcd

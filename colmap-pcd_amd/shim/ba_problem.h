// ba_problem.h -- host-side mirror of the reference's problem assembly, producing the flat pcd_ba_desc.
//
// Restates which residual blocks exist and which parameter blocks are constant, following
//   src/optim/bundle_adjustment.cc:601-682   SetUp / SetUpLocalByLidar / SetUpGlobalByLidar / SetUpAdjustWholeMapByLidar
//   :694-806   AddImageInSphereToProblem     :814-919  AddImageToProblem
//   :927-985   AddPointToProblem             :993-1040 AddLidarToProblem
//   :1047-1100 ParameterizeCameras           :1107-1131 ParameterizePoints
//   src/optim/bundle_adjustment.h:52-116     BundleAdjustmentOptions defaults of THIS fork
//   (refine_focal_length / principal_point / extra_params = false, lidar weights 1 / 100 / 1000)
// The scene containers (Camera, Image, Point3D, Track) are minimal stand-ins for src/base/* with the
// same accessors the assembly code uses; ids are arbitrary 32/64-bit integers as in the reference.
// After BundleAdjusterHip::SetUp*(), Evaluate() runs the HIP kernels; Ceres (or any solver) consumes the
// blocks.  Pure host code up to Evaluate(): the structure logic is unit-tested without a GPU.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <hip/hip_runtime_api.h>   // ReassociateLidar stages its range schedule and selection on the device

#include "../../include/pcdhip.h"
#include "lidar_hip.h"

namespace colmap_hip {

typedef uint32_t camera_t;
typedef uint32_t image_t;
typedef uint64_t point3D_t;
typedef uint32_t point2D_t;
const point3D_t kInvalidPoint3DId = ~0ull;

struct Camera {
  int model_id = 0;
  std::vector<double> params;
  size_t width = 0, height = 0;
};
struct Point2D {
  double xy[2] = {0, 0};
  point3D_t point3D_id = kInvalidPoint3DId;
  bool HasPoint3D() const { return point3D_id != kInvalidPoint3DId; }
};
struct Image {
  camera_t camera_id = 0;
  double qvec[4] = {1, 0, 0, 0};
  double tvec[3] = {0, 0, 0};
  std::vector<Point2D> points2D;
  void NormalizeQvec() {  // base/image.cc: qvec /= norm (identity if zero)
    const double n = std::sqrt(qvec[0] * qvec[0] + qvec[1] * qvec[1] + qvec[2] * qvec[2] + qvec[3] * qvec[3]);
    if (n == 0) { qvec[0] = 1; qvec[1] = qvec[2] = qvec[3] = 0; }
    else for (double& v : qvec) v /= n;
  }
};
struct TrackElement { image_t image_id; point2D_t point2D_idx; };
struct Point3D {
  double xyz[3] = {0, 0, 0};
  std::vector<TrackElement> track;
  int global_opt_num = 0;      // base/point3d.h:82-86
  bool if_in_sphere = false;   // base/point3d.h:156-168
};
struct Reconstruction {
  std::unordered_map<camera_t, Camera> cameras;
  std::unordered_map<image_t, Image> images;
  std::unordered_map<point3D_t, Point3D> points3D;
};

struct BundleAdjustmentOptions {  // optim/bundle_adjustment.h:52-91 (this fork's defaults)
  bool if_add_lidar_constraint = true;
  double proj_lidar_constraint_weight = 1.0;
  double icp_lidar_constraint_weight = 100.0;
  double icp_ground_lidar_constraint_weight = 1000.0;
  int loss_function_type = PCD_LOSS_TRIVIAL;
  double loss_function_scale = 1.0;
  bool refine_focal_length = false, refine_principal_point = false, refine_extra_params = false;
  bool refine_extrinsics = true;
  // Refined intrinsics on the device route (pcd_ba_solve with refine_intrinsics: camera rows in the reduced system, solved
  // as refined_linear_solver_type below says, whatever linear_solver_type says).  false: BundleAdjusterHip::Solve returns false when a refine_* switch
  // leaves a camera parameter variable, and the caller stays on the Ceres route.
  bool refine_intrinsics_on_device = false;
  // ceres::Solver::Options members BundleAdjusterHip::Solve reads (optim/bundle_adjustment.h:96-103)
  int max_num_iterations = 100;
  int max_linear_solver_iterations = 200;
  double function_tolerance = 0.0;
  double gradient_tolerance = 0.0;
  // Linear solver of BundleAdjusterHip::Solve.  ITERATIVE: the block-sparse PCG (inexact steps).  DIRECT: the blocked
  // Cholesky of the dense reduced camera system (exact steps).  AUTO: the reference's switch (optim/
  // bundle_adjustment.cc:500-512: DENSE_SCHUR up to 50 images, SPARSE_SCHUR up to 1000, ITERATIVE_SCHUR above) collapsed
  // onto the two solvers there are here: DIRECT up to kMaxNumImagesDirectSolver images in the config, ITERATIVE above.
  enum class LinearSolverType { ITERATIVE, DIRECT, AUTO };
  LinearSolverType linear_solver_type = LinearSolverType::ITERATIVE;
  static constexpr size_t kMaxNumImagesDirectSolver = 1000;
  // Linear solver when refine_intrinsics_on_device leaves a camera parameter variable (it applies to nothing else).
  // DIRECT: the blocked Cholesky of the bordered system (PCD_LINEAR_CHOLESKY).  ITERATIVE: the bordered PCG
  // (PCD_LINEAR_PCG_CAM), the reference's ITERATIVE_SCHUR + SCHUR_JACOBI with the intrinsics as parameter blocks.  AUTO:
  // by kMaxNumImagesDirectSolver, as linear_solver_type.
  LinearSolverType refined_linear_solver_type = LinearSolverType::DIRECT;
};

class BundleAdjustmentConfig {  // optim/bundle_adjustment.h:118-200, .cc:76-233
 public:
  void AddImage(image_t id) { image_ids_.insert(id); }
  bool HasImage(image_t id) const { return image_ids_.count(id) > 0; }
  void SetConstantCamera(camera_t id) { constant_camera_ids_.insert(id); }
  bool IsConstantCamera(camera_t id) const { return constant_camera_ids_.count(id) > 0; }
  void SetConstantPose(image_t id) { constant_poses_.insert(id); }
  bool HasConstantPose(image_t id) const { return constant_poses_.count(id) > 0; }
  void SetConstantTvec(image_t id, const std::vector<int>& idxs) { constant_tvecs_[id] = idxs; }
  bool HasConstantTvec(image_t id) const { return constant_tvecs_.count(id) > 0; }
  const std::vector<int>& ConstantTvec(image_t id) const { return constant_tvecs_.at(id); }
  void AddVariablePoint(point3D_t id) { variable_point3D_ids_.insert(id); }
  void AddConstantPoint(point3D_t id) { constant_point3D_ids_.insert(id); }
  bool HasVariablePoint(point3D_t id) const { return variable_point3D_ids_.count(id) > 0; }
  bool HasConstantPoint(point3D_t id) const { return constant_point3D_ids_.count(id) > 0; }
  void AddLidarPoint(point3D_t id, const LidarPoint& lp) { lidar_maps_[id] = lp; }
  size_t NumImages() const { return image_ids_.size(); }
  const std::unordered_set<image_t>& Images() const { return image_ids_; }
  const std::unordered_set<point3D_t>& VariablePoints() const { return variable_point3D_ids_; }
  const std::unordered_set<point3D_t>& ConstantPoints() const { return constant_point3D_ids_; }

  // optim/bundle_adjustment.cc:100-147 NumResiduals
  size_t NumResiduals(const Reconstruction& rec) const {
    size_t num_observations = 0;
    for (image_t id : image_ids_)
      for (const Point2D& p : rec.images.at(id).points2D) num_observations += p.HasPoint3D();
    auto extra = [&](point3D_t pid) {
      size_t n = 0;
      for (const TrackElement& te : rec.points3D.at(pid).track) n += !HasImage(te.image_id);
      return n;
    };
    for (point3D_t pid : variable_point3D_ids_) num_observations += extra(pid);
    for (point3D_t pid : constant_point3D_ids_) num_observations += extra(pid);
    return 2 * num_observations;
  }

  std::unordered_map<point3D_t, LidarPoint> lidar_maps_;

 private:
  std::unordered_set<camera_t> constant_camera_ids_;
  std::unordered_set<image_t> image_ids_, constant_poses_;
  std::unordered_set<point3D_t> variable_point3D_ids_, constant_point3D_ids_;
  std::unordered_map<image_t, std::vector<int>> constant_tvecs_;
};

class BundleAdjusterHip {
 public:
  enum class OptimazePhrase { Local, Global, WholeMap, NoLidar };  // (sic) optim/bundle_adjustment.h:205

  BundleAdjusterHip(const BundleAdjustmentOptions& options, const BundleAdjustmentConfig& config)
      : options_(options), config_(config) {}
  ~BundleAdjusterHip() { pcd_ba_destroy(ba_); }

  // ---- assembly (host) -------------------------------------------------------------------------
  void SetUp(Reconstruction* rec, OptimazePhrase phrase) {
    Clear();
    const bool lidar = options_.if_add_lidar_constraint && phrase != OptimazePhrase::NoLidar;
    for (image_t id : Sorted(config_.Images())) {
      if (lidar && phrase == OptimazePhrase::Global) AddImageToProblem(id, rec, /*in_sphere_only=*/true);
      else AddImageToProblem(id, rec, false);
    }
    for (point3D_t pid : Sorted(config_.VariablePoints())) AddPointToProblem(pid, rec);
    if (lidar)
      for (const auto& kv : SortedMap(config_.lidar_maps_)) AddLidarToProblem(kv.first, kv.second, rec);
    if (!(lidar && phrase == OptimazePhrase::WholeMap))   // SetUpAdjustWholeMapByLidar has no such loop (:664-682)
      for (point3D_t pid : Sorted(config_.ConstantPoints())) AddPointToProblem(pid, rec);
    ParameterizeCameras();
    ParameterizePoints(rec);
  }

  size_t NumResiduals() const { return 2 * obs_image_.size() + lidar_point_.size(); }
  // ceres::Solver::Summary::num_residuals_reduced: residual blocks whose parameter blocks are all constant drop out
  size_t NumResidualsReduced() const {
    size_t n = 0;
    for (size_t o = 0; o < obs_image_.size(); ++o) {
      const int im = obs_image_[o];
      if (!image_const_pose_[im] || !point_const_[obs_point_[o]] || CameraVariable(image_cam_[im])) n += 2;
    }
    for (int p : lidar_point_) n += point_const_[p] ? 0 : 1;
    return n;
  }
  // ceres::Solver::Summary::num_effective_parameters_reduced: tangent sizes of the variable parameter blocks --
  // 3 (quaternion) + 3 - #constant tvec entries per variable pose, 3 per variable point, the optimised subset of
  // each variable camera (ParameterizeCameras)
  size_t NumEffectiveParameters() const {
    size_t n = 0;
    for (size_t i = 0; i < poses_.size() / 7; ++i)
      if (image_used_[i] && !image_const_pose_[i]) n += 3 + 3 - __builtin_popcount(image_const_tvec_[i]);
    for (size_t p = 0; p < points_.size() / 3; ++p) n += point_const_[p] ? 0 : 3;
    for (uint8_t v : cam_refine_) n += v;
    return n;
  }
  bool CameraVariable(int cam_idx) const {
    const int k = pcd_camera_num_params(cam_model_[cam_idx]);
    for (int j = 0; j < k; ++j)
      if (cam_refine_[cam_off_[cam_idx] + j]) return true;
    return false;
  }
  size_t NumConstantPoints() const { size_t n = 0; for (uint8_t c : point_const_) n += c; return n; }

  // ---- evaluation (HIP) ------------------------------------------------------------------------
  bool Create(int device = 0) {
    if (NumResiduals() == 0) return false;                // Solve returns false (:489-491)
    pcd_ba_destroy(ba_);
    ba_ = nullptr;
    pcd_ba_desc d{};
    d.device = device;
    d.num_cameras = (int32_t)cam_model_.size(); d.cam_model = cam_model_.data(); d.cam_param_offset = cam_off_.data();
    d.cam_params = cam_params_.data(); d.cam_params_len = cam_params_.size();
    d.num_images = (int32_t)(poses_.size() / 7); d.poses = poses_.data(); d.image_camera = image_cam_.data();
    d.image_const_pose = image_const_pose_.data(); d.image_const_tvec = image_const_tvec_.data();
    d.num_points = (int32_t)(points_.size() / 3); d.points = points_.data(); d.point_const = point_const_.data();
    d.num_obs = obs_image_.size(); d.obs_image = obs_image_.data(); d.obs_point = obs_point_.data(); d.obs_xy = obs_xy_.data();
    d.num_lidar = lidar_point_.size(); d.lidar_point = lidar_point_.data(); d.lidar_abcd = lidar_abcd_.data();
    d.lidar_weight = lidar_w_.data();
    d.loss_type = options_.loss_function_type; d.loss_scale = options_.loss_function_scale;
    bool any_refined = false;
    for (uint8_t v : cam_refine_) any_refined |= v != 0;
    d.camera_refine = any_refined ? cam_refine_.data() : nullptr;   // NULL: intrinsics constant (the fork's default)
    return pcd_ba_create(&d, &ba_) == PCD_OK;
  }
  pcd_ba* handle() const { return ba_; }

  // ---- solve (HIP): the device route end to end, after SetUp() ---------------------------------
  // Create, pcd_ba_solve (LM with the linear solver options_.linear_solver_type selects, the block-sparse PCG on the
  // reduced camera system unless told otherwise; with refined intrinsics the one options_.refined_linear_solver_type
  // selects, the direct solve of the bordered system unless told otherwise), then the accepted poses and
  // points go back into the Reconstruction through image_ids_ / point_ids_; constant poses and points are not
  // written at all.  false when there are no residuals (as the reference, :489-491), when intrinsics are refined and
  // options_.refine_intrinsics_on_device is off (the caller stays on the Ceres route) or when a call fails
  // (pcd_last_error(); with refined intrinsics also when the library refuses: more refined cameras than
  // PCD_BA_MAX_CAMERA_SLOTS).  With refine_intrinsics_on_device the accepted parameters of every variable camera go back
  // into rec->cameras beside poses and points.
  bool Solve(Reconstruction* rec, int device = 0) {
    summary_ = pcd_ba_solve_summary{};
    if (NumResiduals() == 0) return false;
    bool refined = false;
    for (uint8_t v : cam_refine_) refined |= v != 0;
    if (refined && !options_.refine_intrinsics_on_device) return false;
    // after ReassociateLidar the live handle IS the problem (its parameters and terms are the flat arrays'): keep it
    if (!(reassociated_ && ba_) && !Create(device)) return false;
    reassociated_ = false;
    const pcd_ba_solve_opts o = SolveOpts(refined);
    if (pcd_ba_solve(ba_, &o, &summary_, nullptr) != PCD_OK) return false;
    if (pcd_ba_get_parameters(ba_, poses_.data(), points_.data()) != PCD_OK) return false;
    if (refined) {
      if (pcd_ba_get_camera_parameters(ba_, cam_params_.data()) != PCD_OK) return false;
      for (size_t c = 0; c < camera_ids_.size(); ++c) {
        if (!CameraVariable((int)c)) continue;
        Camera& cam = rec->cameras.at(camera_ids_[c]);
        std::copy(cam_params_.begin() + cam_off_[c], cam_params_.begin() + cam_off_[c] + cam.params.size(), cam.params.begin());
      }
    }
    for (size_t i = 0; i < image_ids_.size(); ++i) {
      if (image_const_pose_[i]) continue;
      Image& im = rec->images.at(image_ids_[i]);
      std::copy(poses_.begin() + 7 * i, poses_.begin() + 7 * i + 4, im.qvec);
      std::copy(poses_.begin() + 7 * i + 4, poses_.begin() + 7 * i + 7, im.tvec);
    }
    // A point without a residual block (one FilterPoints deleted: it stays in point_ids_) has meaningless coordinates and,
    // once the caller has run DeletePoint3D on the ids FilterPoints reported, no entry in the Reconstruction: not written
    std::vector<uint8_t> has_block(point_ids_.size(), 0);
    for (int p : obs_point_) has_block[p] = 1;
    for (int p : lidar_point_) has_block[p] = 1;
    for (size_t p = 0; p < point_ids_.size(); ++p) {
      if (point_const_[p] || !has_block[p]) continue;
      auto it = rec->points3D.find(point_ids_[p]);
      if (it == rec->points3D.end()) continue;
      std::copy(points_.begin() + 3 * p, points_.begin() + 3 * p + 3, it->second.xyz);
    }
    return true;
  }
  const pcd_ba_solve_summary& Summary() const { return summary_; }

  // ---- re-association (HIP): the loop of IncrementalMapper::AdjustGlobalBundleByLidar (sfm/incremental_mapper.cc:
  // 1413-1478) and of BundleAdjustmentController::Run (controllers/bundle_adjustment.cc:130-201) on the LIVE handle ----
  // After Create() or Solve(): the handle's current points are associated against `cloud` (anything with handle()
  // returning its pcd_cloud*, lidar::PointCloudProcess for one) and the accepted associations replace the handle's LiDAR
  // terms (pcd_ba_associate_lidar_device): nothing is uploaded again, nothing that depends on the observations is
  // rebuilt.  gate_mode: pcd_gate_mode, PCD_GATE_BOUNDED_SEARCH may be OR-ed in.  max_search_range: the schedule, one
  // entry or one per point in the order of point_ids_ (sfm/incremental_mapper.cc:1423-1427; ignored for
  // PCD_GATE_CONTROLLER).  select: the ids that are queries (the mapper's variable_point3D_ids; NULL: every point of
  // the problem, the controller's loop).  Weights: the options' icp / icp_ground weights.  This call installs
  // nearest-neighbour terms only: Proj terms the problem had are replaced with the rest.  ProjectLidar (below) is the
  // call that produces Proj terms on the live handle, weighted by proj_lidar_constraint_weight.
  // Then config_.lidar_maps_ and the flat term arrays are refreshed from pcd_ba_get_lidar, so NumResiduals() and a
  // later Solve -- which keeps this handle instead of creating a new one -- agree with the handle.
  // false without a live handle, or when a call fails (pcd_last_error()); the problem is then as it was.
  template <typename Cloud>
  bool ReassociateLidar(Cloud& cloud, int gate_mode, const std::vector<double>& max_search_range,
                        const std::unordered_set<point3D_t>* select = nullptr, pcd_ba_assoc_info* info = nullptr) {
    if (!ba_ || !cloud.handle()) return false;
    const size_t P = point_ids_.size();
    struct DevMem {   // freed on every return
      void* p = nullptr;
      ~DevMem() { if (p) (void)hipFree(p); }
      bool put(const void* src, size_t bytes) {
        return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess &&
               (bytes == 0 || hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess);
      }
    } d_range, d_select;
    pcd_ba_assoc_opts o;
    pcd_ba_assoc_opts_default(&o);
    o.gate_mode = gate_mode;
    o.icp_weight = options_.icp_lidar_constraint_weight;
    o.icp_ground_weight = options_.icp_ground_lidar_constraint_weight;
    if ((gate_mode & 0xFF) != PCD_GATE_CONTROLLER) {
      if (max_search_range.size() != 1 && max_search_range.size() != P) return false;
      if (!d_range.put(max_search_range.data(), max_search_range.size() * sizeof(double))) return false;
      o.d_max_range = static_cast<const double*>(d_range.p);
      o.max_range_count = max_search_range.size();
    }
    if (select) {
      std::vector<uint8_t> mask(P, 0);
      for (size_t p = 0; p < P; ++p) mask[p] = select->count(point_ids_[p]) ? 1 : 0;
      if (!d_select.put(mask.data(), P)) return false;
      o.d_select = static_cast<const uint8_t*>(d_select.p);
    }
    pcd_ba_assoc_info local{};
    if (pcd_ba_associate_lidar_device(ba_, cloud.handle(), &o, nullptr, &local) != PCD_OK) return false;
    if (info) *info = local;
    uint64_t L = 0;
    if (pcd_ba_get_lidar(ba_, &L, nullptr, nullptr, nullptr, nullptr, nullptr) != PCD_OK) return false;
    std::vector<int32_t> point(L);
    std::vector<double> abcd(4 * L), w(L), xyz(3 * L);
    std::vector<uint8_t> type(L);
    if (pcd_ba_get_lidar(ba_, &L, point.data(), abcd.data(), w.data(), type.data(), xyz.data()) != PCD_OK) return false;
    lidar_point_ = point; lidar_abcd_ = abcd; lidar_w_ = w;
    config_.lidar_maps_.clear();
    for (uint64_t l = 0; l < L; ++l) {
      LidarPoint lp;
      lp.type = type[l] == PCD_LIDAR_ICP_GROUND ? LidarPointType::IcpGround : LidarPointType::Icp;
      for (int k = 0; k < 3; ++k) lp.xyz[k] = xyz[3 * l + k];
      for (int k = 0; k < 4; ++k) lp.abcd[k] = abcd[4 * l + k];
      if (lp.type == LidarPointType::IcpGround) lp.color = {255, 255, 0};
      else lp.color = {0, 0, 255};
      config_.lidar_maps_[point_ids_[point[l]]] = lp;
    }
    reassociated_ = true;
    return true;
  }
  // ---- the LOCAL round (HIP): sfm/incremental_mapper.cc:1109-1165 on the live handle ----------------------------------
  // Short tracks take the depth-projection route (Project2Image -> PcdProj::SetNewImage on searched_image_ids, then
  // BundleAdjustmentConfig::MatchVariablePoint2LidarPoint), long tracks MatchClosestLidarPoint; both feed one term list.
  // proj: anything with handle() returning its pcd_proj* (lidar::PcdProj), built over the cloud the nearest-neighbour
  // points are associated against.  searched_image_ids: the images that are projected (lidar_searched_image_ids_; ids
  // outside the problem are ignored).  proj_point_ids / nn_point_ids: the points of either route; a point in neither
  // gets no term, a point in both takes the projection route.  max_search_range: one entry or one per point in the
  // order of point_ids_, for the nn points (PCD_GATE_MAPPER_LOCAL); may be empty when nn_point_ids is.
  // Everything runs in pcd_ba_project_lidar_device at the handle's CURRENT poses and points.  Then config_.lidar_maps_
  // and the flat term arrays are refreshed from pcd_ba_get_lidar as ReassociateLidar does; Proj terms get type Proj, the
  // colour red, and dist / angle recomputed from pcd_ba_get_parameters by lidar_hip.h's formulas.
  // false without a live handle or projector, or when a call fails (pcd_last_error()); the problem is then as it was.
  template <typename Projector>
  bool ProjectLidar(Projector& proj, const std::unordered_set<image_t>& searched_image_ids,
                    const std::unordered_set<point3D_t>& proj_point_ids, const std::unordered_set<point3D_t>& nn_point_ids,
                    const std::vector<double>& max_search_range, pcd_ba_proj_info* info = nullptr) {
    if (!ba_ || !proj.handle()) return false;
    const size_t P = point_ids_.size(), I = image_ids_.size();
    struct DevMem {   // freed on every return
      void* p = nullptr;
      ~DevMem() { if (p) (void)hipFree(p); }
      bool put(const void* src, size_t bytes) {
        return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess &&
               (bytes == 0 || hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess);
      }
    } d_range, d_images, d_mode;
    pcd_ba_proj_opts o;
    pcd_ba_proj_opts_default(&o);
    o.cam_width = cam_width_.data();
    o.cam_height = cam_height_.data();
    o.gate_mode = PCD_GATE_MAPPER_LOCAL;
    o.proj_weight = options_.proj_lidar_constraint_weight;
    o.icp_weight = options_.icp_lidar_constraint_weight;
    o.icp_ground_weight = options_.icp_ground_lidar_constraint_weight;
    std::vector<uint8_t> images(I, 0), mode(P, PCD_BA_POINT_NONE);
    for (size_t i = 0; i < I; ++i) images[i] = searched_image_ids.count(image_ids_[i]) ? 1 : 0;
    if (!d_images.put(images.data(), I)) return false;
    o.d_image_select = static_cast<const uint8_t*>(d_images.p);
    for (size_t p = 0; p < P; ++p)
      mode[p] = proj_point_ids.count(point_ids_[p]) ? PCD_BA_POINT_PROJ : nn_point_ids.count(point_ids_[p]) ? PCD_BA_POINT_NN
                                                                                                           : PCD_BA_POINT_NONE;
    if (!d_mode.put(mode.data(), P)) return false;
    o.d_point_mode = static_cast<const uint8_t*>(d_mode.p);
    std::vector<double> range = max_search_range;
    if (range.empty() && nn_point_ids.empty()) range.push_back(0.0);   // nobody reads it: no point has mode 2
    if (range.size() != 1 && range.size() != P) return false;
    if (!d_range.put(range.data(), range.size() * sizeof(double))) return false;
    o.d_max_range = static_cast<const double*>(d_range.p);
    o.max_range_count = range.size();
    pcd_ba_proj_info local{};
    if (pcd_ba_project_lidar_device(ba_, proj.handle(), &o, nullptr, &local) != PCD_OK) return false;
    if (info) *info = local;
    uint64_t L = 0;
    if (pcd_ba_get_lidar(ba_, &L, nullptr, nullptr, nullptr, nullptr, nullptr) != PCD_OK) return false;
    std::vector<int32_t> point(L);
    std::vector<double> abcd(4 * L), w(L), xyz(3 * L), X(3 * P);
    std::vector<uint8_t> type(L);
    if (pcd_ba_get_lidar(ba_, &L, point.data(), abcd.data(), w.data(), type.data(), xyz.data()) != PCD_OK) return false;
    if (pcd_ba_get_parameters(ba_, nullptr, X.data()) != PCD_OK) return false;
    lidar_point_ = point; lidar_abcd_ = abcd; lidar_w_ = w;
    config_.lidar_maps_.clear();
    for (uint64_t l = 0; l < L; ++l) {
      LidarPoint lp;
      lp.type = type[l] == PCD_LIDAR_PROJ ? LidarPointType::Proj
                : type[l] == PCD_LIDAR_ICP_GROUND ? LidarPointType::IcpGround : LidarPointType::Icp;
      for (int k = 0; k < 3; ++k) lp.xyz[k] = xyz[3 * l + k];
      for (int k = 0; k < 4; ++k) lp.abcd[k] = abcd[4 * l + k];
      if (lp.type == LidarPointType::Proj) {   // lidar_hip.h MatchVariablePoint2LidarPoint: point-to-plane, |cos|, red
        const double* x = &X[3 * (size_t)point[l]];
        const double a = lp.abcd[0], b = lp.abcd[1], c = lp.abcd[2], d = lp.abcd[3];
        lp.dist = std::fabs((x[0] * a + x[1] * b + x[2] * c) + d);
        const double v[3] = {x[0] - lp.xyz[0], x[1] - lp.xyz[1], x[2] - lp.xyz[2]};
        lp.angle = std::fabs((a * v[0] + b * v[1] + c * v[2]) / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
        lp.color = {255, 0, 0};
      } else if (lp.type == LidarPointType::IcpGround) {
        lp.color = {255, 255, 0};
      } else {
        lp.color = {0, 255, 0};   // the colour of the local call site (ToLidarPoint, PCD_GATE_MAPPER_LOCAL)
      }
      config_.lidar_maps_[point_ids_[point[l]]] = lp;
    }
    reassociated_ = true;
    return true;
  }
  // ---- the post-BA filter (HIP): IncrementalMapper::FilterPoints / Reconstruction::FilterPoints3D (base/reconstruction.cc:
  // 760-769) on the LIVE handle, at its current parameters (after Create() or Solve()) ------------------------------------
  // pcd_ba_filter_points_device over every point of the problem.  erased (may be NULL) receives the (image_id,
  // point2D_idx) of every observation the filter erases on a point it keeps, for the caller's DeleteObservation; deleted
  // (may be NULL) the ids of the points it deletes, for DeletePoint3D, which removes their remaining observations itself
  // (a point that has no observation in the problem, such as one an earlier call deleted, is not reported again).
  // With `apply` the flags are applied on the device (pcd_ba_remove_observations_device: nothing is uploaded, no second
  // Create) and the flat arrays -- obs_image_ / obs_point_ / obs_xy_ / obs_point2D_ and the term vectors, with
  // config_.lidar_maps_ -- are compacted by the same rule, so NumResiduals(), a later Create() and a later Solve (which
  // keeps this handle) agree with the handle.  A deleted point stays in point_ids_ without a residual block.
  // Returns the reference's num_filtered (elements for the reprojection filter, one per point for the angle filter);
  // *ok (may be NULL) is false without a live handle or when a call fails (pcd_last_error()): the problem is then as it was.
  size_t FilterPoints(double max_reproj_error, double min_tri_angle, bool apply,
                      std::vector<std::pair<image_t, point2D_t>>* erased = nullptr, std::vector<point3D_t>* deleted = nullptr,
                      bool* ok = nullptr) {
    if (ok) *ok = false;
    if (erased) erased->clear();
    if (deleted) deleted->clear();
    if (!ba_) return 0;
    const size_t O = obs_image_.size(), P = point_ids_.size();
    struct DevMem {   // freed on every return
      void* p = nullptr;
      ~DevMem() { if (p) (void)hipFree(p); }
    } d_flags, d_summary;
    if (hipMalloc(&d_flags.p, O + P + 1) != hipSuccess || hipMalloc(&d_summary.p, 4 * sizeof(double)) != hipSuccess) return 0;
    pcd_ba_filter_opts fo;
    pcd_ba_filter_opts_default(&fo);
    fo.max_reproj_error = max_reproj_error;
    fo.min_tri_angle_deg = min_tri_angle;
    pcd_ba_filter_out out{};
    out.obs_erase = static_cast<uint8_t*>(d_flags.p);
    out.point_delete = static_cast<uint8_t*>(d_flags.p) + O;
    out.summary = static_cast<double*>(d_summary.p);
    if (pcd_ba_filter_points_device(ba_, &fo, &out, nullptr) != PCD_OK) return 0;
    std::vector<uint8_t> flags(O + P + 1);
    double summary[4] = {0, 0, 0, 0};
    if (hipMemcpy(flags.data(), d_flags.p, O + P, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(summary, d_summary.p, sizeof summary, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    const uint8_t* erase = flags.data(), *pdel = flags.data() + O;
    if (apply && pcd_ba_remove_observations_device(ba_, out.obs_erase, out.point_delete, nullptr, nullptr, nullptr) != PCD_OK)
      return 0;
    for (size_t o = 0; o < O; ++o)
      if (erased && erase[o] && !pdel[obs_point_[o]]) erased->emplace_back(image_ids_[obs_image_[o]], obs_point2D_[o]);
    // a point without observations in the problem (one an earlier call emptied) is no news to the caller
    std::vector<uint32_t> track_len(P, 0);
    for (size_t o = 0; o < O; ++o) track_len[obs_point_[o]]++;
    for (size_t p = 0; p < P; ++p)
      if (deleted && pdel[p] && track_len[p]) deleted->push_back(point_ids_[p]);
    if (apply) {
      size_t n = 0;
      for (size_t o = 0; o < O; ++o) {
        if (erase[o] || pdel[obs_point_[o]]) continue;
        obs_image_[n] = obs_image_[o]; obs_point_[n] = obs_point_[o]; obs_point2D_[n] = obs_point2D_[o];
        obs_xy_[2 * n] = obs_xy_[2 * o]; obs_xy_[2 * n + 1] = obs_xy_[2 * o + 1];
        ++n;
      }
      obs_image_.resize(n); obs_point_.resize(n); obs_point2D_.resize(n); obs_xy_.resize(2 * n);
      size_t m = 0;
      for (size_t l = 0; l < lidar_point_.size(); ++l) {
        if (pdel[lidar_point_[l]]) { config_.lidar_maps_.erase(point_ids_[lidar_point_[l]]); continue; }
        lidar_point_[m] = lidar_point_[l]; lidar_w_[m] = lidar_w_[l];
        for (int k = 0; k < 4; ++k) lidar_abcd_[4 * m + k] = lidar_abcd_[4 * l + k];
        ++m;
      }
      lidar_point_.resize(m); lidar_w_.resize(m); lidar_abcd_.resize(4 * m);
      reassociated_ = true;   // the live handle is the problem: Solve keeps it
    }
    if (ok) *ok = true;
    return (size_t)summary[0];
  }
  // ---- rows and points added to the LIVE handle (HIP): what IncrementalMapper::CompleteAndMergeTracks and Retriangulate
  // (controllers/incremental_mapper.cc:157-162, :178) change in the problem between two adjustments ----------------------
  // A completed track is a list of elements on a point the problem has; a retriangulated point is an entry of new_points
  // with its elements; a merge (Reconstruction::MergePoints3D) is FilterPoints-style removal of the two points by the
  // caller followed by one new point with the union of their elements.
  struct NewElement { image_t image_id; point2D_t point2D_idx; point3D_t point3D_id; double xy[2]; };
  typedef std::pair<point3D_t, std::array<double, 3>> NewPoint;
  // The flat rows AddObservations hands to pcd_ba_add_observations, in that order: new point k becomes row P + k, an
  // element's point is the new row of its id if new_points has it (a re-created id is a new row; the row a deleted point
  // left behind stays dead), otherwise the row point_ids_ has for it.
  struct Addition {
    std::vector<int32_t> obs_image, obs_point;
    std::vector<double> obs_xy, points;
    std::vector<point2D_t> obs_point2D;
    std::vector<point3D_t> point_ids;
  };
  // false, *out untouched: an image that is not in the problem, a point id that is neither in point_ids_ nor among
  // new_points, or an id twice in new_points.  Pure host code.
  bool PlanAddition(const std::vector<NewElement>& elements, const std::vector<NewPoint>& new_points, Addition* out) const {
    Addition a;
    std::unordered_map<point3D_t, int> fresh;
    const int P = (int)point_ids_.size();
    for (const NewPoint& np : new_points) {
      if (!fresh.emplace(np.first, P + (int)a.point_ids.size()).second) return false;
      a.point_ids.push_back(np.first);
      a.points.insert(a.points.end(), np.second.begin(), np.second.end());
    }
    for (const NewElement& e : elements) {
      const auto im = image_index_.find(e.image_id);
      if (im == image_index_.end()) return false;
      int p;
      const auto f = fresh.find(e.point3D_id);
      if (f != fresh.end()) p = f->second;
      else {
        const auto it = point_index_.find(e.point3D_id);
        if (it == point_index_.end()) return false;
        p = it->second;
      }
      a.obs_image.push_back(im->second);
      a.obs_point.push_back(p);
      a.obs_point2D.push_back(e.point2D_idx);
      a.obs_xy.push_back(e.xy[0]);
      a.obs_xy.push_back(e.xy[1]);
    }
    *out = std::move(a);
    return true;
  }
  // pcd_ba_add_observations on the live handle, and the same rows appended to point_ids_, obs_image_, obs_point_,
  // obs_point2D_, obs_xy_, the point mirrors (points_, point_const_ = 0) and point3D_num_observations_, so that
  // FilterPoints, NumResiduals(), a later Create() and Solve's write-back (which keeps this handle) agree with the handle.
  // New points are variable and carry no LiDAR term until the next ReassociateLidar / ProjectLidar, whose per-point
  // arguments then cover them.  Returns the number of rows added; *ok (may be NULL) is false, with nothing changed, without
  // a live handle, when PlanAddition refuses, or when the call fails (pcd_last_error()).
  size_t AddObservations(const std::vector<NewElement>& elements, const std::vector<NewPoint>& new_points, bool* ok = nullptr) {
    if (ok) *ok = false;
    if (!ba_) return 0;
    Addition a;
    if (!PlanAddition(elements, new_points, &a)) return 0;
    if (pcd_ba_add_observations(ba_, a.points.data(), a.point_ids.size(), a.obs_image.data(), a.obs_point.data(),
                                a.obs_xy.data(), a.obs_image.size(), nullptr) != PCD_OK)
      return 0;
    for (size_t k = 0; k < a.point_ids.size(); ++k) {
      point_index_[a.point_ids[k]] = (int)point_ids_.size();
      point_ids_.push_back(a.point_ids[k]);
      point_const_.push_back(0);
      point3D_num_observations_[a.point_ids[k]] = 0;   // a re-created id starts over
    }
    points_.insert(points_.end(), a.points.begin(), a.points.end());
    for (size_t o = 0; o < a.obs_image.size(); ++o) {
      AddObservation(a.obs_image[o], a.obs_point[o], a.obs_point2D[o], &a.obs_xy[2 * o]);
      point3D_num_observations_[point_ids_[a.obs_point[o]]] += 1;
    }
    reassociated_ = true;   // the live handle is the problem: Solve keeps it
    if (ok) *ok = true;
    return a.obs_image.size();
  }
  // ---- one global round (HIP): IncrementalMapper::AdjustGlobalBundleByLidar (sfm/incremental_mapper.cc:1297-1493) on the
  // LIVE handle, which holds the whole map (after Create() or Solve()) ----------------------------------------------------
  // pcd_ba_window_create_device derives the sphere sub-problem around center_image_id (:1347-1408: images farther than
  // `radius` from its projection centre get a constant pose, only points seen from inside take part, with all their
  // observations) as a second handle; its active points search `cloud` within kd_max - GlobalOptNum * drop, at least
  // kd_min (:1423-1427), and the accepted associations become the window's LiDAR terms; pcd_ba_solve refines the window
  // with Solve's options; pcd_ba_window_commit_device carries the parameters back into the live handle.  Nothing is
  // downloaded to select and nothing is uploaded or rebuilt on the live handle, which keeps its rows, its terms and its
  // co-visibility structure.  Then the variable poses inside the sphere and the active variable points go back into the
  // Reconstruction and the flat mirrors, and GlobalOptNum advances for the active points (:1483-1487).  terms (may be
  // NULL) receives the round's LiDAR terms by point id.
  // The round's terms live on the window and go with it: the live handle, the flat lidar_* mirrors and
  // config_.lidar_maps_ keep what they held before the call (the whole map's terms, if any), as the reference's
  // ba_config of one round does not outlive it.  A Solve after GlobalRound keeps the live handle (it IS the problem, at
  // the committed parameters) and therefore adjusts the whole map WITHOUT the round's terms; a caller who wants them on
  // the whole map takes them from `terms` into the config of a new SetUp.
  // false without a live handle or cloud, for an image that is not in the problem, when intrinsics are refined and
  // options_.refine_intrinsics_on_device is off, or when a call fails (pcd_last_error()); the problem is then as it was.
  struct GlobalRoundInfo { pcd_ba_window_info window; pcd_ba_assoc_info assoc; pcd_ba_solve_summary solve; };
  template <typename Cloud>
  bool GlobalRound(Reconstruction* rec, Cloud& cloud, image_t center_image_id, double radius, double kd_max = 1.5,
                   double kd_min = 0.2, double drop = 0.1, GlobalRoundInfo* info = nullptr,
                   std::unordered_map<point3D_t, LidarPoint>* terms = nullptr) {
    if (info) *info = GlobalRoundInfo{};
    if (!ba_ || !cloud.handle()) return false;
    const auto center = image_index_.find(center_image_id);
    if (center == image_index_.end()) return false;
    bool refined = false;
    for (uint8_t v : cam_refine_) refined |= v != 0;
    if (refined && !options_.refine_intrinsics_on_device) return false;
    const size_t P = point_ids_.size(), I = image_ids_.size();
    struct DevMem {   // freed on every return
      void* p = nullptr;
      ~DevMem() { if (p) (void)hipFree(p); }
    } d_flags, d_range;
    struct Window {   // destroyed on every return
      pcd_ba* h = nullptr;
      ~Window() { pcd_ba_destroy(h); }
    } win;
    if (hipMalloc(&d_flags.p, I + P + 1) != hipSuccess || hipMalloc(&d_range.p, (P + 1) * sizeof(double)) != hipSuccess)
      return false;
    uint8_t* d_in = static_cast<uint8_t*>(d_flags.p), *d_active = d_in + I;
    GlobalRoundInfo r{};
    pcd_ba_window_opts wo;
    pcd_ba_window_opts_default(&wo);
    wo.center_image = center->second;
    wo.radius = radius;
    if (pcd_ba_window_create_device(ba_, &wo, d_in, d_active, nullptr, nullptr, &win.h, &r.window) != PCD_OK) return false;
    std::vector<int32_t> opt_num(P, 0);
    for (size_t p = 0; p < P; ++p) {
      const auto it = rec->points3D.find(point_ids_[p]);
      if (it != rec->points3D.end()) opt_num[p] = it->second.global_opt_num;
    }
    std::vector<double> range(P);
    if (pcd_search_range_schedule(opt_num.data(), P, kd_max, kd_min, drop, range.data()) != PCD_OK) return false;
    if (hipMemcpy(d_range.p, range.data(), P * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return false;
    pcd_ba_assoc_opts ao;
    pcd_ba_assoc_opts_default(&ao);
    ao.gate_mode = PCD_GATE_MAPPER_GLOBAL;
    ao.icp_weight = options_.icp_lidar_constraint_weight;
    ao.icp_ground_weight = options_.icp_ground_lidar_constraint_weight;
    ao.d_max_range = static_cast<const double*>(d_range.p);
    ao.max_range_count = P;
    ao.d_select = d_active;
    if (pcd_ba_associate_lidar_device(win.h, cloud.handle(), &ao, nullptr, &r.assoc) != PCD_OK) return false;
    const pcd_ba_solve_opts so = SolveOpts(refined);
    if (pcd_ba_solve(win.h, &so, &r.solve, nullptr) != PCD_OK) return false;
    std::vector<uint8_t> flags(I + P + 1);
    if (hipMemcpy(flags.data(), d_flags.p, I + P, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (terms) {
      terms->clear();
      uint64_t L = 0;
      if (pcd_ba_get_lidar(win.h, &L, nullptr, nullptr, nullptr, nullptr, nullptr) != PCD_OK) return false;
      std::vector<int32_t> point(L);
      std::vector<double> abcd(4 * L), w(L), xyz(3 * L);
      std::vector<uint8_t> type(L);
      if (pcd_ba_get_lidar(win.h, &L, point.data(), abcd.data(), w.data(), type.data(), xyz.data()) != PCD_OK) return false;
      for (uint64_t l = 0; l < L; ++l) {
        LidarPoint lp;
        lp.type = type[l] == PCD_LIDAR_ICP_GROUND ? LidarPointType::IcpGround : LidarPointType::Icp;
        for (int k = 0; k < 3; ++k) lp.xyz[k] = xyz[3 * l + k];
        for (int k = 0; k < 4; ++k) lp.abcd[k] = abcd[4 * l + k];
        if (lp.type == LidarPointType::IcpGround) lp.color = {255, 255, 0};
        else lp.color = {0, 0, 255};
        (*terms)[point_ids_[point[l]]] = lp;
      }
    }
    // from here on the problem changes: the live handle first, then its mirrors
    if (pcd_ba_window_commit_device(win.h, ba_, nullptr) != PCD_OK) return false;
    if (pcd_ba_get_parameters(ba_, poses_.data(), points_.data()) != PCD_OK) return false;
    if (refined && pcd_ba_get_camera_parameters(ba_, cam_params_.data()) != PCD_OK) return false;
    const uint8_t* in = flags.data(), *active = flags.data() + I;
    for (size_t i = 0; i < I; ++i) {
      if (image_const_pose_[i] || !in[i]) continue;
      Image& im = rec->images.at(image_ids_[i]);
      std::copy(poses_.begin() + 7 * i, poses_.begin() + 7 * i + 4, im.qvec);
      std::copy(poses_.begin() + 7 * i + 4, poses_.begin() + 7 * i + 7, im.tvec);
    }
    for (size_t p = 0; p < P; ++p) {
      if (!active[p]) continue;
      auto it = rec->points3D.find(point_ids_[p]);
      if (it == rec->points3D.end()) continue;
      if (!point_const_[p]) std::copy(points_.begin() + 3 * p, points_.begin() + 3 * p + 3, it->second.xyz);
      it->second.global_opt_num += 1;
    }
    if (refined)
      for (size_t c = 0; c < camera_ids_.size(); ++c) {
        if (!CameraVariable((int)c)) continue;
        Camera& cam = rec->cameras.at(camera_ids_[c]);
        std::copy(cam_params_.begin() + cam_off_[c], cam_params_.begin() + cam_off_[c] + cam.params.size(), cam.params.begin());
      }
    reassociated_ = true;   // the live handle is the problem: Solve keeps it
    summary_ = r.solve;
    if (info) *info = r;
    return true;
  }
  // ---- one local round (HIP): IncrementalMapper::AdjustLocalBundle (sfm/incremental_mapper.cc:1004-1213) on the LIVE
  // handle, which holds the whole map -----------------------------------------------------------------------------------
  // pcd_ba_local_bundle_device picks the bundle of image_id (FindLocalBundle, :1747-1914); pcd_ba_local_window_create_device
  // derives the sub-problem of the image, its bundle and the points the image observes with at most max_track_length rows
  // (:1110-1134) as a second handle; those points search `cloud` within kd_max - GlobalOptNum * drop, at least kd_min
  // (:1159-1164), and the accepted associations become the window's LiDAR terms; pcd_ba_solve refines the window with
  // Solve's options; pcd_ba_window_commit_device carries the parameters back.  Then the variable poses of the bundle and
  // the points go back into the Reconstruction and the flat mirrors.  The camera-constness rule (:1064-1080), the
  // depth-projection terms (ProjectLidar on a handle of one's own) and GlobalOptNum stay with the caller.  The live handle
  // keeps its rows, its terms and its co-visibility structure; the round's terms go with the window.
  // false without a live handle or cloud, for an image that is not in the problem, when intrinsics are refined and
  // options_.refine_intrinsics_on_device is off, or when a call fails (pcd_last_error()).  Up to and including a failed
  // commit the problem is then as it was.  Behind the commit only the read-backs of the live handle's parameters can
  // fail: the handle then holds the round's result, the flat mirrors and the Reconstruction do not, and Create() or the
  // next successful read brings them together.
  struct LocalRoundInfo {
    std::vector<image_t> bundle;
    pcd_ba_local_window_info window; pcd_ba_assoc_info assoc; pcd_ba_solve_summary solve;
  };
  template <typename Cloud>
  bool LocalRound(Reconstruction* rec, Cloud& cloud, image_t image_id, int num_images = 6, double min_tri_angle = 6.0,
                  uint32_t max_track_length = 1000, double kd_max = 1.5, double kd_min = 0.2, double drop = 0.1,
                  LocalRoundInfo* info = nullptr) {
    if (info) *info = LocalRoundInfo{};
    if (!ba_ || !cloud.handle() || num_images < 2) return false;
    const auto image = image_index_.find(image_id);
    if (image == image_index_.end()) return false;
    bool refined = false;
    for (uint8_t v : cam_refine_) refined |= v != 0;
    if (refined && !options_.refine_intrinsics_on_device) return false;
    const size_t P = point_ids_.size(), I = image_ids_.size(), cap = (size_t)num_images - 1;
    struct DevMem {   // freed on every return
      void* p = nullptr;
      ~DevMem() { if (p) (void)hipFree(p); }
    } d_flags, d_range, d_bundle;
    struct Window {   // destroyed on every return
      pcd_ba* h = nullptr;
      ~Window() { pcd_ba_destroy(h); }
    } win;
    if (hipMalloc(&d_flags.p, I + P + 1) != hipSuccess || hipMalloc(&d_range.p, (P + 1) * sizeof(double)) != hipSuccess ||
        hipMalloc(&d_bundle.p, (cap + 1) * sizeof(int32_t)) != hipSuccess)
      return false;
    uint8_t* d_set = static_cast<uint8_t*>(d_flags.p), *d_variable = d_set + I;
    int32_t* d_ids = static_cast<int32_t*>(d_bundle.p), *d_num = d_ids + cap;
    LocalRoundInfo r{};
    pcd_ba_local_bundle_opts bo;
    pcd_ba_local_bundle_opts_default(&bo);
    bo.image = image->second;
    bo.num_images = num_images;
    bo.min_tri_angle_deg = min_tri_angle;
    if (pcd_ba_local_bundle_device(ba_, &bo, d_ids, d_num, d_set, nullptr, nullptr, nullptr) != PCD_OK) return false;
    pcd_ba_local_window_opts wo;
    pcd_ba_local_window_opts_default(&wo);
    wo.d_image_set = d_set;
    wo.image = image->second;
    wo.max_track_length = max_track_length;
    if (pcd_ba_local_window_create_device(ba_, &wo, d_variable, nullptr, nullptr, &win.h, &r.window) != PCD_OK) return false;
    std::vector<int32_t> ids(cap + 1);
    if (hipMemcpy(ids.data(), d_bundle.p, (cap + 1) * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int32_t k = 0; k < ids[cap]; ++k) r.bundle.push_back(image_ids_[ids[k]]);
    std::vector<int32_t> opt_num(P, 0);
    for (size_t p = 0; p < P; ++p) {
      const auto it = rec->points3D.find(point_ids_[p]);
      if (it != rec->points3D.end()) opt_num[p] = it->second.global_opt_num;
    }
    std::vector<double> range(P);
    if (pcd_search_range_schedule(opt_num.data(), P, kd_max, kd_min, drop, range.data()) != PCD_OK) return false;
    if (hipMemcpy(d_range.p, range.data(), P * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return false;
    pcd_ba_assoc_opts ao;
    pcd_ba_assoc_opts_default(&ao);
    ao.gate_mode = PCD_GATE_MAPPER_LOCAL;
    ao.icp_weight = options_.icp_lidar_constraint_weight;
    ao.icp_ground_weight = options_.icp_ground_lidar_constraint_weight;
    ao.d_max_range = static_cast<const double*>(d_range.p);
    ao.max_range_count = P;
    ao.d_select = d_variable;
    if (pcd_ba_associate_lidar_device(win.h, cloud.handle(), &ao, nullptr, &r.assoc) != PCD_OK) return false;
    const pcd_ba_solve_opts so = SolveOpts(refined);
    if (pcd_ba_solve(win.h, &so, &r.solve, nullptr) != PCD_OK) return false;
    std::vector<uint8_t> flags(I + P + 1);
    if (hipMemcpy(flags.data(), d_flags.p, I + P, hipMemcpyDeviceToHost) != hipSuccess) return false;
    // from here on the problem changes: the live handle first, then its mirrors
    if (pcd_ba_window_commit_device(win.h, ba_, nullptr) != PCD_OK) return false;
    if (pcd_ba_get_parameters(ba_, poses_.data(), points_.data()) != PCD_OK) return false;
    if (refined && pcd_ba_get_camera_parameters(ba_, cam_params_.data()) != PCD_OK) return false;
    for (size_t i = 0; i < I; ++i) {
      if (image_const_pose_[i] || !flags[i]) continue;
      Image& im = rec->images.at(image_ids_[i]);
      std::copy(poses_.begin() + 7 * i, poses_.begin() + 7 * i + 4, im.qvec);
      std::copy(poses_.begin() + 7 * i + 4, poses_.begin() + 7 * i + 7, im.tvec);
    }
    for (size_t p = 0; p < P; ++p) {   // a point the window held constant kept its bits: the copy changes nothing there
      if (point_const_[p]) continue;
      auto it = rec->points3D.find(point_ids_[p]);
      if (it != rec->points3D.end()) std::copy(points_.begin() + 3 * p, points_.begin() + 3 * p + 3, it->second.xyz);
    }
    if (refined)
      for (size_t c = 0; c < camera_ids_.size(); ++c) {
        if (!CameraVariable((int)c)) continue;
        Camera& cam = rec->cameras.at(camera_ids_[c]);
        std::copy(cam_params_.begin() + cam_off_[c], cam_params_.begin() + cam_off_[c] + cam.params.size(), cam.params.begin());
      }
    reassociated_ = true;   // the live handle is the problem: Solve keeps it
    summary_ = r.solve;
    if (info) *info = r;
    return true;
  }
  const BundleAdjustmentConfig& config() const { return config_; }
  // what Solve hands to pcd_ba_solve: AUTO goes by the number of images in the config, as the reference does
  bool UsesDirectSolver() const {
    using T = BundleAdjustmentOptions::LinearSolverType;
    return options_.linear_solver_type == T::DIRECT ||
           (options_.linear_solver_type == T::AUTO &&
            config_.NumImages() <= BundleAdjustmentOptions::kMaxNumImagesDirectSolver);
  }
  // the options Solve and GlobalRound hand to pcd_ba_solve
  pcd_ba_solve_opts SolveOpts(bool refined) const {
    pcd_ba_solve_opts o;
    pcd_ba_solve_opts_default(&o);
    o.max_num_iterations = options_.max_num_iterations;
    o.function_tolerance = options_.function_tolerance;
    o.gradient_tolerance = options_.gradient_tolerance;
    o.linear.max_iterations = options_.max_linear_solver_iterations;
    if (refined) o.linear_solver = RefinedUsesDirectSolver() ? PCD_LINEAR_CHOLESKY : PCD_LINEAR_PCG_CAM;
    else o.linear_solver = UsesDirectSolver() ? PCD_LINEAR_CHOLESKY : PCD_LINEAR_PCG;
    o.refine_intrinsics = refined ? 1 : 0;
    return o;
  }
  // the same choice for a solve with refined intrinsics (options_.refined_linear_solver_type)
  bool RefinedUsesDirectSolver() const {
    using T = BundleAdjustmentOptions::LinearSolverType;
    return options_.refined_linear_solver_type == T::DIRECT ||
           (options_.refined_linear_solver_type == T::AUTO &&
            config_.NumImages() <= BundleAdjustmentOptions::kMaxNumImagesDirectSolver);
  }

  // flat arrays (also what a solver scatters back into the Reconstruction)
  std::vector<int32_t> cam_model_, cam_off_, image_cam_, obs_image_, obs_point_, lidar_point_;
  std::vector<double> cam_params_, poses_, points_, obs_xy_, lidar_abcd_, lidar_w_;
  std::vector<uint8_t> image_const_pose_, image_const_tvec_, point_const_, image_used_;
  std::vector<uint8_t> cam_refine_;      // per entry of cam_params_: 1 = optimised (pcd_ba_desc.camera_refine)
  std::vector<camera_t> camera_ids_;     // flat index -> id
  std::vector<uint64_t> cam_width_, cam_height_;   // Camera::Width / Height by flat index (ProjectLidar)
  std::vector<image_t> image_ids_;       // flat index -> id
  std::vector<point3D_t> point_ids_;
  std::vector<point2D_t> obs_point2D_;   // per observation: its index among the image's points2D (FilterPoints hands it back)

 private:
  template <typename S>
  static std::vector<typename S::value_type> Sorted(const S& s) {   // deterministic order (hash order is not)
    std::vector<typename S::value_type> v(s.begin(), s.end());
    std::sort(v.begin(), v.end());
    return v;
  }
  template <typename M>
  static std::map<typename M::key_type, typename M::mapped_type> SortedMap(const M& m) {
    return std::map<typename M::key_type, typename M::mapped_type>(m.begin(), m.end());
  }
  void Clear() {
    cam_model_.clear(); cam_off_.clear(); image_cam_.clear(); obs_image_.clear(); obs_point_.clear();
    lidar_point_.clear(); cam_params_.clear(); poses_.clear(); points_.clear(); obs_xy_.clear();
    lidar_abcd_.clear(); lidar_w_.clear(); image_const_pose_.clear(); image_const_tvec_.clear();
    point_const_.clear(); image_used_.clear(); image_ids_.clear(); point_ids_.clear();
    cam_refine_.clear(); camera_ids_.clear(); cam_width_.clear(); cam_height_.clear();
    cam_index_.clear(); image_index_.clear(); point_index_.clear(); point3D_num_observations_.clear();
    obs_point2D_.clear();
    reassociated_ = false;
  }
  int CameraIndex(camera_t id, const Reconstruction* rec) {
    auto it = cam_index_.find(id);
    if (it != cam_index_.end()) return it->second;
    const Camera& c = rec->cameras.at(id);
    const int idx = (int)cam_model_.size();
    cam_index_[id] = idx;
    camera_ids_.push_back(id);
    cam_width_.push_back(c.width); cam_height_.push_back(c.height);
    cam_model_.push_back(c.model_id);
    cam_off_.push_back((int32_t)cam_params_.size());
    cam_params_.insert(cam_params_.end(), c.params.begin(), c.params.end());
    return idx;
  }
  // const_pose_block: the residual blocks of this image use the constant-pose functor
  int ImageIndex(image_t id, Reconstruction* rec, bool const_pose_block) {
    auto it = image_index_.find(id);
    if (it != image_index_.end()) return it->second;
    const Image& im = rec->images.at(id);
    const int idx = (int)image_cam_.size();
    image_index_[id] = idx;
    image_ids_.push_back(id);
    image_cam_.push_back(CameraIndex(im.camera_id, rec));
    poses_.insert(poses_.end(), im.qvec, im.qvec + 4);
    poses_.insert(poses_.end(), im.tvec, im.tvec + 3);
    image_const_pose_.push_back(const_pose_block ? 1 : 0);
    uint8_t mask = 0;
    if (!const_pose_block && config_.HasConstantTvec(id))
      for (int k : config_.ConstantTvec(id)) mask |= (uint8_t)(1u << k);   // SetSubsetManifold(3, idxs) :912-915
    image_const_tvec_.push_back(mask);
    image_used_.push_back(0);
    return idx;
  }
  int PointIndex(point3D_t id, const Reconstruction* rec) {
    auto it = point_index_.find(id);
    if (it != point_index_.end()) return it->second;
    const Point3D& p = rec->points3D.at(id);
    const int idx = (int)point_const_.size();
    point_index_[id] = idx;
    point_ids_.push_back(id);
    points_.insert(points_.end(), p.xyz, p.xyz + 3);
    point_const_.push_back(0);
    return idx;
  }
  void AddObservation(int image_idx, int point_idx, point2D_t point2D_idx, const double xy[2]) {
    obs_point2D_.push_back(point2D_idx);
    obs_image_.push_back(image_idx);
    obs_point_.push_back(point_idx);
    obs_xy_.push_back(xy[0]);
    obs_xy_.push_back(xy[1]);
    image_used_[image_idx] = 1;
  }
  // :814-919 and :694-806 (in_sphere_only skips points with !IfInSphere(), :734)
  void AddImageToProblem(image_t image_id, Reconstruction* rec, bool in_sphere_only) {
    Image& image = rec->images.at(image_id);
    image.NormalizeQvec();                                                                     // :823
    const bool constant_pose = !options_.refine_extrinsics || config_.HasConstantPose(image_id);  // :831
    const int ii = ImageIndex(image_id, rec, constant_pose);
    for (size_t k = 0; k < image.points2D.size(); ++k) {
      const Point2D& p2 = image.points2D[k];
      if (!p2.HasPoint3D()) continue;
      if (in_sphere_only && !rec->points3D.at(p2.point3D_id).if_in_sphere) continue;
      point3D_num_observations_[p2.point3D_id] += 1;
      AddObservation(ii, PointIndex(p2.point3D_id, rec), (point2D_t)k, p2.xy);
    }
  }
  // :927-985: observations of the point from images outside the config -> constant-pose blocks
  void AddPointToProblem(point3D_t pid, Reconstruction* rec) {
    const Point3D& p = rec->points3D.at(pid);
    if (point3D_num_observations_[pid] == p.track.size()) return;
    for (const TrackElement& te : p.track) {
      if (config_.HasImage(te.image_id)) continue;
      point3D_num_observations_[pid] += 1;
      Image& image = rec->images.at(te.image_id);
      if (cam_index_.count(image.camera_id) == 0) config_.SetConstantCamera(image.camera_id);   // :951-954
      const int ii = ImageIndex(te.image_id, rec, /*const_pose_block=*/true);
      AddObservation(ii, PointIndex(pid, rec), te.point2D_idx, image.points2D.at(te.point2D_idx).xy);
    }
  }
  // :993-1040
  void AddLidarToProblem(point3D_t pid, const LidarPoint& lp, const Reconstruction* rec) {
    for (int i = 0; i < 4; ++i)
      if (std::isnan(lp.abcd[i])) return;                                                       // :1005-1009
    double w;
    if (lp.type == LidarPointType::Proj) w = options_.proj_lidar_constraint_weight;            // :1013-1028
    else if (lp.type == LidarPointType::Icp) w = options_.icp_lidar_constraint_weight;
    else w = options_.icp_ground_lidar_constraint_weight;
    lidar_point_.push_back(PointIndex(pid, rec));
    lidar_abcd_.insert(lidar_abcd_.end(), lp.abcd.begin(), lp.abcd.end());
    lidar_w_.push_back(w);
  }
  // :1047-1100: which camera parameters are optimised
  void ParameterizeCameras() {
    const bool constant_camera =
        !options_.refine_focal_length && !options_.refine_principal_point && !options_.refine_extra_params;
    cam_refine_.assign(cam_params_.size(), 0);
    for (size_t c = 0; c < cam_model_.size(); ++c) {
      if (constant_camera || config_.IsConstantCamera(camera_ids_[c])) continue;   // SetParameterBlockConstant
      uint8_t group[PCD_CAM_JAC_STRIDE];
      if (pcd_camera_param_groups(cam_model_[c], group) != PCD_OK) continue;
      const int k = pcd_camera_num_params(cam_model_[c]);
      for (int j = 0; j < k; ++j) {                                                // SubsetManifold for the rest
        const bool refine = group[j] == 0 ? options_.refine_focal_length
                          : group[j] == 1 ? options_.refine_principal_point : options_.refine_extra_params;
        cam_refine_[cam_off_[c] + j] = refine ? 1 : 0;
      }
    }
  }
  // :1107-1131
  void ParameterizePoints(const Reconstruction* rec) {
    for (const auto& kv : point3D_num_observations_) {
      auto it = point_index_.find(kv.first);
      if (it == point_index_.end()) continue;
      if (rec->points3D.at(kv.first).track.size() > kv.second) point_const_[it->second] = 1;
    }
    for (point3D_t pid : config_.ConstantPoints()) {
      auto it = point_index_.find(pid);
      if (it != point_index_.end()) point_const_[it->second] = 1;
    }
  }

  const BundleAdjustmentOptions options_;
  BundleAdjustmentConfig config_;
  pcd_ba* ba_ = nullptr;
  pcd_ba_solve_summary summary_{};
  bool reassociated_ = false;   // ReassociateLidar ran on ba_ since the last Create: Solve keeps the handle
  std::unordered_map<camera_t, int> cam_index_;
  std::unordered_map<image_t, int> image_index_;
  std::unordered_map<point3D_t, int> point_index_;
  std::unordered_map<point3D_t, size_t> point3D_num_observations_;
};

}  // namespace colmap_hip

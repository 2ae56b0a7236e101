// test_ba_add.cc -- BundleAdjusterHip::AddObservations (ba_problem.h): the rows CompleteAndMergeTracks and Retriangulate
// add between two adjustments, appended to the live handle on the device behind the reference's bookkeeping.
//   ./test_ba_add          the refusals and the bookkeeping that need no GPU
//   ./test_ba_add --gpu    Solve, FilterPoints(apply), AddObservations (a completed track, a retriangulated point, a merge
//                          as delete-two-add-one), Solve, against a second handle created from the shim's flat arrays
//                          (fails if no gfx950 device)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "ba_problem.h"

using namespace colmap_hip;
typedef BundleAdjusterHip::NewElement NewElement;
typedef BundleAdjusterHip::NewPoint NewPoint;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

constexpr size_t kImages = 4, kNear = 60, kOpen = 5;   // points 1 .. kNear; the first kOpen are not yet matched in image 3
constexpr point3D_t kRetri = 1000, kMergeA = 2001, kMergeB = 2002, kMerged = 2003;
constexpr double kF = 1200.0;

static void Project(const Image& im, const double xyz[3], double xy[2]) {
  const double X = xyz[0] + im.tvec[0], Y = xyz[1] + im.tvec[1], Z = xyz[2] + im.tvec[2];
  xy[0] = kF * X / Z + 500.0;
  xy[1] = kF * Y / Z + 500.0;
}

// Identity rotations, t = (i - 1.5, 0.3 i, 10): any two images see a point near the origin under more than 5 degrees.
// Every image has a feature for every near point (index p - 1), for the point a later retriangulation creates (index
// kNear) and for the duplicated point (index kNear + 1).  In the problem at first: near point p in every image, but
// p <= kOpen not in image 3; kMergeA = the duplicated point as image 0 sees it, kMergeB = as image 1 sees it (two tracks
// of length 1, which FilterPoints deletes).  retri / dup: where the two later points are.
static void GenerateReconstruction(Reconstruction* rec, double retri[3], double dup[3]) {
  std::mt19937 rng(0);
  std::uniform_real_distribution<double> u(-1.0, 1.0), px(-1.0, 1.0);
  for (point3D_t p = 1; p <= kNear; ++p) {
    Point3D pt;
    for (double& c : pt.xyz) c = u(rng);
    rec->points3D[p] = pt;
  }
  for (int k = 0; k < 3; ++k) { retri[k] = u(rng); dup[k] = u(rng); }
  Point3D a, b;
  for (int k = 0; k < 3; ++k) { a.xyz[k] = dup[k] + 0.01; b.xyz[k] = dup[k] - 0.01; }
  rec->points3D[kMergeA] = a;
  rec->points3D[kMergeB] = b;
  Camera cam;
  cam.model_id = PCD_CAM_SIMPLE_RADIAL;
  cam.params = {kF, 500.0, 500.0, 0.0};
  rec->cameras[0] = cam;
  for (image_t i = 0; i < kImages; ++i) {
    Image im;
    im.camera_id = 0;
    im.tvec[0] = (double)i - 1.5; im.tvec[1] = 0.3 * i; im.tvec[2] = 10;
    for (point3D_t p = 1; p <= kNear + 2; ++p) {
      const double* xyz = p <= kNear ? rec->points3D[p].xyz : p == kNear + 1 ? retri : dup;
      Point2D p2;
      Project(im, xyz, p2.xy);
      p2.xy[0] += px(rng); p2.xy[1] += px(rng);
      if (p <= kNear && !(p <= kOpen && i == 3)) {
        p2.point3D_id = p;
        rec->points3D[p].track.push_back({i, (point2D_t)(p - 1)});
      }
      if (p == kNear + 2 && i < 2) {
        p2.point3D_id = i == 0 ? kMergeA : kMergeB;
        rec->points3D[p2.point3D_id].track.push_back({i, (point2D_t)(p - 1)});
      }
      im.points2D.push_back(p2);
    }
    rec->images[i] = im;
  }
}

static NewElement Element(const Reconstruction& rec, image_t i, point2D_t idx, point3D_t id) {
  const Point2D& p2 = rec.images.at(i).points2D.at(idx);
  return NewElement{i, idx, id, {p2.xy[0], p2.xy[1]}};
}

// the three kinds of addition, and the Reconstruction brought along the way the reference's triangulator does
static void MakeAdditions(Reconstruction* rec, const double retri[3], const double dup[3], std::vector<NewElement>* elements,
                          std::vector<NewPoint>* new_points) {
  auto attach = [&](image_t i, point2D_t idx, point3D_t id) {
    elements->push_back(Element(*rec, i, idx, id));
    rec->images.at(i).points2D.at(idx).point3D_id = id;
    rec->points3D[id].track.push_back({i, idx});
  };
  for (point3D_t p = 1; p <= kOpen; ++p) attach(3, (point2D_t)(p - 1), p);                 // completed tracks
  new_points->push_back({kRetri, {retri[0], retri[1], retri[2]}});                         // a retriangulated point
  for (int k = 0; k < 3; ++k) rec->points3D[kRetri].xyz[k] = retri[k];
  for (image_t i = 1; i < kImages; ++i) attach(i, (point2D_t)kNear, kRetri);
  new_points->push_back({kMerged, {dup[0], dup[1], dup[2]}});                              // the merge: one for two
  for (int k = 0; k < 3; ++k) rec->points3D[kMerged].xyz[k] = dup[k];
  attach(0, (point2D_t)(kNear + 1), kMerged);
  attach(1, (point2D_t)(kNear + 1), kMerged);
}

static void TestRefusalsAndBookkeeping() {
  pcd_ba_add_info info;
  std::memset(&info, 0xFF, sizeof info);
  CHECK(pcd_ba_add_observations_device(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &info) == PCD_ERR_INVALID);
  CHECK(info.num_obs == 0 && info.num_points_added == 0 && info.rebuild_ms == 0.0);
  CHECK(pcd_ba_add_observations(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr) == PCD_ERR_INVALID);
  Reconstruction rec;
  double retri[3], dup[3];
  GenerateReconstruction(&rec, retri, dup);
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < 3; ++i) config.AddImage(i);   // image 3 is not in the problem: no point of images 0-2 has it
  BundleAdjusterHip ba(BundleAdjustmentOptions(), config);
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  const size_t O = ba.obs_image_.size(), P = ba.point_ids_.size();
  CHECK(P == kNear + 2 && O > 0 && ba.points_.size() == 3 * P);
  const bool has_image3 = std::find(ba.image_ids_.begin(), ba.image_ids_.end(), (image_t)3) != ba.image_ids_.end();
  // (AddPointToProblem brings image 3 in as a constant-pose image when a point's track reaches into it)
  std::vector<NewElement> elements = {Element(rec, 1, (point2D_t)kNear, kRetri), Element(rec, 0, 7, 8),
                                      Element(rec, 2, (point2D_t)kNear, kRetri), Element(rec, 1, 0, kMergeA)};
  std::vector<NewPoint> new_points = {{kRetri, {retri[0], retri[1], retri[2]}}, {kMergeA, {9.0, 8.0, 7.0}}};
  BundleAdjusterHip::Addition plan;
  CHECK(ba.PlanAddition(elements, new_points, &plan));
  auto row = [&](point3D_t id) { return (int32_t)(std::find(ba.point_ids_.begin(), ba.point_ids_.end(), id) - ba.point_ids_.begin()); };
  auto img = [&](image_t id) { return (int32_t)(std::find(ba.image_ids_.begin(), ba.image_ids_.end(), id) - ba.image_ids_.begin()); };
  // new points get P, P + 1 in the order given; an id the problem has already is a new row when it is re-created
  CHECK(plan.point_ids == std::vector<point3D_t>({kRetri, kMergeA}));
  CHECK(plan.points == std::vector<double>({retri[0], retri[1], retri[2], 9.0, 8.0, 7.0}));
  CHECK(plan.obs_image == std::vector<int32_t>({img(1), img(0), img(2), img(1)}));
  CHECK(plan.obs_point == std::vector<int32_t>({(int32_t)P, row(8), (int32_t)P, (int32_t)P + 1}));
  CHECK(row(kMergeA) < (int32_t)P && row(8) < (int32_t)P);
  CHECK(plan.obs_point2D == std::vector<point2D_t>({(point2D_t)kNear, 7, (point2D_t)kNear, 0}));
  CHECK(plan.obs_xy.size() == 8 && plan.obs_xy[2] == rec.images.at(0).points2D[7].xy[0] &&
        plan.obs_xy[7] == rec.images.at(1).points2D[0].xy[1]);
  // the refusals, *out untouched: an image outside the problem, an unknown point, an id twice among the new points
  BundleAdjusterHip::Addition keep = plan;
  if (!has_image3) CHECK(!ba.PlanAddition({Element(rec, 3, 0, 1)}, {}, &plan));
  CHECK(!ba.PlanAddition({NewElement{77, 0, 1, {0, 0}}}, {}, &plan));
  CHECK(!ba.PlanAddition({Element(rec, 0, (point2D_t)kNear, kRetri)}, {}, &plan));
  CHECK(!ba.PlanAddition({}, {new_points[0], new_points[0]}, &plan));
  CHECK(plan.obs_point == keep.obs_point && plan.point_ids == keep.point_ids);
  CHECK(ba.PlanAddition({}, {}, &plan) && plan.obs_image.empty() && plan.point_ids.empty());
  // no live handle: AddObservations says so and touches nothing
  bool ok = true;
  const size_t residuals = ba.NumResiduals();
  CHECK(ba.AddObservations(elements, new_points, &ok) == 0 && !ok);
  CHECK(ba.NumResiduals() == residuals && ba.point_ids_.size() == P && ba.points_.size() == 3 * P && ba.obs_point2D_.size() == O);
}

static bool SameBits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

struct Evaluation { double cost = -1.0; std::vector<double> residuals; };
static Evaluation Evaluate(pcd_ba* h, size_t n) {
  Evaluation e;
  e.residuals.resize(n);
  pcd_ba_out o{};
  o.cost = &e.cost;
  o.residuals = e.residuals.data();
  CHECK(pcd_ba_evaluate(h, &o) == PCD_OK);
  return e;
}

// a second handle from the shim's own flat arrays (what Create hands to pcd_ba_create)
static pcd_ba* Fresh(const BundleAdjusterHip& ba, const BundleAdjustmentOptions& opt) {
  pcd_ba_desc d{};
  d.num_cameras = (int32_t)ba.cam_model_.size(); d.cam_model = ba.cam_model_.data(); d.cam_param_offset = ba.cam_off_.data();
  d.cam_params = ba.cam_params_.data(); d.cam_params_len = ba.cam_params_.size();
  d.num_images = (int32_t)(ba.poses_.size() / 7); d.poses = ba.poses_.data(); d.image_camera = ba.image_cam_.data();
  d.image_const_pose = ba.image_const_pose_.data(); d.image_const_tvec = ba.image_const_tvec_.data();
  d.num_points = (int32_t)(ba.points_.size() / 3); d.points = ba.points_.data(); d.point_const = ba.point_const_.data();
  d.num_obs = ba.obs_image_.size(); d.obs_image = ba.obs_image_.data(); d.obs_point = ba.obs_point_.data(); d.obs_xy = ba.obs_xy_.data();
  d.num_lidar = ba.lidar_point_.size(); d.lidar_point = ba.lidar_point_.data(); d.lidar_abcd = ba.lidar_abcd_.data();
  d.lidar_weight = ba.lidar_w_.data();
  d.loss_type = opt.loss_function_type; d.loss_scale = opt.loss_function_scale;
  pcd_ba* h = nullptr;
  CHECK(pcd_ba_create(&d, &h) == PCD_OK);
  return h;
}

static void TestAdd() {
  Reconstruction rec;
  double retri[3], dup[3];
  GenerateReconstruction(&rec, retri, dup);
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < kImages; ++i) config.AddImage(i);
  config.SetConstantPose(0);
  config.SetConstantTvec(1, {0});
  for (point3D_t p = 2; p <= kNear; p += 9) {           // LiDAR terms on 7 points
    LidarPoint lp;
    lp.type = LidarPointType::Icp;
    lp.abcd = {0.0, 0.0, 1.0, -rec.points3D[p].xyz[2] + 0.01};
    config.AddLidarPoint(p, lp);
  }
  BundleAdjustmentOptions opt;
  opt.max_num_iterations = 10;
  opt.if_add_lidar_constraint = true;
  BundleAdjusterHip ba(opt, config);
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::Local);
  const size_t O0 = ba.obs_image_.size(), P0 = ba.point_ids_.size(), L = ba.lidar_point_.size();
  CHECK(O0 == kImages * kNear - kOpen + 2 && P0 == kNear + 2 && L == 7);
  // adjust, filter: the two single-view duplicates go
  CHECK(ba.Solve(&rec));
  pcd_ba* live = ba.handle();
  bool ok = false;
  std::vector<std::pair<image_t, point2D_t>> erased;
  std::vector<point3D_t> deleted;
  ba.FilterPoints(8.0, 1.5, true, &erased, &deleted, &ok);
  CHECK(ok && erased.empty() && deleted == std::vector<point3D_t>({kMergeA, kMergeB}));
  for (const point3D_t id : deleted) {
    for (const TrackElement& te : rec.points3D.at(id).track)
      rec.images.at(te.image_id).points2D.at(te.point2D_idx).point3D_id = kInvalidPoint3DId;
    rec.points3D.erase(id);
  }
  const size_t O1 = ba.obs_image_.size();
  CHECK(O1 == O0 - 2);
  // complete, retriangulate, merge
  std::vector<NewElement> elements;
  std::vector<NewPoint> new_points;
  MakeAdditions(&rec, retri, dup, &elements, &new_points);
  CHECK(elements.size() == kOpen + 3 + 2);
  // a refused call first: nothing changes, on the handle or in the arrays
  std::vector<NewElement> bad = elements;
  bad.back().point3D_id = 4242;
  CHECK(ba.AddObservations(bad, new_points, &ok) == 0 && !ok && ba.obs_image_.size() == O1 && ba.point_ids_.size() == P0);
  CHECK(ba.AddObservations(elements, new_points, &ok) == elements.size() && ok && ba.handle() == live);
  const size_t O2 = O1 + elements.size(), P2 = P0 + 2;
  CHECK(ba.obs_image_.size() == O2 && ba.obs_point_.size() == O2 && ba.obs_point2D_.size() == O2 && ba.obs_xy_.size() == 2 * O2);
  CHECK(ba.point_ids_.size() == P2 && ba.points_.size() == 3 * P2 && ba.point_const_.size() == P2);
  CHECK(ba.point_ids_[P0] == kRetri && ba.point_ids_[P0 + 1] == kMerged && !ba.point_const_[P0] && !ba.point_const_[P0 + 1]);
  CHECK(ba.NumResiduals() == 2 * O2 + L);
  for (size_t o = O1; o < O2; ++o) {                     // the rows as given, and each leads back to its point
    const NewElement& e = elements[o - O1];
    CHECK(ba.image_ids_[ba.obs_image_[o]] == e.image_id && ba.obs_point2D_[o] == e.point2D_idx);
    CHECK(ba.point_ids_[ba.obs_point_[o]] == e.point3D_id && ba.obs_xy_[2 * o] == e.xy[0] && ba.obs_xy_[2 * o + 1] == e.xy[1]);
    CHECK(rec.images.at(e.image_id).points2D[e.point2D_idx].point3D_id == e.point3D_id);
  }
  for (size_t o = 0; o < O1; ++o) CHECK(ba.obs_point_[o] < (int32_t)P0);
  // the live handle against one created from the grown arrays: the same bits, before and after a solve
  pcd_ba* fresh = Fresh(ba, opt);
  const Evaluation a = Evaluate(live, 2 * O2 + L), b = Evaluate(fresh, 2 * O2 + L);
  CHECK(std::memcmp(&a.cost, &b.cost, sizeof a.cost) == 0 && SameBits(a.residuals, b.residuals));
  const Reconstruction before = rec;
  CHECK(ba.Solve(&rec) && ba.handle() == live);           // Solve keeps the handle the addition left
  CHECK(ba.Summary().final_cost < ba.Summary().initial_cost);
  pcd_ba_solve_opts so;
  pcd_ba_solve_opts_default(&so);
  so.max_num_iterations = opt.max_num_iterations;
  so.function_tolerance = opt.function_tolerance;
  so.gradient_tolerance = opt.gradient_tolerance;
  so.linear.max_iterations = opt.max_linear_solver_iterations;
  so.linear_solver = ba.UsesDirectSolver() ? PCD_LINEAR_CHOLESKY : PCD_LINEAR_PCG;
  pcd_ba_solve_summary sm{};
  CHECK(pcd_ba_solve(fresh, &so, &sm, nullptr) == PCD_OK);
  CHECK(sm.initial_cost == ba.Summary().initial_cost && sm.final_cost == ba.Summary().final_cost);
  CHECK(sm.num_iterations == ba.Summary().num_iterations);
  std::vector<double> poses(7 * ba.image_ids_.size()), points(3 * P2);
  CHECK(pcd_ba_get_parameters(fresh, poses.data(), points.data()) == PCD_OK);
  CHECK(SameBits(poses, ba.poses_) && SameBits(points, ba.points_));
  pcd_ba_destroy(fresh);
  // the write-back reaches the new points; the dead rows of the merged pair are not written anywhere
  for (const point3D_t id : {kRetri, kMerged, (point3D_t)1}) {
    const size_t p = std::find(ba.point_ids_.begin(), ba.point_ids_.end(), id) - ba.point_ids_.begin();
    CHECK(std::memcmp(rec.points3D.at(id).xyz, &ba.points_[3 * p], 3 * sizeof(double)) == 0);
    CHECK(std::memcmp(rec.points3D.at(id).xyz, before.points3D.at(id).xyz, 3 * sizeof(double)) != 0);
  }
  CHECK(rec.points3D.count(kMergeA) == 0 && rec.points3D.count(kMergeB) == 0);
  // and the filter keeps the completed and the new tracks
  const size_t again = ba.FilterPoints(8.0, 1.5, false, &erased, &deleted, &ok);
  CHECK(ok && again == 0 && erased.empty() && deleted.empty());
  std::printf("AddObservations: %zu rows, 2 points; cost %.6g -> %.6g\n", elements.size(), ba.Summary().initial_cost,
              ba.Summary().final_cost);
}

int main(int argc, char** argv) {
  TestRefusalsAndBookkeeping();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) {
    if (pcd_device_count() < 1) { std::printf("FAIL: --gpu given but no gfx950 device\n"); return 1; }
    TestAdd();
  }
  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

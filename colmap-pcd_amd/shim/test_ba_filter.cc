// test_ba_filter.cc -- BundleAdjusterHip::FilterPoints (ba_problem.h): Reconstruction::FilterPoints3D on the live handle,
// applied on the device, behind the reference's bookkeeping.
//   ./test_ba_filter          the refusals that need no GPU
//   ./test_ba_filter --gpu    filter, apply, compare with a fresh handle, solve on (fails if no gfx950 device)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

#include "ba_problem.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

constexpr size_t kImages = 4, kNear = 120, kFar = 6;   // points 1 .. kNear around the origin, then kFar points 600 m away
constexpr double kF = 1200.0;

// the shape of test_ba_solve.cc's GenerateReconstruction (every image observes every point, identity rotations, t =
// (U(-1,1), U(-1,1), 10), +-1 px noise) with one camera; the far points subtend ~0.2 degrees from any two images; every 10th
// near point has its observation in image (p % kImages) moved by 60 px
static void GenerateReconstruction(Reconstruction* rec, std::set<std::pair<image_t, point2D_t>>* moved) {
  std::mt19937 rng(0);
  std::uniform_real_distribution<double> u(-1.0, 1.0), px(-1.0, 1.0);
  for (point3D_t p = 1; p <= kNear + kFar; ++p) {
    Point3D pt;
    for (double& c : pt.xyz) c = u(rng);
    if (p > kNear) pt.xyz[2] += 600.0;
    rec->points3D[p] = pt;
  }
  Camera cam;
  cam.model_id = PCD_CAM_SIMPLE_RADIAL;
  cam.params = {kF, 500.0, 500.0, 0.0};
  rec->cameras[0] = cam;
  for (image_t i = 0; i < kImages; ++i) {
    Image im;
    im.camera_id = 0;
    im.tvec[0] = u(rng); im.tvec[1] = u(rng); im.tvec[2] = 10;
    for (point3D_t p = 1; p <= kNear + kFar; ++p) {
      const Point3D& pt = rec->points3D[p];
      const double X = pt.xyz[0] + im.tvec[0], Y = pt.xyz[1] + im.tvec[1], Z = pt.xyz[2] + im.tvec[2];
      Point2D p2;
      p2.xy[0] = kF * X / Z + 500.0 + px(rng);
      p2.xy[1] = kF * Y / Z + 500.0 + px(rng);
      if (p <= kNear && p % 10 == 0 && p % kImages == i) {
        p2.xy[0] += 60.0;
        moved->insert({i, (point2D_t)(p - 1)});
      }
      p2.point3D_id = p;
      im.points2D.push_back(p2);
      rec->points3D[p].track.push_back({i, (point2D_t)(p - 1)});
    }
    rec->images[i] = im;
  }
}

static void TestRefusals() {
  pcd_ba_filter_opts fo;
  std::memset(&fo, 0xFF, sizeof fo);
  pcd_ba_filter_opts_default(&fo);
  CHECK(fo.max_reproj_error == 8.0 && fo.min_tri_angle_deg == 1.5 && fo.reserved[0] == 0 && fo.reserved[7] == 0);
  pcd_ba_filter_out out{};
  CHECK(pcd_ba_filter_points_device(nullptr, &fo, &out, nullptr) == PCD_ERR_INVALID);
  CHECK(pcd_ba_filter_points(nullptr, &fo, &out) == PCD_ERR_INVALID);
  pcd_ba_remove_info info;
  std::memset(&info, 0xFF, sizeof info);
  CHECK(pcd_ba_remove_observations_device(nullptr, nullptr, nullptr, nullptr, nullptr, &info) == PCD_ERR_INVALID);
  CHECK(info.num_obs == 0 && info.num_obs_removed == 0);
  // no live handle: FilterPoints says so and touches nothing
  Reconstruction rec;
  std::set<std::pair<image_t, point2D_t>> moved;
  GenerateReconstruction(&rec, &moved);
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < kImages; ++i) config.AddImage(i);
  BundleAdjusterHip ba(BundleAdjustmentOptions(), config);
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(ba.obs_point2D_.size() == ba.obs_image_.size() && ba.obs_image_.size() == kImages * (kNear + kFar));
  for (size_t o = 0; o < ba.obs_image_.size(); ++o)     // an observation's point2D index leads back to its point
    CHECK(rec.images.at(ba.image_ids_[ba.obs_image_[o]]).points2D[ba.obs_point2D_[o]].point3D_id == ba.point_ids_[ba.obs_point_[o]]);
  bool ok = true;
  std::vector<std::pair<image_t, point2D_t>> erased(3);
  std::vector<point3D_t> deleted(3);
  const size_t residuals = ba.NumResiduals();
  CHECK(ba.FilterPoints(8.0, 1.5, true, &erased, &deleted, &ok) == 0 && !ok && erased.empty() && deleted.empty());
  CHECK(ba.NumResiduals() == residuals);
}

static double Cost(BundleAdjusterHip& ba) {
  double c = -1.0;
  pcd_ba_out o{};
  o.cost = &c;
  CHECK(pcd_ba_evaluate(ba.handle(), &o) == PCD_OK);
  return c;
}

// what the caller does with FilterPoints' lists: Reconstruction::DeleteObservation / DeletePoint3D (base/reconstruction.cc)
static void ApplyToReconstruction(Reconstruction* rec, const std::vector<std::pair<image_t, point2D_t>>& erased,
                                  const std::vector<point3D_t>& deleted) {
  for (const auto& e : erased) {
    Point2D& p2 = rec->images.at(e.first).points2D.at(e.second);
    std::vector<TrackElement>& track = rec->points3D.at(p2.point3D_id).track;
    for (size_t k = 0; k < track.size(); ++k)
      if (track[k].image_id == e.first && track[k].point2D_idx == e.second) { track.erase(track.begin() + k); break; }
    p2.point3D_id = kInvalidPoint3DId;
  }
  for (const point3D_t id : deleted) {
    for (const TrackElement& te : rec->points3D.at(id).track)
      rec->images.at(te.image_id).points2D.at(te.point2D_idx).point3D_id = kInvalidPoint3DId;
    rec->points3D.erase(id);
  }
}

// after a Solve: every point left in the Reconstruction that has a residual block holds the handle's coordinates
static size_t CheckWrittenBack(BundleAdjusterHip& ba, const Reconstruction& rec, const Reconstruction& before) {
  std::vector<double> poses(7 * ba.image_ids_.size()), points(3 * ba.point_ids_.size());
  CHECK(pcd_ba_get_parameters(ba.handle(), poses.data(), points.data()) == PCD_OK);
  std::vector<uint8_t> has_block(ba.point_ids_.size(), 0);
  for (int p : ba.obs_point_) has_block[p] = 1;
  size_t moved = 0;
  for (size_t p = 0; p < ba.point_ids_.size(); ++p) {
    auto it = rec.points3D.find(ba.point_ids_[p]);
    if (it == rec.points3D.end()) { CHECK(!has_block[p]); continue; }
    CHECK(has_block[p]);
    CHECK(std::memcmp(it->second.xyz, &points[3 * p], 3 * sizeof(double)) == 0);
    moved += std::memcmp(it->second.xyz, before.points3D.at(ba.point_ids_[p]).xyz, 3 * sizeof(double)) != 0;
  }
  return moved;
}

static void TestFilter() {
  Reconstruction rec;
  std::set<std::pair<image_t, point2D_t>> moved;
  GenerateReconstruction(&rec, &moved);
  CHECK(moved.size() == kNear / 10);
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < kImages; ++i) config.AddImage(i);
  config.SetConstantPose(0);
  config.SetConstantTvec(1, {0});
  for (point3D_t p = 2; p <= kNear + kFar; p += 17) {   // LiDAR terms on 8 points, the last of them far point kNear + 1 (= 121)
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
  const size_t O = ba.obs_image_.size(), L = ba.lidar_point_.size();
  CHECK(O == kImages * (kNear + kFar) && L == 8);
  CHECK(ba.Create());
  // look, do not touch
  bool ok = false;
  std::vector<std::pair<image_t, point2D_t>> erased;
  std::vector<point3D_t> deleted;
  const size_t nf = ba.FilterPoints(8.0, 1.5, false, &erased, &deleted, &ok);
  CHECK(ok && ba.NumResiduals() == 2 * O + L);
  using PairSet = std::set<std::pair<image_t, point2D_t>>;
  CHECK(PairSet(erased.begin(), erased.end()) == moved);
  CHECK(deleted.size() == kFar);
  for (size_t k = 0; k < deleted.size(); ++k) CHECK(deleted[k] == kNear + 1 + k);
  CHECK(nf == erased.size() + deleted.size());          // elements for the first filter, one per point for the second
  std::vector<std::pair<image_t, point2D_t>> e0;
  CHECK(ba.FilterPoints(8.0, 0.0, false, &e0, &deleted, &ok) == moved.size() && ok && deleted.empty() && e0 == erased);
  // apply: the handle and the flat arrays lose the same rows
  std::vector<std::pair<image_t, point2D_t>> erased2;
  CHECK(ba.FilterPoints(8.0, 1.5, true, &erased2, &deleted, &ok) == nf && ok && erased2 == erased && deleted.size() == kFar);
  const std::vector<point3D_t> deleted2 = deleted;
  const size_t O2 = O - moved.size() - kImages * kFar;
  CHECK(ba.obs_image_.size() == O2 && ba.obs_xy_.size() == 2 * O2 && ba.obs_point2D_.size() == O2);
  CHECK(ba.lidar_point_.size() == L - 1 && ba.config().lidar_maps_.count(kNear + 1) == 0);
  CHECK(ba.NumResiduals() == 2 * O2 + L - 1);
  uint64_t terms = 0;
  CHECK(pcd_ba_get_lidar(ba.handle(), &terms, nullptr, nullptr, nullptr, nullptr, nullptr) == PCD_OK && terms == L - 1);
  for (size_t o = 0; o < O2; ++o) {
    CHECK(moved.count(std::make_pair(ba.image_ids_[ba.obs_image_[o]], ba.obs_point2D_[o])) == 0);
    CHECK(ba.point_ids_[ba.obs_point_[o]] <= kNear);
  }
  // the live handle against one created from the compacted arrays: the same bits
  pcd_ba* live = ba.handle();
  const double cost_live = Cost(ba);
  std::vector<double> res_live(2 * O2 + L - 1), res_fresh(2 * O2 + L - 1);
  pcd_ba_out o{};
  o.residuals = res_live.data();
  CHECK(pcd_ba_evaluate(live, &o) == PCD_OK);
  CHECK(ba.FilterPoints(8.0, 1.5, false, &erased, &deleted, &ok) == 0 && ok && erased.empty() && deleted.empty());
  CHECK(ba.Create());
  const double cost_fresh = Cost(ba);
  o.residuals = res_fresh.data();
  CHECK(pcd_ba_evaluate(ba.handle(), &o) == PCD_OK);
  CHECK(std::memcmp(&cost_live, &cost_fresh, sizeof cost_live) == 0);
  CHECK(std::memcmp(res_live.data(), res_fresh.data(), res_live.size() * sizeof(double)) == 0);
  // the caller applies the lists: the deleted points leave the Reconstruction but stay in point_ids_
  ApplyToReconstruction(&rec, erased2, deleted2);
  CHECK(rec.points3D.size() == kNear && rec.points3D.count(kNear + 1) == 0);
  // adjust, filter, adjust: Solve after an applied filter writes the surviving points only; the second FilterPoints
  // applies on the handle Solve left, and Solve keeps it
  const Reconstruction before = rec;
  CHECK(ba.Solve(&rec));
  const double first = ba.Summary().final_cost;
  CHECK(ba.Summary().final_cost < ba.Summary().initial_cost);
  CHECK(rec.points3D.size() == kNear && CheckWrittenBack(ba, rec, before) == kNear);   // every survivor moved, nothing came back
  pcd_ba* solved = ba.handle();
  const size_t again = ba.FilterPoints(8.0, 1.5, true, &erased, &deleted, &ok);
  CHECK(ok && again == erased.size() + deleted.size());
  ApplyToReconstruction(&rec, erased, deleted);
  CHECK(ba.Solve(&rec) && ba.handle() == solved);
  CHECK(ba.Summary().initial_cost <= first * (1 + 1e-12));
  CheckWrittenBack(ba, rec, before);
  CHECK(rec.points3D.size() == kNear - deleted.size());
  std::printf("FilterPoints: %zu filtered (%zu elements, %zu points), then %zu; cost %.6g -> %.6g\n", nf, moved.size(), kFar,
              again, first, ba.Summary().final_cost);
}

int main(int argc, char** argv) {
  TestRefusals();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) {
    if (pcd_device_count() < 1) { std::printf("FAIL: --gpu given but no gfx950 device\n"); return 1; }
    TestFilter();
  }
  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

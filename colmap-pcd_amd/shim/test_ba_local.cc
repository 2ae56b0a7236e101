// test_ba_local.cc -- BundleAdjusterHip::LocalRound (ba_problem.h): one IncrementalMapper::AdjustLocalBundle on the live
// whole-map handle -- FindLocalBundle and the local sub-problem derived on the device -- against FindLocalBundle restated
// here on the Reconstruction and the counts of the sub-problem worked out from it.
//   ./test_ba_local          the refusals that need no GPU, and the host selection of the mock scene
//   ./test_ba_local --gpu    the round on the device (fails if no gfx950 device)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>

#include "ba_problem.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// The scene of test_ba_window.cc: six images in two groups 3 m apart (centres near x = 0, 0.2, 0.4 and 3, 3.2, 3.4,
// identity rotations, looking along z from z = -10).  Points 1 .. kNear are seen by images 0-3, the kFar others by 3-5.
constexpr size_t kImages = 6, kNear = 100, kFar = 50;
constexpr double kF = 1200.0;

static void GenerateReconstruction(Reconstruction* rec) {
  std::mt19937 rng(0);
  std::uniform_real_distribution<double> u(-1.0, 1.0), px(-1.0, 1.0);
  for (point3D_t p = 1; p <= kNear + kFar; ++p) {
    Point3D pt;
    for (double& c : pt.xyz) c = u(rng);
    if (p > kNear) pt.xyz[0] += 3.2;
    rec->points3D[p] = pt;
  }
  Camera cam;
  cam.model_id = PCD_CAM_SIMPLE_RADIAL;
  cam.params = {kF, 500.0, 500.0, 0.0};
  rec->cameras[0] = cam;
  for (image_t i = 0; i < kImages; ++i) {
    Image im;
    im.camera_id = 0;
    const double cx = (i < 3 ? 0.0 : 3.0) + 0.2 * (i % 3);
    im.tvec[0] = -cx; im.tvec[1] = 0.1 * u(rng); im.tvec[2] = 10;
    for (point3D_t p = 1; p <= kNear + kFar; ++p) {
      const bool sees = p <= kNear ? i <= 3 : i >= 3;
      if (!sees) continue;
      const Point3D& pt = rec->points3D[p];
      const double X = pt.xyz[0] + im.tvec[0], Y = pt.xyz[1] + im.tvec[1], Z = pt.xyz[2] + im.tvec[2];
      Point2D p2;
      p2.xy[0] = kF * X / Z + 500.0 + px(rng);
      p2.xy[1] = kF * Y / Z + 500.0 + px(rng);
      p2.point3D_id = p;
      rec->points3D[p].track.push_back({i, (point2D_t)im.points2D.size()});
      im.points2D.push_back(p2);
    }
    rec->images[i] = im;
  }
}

// the planes of test_ba_reassoc.cc: y = 1.05 (ground) and z = 1.05, 3 cm spacing over [-1.2, 1.2]^2, as a raw scan
static void Planes(std::vector<float>* xyz, std::vector<float>* nrm) {
  const double n2[3] = {0.05, 0.02, -1.0};
  const double l2 = std::sqrt(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2]);
  auto push = [&](double x, double y, double z, double nx, double ny, double nz) {
    xyz->push_back((float)z); xyz->push_back((float)-x); xyz->push_back((float)-y);
    nrm->push_back((float)nz); nrm->push_back((float)-nx); nrm->push_back((float)-ny);
  };
  for (int i = 0; i <= 80; ++i)
    for (int j = 0; j <= 80; ++j) {
      const double a = -1.2 + 0.03 * i, b = -1.2 + 0.03 * j;
      push(a, 1.05, b, 0.0, -1.0, 0.0);
      push(a, b, 1.05, n2[0] / l2, n2[1] / l2, n2[2] / l2);
    }
}

// sfm/incremental_mapper.cc:1747-1914 on the Reconstruction (identity rotations: the projection centre is -tvec); ties in
// the shared count go to the lower image id, the library's choice
static std::vector<image_t> FindLocalBundleOnHost(const Reconstruction& rec, image_t image_id, int num_images, double min_deg) {
  const Image& image = rec.images.at(image_id);
  std::map<image_t, size_t> shared;
  std::vector<const double*> X;
  for (const Point2D& p2 : image.points2D) {
    if (!p2.HasPoint3D()) continue;
    X.push_back(rec.points3D.at(p2.point3D_id).xyz);
    for (const auto& el : rec.points3D.at(p2.point3D_id).track)
      if (el.image_id != image_id) shared[el.image_id] += 1;
  }
  std::vector<std::pair<image_t, size_t>> cand(shared.begin(), shared.end());
  std::stable_sort(cand.begin(), cand.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
  const size_t eff = std::min<size_t>(num_images - 1, cand.size()), n = X.size();
  std::vector<image_t> out;
  if (cand.size() == eff) {
    for (const auto& c : cand) out.push_back(c.first);
    return out;
  }
  auto percentile = [&](image_t j) {
    const Image& other = rec.images.at(j);
    std::vector<double> a;
    for (const double* x : X) {
      double base2 = 0, r1 = 0, r2 = 0;
      for (int k = 0; k < 3; ++k) {
        const double c1 = -image.tvec[k], c2 = -other.tvec[k];
        base2 += (c1 - c2) * (c1 - c2); r1 += (x[k] - c1) * (x[k] - c1); r2 += (x[k] - c2) * (x[k] - c2);
      }
      const double den = 2.0 * std::sqrt(r1 * r2);
      const double ang = den == 0.0 ? 0.0 : std::abs(std::acos((r1 + r2 - base2) / den));
      a.push_back(std::min(ang, M_PI - ang));
    }
    std::sort(a.begin(), a.end());
    return a[std::min<size_t>(n - 1, (size_t)std::round(0.75 * (double)(n - 1)))];
  };
  const double m = min_deg * 0.0174532925199432954743716805978692718781530857086181640625;
  const double div[8] = {1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0}, frac[8] = {0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1};
  std::vector<double> tri(cand.size(), -1.0);
  std::vector<char> used(cand.size(), 0);
  for (int k = 0; k < 8 && out.size() < eff; ++k)
    for (size_t c = 0; c < cand.size() && out.size() < eff; ++c) {
      if ((double)cand[c].second < frac[k] * (double)n) break;
      if (used[c]) continue;
      if (tri[c] < 0.0) tri[c] = percentile(cand[c].first);
      if (tri[c] >= m / div[k]) { out.push_back(cand[c].first); used[c] = 1; }
    }
  for (size_t c = 0; c < cand.size() && out.size() < eff; ++c)
    if (!used[c]) { out.push_back(cand[c].first); used[c] = 1; }
  return out;
}

static BundleAdjustmentConfig WholeMap() {
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < kImages; ++i) config.AddImage(i);
  config.SetConstantPose(0);
  for (point3D_t p = 1; p <= kNear + kFar; ++p) config.AddVariablePoint(p);
  return config;
}

static void TestRefusals() {
  pcd_ba_local_bundle_opts bo;
  std::memset(&bo, 0xFF, sizeof bo);
  pcd_ba_local_bundle_opts_default(&bo);
  CHECK(bo.image == -1 && bo.num_images == 6 && bo.min_tri_angle_deg == 6.0 && bo.reserved[7] == 0);
  pcd_ba_local_window_opts wo;
  std::memset(&wo, 0xFF, sizeof wo);
  pcd_ba_local_window_opts_default(&wo);
  CHECK(!wo.d_image_set && !wo.d_point_variable && wo.image == -1 && wo.max_track_length == 1000 && !wo.d_extra_const_pose);
  int32_t out[8];
  uint8_t set[8];
  CHECK(pcd_ba_local_bundle_device(nullptr, &bo, out, out, set, nullptr, nullptr, nullptr) == PCD_ERR_INVALID);
  CHECK(pcd_ba_local_bundle(nullptr, &bo, out, out, nullptr, nullptr) == PCD_ERR_INVALID);
  pcd_ba* w = reinterpret_cast<pcd_ba*>(1);
  pcd_ba_local_window_info info;
  std::memset(&info, 0xFF, sizeof info);
  CHECK(pcd_ba_local_window_create_device(nullptr, &wo, nullptr, nullptr, nullptr, &w, &info) == PCD_ERR_INVALID);
  CHECK(w == nullptr && info.num_obs == 0 && info.num_points_fixed == 0);
  // the host selection of the mock scene.  Image 1 shares its 100 rows with images 0, 2 and 3 alike: three candidates.
  // Room for three: the copy path, in index order.  Room for two: image 3, 2.8 m away, has the angle of the first pass;
  // images 0 and 2, 0.2 m away at a depth of 10 m, see about 0.02 rad and wait for a late pass, image 0 first
  Reconstruction rec;
  GenerateReconstruction(&rec);
  CHECK(FindLocalBundleOnHost(rec, 1, 6, 6.0) == std::vector<image_t>({0, 2, 3}));
  CHECK(FindLocalBundleOnHost(rec, 1, 4, 6.0) == std::vector<image_t>({0, 2, 3}));
  CHECK(FindLocalBundleOnHost(rec, 1, 3, 6.0) == std::vector<image_t>({3, 0}));
  CHECK(FindLocalBundleOnHost(rec, 1, 2, 6.0) == std::vector<image_t>({3}));
  CHECK(FindLocalBundleOnHost(rec, 5, 6, 6.0) == std::vector<image_t>({3, 4}));
  // no live handle: LocalRound says so and touches nothing
  BundleAdjusterHip ba(BundleAdjustmentOptions(), WholeMap());
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  struct NoCloud { pcd_cloud* handle() const { return nullptr; } } none;
  const Reconstruction before = rec;
  BundleAdjusterHip::LocalRoundInfo li;
  li.bundle.push_back(7);
  CHECK(!ba.LocalRound(&rec, none, 1, 6, 6.0, 1000, 1.5, 0.2, 0.1, &li));
  CHECK(li.bundle.empty() && li.window.num_obs == 0 && li.solve.num_iterations == 0);
  for (const auto& kv : before.points3D)
    CHECK(std::memcmp(rec.points3D.at(kv.first).xyz, kv.second.xyz, sizeof kv.second.xyz) == 0);
}

static void TestLocalRound() {
  Reconstruction rec;
  GenerateReconstruction(&rec);
  std::mt19937 rng(7);
  std::normal_distribution<double> n(0.0, 0.02);
  for (auto& kv : rec.points3D)
    for (double& c : kv.second.xyz) c += n(rng);
  const Reconstruction start = rec;
  BundleAdjustmentOptions opt;
  opt.max_num_iterations = 8;
  opt.linear_solver_type = BundleAdjustmentOptions::LinearSolverType::DIRECT;
  std::vector<float> cxyz, cnrm;
  Planes(&cxyz, &cnrm);
  lidar::PointCloudProcess pcp;
  CHECK(pcp.InitializeFromRawCloud(cxyz.data(), cnrm.data(), cxyz.size() / 3));
  BundleAdjusterHip ba(opt, WholeMap());
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(!ba.LocalRound(&rec, pcp, 1));                   // no live handle yet
  CHECK(ba.Create());
  pcd_ba* live = ba.handle();
  CHECK(!ba.LocalRound(&rec, pcp, 77));                  // an image the problem does not have
  CHECK(!ba.LocalRound(&rec, pcp, 1, 1));                // num_images below 2
  const std::vector<image_t> expect = FindLocalBundleOnHost(start, 1, 3, 6.0);
  CHECK(expect == std::vector<image_t>({3, 0}));
  BundleAdjusterHip::LocalRoundInfo li;
  CHECK(ba.LocalRound(&rec, pcp, 1, 3, 6.0, 1000, 1.5, 0.2, 0.1, &li));
  CHECK(li.bundle == expect);
  CHECK(ba.handle() == live && ba.NumResiduals() == 2 * (4 * kNear + 3 * kFar));   // the live handle keeps its rows
  // images 0, 1, 3 are in.  The near points are variable and keep their four rows, the one on image 2 as a constant-pose
  // block; the far points are not variable, keep their row on image 3 alone and become constant
  CHECK(li.window.num_images_in == 3 && li.window.num_points_variable == kNear && li.window.num_points_fixed == kFar);
  CHECK(li.window.num_obs == 4 * kNear + kFar && li.window.num_lidar == 0);
  CHECK(li.window.num_pose_rows == 2 * kNear + kFar);    // images 1 and 3: image 0 is constant, image 2 is outside
  CHECK(li.assoc.num_queries == kNear && li.assoc.num_terms > 0);
  CHECK(li.solve.num_accepted >= 1 && li.solve.final_cost < li.solve.initial_cost);
  size_t moved_near = 0, moved_far = 0;
  for (const auto& kv : start.points3D) {
    const Point3D& now = rec.points3D.at(kv.first);
    (kv.first <= kNear ? moved_near : moved_far) += std::memcmp(now.xyz, kv.second.xyz, sizeof now.xyz) != 0;
    CHECK(now.global_opt_num == kv.second.global_opt_num);
  }
  CHECK(moved_near == kNear && moved_far == 0);
  for (image_t i = 0; i < kImages; ++i) {
    const bool moved = std::memcmp(rec.images.at(i).tvec, start.images.at(i).tvec, sizeof start.images.at(i).tvec) != 0;
    CHECK(moved == (i == 1 || i == 3));
  }
  std::vector<double> poses(7 * kImages), points(3 * (kNear + kFar));
  CHECK(pcd_ba_get_parameters(live, poses.data(), points.data()) == PCD_OK);
  CHECK(poses == ba.poses_ && points == ba.points_);     // the commit reached the live handle, the mirrors follow it
  std::printf("LocalRound: bundle of %zu, %llu points variable, %llu fixed, %llu terms, cost %.6g -> %.6g\n", li.bundle.size(),
              (unsigned long long)li.window.num_points_variable, (unsigned long long)li.window.num_points_fixed,
              (unsigned long long)li.assoc.num_terms, li.solve.initial_cost, li.solve.final_cost);
  // a second round on the same handle, the copy path: image 5 shares rows with 3 and 4 alone
  CHECK(ba.LocalRound(&rec, pcp, 5, 6, 6.0, 1000, 1.5, 0.2, 0.1, &li));
  CHECK(ba.handle() == live && li.bundle == std::vector<image_t>({3, 4}) && li.window.num_points_variable == kFar);
  CHECK(li.window.num_points_fixed == kNear && li.window.num_obs == 3 * kFar + kNear);
}

int main(int argc, char** argv) {
  TestRefusals();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) {
    if (pcd_device_count() < 1) { std::printf("FAIL: --gpu given but no gfx950 device\n"); return 1; }
    TestLocalRound();
  }
  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

// test_ba_window.cc -- BundleAdjusterHip::GlobalRound (ba_problem.h): one IncrementalMapper::AdjustGlobalBundleByLidar on
// the live whole-map handle through the sphere window derived on the device, against the host route: the same selection
// restated here, SetUpGlobalByLidar's assembly (if_in_sphere) and a fresh handle.
//   ./test_ba_window          the refusals that need no GPU, and the host selection of the mock scene
//   ./test_ba_window --gpu    the round on the device against the host route (fails if no gfx950 device)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

#include "ba_problem.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// Six images in two groups, 3 m apart: centres near x = 0, 0.2, 0.4 and x = 3, 3.2, 3.4 (identity rotations, looking
// along z from z = -10).  Points 1 .. kNear lie around the origin and are seen by images 0-2 AND by image 3; points
// kNear + 1 .. kNear + kFar lie around x = 3.2 and are seen by images 3-5 alone.  +-1 px noise, one camera.
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

// sfm/incremental_mapper.cc:1349-1408 on the Reconstruction: the images within `radius` of the centre image (Eigen's
// toRotationMatrix on the stored quaternion) and the points they see
static void SelectOnHost(const Reconstruction& rec, image_t center, double radius, std::set<image_t>* in, std::set<point3D_t>* active) {
  auto centre = [](const Image& im, double c[3]) {
    const double w = im.qvec[0], x = im.qvec[1], y = im.qvec[2], z = im.qvec[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx},
                            {txz - twy, tyz + twx, 1 - (txx + tyy)}};
    for (int k = 0; k < 3; ++k) c[k] = -((R[0][k] * im.tvec[0] + R[1][k] * im.tvec[1]) + R[2][k] * im.tvec[2]);
  };
  double cc[3];
  centre(rec.images.at(center), cc);
  for (const auto& kv : rec.images) {
    double c[3];
    centre(kv.second, c);
    const double dx = cc[0] - c[0], dy = cc[1] - c[1], dz = cc[2] - c[2];
    if (std::sqrt((dx * dx + dy * dy) + dz * dz) <= radius) in->insert(kv.first);
  }
  for (image_t i : *in)
    for (const Point2D& p2 : rec.images.at(i).points2D)
      if (p2.HasPoint3D()) active->insert(p2.point3D_id);
}

static BundleAdjustmentConfig WholeMap() {
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < kImages; ++i) config.AddImage(i);
  config.SetConstantPose(0);
  for (point3D_t p = 1; p <= kNear + kFar; ++p) config.AddVariablePoint(p);
  return config;
}

static void TestRefusals() {
  pcd_ba_window_opts wo;
  std::memset(&wo, 0xFF, sizeof wo);
  pcd_ba_window_opts_default(&wo);
  CHECK(wo.center_image == -1 && wo.radius == 40.0 && !wo.d_image_set && !wo.d_extra_const_pose && wo.reserved[7] == 0);
  pcd_ba* w = reinterpret_cast<pcd_ba*>(1);
  pcd_ba_window_info info;
  std::memset(&info, 0xFF, sizeof info);
  CHECK(pcd_ba_window_create_device(nullptr, &wo, nullptr, nullptr, nullptr, nullptr, &w, &info) == PCD_ERR_INVALID);
  CHECK(w == nullptr && info.num_obs == 0 && info.num_images_in == 0);
  CHECK(pcd_ba_window_commit_device(nullptr, nullptr, nullptr) == PCD_ERR_INVALID);
  // the host selection of the mock scene: a sphere of 1 m around image 1 holds the first group
  Reconstruction rec;
  GenerateReconstruction(&rec);
  std::set<image_t> in;
  std::set<point3D_t> active;
  SelectOnHost(rec, 1, 1.0, &in, &active);
  CHECK(in == std::set<image_t>({0, 1, 2}) && active.size() == kNear && *active.rbegin() == kNear);
  // no live handle: GlobalRound says so and touches nothing
  BundleAdjusterHip ba(BundleAdjustmentOptions(), WholeMap());
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(ba.obs_image_.size() == 4 * kNear + 3 * kFar);
  struct NoCloud { pcd_cloud* handle() const { return nullptr; } } none;
  const Reconstruction before = rec;
  BundleAdjusterHip::GlobalRoundInfo gi;
  std::memset(&gi, 0xFF, sizeof gi);
  CHECK(!ba.GlobalRound(&rec, none, 1, 1.0, 1.5, 0.2, 0.1, &gi));
  CHECK(gi.window.num_obs == 0 && gi.solve.num_iterations == 0);
  for (const auto& kv : before.points3D) {
    CHECK(rec.points3D.at(kv.first).global_opt_num == 0);
    CHECK(std::memcmp(rec.points3D.at(kv.first).xyz, kv.second.xyz, sizeof kv.second.xyz) == 0);
  }
}

static void TestGlobalRound() {
  Reconstruction rec;
  GenerateReconstruction(&rec);
  std::mt19937 rng(7);
  std::normal_distribution<double> n(0.0, 0.02);
  for (auto& kv : rec.points3D)
    for (double& c : kv.second.xyz) c += n(rng);
  for (point3D_t p = 1; p <= kNear; p += 2) rec.points3D[p].global_opt_num = 9;   // 1.5 - 0.9 = 0.6 m; the others 1.5 m
  const Reconstruction start = rec;
  BundleAdjustmentOptions opt;
  opt.max_num_iterations = 8;
  opt.linear_solver_type = BundleAdjustmentOptions::LinearSolverType::DIRECT;
  std::vector<float> cxyz, cnrm;
  Planes(&cxyz, &cnrm);
  lidar::PointCloudProcess pcp;
  CHECK(pcp.InitializeFromRawCloud(cxyz.data(), cnrm.data(), cxyz.size() / 3));

  // the device route: the whole map lives in one handle; the round derives its window from it
  BundleAdjusterHip ba(opt, WholeMap());
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(!ba.GlobalRound(&rec, pcp, 1, 1.0));             // no live handle yet
  CHECK(ba.Create());
  pcd_ba* live = ba.handle();
  CHECK(!ba.GlobalRound(&rec, pcp, 77, 1.0));            // an image the problem does not have
  BundleAdjusterHip::GlobalRoundInfo gi;
  std::unordered_map<point3D_t, LidarPoint> terms;
  CHECK(ba.GlobalRound(&rec, pcp, 1, 1.0, 1.5, 0.2, 0.1, &gi, &terms));
  CHECK(ba.handle() == live && ba.NumResiduals() == 2 * (4 * kNear + 3 * kFar));   // the live handle keeps its rows
  CHECK(gi.window.num_images_in == 3 && gi.window.num_points_active == kNear && gi.window.num_obs == 4 * kNear);
  CHECK(gi.window.num_pose_rows == 2 * kNear);           // images 1 and 2: image 0 is constant, image 3 is outside
  CHECK(gi.assoc.num_queries == kNear && gi.assoc.num_terms > 0 && gi.assoc.num_terms == terms.size());
  CHECK(gi.solve.num_accepted >= 1 && gi.solve.final_cost < gi.solve.initial_cost);
  size_t moved_in = 0, moved_out = 0;
  for (const auto& kv : start.points3D) {
    const Point3D& now = rec.points3D.at(kv.first);
    const bool moved = std::memcmp(now.xyz, kv.second.xyz, sizeof now.xyz) != 0;
    (kv.first <= kNear ? moved_in : moved_out) += moved;
    CHECK(now.global_opt_num == kv.second.global_opt_num + (kv.first <= kNear ? 1 : 0));
  }
  CHECK(moved_in == kNear && moved_out == 0);
  for (image_t i = 0; i < kImages; ++i) {
    const bool moved = std::memcmp(rec.images.at(i).tvec, start.images.at(i).tvec, sizeof start.images.at(i).tvec) != 0;
    CHECK(moved == (i == 1 || i == 2));
  }
  std::vector<double> poses(7 * kImages), points(3 * (kNear + kFar));
  CHECK(pcd_ba_get_parameters(live, poses.data(), points.data()) == PCD_OK);
  CHECK(poses == ba.poses_ && points == ba.points_);     // the commit reached the live handle, the mirrors follow it

  // the host route: select on the Reconstruction as it was, assemble with SetUpGlobalByLidar's rule, a fresh handle
  Reconstruction host = start;
  std::set<image_t> in;
  std::set<point3D_t> active;
  SelectOnHost(host, 1, 1.0, &in, &active);
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < kImages; ++i) {
    config.AddImage(i);
    if (!in.count(i)) config.SetConstantPose(i);
  }
  config.SetConstantPose(0);
  for (point3D_t p : active) { config.AddVariablePoint(p); host.points3D.at(p).if_in_sphere = true; }
  for (const auto& kv : terms) config.AddLidarPoint(kv.first, kv.second);
  BundleAdjusterHip hb(opt, config);
  hb.SetUp(&host, BundleAdjusterHip::OptimazePhrase::Global);
  CHECK(hb.obs_image_.size() == gi.window.num_obs && gi.window.num_lidar == 0 && hb.lidar_point_.size() == terms.size());
  CHECK(hb.NumResiduals() == 2 * gi.window.num_obs + gi.assoc.num_terms);
  CHECK(hb.Solve(&host));
  // The two problems hold the same residual blocks over differently numbered points and images, so sums run in another
  // order: costs agree to rounding (1e-12 relative: a few hundred terms of equal sign), and with the exact (Cholesky)
  // steps of both the accepted parameters agree far below the 1e-9 asked here.
  CHECK(std::fabs(hb.Summary().initial_cost - gi.solve.initial_cost) <= 1e-12 * gi.solve.initial_cost);
  CHECK(hb.Summary().num_iterations == gi.solve.num_iterations && hb.Summary().num_accepted == gi.solve.num_accepted);
  CHECK(std::fabs(hb.Summary().final_cost - gi.solve.final_cost) <= 1e-9 * gi.solve.final_cost);
  double worst = 0.0;
  for (const auto& kv : host.points3D)
    for (int k = 0; k < 3; ++k) worst = std::max(worst, std::fabs(kv.second.xyz[k] - rec.points3D.at(kv.first).xyz[k]));
  for (const auto& kv : host.images)
    for (int k = 0; k < 3; ++k) worst = std::max(worst, std::fabs(kv.second.tvec[k] - rec.images.at(kv.first).tvec[k]));
  CHECK(worst <= 1e-9);
  std::printf("GlobalRound: %llu of %zu images in, %llu points active, %llu terms, cost %.6g -> %.6g; host route differs by %.3g\n",
              (unsigned long long)gi.window.num_images_in, kImages, (unsigned long long)gi.window.num_points_active,
              (unsigned long long)gi.assoc.num_terms, gi.solve.initial_cost, gi.solve.final_cost, worst);
  // a second round around the other group on the same handle
  CHECK(ba.GlobalRound(&rec, pcp, 4, 1.0, 1.5, 0.2, 0.1, &gi));
  CHECK(ba.handle() == live && gi.window.num_images_in == 3 && gi.window.num_points_active == kNear + kFar);
  CHECK(rec.points3D.at(1).global_opt_num == start.points3D.at(1).global_opt_num + 2 && rec.points3D.at(kNear + 1).global_opt_num == 1);
}

int main(int argc, char** argv) {
  TestRefusals();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) {
    if (pcd_device_count() < 1) { std::printf("FAIL: --gpu given but no gfx950 device\n"); return 1; }
    TestGlobalRound();
  }
  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

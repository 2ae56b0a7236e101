// test_ba_solve_cam.cc -- BundleAdjusterHip::Solve with refined intrinsics on the device route
// (BundleAdjustmentOptions::refine_intrinsics_on_device, ba_problem.h; pcd_ba_solve with refine_intrinsics).
//   ./test_ba_solve_cam          what needs no GPU: with the option off a refined problem is refused as before
//   ./test_ba_solve_cam --gpu    option on: Solve equals pcd_ba_solve through the C ABI bit for bit, the camera in the
//                                Reconstruction is updated, more refined cameras than the library carries -> false
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "ba_problem.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// test_ba_solve.cc's scene with the cameras dealt out: image i on camera i % num_cameras (1: one shared camera, the usual
// dataset), every image observes every point, SIMPLE_RADIAL f = 1200 in the observations, `focal` in the Reconstruction
static void GenerateReconstruction(size_t num_images, size_t num_points, size_t num_cameras, double focal, Reconstruction* rec) {
  std::mt19937 rng(0);
  std::uniform_real_distribution<double> u(-1.0, 1.0), px(-2.0, 2.0);
  for (point3D_t p = 1; p <= num_points; ++p) {
    Point3D pt;
    for (double& c : pt.xyz) c = u(rng);
    rec->points3D[p] = pt;
  }
  for (camera_t c = 0; c < num_cameras; ++c) {
    Camera cam;
    cam.model_id = PCD_CAM_SIMPLE_RADIAL;
    cam.params = {focal, 500.0, 500.0, 0.0};
    rec->cameras[c] = cam;
  }
  for (image_t i = 0; i < num_images; ++i) {
    Image im;
    im.camera_id = (camera_t)(i % num_cameras);
    im.tvec[0] = u(rng); im.tvec[1] = u(rng); im.tvec[2] = 10;
    for (point3D_t p = 1; p <= num_points; ++p) {
      const Point3D& pt = rec->points3D[p];
      const double X = pt.xyz[0] + im.tvec[0], Y = pt.xyz[1] + im.tvec[1], Z = pt.xyz[2] + im.tvec[2];
      Point2D p2;
      p2.xy[0] = 1200.0 * X / Z + 500.0 + px(rng);
      p2.xy[1] = 1200.0 * Y / Z + 500.0 + px(rng);
      p2.point3D_id = p;
      im.points2D.push_back(p2);
      rec->points3D[p].track.push_back({i, (point2D_t)(p - 1)});
    }
    rec->images[i] = im;
  }
}

static BundleAdjustmentConfig Config(size_t num_images) {
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < num_images; ++i) config.AddImage(i);
  config.SetConstantPose(0);
  config.SetConstantTvec(1, {0});
  return config;
}

static void TestOptionOff() {
  Reconstruction rec;
  GenerateReconstruction(3, 20, 1, 1230.0, &rec);
  BundleAdjustmentOptions o;
  CHECK(!o.refine_intrinsics_on_device);           // the default: today's behaviour
  o.refine_focal_length = true;
  BundleAdjusterHip refined(o, Config(3));
  refined.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(refined.CameraVariable(0));
  CHECK(!refined.Solve(&rec));                     // intrinsics refined, option off: the Ceres route's job
  CHECK(rec.cameras.at(0).params[0] == 1230.0);
}

static void TestSolve() {
  const size_t I = 5, P = 120;
  Reconstruction rec;
  GenerateReconstruction(I, P, 1, 1230.0, &rec);   // the focal length starts 2.5 % off
  BundleAdjustmentOptions opt;
  opt.max_num_iterations = 8;
  opt.refine_focal_length = true;
  opt.refine_intrinsics_on_device = true;          // linear_solver_type stays ITERATIVE: the direct solver is taken anyway
  const Reconstruction before = rec;
  BundleAdjusterHip ba(opt, Config(I));
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(ba.Solve(&rec));
  const pcd_ba_solve_summary& sm = ba.Summary();
  const double f = rec.cameras.at(0).params[0];
  std::printf("Solve with the focal length refined: cost %.6g -> %.6g, %d iterations, %d accepted, f 1230 -> %.3f\n",
              sm.initial_cost, sm.final_cost, sm.num_iterations, sm.num_accepted, f);
  CHECK(sm.num_accepted >= 1 && sm.final_cost < sm.initial_cost);
  CHECK(f != 1230.0 && std::isfinite(f));          // the camera in the Reconstruction is updated
  for (int k = 1; k < 4; ++k) CHECK(rec.cameras.at(0).params[k] == before.cameras.at(0).params[k]);   // constant
  // the same problem through the C ABI: bit for bit what Solve wrote into the Reconstruction
  Reconstruction rec2 = before;
  BundleAdjusterHip raw(opt, Config(I));
  raw.SetUp(&rec2, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(raw.Create());
  pcd_ba_solve_opts o;
  pcd_ba_solve_opts_default(&o);
  o.max_num_iterations = opt.max_num_iterations;
  o.linear.max_iterations = opt.max_linear_solver_iterations;
  o.linear_solver = PCD_LINEAR_CHOLESKY;
  o.refine_intrinsics = 1;
  pcd_ba_solve_summary s2{};
  CHECK(pcd_ba_solve(raw.handle(), &o, &s2, nullptr) == PCD_OK);
  CHECK(s2.final_cost == sm.final_cost && s2.num_accepted == sm.num_accepted);
  std::vector<double> poses(7 * I), points(3 * P), cams(4);
  CHECK(pcd_ba_get_parameters(raw.handle(), poses.data(), points.data()) == PCD_OK);
  CHECK(pcd_ba_get_camera_parameters(raw.handle(), cams.data()) == PCD_OK);
  CHECK(std::memcmp(cams.data(), rec.cameras.at(0).params.data(), 4 * sizeof(double)) == 0);
  for (size_t i = 0; i < raw.image_ids_.size(); ++i) {
    const Image& im = rec.images.at(raw.image_ids_[i]);
    CHECK(std::memcmp(im.qvec, &poses[7 * i], 4 * sizeof(double)) == 0);
    CHECK(std::memcmp(im.tvec, &poses[7 * i + 4], 3 * sizeof(double)) == 0);
  }
  for (size_t p = 0; p < raw.point_ids_.size(); ++p)
    CHECK(std::memcmp(rec.points3D.at(raw.point_ids_[p]).xyz, &points[3 * p], 3 * sizeof(double)) == 0);
  // without the flag the C ABI refuses the refined handle as before
  o.refine_intrinsics = 0;
  CHECK(pcd_ba_solve(raw.handle(), &o, &s2, nullptr) == PCD_ERR_UNSUPPORTED);
}

static void TestTooManyCameras() {
  const size_t I = PCD_BA_MAX_CAMERA_SLOTS + 1;
  Reconstruction rec;
  GenerateReconstruction(I, 40, I, 1230.0, &rec);   // one camera per image
  BundleAdjustmentOptions opt;
  opt.refine_focal_length = true;
  opt.refine_intrinsics_on_device = true;
  const Reconstruction before = rec;
  BundleAdjusterHip ba(opt, Config(I));
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(!ba.Solve(&rec));                          // the library refuses: the caller stays on the Ceres route
  CHECK(std::strstr(pcd_last_error(), "PCD_BA_MAX_CAMERA_SLOTS") != nullptr);
  CHECK(rec.cameras.at(0).params[0] == before.cameras.at(0).params[0]);
}

int main(int argc, char** argv) {
  TestOptionOff();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) {
    if (pcd_device_count() < 1) { std::printf("FAIL: --gpu given but no gfx950 device\n"); return 1; }
    TestSolve();
    TestTooManyCameras();
  }
  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

// test_ba_solve_cam_pcg.cc -- the linear solver of BundleAdjusterHip::Solve with refined intrinsics
// (BundleAdjustmentOptions::refined_linear_solver_type, ba_problem.h; pcd_ba_solve with PCD_LINEAR_PCG_CAM).
//   ./test_ba_solve_cam_pcg          what needs no GPU: the default is DIRECT, AUTO picks by the number of images
//   ./test_ba_solve_cam_pcg --gpu    ITERATIVE: Solve equals pcd_ba_solve(PCD_LINEAR_PCG_CAM, refine_intrinsics) through the
//                                    C ABI bit for bit and the camera in the Reconstruction is updated; the default
//                                    equals the Cholesky route bit for bit
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

// the solver choice on the host: the default, and AUTO by the number of images in the config (no 1001-image solve)
static void TestSolverChoice() {
  using T = BundleAdjustmentOptions::LinearSolverType;
  Reconstruction rec;
  GenerateReconstruction(3, 20, 1, 1230.0, &rec);
  BundleAdjustmentOptions o;
  CHECK(o.refined_linear_solver_type == T::DIRECT);            // the default: today's behaviour
  o.linear_solver_type = T::ITERATIVE;
  CHECK(BundleAdjusterHip(o, Config(3)).RefinedUsesDirectSolver());   // whatever linear_solver_type says
  o.refined_linear_solver_type = T::ITERATIVE;
  o.linear_solver_type = T::DIRECT;
  CHECK(!BundleAdjusterHip(o, Config(3)).RefinedUsesDirectSolver());
  CHECK(BundleAdjusterHip(o, Config(3)).UsesDirectSolver());          // and the unrefined choice does not move
  o.refined_linear_solver_type = T::AUTO;
  CHECK(BundleAdjusterHip(o, Config(BundleAdjustmentOptions::kMaxNumImagesDirectSolver)).RefinedUsesDirectSolver());
  CHECK(!BundleAdjusterHip(o, Config(BundleAdjustmentOptions::kMaxNumImagesDirectSolver + 1)).RefinedUsesDirectSolver());
}

// Solve with `type` against pcd_ba_solve with `solver` through the C ABI: bit for bit
static void TestSolve(BundleAdjustmentOptions::LinearSolverType type, int solver, const char* name) {
  const size_t I = 5, P = 120;
  Reconstruction rec;
  GenerateReconstruction(I, P, 1, 1230.0, &rec);   // the focal length starts 2.5 % off
  BundleAdjustmentOptions opt;
  opt.max_num_iterations = 8;
  opt.refine_focal_length = true;
  opt.refine_intrinsics_on_device = true;
  opt.refined_linear_solver_type = type;
  const Reconstruction before = rec;
  BundleAdjusterHip ba(opt, Config(I));
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(ba.Solve(&rec));
  const pcd_ba_solve_summary& sm = ba.Summary();
  const double f = rec.cameras.at(0).params[0];
  std::printf("Solve with the focal length refined, %s: cost %.6g -> %.6g, %d iterations, %d accepted, f 1230 -> %.3f\n",
              name, sm.initial_cost, sm.final_cost, sm.num_iterations, sm.num_accepted, f);
  CHECK(sm.num_accepted >= 1 && sm.final_cost < sm.initial_cost);
  CHECK(f != 1230.0 && std::isfinite(f));          // the camera in the Reconstruction is updated
  for (int k = 1; k < 4; ++k) CHECK(rec.cameras.at(0).params[k] == before.cameras.at(0).params[k]);   // constant
  Reconstruction rec2 = before;
  BundleAdjusterHip raw(opt, Config(I));
  raw.SetUp(&rec2, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(raw.Create());
  pcd_ba_solve_opts o;
  pcd_ba_solve_opts_default(&o);
  o.max_num_iterations = opt.max_num_iterations;
  o.linear.max_iterations = opt.max_linear_solver_iterations;
  o.linear_solver = solver;
  o.refine_intrinsics = 1;
  pcd_ba_solve_summary s2{};
  std::vector<pcd_ba_solve_iteration> its(opt.max_num_iterations);
  CHECK(pcd_ba_solve(raw.handle(), &o, &s2, its.data()) == PCD_OK);
  CHECK(s2.final_cost == sm.final_cost && s2.num_accepted == sm.num_accepted && s2.num_iterations == sm.num_iterations);
  for (int k = 0; k < s2.num_iterations; ++k)      // the PCG iterates, the direct solve does not
    CHECK(solver == PCD_LINEAR_PCG_CAM ? its[k].linear_iterations > 0 : its[k].linear_iterations == 0);
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
}

int main(int argc, char** argv) {
  TestSolverChoice();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) {
    if (pcd_device_count() < 1) { std::printf("FAIL: --gpu given but no gfx950 device\n"); return 1; }
    TestSolve(BundleAdjustmentOptions::LinearSolverType::ITERATIVE, PCD_LINEAR_PCG_CAM, "bordered PCG");
    TestSolve(BundleAdjustmentOptions::LinearSolverType::DIRECT, PCD_LINEAR_CHOLESKY, "Cholesky (the default)");
  }
  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

// test_ba_cholesky.cc -- BundleAdjusterHip::Solve (ba_problem.h) with the direct linear solver: the device LM whose
// steps come from the library's blocked Cholesky of the reduced camera system.
//   ./test_ba_cholesky          the solver choice, which needs no GPU (ITERATIVE is the default, AUTO by image count)
//   ./test_ba_cholesky --gpu    Solve with DIRECT and with AUTO on mock reconstructions (fails if no gfx950 device)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "ba_problem.h"

using namespace colmap_hip;
using LinearSolverType = BundleAdjustmentOptions::LinearSolverType;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// shape of bundle_adjustment_test.cc:123-184 GenerateReconstruction, as test_ba_solve.cc builds it: every image
// observes every point, SIMPLE_RADIAL f = 1200, 1000 x 1000, identity rotation, t = (U(-1,1), U(-1,1), 10), +-2 px noise
static void GenerateReconstruction(size_t num_images, size_t num_points, Reconstruction* rec) {
  std::mt19937 rng(0);
  std::uniform_real_distribution<double> u(-1.0, 1.0), px(-2.0, 2.0);
  for (point3D_t p = 1; p <= num_points; ++p) {
    Point3D pt;
    for (double& c : pt.xyz) c = u(rng);
    rec->points3D[p] = pt;
  }
  for (image_t i = 0; i < num_images; ++i) {
    Camera cam;
    cam.model_id = PCD_CAM_SIMPLE_RADIAL;
    cam.params = {1200.0, 500.0, 500.0, 0.0};
    rec->cameras[i] = cam;
    Image im;
    im.camera_id = i;
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
  return config;
}

static void TestChoice() {
  BundleAdjustmentOptions d;
  CHECK(d.linear_solver_type == LinearSolverType::ITERATIVE);
  CHECK(!BundleAdjusterHip(d, Config(12)).UsesDirectSolver());            // the default stays the PCG
  d.linear_solver_type = LinearSolverType::DIRECT;
  CHECK(BundleAdjusterHip(d, Config(2000)).UsesDirectSolver());
  d.linear_solver_type = LinearSolverType::AUTO;
  CHECK(BundleAdjusterHip(d, Config(12)).UsesDirectSolver());
  CHECK(BundleAdjusterHip(d, Config(1000)).UsesDirectSolver());
  CHECK(!BundleAdjusterHip(d, Config(1001)).UsesDirectSolver());          // the reference goes iterative above 1000
}

static double Cost(BundleAdjusterHip& ba) {
  double c = -1.0;
  pcd_ba_out o{};
  o.cost = &c;
  CHECK(pcd_ba_evaluate(ba.handle(), &o) == PCD_OK);
  return c;
}

static void TestSolve(size_t num_images, size_t num_points, LinearSolverType type, bool const_tvec) {
  Reconstruction rec;
  GenerateReconstruction(num_images, num_points, &rec);
  std::mt19937 rng(7);
  std::normal_distribution<double> n(0.0, 0.02);
  for (auto& kv : rec.points3D)
    for (double& c : kv.second.xyz) c += n(rng);   // something to optimise
  BundleAdjustmentConfig config = Config(num_images);
  if (const_tvec) config.SetConstantTvec(1, {0});
  config.AddConstantPoint(3); config.AddConstantPoint(7);
  BundleAdjustmentOptions opt;
  opt.max_num_iterations = 10;
  opt.linear_solver_type = type;
  const Reconstruction before = rec;
  BundleAdjusterHip ba(opt, config);
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::NoLidar);
  CHECK(ba.UsesDirectSolver());
  CHECK(ba.Create());
  const double cost0 = Cost(ba);
  CHECK(ba.Solve(&rec));
  const pcd_ba_solve_summary& sm = ba.Summary();
  std::printf("Solve (direct) %zu images / %zu points: cost %.6g -> %.6g, %d iterations, %d accepted, %.2f ms (linear %.2f ms)\n",
              num_images, num_points, sm.initial_cost, sm.final_cost, sm.num_iterations, sm.num_accepted, sm.total_ms,
              sm.linear_solver_ms);
  CHECK(sm.num_accepted >= 1 && sm.num_iterations <= 10);
  CHECK(std::fabs(sm.initial_cost - cost0) <= 1e-9 * cost0);
  CHECK(sm.final_cost < sm.initial_cost);
  CHECK(std::fabs(Cost(ba) - sm.final_cost) <= 1e-9 * sm.final_cost);
  CHECK(sm.linear_solver_ms > 0.0);
  // the scratch of the direct solve is in the handle: (n_padded + 192) n_padded doubles, n_padded = 96 at these sizes
  pcd_ba_schur_info si{};
  CHECK(pcd_ba_schur_stats(ba.handle(), &si) == PCD_OK);
  CHECK(si.scratch_bytes >= 8u * 96u * 96u);
  size_t moved = 0;
  for (size_t i = 0; i < ba.image_ids_.size(); ++i) {
    const Image& im = rec.images.at(ba.image_ids_[i]);
    const Image& was = before.images.at(ba.image_ids_[i]);
    if (ba.image_const_pose_[i]) {
      CHECK(std::memcmp(im.qvec, was.qvec, sizeof im.qvec) == 0 && std::memcmp(im.tvec, was.tvec, sizeof im.tvec) == 0);
    } else {
      moved += std::memcmp(im.tvec, was.tvec, sizeof im.tvec) != 0;
      for (int k = 0; k < 3; ++k)
        if ((ba.image_const_tvec_[i] >> k) & 1) CHECK(std::memcmp(&im.tvec[k], &was.tvec[k], sizeof(double)) == 0);
      const double nq = std::sqrt(im.qvec[0] * im.qvec[0] + im.qvec[1] * im.qvec[1] + im.qvec[2] * im.qvec[2] + im.qvec[3] * im.qvec[3]);
      CHECK(std::fabs(nq - 1.0) < 1e-12);
    }
  }
  CHECK(moved + 1 == ba.image_ids_.size());
  size_t points_moved = 0;
  for (size_t p = 0; p < ba.point_ids_.size(); ++p) {
    const Point3D& pt = rec.points3D.at(ba.point_ids_[p]);
    const Point3D& was = before.points3D.at(ba.point_ids_[p]);
    if (ba.point_const_[p]) CHECK(std::memcmp(pt.xyz, was.xyz, sizeof pt.xyz) == 0);
    else points_moved += std::memcmp(pt.xyz, was.xyz, sizeof pt.xyz) != 0;
  }
  CHECK(ba.NumConstantPoints() == 2u && points_moved + 2 == ba.point_ids_.size());
}

int main(int argc, char** argv) {
  TestChoice();
  if (argc > 1 && std::strcmp(argv[1], "--gpu") == 0) {
    if (pcd_device_count() < 1) { std::printf("FAIL: --gpu given but no gfx950 device\n"); return 1; }
    TestSolve(6, 400, LinearSolverType::DIRECT, true);
    TestSolve(12, 300, LinearSolverType::AUTO, false);   // AUTO picks the direct solver at 12 images
  }
  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

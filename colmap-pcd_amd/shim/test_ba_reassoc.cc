// test_ba_reassoc.cc -- BundleAdjusterHip::ReassociateLidar (ba_problem.h): associate, solve, associate again on the
// live handle (tests/test_ba_lidar_gpu.py builds and runs it: ./shim/test_ba_reassoc <scene.bin>; it needs a gfx950).
//
// A mock reconstruction as test_ba_solve.cc builds its own, and a cloud of two planes around its points.  Round 1
// associates every point and solves; round 2 associates a selection with a tighter radius and solves on the same
// handle.  The scene of round 1 (the flat problem, the cloud, the radius) is written to <scene.bin> and the cost after
// the first Solve is printed, so that the test can run the Python route on the same scene and compare.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

#include "ba_problem.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// shape of bundle_adjustment_test.cc:123-184 GenerateReconstruction, as in test_ba_solve.cc
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

// Two planes in the frame of the index, 3 cm spacing over [-1.2, 1.2]^2: y = 1.05 with normal (0, -1, 0) (ground: the
// normal is along y) and z = 1.05 with normal (0.05, 0.02, -1) normalised.  Rows go in as a raw scan: index frame
// (x, y, z) = (-raw_y, -raw_z, raw_x), so raw = (z, -x, -y), normals alike.
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

template <typename T>
static void Block(FILE* f, const char* name, const char* dtype, const std::vector<T>& v) {
  std::fprintf(f, "%s %s %zu\n", name, dtype, v.size());
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

static double Cost(BundleAdjusterHip& ba) {
  double c = -1.0;
  pcd_ba_out o{};
  o.cost = &c;
  CHECK(pcd_ba_evaluate(ba.handle(), &o) == PCD_OK);
  return c;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_ba_reassoc <scene.bin>\n");
    return 2;
  }
  if (pcd_device_count() < 1) { std::printf("FAIL: no gfx950 device\n"); return 1; }
  const size_t num_images = 4, num_points = 150;
  Reconstruction rec;
  GenerateReconstruction(num_images, num_points, &rec);
  std::mt19937 rng(7);
  std::normal_distribution<double> n(0.0, 0.02);
  for (auto& kv : rec.points3D)
    for (double& c : kv.second.xyz) c += n(rng);
  BundleAdjustmentConfig config;
  for (image_t i = 0; i < num_images; ++i) config.AddImage(i);
  config.SetConstantPose(0);
  config.SetConstantTvec(1, {0});
  BundleAdjustmentOptions opt;
  opt.max_num_iterations = 10;
  opt.icp_lidar_constraint_weight = 40.0;            // not the defaults: the call must take them from the options
  opt.icp_ground_lidar_constraint_weight = 300.0;

  std::vector<float> cxyz, cnrm;
  Planes(&cxyz, &cnrm);
  lidar::PointCloudProcess pcp;
  CHECK(pcp.InitializeFromRawCloud(cxyz.data(), cnrm.data(), cxyz.size() / 3));

  BundleAdjusterHip ba(opt, config);
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::Local);
  const size_t O = ba.obs_image_.size();
  CHECK(O == num_images * num_points && ba.NumResiduals() == 2 * O);
  CHECK(!ba.ReassociateLidar(pcp, PCD_GATE_MAPPER_GLOBAL, {0.6}));   // no live handle yet
  CHECK(ba.Create());

  {   // the scene of round 1, for the Python route
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f != nullptr);
    if (f) {
      Block(f, "cam_model", "i4", ba.cam_model_); Block(f, "cam_off", "i4", ba.cam_off_);
      Block(f, "cam_params", "f8", ba.cam_params_); Block(f, "poses", "f8", ba.poses_);
      Block(f, "image_camera", "i4", ba.image_cam_); Block(f, "points", "f8", ba.points_);
      Block(f, "obs_image", "i4", ba.obs_image_); Block(f, "obs_point", "i4", ba.obs_point_);
      Block(f, "obs_xy", "f8", ba.obs_xy_); Block(f, "image_const_pose", "u1", ba.image_const_pose_);
      Block(f, "image_const_tvec", "u1", ba.image_const_tvec_); Block(f, "point_const", "u1", ba.point_const_);
      Block(f, "cloud_xyz", "f4", cxyz); Block(f, "cloud_nrm", "f4", cnrm);
      CHECK(std::fclose(f) == 0);
    }
  }

  // round 1: every point, 0.6 m
  const std::vector<double> wrong(7, 0.5);
  CHECK(!ba.ReassociateLidar(pcp, PCD_GATE_MAPPER_GLOBAL, wrong));   // neither 1 nor P entries: the problem stays
  CHECK(ba.NumResiduals() == 2 * O);
  pcd_ba_assoc_info info{};
  CHECK(ba.ReassociateLidar(pcp, PCD_GATE_MAPPER_GLOBAL, {0.6}, nullptr, &info));
  CHECK(info.num_queries == num_points && info.num_terms > 0 && info.num_terms < num_points);
  CHECK(info.num_icp > 0 && info.num_icp_ground > 0 && info.num_icp + info.num_icp_ground == info.num_terms);
  CHECK(ba.NumResiduals() == 2 * O + info.num_terms);
  CHECK(ba.config().lidar_maps_.size() == info.num_terms && ba.lidar_point_.size() == info.num_terms);
  size_t ground = 0;
  for (size_t l = 0; l < ba.lidar_w_.size(); ++l) {
    CHECK(ba.lidar_w_[l] == 40.0 || ba.lidar_w_[l] == 300.0);
    ground += ba.lidar_w_[l] == 300.0;
  }
  CHECK(ground == info.num_icp_ground);
  pcd_ba* live = ba.handle();
  const double cost1 = Cost(ba);
  CHECK(ba.Solve(&rec));
  CHECK(ba.handle() == live);                        // Solve kept the handle the terms were installed on
  const pcd_ba_solve_summary sm1 = ba.Summary();
  CHECK(std::fabs(sm1.initial_cost - cost1) <= 1e-9 * cost1 && sm1.final_cost < sm1.initial_cost && sm1.num_accepted >= 1);
  std::printf("round 1: %llu terms (%llu icp, %llu ground), cost %.17g -> %.17g, assoc %.3f ms, rebuild %.3f ms\n",
              (unsigned long long)info.num_terms, (unsigned long long)info.num_icp,
              (unsigned long long)info.num_icp_ground, sm1.initial_cost, sm1.final_cost, info.assoc_ms, info.rebuild_ms);
  std::printf("ROUND1 %llu %.17g %.17g\n", (unsigned long long)info.num_terms, sm1.initial_cost, sm1.final_cost);

  // round 2: the refined points, a tighter radius, two points in three
  std::unordered_set<point3D_t> select;
  for (point3D_t p = 1; p <= num_points; ++p)
    if (p % 3 != 0) select.insert(p);
  pcd_ba_assoc_info info2{};
  CHECK(ba.ReassociateLidar(pcp, PCD_GATE_MAPPER_GLOBAL | PCD_GATE_BOUNDED_SEARCH, {0.4}, &select, &info2));
  CHECK(info2.num_queries == select.size() && info2.num_terms > 0 && info2.num_terms <= info.num_terms);
  CHECK(ba.NumResiduals() == 2 * O + info2.num_terms);
  for (const auto& kv : ba.config().lidar_maps_) CHECK(select.count(kv.first) == 1);
  CHECK(ba.handle() == live);
  CHECK(ba.Solve(&rec));
  CHECK(ba.handle() == live);
  CHECK(ba.Summary().final_cost <= ba.Summary().initial_cost);
  // a Solve after a new SetUp builds its handle again, from the refreshed lidar_maps_: the same number of terms
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::Local);
  CHECK(ba.NumResiduals() == 2 * O + info2.num_terms);

  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

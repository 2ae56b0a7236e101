// test_ba_proj.cc -- BundleAdjusterHip::ProjectLidar (ba_problem.h): the local round's two association routes installed
// on the live handle in one call (tests/test_ba_proj_gpu.py builds and runs it: ./shim/test_ba_proj; it needs a gfx950).
//
// A mock reconstruction as test_ba_reassoc.cc builds its own, with OPENCV cameras of 1000 x 1000 pixels, and that test's
// cloud of two planes.  Round 1: every point takes the depth-projection route from three of the four images; the
// installed terms are compared, bit for bit, with the host route the shim had before (PcdProj::SetNewImages into
// per-image maps, MatchVariablePoint2LidarPoint per point).  Round 2, after a Solve on the same handle: two points in
// three by projection, the rest by nearest neighbour, at the refined parameters.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

#include "ba_problem.h"
#include "pcd_proj_hip.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

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
    cam.model_id = PCD_CAM_OPENCV;
    cam.params = {1200.0, 1190.0, 500.0, 500.0, 0.01, -0.002, 1e-4, -1e-4};
    cam.width = cam.height = 1000;
    rec->cameras[i] = cam;
    Image im;
    im.camera_id = i;
    im.tvec[0] = u(rng); im.tvec[1] = u(rng); im.tvec[2] = 10;
    for (point3D_t p = 1; p <= num_points; ++p) {
      const Point3D& pt = rec->points3D[p];
      const double X = pt.xyz[0] + im.tvec[0], Y = pt.xyz[1] + im.tvec[1], Z = pt.xyz[2] + im.tvec[2];
      Point2D p2;
      p2.xy[0] = 1200.0 * X / Z + 500.0 + px(rng);
      p2.xy[1] = 1190.0 * Y / Z + 500.0 + px(rng);
      p2.point3D_id = p;
      im.points2D.push_back(p2);
      rec->points3D[p].track.push_back({i, (point2D_t)(p - 1)});
    }
    rec->images[i] = im;
  }
}

// test_ba_reassoc.cc's planes: y = 1.05 (ground) and z = 1.05 in the frame of the index, pushed as a raw scan
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

static bool SameBits(const double* a, const double* b, int n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

int main() {
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
  opt.proj_lidar_constraint_weight = 2.5;            // not the defaults: the call must take them from the options
  opt.icp_lidar_constraint_weight = 40.0;
  opt.icp_ground_lidar_constraint_weight = 300.0;

  std::vector<float> cxyz, cnrm;
  Planes(&cxyz, &cnrm);
  lidar::PointCloudProcess pcp;
  CHECK(pcp.InitializeFromRawCloud(cxyz.data(), cnrm.data(), cxyz.size() / 3));
  lidar::PcdProj proj{lidar::PcdProjectionOptions()};
  CHECK(proj.BuildSubMap(pcp.handle()));

  BundleAdjusterHip ba(opt, config);
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::Local);
  const size_t O = ba.obs_image_.size();
  CHECK(O == num_images * num_points && ba.NumResiduals() == 2 * O);
  std::unordered_set<image_t> searched = {0, 1, 3};
  std::unordered_set<point3D_t> all_points, none;
  for (point3D_t p = 1; p <= num_points; ++p) all_points.insert(p);
  CHECK(!ba.ProjectLidar(proj, searched, all_points, none, {}));     // no live handle yet
  CHECK(ba.Create());
  lidar::PcdProj unbuilt{lidar::PcdProjectionOptions()};
  CHECK(!ba.ProjectLidar(unbuilt, searched, all_points, none, {}));  // no projector

  // round 1: every point by projection from images 0, 1, 3
  pcd_ba_proj_info info{};
  CHECK(ba.ProjectLidar(proj, searched, all_points, none, {}, &info));
  CHECK(info.num_images == 3 && info.num_features == 3 * num_points && info.num_found > 0 && info.num_found <= info.num_features);
  CHECK(info.num_terms > 0 && info.num_proj == info.num_terms && info.num_icp == 0 && info.num_icp_ground == 0 && info.pairs > 0);
  CHECK(ba.NumResiduals() == 2 * O + info.num_terms);
  CHECK(ba.config().lidar_maps_.size() == info.num_terms && ba.lidar_point_.size() == info.num_terms);
  for (double w : ba.lidar_w_) CHECK(w == 2.5);
  {   // the host route at the same parameters
    std::map<image_t, std::map<uint64_t, lidar::PcdProj::Vector6>> maps;
    std::vector<const Image*> images;
    std::vector<const Camera*> cameras;
    std::vector<std::map<uint64_t, lidar::PcdProj::Vector6>*> out;
    for (image_t i : {0u, 1u, 3u}) {
      images.push_back(&rec.images.at(i));
      cameras.push_back(&rec.cameras.at(rec.images.at(i).camera_id));
      out.push_back(&maps[i]);
    }
    CHECK(proj.SetNewImages(images, cameras, out));
    size_t matched = 0, several = 0;
    for (point3D_t p = 1; p <= num_points; ++p) {
      std::vector<image_t> track;
      for (const auto& el : rec.points3D.at(p).track) track.push_back(el.image_id);
      size_t cands = 0;
      for (image_t i : track) cands += maps.count(i) && maps.at(i).count(p);
      several += cands >= 2;
      LidarPoint want;
      const bool has = MatchVariablePoint2LidarPoint(maps, p, rec.points3D.at(p).xyz, track, &want);
      const auto it = ba.config().lidar_maps_.find(p);
      const bool nan_plane = has && (std::isnan(want.abcd[0]) || std::isnan(want.abcd[1]) || std::isnan(want.abcd[2]) || std::isnan(want.abcd[3]));
      CHECK((has && !nan_plane) == (it != ba.config().lidar_maps_.end()));
      if (!has || nan_plane || it == ba.config().lidar_maps_.end()) continue;
      ++matched;
      const LidarPoint& got = it->second;
      CHECK(got.type == LidarPointType::Proj && got.color[0] == 255 && got.color[1] == 0 && got.color[2] == 0);
      CHECK(SameBits(got.abcd.data(), want.abcd.data(), 4) && SameBits(got.xyz.data(), want.xyz.data(), 3));
      CHECK(SameBits(&got.dist, &want.dist, 1) && SameBits(&got.angle, &want.angle, 1));
    }
    CHECK(matched == info.num_terms && several > num_points / 2);
    std::printf("round 1: %llu of %llu features found, %llu Proj terms, %zu points with several candidates, proj %.3f ms, "
                "rebuild %.3f ms\n", (unsigned long long)info.num_found, (unsigned long long)info.num_features,
                (unsigned long long)info.num_terms, several, info.proj_ms, info.rebuild_ms);
  }
  pcd_ba* live = ba.handle();
  CHECK(ba.Solve(&rec));
  CHECK(ba.handle() == live);                        // Solve kept the handle the terms were installed on
  CHECK(ba.Summary().final_cost < ba.Summary().initial_cost && ba.Summary().num_accepted >= 1);

  // round 2: the refined parameters; two points in three by projection, the rest by nearest neighbour within 0.6 m
  std::unordered_set<point3D_t> by_proj, by_nn;
  for (point3D_t p = 1; p <= num_points; ++p) (p % 3 != 0 ? by_proj : by_nn).insert(p);
  const std::vector<double> wrong(7, 0.5);
  CHECK(!ba.ProjectLidar(proj, searched, by_proj, by_nn, wrong));    // neither 1 nor P entries: the problem stays
  CHECK(ba.NumResiduals() == 2 * O + info.num_terms);
  pcd_ba_proj_info info2{};
  CHECK(ba.ProjectLidar(proj, searched, by_proj, by_nn, {0.6}, &info2));
  CHECK(info2.num_proj > 0 && info2.num_icp + info2.num_icp_ground > 0);
  CHECK(info2.num_terms == info2.num_proj + info2.num_icp + info2.num_icp_ground);
  CHECK(ba.NumResiduals() == 2 * O + info2.num_terms && ba.config().lidar_maps_.size() == info2.num_terms);
  size_t n_proj = 0;
  for (const auto& kv : ba.config().lidar_maps_) {
    const bool is_proj = kv.second.type == LidarPointType::Proj;
    n_proj += is_proj;
    CHECK(is_proj == (by_proj.count(kv.first) == 1));
  }
  CHECK(n_proj == info2.num_proj);
  for (size_t l = 0; l < ba.lidar_w_.size(); ++l) CHECK(ba.lidar_w_[l] == 2.5 || ba.lidar_w_[l] == 40.0 || ba.lidar_w_[l] == 300.0);
  CHECK(ba.handle() == live);
  CHECK(ba.Solve(&rec));
  CHECK(ba.handle() == live && ba.Summary().final_cost <= ba.Summary().initial_cost);
  // a Solve after a new SetUp builds its handle again, from the refreshed lidar_maps_: the same number of terms
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::Local);
  CHECK(ba.NumResiduals() == 2 * O + info2.num_terms);

  std::printf(g_fail ? "%d FAILED\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

// test_voxel.cc -- PointCloudProcess::SetDownsample and LoadDownsizedMap / GetDownsizedMap
// (tests/test_voxel_gpu.py builds and runs it: ./shim/test_voxel <scratch.ply>).
//
// A raw scan -- x y z only, 1 cm spacing -- goes through the manual's preparation on the device: downsampled to 4 cm,
// then normals at 15 cm, and the queries find their plane.  The viewer's downsized map (lidar/ply.cc:59-84) comes from
// the same handle through the second path.
#include <cmath>
#include <cstdio>
#include <set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "lidar_hip.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)

// a 120 x 120 patch in the raw LiDAR frame: the plane x = 4.02 (depth), 1 cm spacing, a deterministic ripple of a millimetre
static std::vector<float> patch() {
  std::vector<float> p;
  uint32_t lcg = 12345u;
  for (int i = 0; i < 120; ++i)
    for (int j = 0; j < 120; ++j) {
      lcg = lcg * 1664525u + 1013904223u;
      const float w = ((lcg >> 8) & 0xFFFF) / 65535.0f * 0.002f - 0.001f;
      p.push_back(4.02f + w);
      p.push_back(-0.6f + 0.01f * i + 0.003f);
      p.push_back(-0.6f + 0.01f * j + 0.003f);
    }
  return p;
}

static bool write_ply(const std::string& path, const std::vector<float>& xyz, bool with_normals) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return false;
  const size_t n = xyz.size() / 3;
  std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n", n);
  if (with_normals) std::fprintf(f, "property float normal_x\nproperty float normal_y\nproperty float normal_z\n");
  std::fprintf(f, "end_header\n");
  for (size_t i = 0; i < n; ++i) {
    std::fprintf(f, "%.9g %.9g %.9g", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    if (with_normals) std::fprintf(f, " 0 1 0");
    std::fprintf(f, "\n");
  }
  return std::fclose(f) == 0;
}

// occupied voxels of the transformed cloud (x,y,z) -> (-y,-z,x) by the definition of pcdhip.h: one float multiply, floor
static size_t voxels_of(const std::vector<float>& raw, float leaf) {
  const float inv = 1.0f / leaf;
  std::set<std::tuple<int, int, int>> s;
  for (size_t i = 0; i < raw.size() / 3; ++i) {
    const float p[3] = {-raw[3 * i + 1], -raw[3 * i + 2], raw[3 * i]};
    const float a = p[0] * inv, b = p[1] * inv, c = p[2] * inv;
    s.insert(std::make_tuple((int)std::floor(a), (int)std::floor(b), (int)std::floor(c)));
  }
  return s.size();
}

// queries 5 cm in front of the patch, in the frame of the index: (x,y,z) -> (-y,-z,x)
static void queries(std::vector<uint64_t>* ids, std::vector<double>* q) {
  for (int i = 0; i < 10; ++i)
    for (int j = 0; j < 10; ++j) {
      const double raw[3] = {3.97, -0.45 + 0.09 * i + 0.013, -0.45 + 0.09 * j + 0.017};
      ids->push_back(ids->size() + 1);
      q->push_back(-raw[1]);
      q->push_back(-raw[2]);
      q->push_back(raw[0]);
    }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_voxel <scratch.ply>\n");
    return 2;
  }
  const std::string path = argv[1];
  const std::vector<float> xyz = patch();
  const size_t n = xyz.size() / 3;
  std::vector<uint64_t> ids;
  std::vector<double> q;
  queries(&ids, &q);
  const std::vector<double> range = {1.5};
  const size_t v4 = voxels_of(xyz, 0.04f);
  CHECK(v4 >= 900 && v4 < n / 8);

  CHECK(write_ply(path, xyz, false));
  {   // default: no downsampling, the reference's behaviour
    lidar::PointCloudProcess pcp(path);
    CHECK(!pcp.LoadDownsizedMap());   // nothing loaded yet
    CHECK(pcp.Initialize());
    CHECK(pcp.size() == n);
    CHECK(pcp.downsample_info().num_input == 0 && pcp.downsample_info().num_output == 0);
    // the viewer's path on the full cloud: 1 m voxels, then 16 m voxels
    CHECK(pcp.LoadDownsizedMap());
    CHECK(pcp.GetDownsizedMap().size() == 8 * voxels_of(xyz, 1.0f));
    CHECK(pcp.LoadDownsizedMap(16.0));
    const std::vector<float>& one = pcp.GetDownsizedMap();
    // the patch straddles the origin of the first two axes: four voxels of 60 x 60 points each, so the mean of the
    // four rows is the mean of the cloud
    CHECK(one.size() == 8 * 4);
    if (one.size() == 8 * 4) {
      double m[3] = {0, 0, 0}, got[3] = {0, 0, 0};
      for (size_t i = 0; i < n; ++i) { m[0] += -xyz[3 * i + 1]; m[1] += -xyz[3 * i + 2]; m[2] += xyz[3 * i]; }
      for (int r = 0; r < 4; ++r) {
        for (int k = 0; k < 3; ++k) got[k] += one[8 * r + k] / 4.0;
        CHECK(one[8 * r + 3] == 0.f && one[8 * r + 4] == 0.f && one[8 * r + 5] == 0.f && one[8 * r + 6] == 0.f);   // no normals: none
      }
      for (int k = 0; k < 3; ++k) CHECK(std::fabs(got[k] - m[k] / n) <= 1e-6);
      CHECK(one[0] < 0.f && one[1] < 0.f && one[8] > 0.f && one[9] < 0.f && one[17] > 0.f);   // ascending key, x fastest
    }
    CHECK(pcp.size() == n);           // cloud_ itself is untouched
  }
  {   // the manual's order: downsample to 4 cm, then normals at 15 cm on the downsampled cloud
    lidar::PointCloudProcess pcp(path);
    pcp.SetDownsample(0.04f, 1);
    pcp.SetNormalEstimation(0.15f, 3, lidar::PointCloudProcess::NormalEstimation::WhenMissing);
    CHECK(pcp.Initialize());
    const pcd_voxel_info& di = pcp.downsample_info();
    CHECK(di.num_input == n && di.num_voxels == v4 && di.num_output == v4 && di.num_dropped_rows == 0);
    CHECK(di.max_points_per_voxel >= 9 && di.max_points_per_voxel <= 25);
    CHECK(pcp.size() == v4);
    CHECK(pcp.normals_info().num_estimated == v4);   // estimated on the downsampled rows, all of them
    CHECK(pcp.normals_info().num_too_few == 0 && pcp.normals_info().num_degenerate == 0);
    std::unordered_map<uint64_t, LidarPoint> m;
    CHECK(MatchClosestLidarPoints(pcp, ids, q, range, PCD_GATE_MAPPER_LOCAL, &m));
    CHECK(m.size() == ids.size());
    for (const auto& kv : m) {
      const auto& p = kv.second.LidarABCD();
      CHECK(std::fabs(p[2] + 1.0) < 1e-2 && std::fabs(p[0]) < 0.1 && std::fabs(p[1]) < 0.1);
      CHECK(std::fabs(kv.second.Dist() - 0.05) < 0.03);
    }
    // the downsized map of a downsampled cloud: voxels of voxel centres, still one plane
    CHECK(pcp.LoadDownsizedMap(0.5));
    const std::vector<float>& dm = pcp.GetDownsizedMap();
    CHECK(dm.size() >= 8 * 4 && dm.size() <= 8 * 64);
    for (size_t i = 0; i < dm.size() / 8; ++i) {
      CHECK(std::fabs(dm[8 * i + 2] - 4.02f) < 2e-3f);
      CHECK(std::fabs(dm[8 * i + 6] + 1.0f) < 1e-2f);   // the estimated normals, summed and normalised
    }
  }
  {   // min_points above every voxel's count: everything is dropped, the cloud is empty and nothing associates
    lidar::PointCloudProcess pcp(path);
    pcp.SetDownsample(0.04f, 1000);
    CHECK(pcp.Initialize());
    CHECK(pcp.size() == 0 && pcp.downsample_info().num_dropped_rows == n && pcp.downsample_info().num_voxels == v4);
    std::unordered_map<uint64_t, LidarPoint> m;
    CHECK(MatchClosestLidarPoints(pcp, ids, q, range, PCD_GATE_MAPPER_LOCAL, &m));
    CHECK(m.empty());
  }
  CHECK(write_ply(path, xyz, true));
  {   // a file with normals: (0,1,0) -> (-1,-0,0) on every row, so every voxel's normal is exactly that
    lidar::PointCloudProcess pcp(path);
    pcp.SetDownsample(0.04f, 0);
    CHECK(pcp.Initialize());
    CHECK(pcp.size() == v4);
    std::vector<float> px(3 * v4), pn(3 * v4);
    CHECK(pcd_cloud_download(pcp.handle(), px.data(), pn.data()) == PCD_OK);
    bool all = true;
    for (size_t i = 0; i < v4; ++i) all = all && pn[3 * i] == -1.0f && pn[3 * i + 1] == 0.0f && pn[3 * i + 2] == 0.0f;
    CHECK(all);
  }
  std::printf(g_fail ? "FAILED (%d)\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

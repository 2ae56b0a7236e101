// test_normals.cc -- PointCloudProcess::SetNormalEstimation on a PLY without normal properties
// (tests/test_normals_gpu.py builds and runs it: ./shim/test_normals <scratch.ply>).
//
// A raw scan -- x y z only -- loads with normals 0 and associates nothing (lidar/ply.cc:101); with the shim's
// WhenMissing mode the normals are estimated on the device and the same queries find their planes.
#include <cmath>
#include <cstdio>
#include <string>
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

// a 40 x 40 patch in the raw LiDAR frame: the plane x = 4 (depth), 4 cm spacing, a deterministic ripple of a millimetre
static std::vector<float> patch() {
  std::vector<float> p;
  uint32_t lcg = 12345u;
  for (int i = 0; i < 40; ++i)
    for (int j = 0; j < 40; ++j) {
      lcg = lcg * 1664525u + 1013904223u;
      const float w = ((lcg >> 8) & 0xFFFF) / 65535.0f * 0.002f - 0.001f;
      p.push_back(4.0f + w);
      p.push_back(-0.8f + 0.04f * i);
      p.push_back(-0.8f + 0.04f * j);
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
    if (with_normals) std::fprintf(f, " 0 1 0");   // deliberately NOT the patch's normal: must survive WhenMissing
    std::fprintf(f, "\n");
  }
  return std::fclose(f) == 0;
}

// queries 5 cm in front of the patch, in the frame of the index: (x,y,z) -> (-y,-z,x)
static void queries(std::vector<uint64_t>* ids, std::vector<double>* q) {
  for (int i = 0; i < 10; ++i)
    for (int j = 0; j < 10; ++j) {
      const double raw[3] = {3.95, -0.5 + 0.1 * i + 0.013, -0.5 + 0.1 * j + 0.017};
      ids->push_back(ids->size() + 1);
      q->push_back(-raw[1]);
      q->push_back(-raw[2]);
      q->push_back(raw[0]);
    }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_normals <scratch.ply>\n");
    return 2;
  }
  const std::string path = argv[1];
  const std::vector<float> xyz = patch();
  std::vector<uint64_t> ids;
  std::vector<double> q;
  queries(&ids, &q);
  const std::vector<double> range = {1.5};

  CHECK(write_ply(path, xyz, false));
  {
    std::vector<float> a, b;
    bool has = true;
    CHECK(ReadPlyXYZNormal(path, &a, &b, &has) && !has && a.size() == xyz.size());
  }
  {   // default mode: the reference's behaviour, nothing associates
    lidar::PointCloudProcess pcp(path);
    CHECK(pcp.Initialize());
    std::unordered_map<uint64_t, LidarPoint> m;
    CHECK(MatchClosestLidarPoints(pcp, ids, q, range, PCD_GATE_MAPPER_LOCAL, &m));
    CHECK(m.empty());
    CHECK(pcp.normals_info().num_estimated == 0);
  }
  {   // WhenMissing: the file has no normal properties, so they are estimated
    lidar::PointCloudProcess pcp(path);
    pcp.SetNormalEstimation(0.15f, 3, lidar::PointCloudProcess::NormalEstimation::WhenMissing);
    CHECK(pcp.Initialize());
    CHECK(pcp.normals_info().num_estimated == xyz.size() / 3);
    CHECK(pcp.normals_info().num_too_few == 0 && pcp.normals_info().num_degenerate == 0);
    std::unordered_map<uint64_t, LidarPoint> m;
    CHECK(MatchClosestLidarPoints(pcp, ids, q, range, PCD_GATE_MAPPER_LOCAL, &m));
    CHECK(m.size() == ids.size());
    for (const auto& kv : m) {
      // raw plane x = const -> normal along z of the index frame, towards the sensor at the origin: (0,0,-1)
      const auto& p = kv.second.LidarABCD();
      CHECK(std::fabs(p[2] + 1.0) < 1e-2 && std::fabs(p[0]) < 0.1 && std::fabs(p[1]) < 0.1);
      CHECK(std::fabs(kv.second.Dist() - 0.05) < 0.03);
    }
  }
  CHECK(write_ply(path, xyz, true));
  {   // WhenMissing on a file that has normals: they stay
    bool has = false;
    std::vector<float> a, b;
    CHECK(ReadPlyXYZNormal(path, &a, &b, &has) && has);
    lidar::PointCloudProcess pcp(path);
    pcp.SetNormalEstimation(0.15f, 3, lidar::PointCloudProcess::NormalEstimation::WhenMissing);
    CHECK(pcp.Initialize());
    CHECK(pcp.normals_info().num_estimated == 0);
    std::vector<float> px(xyz.size()), pn(xyz.size());
    CHECK(pcd_cloud_download(pcp.handle(), px.data(), pn.data()) == PCD_OK);
    CHECK(pn[0] == -1.0f && pn[1] == -0.0f && pn[2] == 0.0f);   // (0,1,0) -> (-ny,-nz,nx)
  }
  {   // Always: replaced
    lidar::PointCloudProcess pcp(path);
    pcp.SetNormalEstimation(0.15f, 3, lidar::PointCloudProcess::NormalEstimation::Always);
    CHECK(pcp.Initialize());
    CHECK(pcp.normals_info().num_estimated == xyz.size() / 3);
    std::vector<float> px(xyz.size()), pn(xyz.size());
    CHECK(pcd_cloud_download(pcp.handle(), px.data(), pn.data()) == PCD_OK);
    CHECK(std::fabs(pn[2] + 1.0f) < 1e-2f);
  }
  std::printf(g_fail ? "FAILED (%d)\n" : "ALL OK\n", g_fail);
  return g_fail ? 1 : 0;
}

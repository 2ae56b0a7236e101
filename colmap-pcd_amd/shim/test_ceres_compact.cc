// test_ceres_compact.cc -- the compact Ceres route (ceres_compact.h, the compact mode of ceres_adapter.h).
//   ./test_ceres_compact expand <cases> <out>   rebuild jac_q / jac_t / jac_X of every case (tests/test_ceres_compact_cpu.py
//                                               compares them with the Jet oracle); no GPU
//   ./test_ceres_compact adapter <cases>        HipReprojectionBlock / HipLidarBlock::Evaluate on hand-filled compact
//                                               buffers: variable and constant pose, NULL Jacobians; no GPU
//   ./test_ceres_compact --gpu                  HipEvaluation and HipBlockRecorder with compact mode off and on: every
//                                               block's Evaluate output must be bit-identical between the two
// <cases>: int64 N, then N x {q[4], X[3], rec[8]} doubles.  <out>: N x {jac_q[8], jac_t[6], jac_X[6]} doubles.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ceres_adapter.h"

using namespace colmap_hip;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

struct Case { double q[4], X[3], rec[8]; };

static bool ReadCases(const char* path, std::vector<Case>* cases) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int64_t n = 0;
  bool ok = std::fread(&n, sizeof n, 1, f) == 1 && n >= 0 && n < (1 << 24);
  if (ok) {
    cases->resize((size_t)n);
    ok = std::fread(cases->data(), sizeof(Case), (size_t)n, f) == (size_t)n;
  }
  std::fclose(f);
  return ok;
}

static bool SameBits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

static int Expand(const char* in, const char* out) {
  std::vector<Case> cases;
  if (!ReadCases(in, &cases)) { std::printf("cannot read %s\n", in); return 1; }
  std::vector<double> res(20 * cases.size());
  for (size_t i = 0; i < cases.size(); ++i)
    ExpandReprojectionBlock(cases[i].q, cases[i].X, cases[i].rec, &res[20 * i], &res[20 * i + 8], &res[20 * i + 14]);
  FILE* f = std::fopen(out, "wb");
  if (!f || std::fwrite(res.data(), sizeof(double), res.size(), f) != res.size()) { std::printf("cannot write %s\n", out); return 1; }
  std::fclose(f);
  std::printf("expanded %zu cases\nALL OK\n", cases.size());
  return 0;
}

// a Jacobian destination with guard entries behind it: Evaluate must write exactly n entries or nothing
struct Dest {
  static constexpr double kGuard = -777.0;
  std::vector<double> v;
  size_t n;
  explicit Dest(size_t n_) : v(n_ + 2, kGuard), n(n_) {}
  bool Untouched() const { for (double x : v) if (x != kGuard) return false; return true; }
  bool Filled(const double* expect) const { return SameBits(v.data(), expect, n) && v[n] == kGuard && v[n + 1] == kGuard; }
};

static int Adapter(const char* in) {
  std::vector<Case> cases;
  if (!ReadCases(in, &cases) || cases.empty()) { std::printf("cannot read %s\n", in); return 1; }
  const size_t O = cases.size(), L = 3;
  const int K = 4, CS = 5;                                 // a 4-parameter camera in a handle whose widest camera has 5
  // the buffers PrepareForEvaluation would leave, filled by hand: observation o belongs to image o
  std::vector<double> records(8 * O), poses(7 * O), jac_cam(2 * CS * O), lres(L), jl(3 * L), res_only(2 * O);
  std::vector<int32_t> obs_image(O);
  for (size_t o = 0; o < O; ++o) {
    std::memcpy(&records[8 * o], cases[o].rec, sizeof cases[o].rec);
    std::memcpy(&poses[7 * o], cases[o].q, sizeof cases[o].q);
    for (int k = 0; k < 3; ++k) poses[7 * o + 4 + k] = 0.25 * (k + 1);
    obs_image[o] = (int32_t)o;
    for (int k = 0; k < 2 * CS; ++k) jac_cam[2 * CS * o + k] = (k % CS) < K ? 1000.0 * o + k + 0.5 : 0.0;
    res_only[2 * o] = 3.0 * o + 1.0; res_only[2 * o + 1] = 3.0 * o + 2.0;
  }
  for (size_t l = 0; l < L; ++l) { lres[l] = 10.0 + l; for (int k = 0; k < 3; ++k) jl[3 * l + k] = 100.0 * l + k; }
  HipBlockBuffers buf;
  buf.compact = true;
  buf.num_obs = O;
  buf.have_jacobians = true;
  buf.poses = poses.data();
  buf.obs_image = obs_image.data();
  buf.c.records = records.data(); buf.c.lidar_residuals = lres.data(); buf.c.jac_lidar = jl.data();
  buf.c.jac_cam = jac_cam.data(); buf.c.cam_stride = CS;
  double cam[K] = {1, 2, 3, 4}, tvec[3] = {0, 0, 0};
  for (size_t o = 0; o < O; ++o) {
    const Case& c = cases[o];
    // Ceres' own quaternion for the variable-pose block differs from the one in the pose buffer here, so a block
    // that read the wrong one shows
    const double* qv = cases[(o + 1) % O].q;
    double ejq[8], ejt[6], ejx[6], ejx_const[6], ejc[2 * K];
    ExpandReprojectionBlock(qv, c.X, c.rec, ejq, ejt, ejx);
    ExpandReprojectionBlock(c.q, c.X, c.rec, nullptr, nullptr, ejx_const);
    CHECK(SameBits(ejt, c.rec + 2, 6));                    // jac_t = M
    for (int r = 0; r < 2; ++r) for (int k = 0; k < K; ++k) ejc[K * r + k] = jac_cam[(2 * o + r) * CS + k];
    const double* expect[4] = {ejq, ejt, ejx, ejc};
    const double* expect_const[2] = {ejx_const, ejc};
    // variable pose: (qvec, tvec, xyz, camera)
    HipReprojectionBlock var(&buf, o, false, K);
    CHECK(var.parameter_block_sizes().size() == 4);
    double q[4]; std::memcpy(q, qv, sizeof q);
    double X[3]; std::memcpy(X, c.X, sizeof X);
    const double* params[4] = {q, tvec, X, cam};
    for (int null_at = -1; null_at < 4; ++null_at) {       // all blocks wanted, then each one constant in turn
      Dest d[4] = {Dest(8), Dest(6), Dest(6), Dest(2 * K)};
      double* jp[4];
      for (int k = 0; k < 4; ++k) jp[k] = k == null_at ? nullptr : d[k].v.data();
      double r[2] = {0, 0};
      CHECK(var.Evaluate(params, r, jp));
      CHECK(SameBits(r, c.rec, 2));
      for (int k = 0; k < 4; ++k) CHECK(k == null_at ? d[k].Untouched() : d[k].Filled(expect[k]));
    }
    {
      double r[2] = {0, 0};
      CHECK(var.Evaluate(params, r, nullptr) && SameBits(r, c.rec, 2));   // jacobians == NULL
    }
    // constant pose: (xyz, camera), block order 3, K; the pose comes from the gathered buffer
    HipReprojectionBlock cst(&buf, o, true, K);
    CHECK(cst.parameter_block_sizes().size() == 2 && cst.parameter_block_sizes()[0] == 3 && cst.parameter_block_sizes()[1] == K);
    const double* cparams[2] = {X, cam};
    for (int null_at = -1; null_at < 2; ++null_at) {
      Dest d[2] = {Dest(6), Dest(2 * K)};
      double* jp[2];
      for (int k = 0; k < 2; ++k) jp[k] = k == null_at ? nullptr : d[k].v.data();
      double r[2] = {0, 0};
      CHECK(cst.Evaluate(cparams, r, jp));
      CHECK(SameBits(r, c.rec, 2));
      for (int k = 0; k < 2; ++k) CHECK(k == null_at ? d[k].Untouched() : d[k].Filled(expect_const[k]));
    }
    {
      double r[2] = {0, 0};
      CHECK(cst.Evaluate(cparams, r, nullptr) && SameBits(r, c.rec, 2));
    }
  }
  // camera Jacobians wanted but not prepared: the block says so
  {
    HipBlockBuffers nc = buf;
    nc.c.jac_cam = nullptr;
    HipReprojectionBlock var(&nc, 0, false, K);
    const double* params[4] = {cases[0].q, tvec, cases[0].X, cam};
    Dest d[4] = {Dest(8), Dest(6), Dest(6), Dest(2 * K)};
    double* jp[4] = {d[0].v.data(), d[1].v.data(), d[2].v.data(), d[3].v.data()};
    double r[2];
    CHECK(!var.Evaluate(params, r, jp));
    jp[3] = nullptr;
    CHECK(var.Evaluate(params, r, jp) && d[3].Untouched());
  }
  // a residual-only pass: records == NULL, residuals [2 O]
  {
    HipBlockBuffers ro = buf;
    ro.have_jacobians = false;
    ro.c.records = nullptr; ro.c.jac_lidar = nullptr; ro.c.jac_cam = nullptr; ro.c.residuals = res_only.data();
    HipReprojectionBlock var(&ro, O - 1, false, K), cst(&ro, 0, true, K);
    const double* params[4] = {cases[O - 1].q, tvec, cases[O - 1].X, cam};
    const double* cparams[2] = {cases[0].X, cam};
    double r[2] = {0, 0};
    CHECK(var.Evaluate(params, r, nullptr) && r[0] == res_only[2 * (O - 1)] && r[1] == res_only[2 * (O - 1) + 1]);
    CHECK(cst.Evaluate(cparams, r, nullptr) && r[0] == res_only[0] && r[1] == res_only[1]);
    Dest d[4] = {Dest(8), Dest(6), Dest(6), Dest(2 * K)};
    double* jp[4] = {d[0].v.data(), d[1].v.data(), d[2].v.data(), d[3].v.data()};
    CHECK(!var.Evaluate(params, r, jp));                   // Jacobians were not prepared
    for (const Dest& x : d) CHECK(x.Untouched());
    HipLidarBlock lb(&ro, 1);
    double lr = 0, lj[3];
    double* ljp[1] = {lj};
    CHECK(lb.Evaluate(nullptr, &lr, nullptr) && lr == lres[1]);
    CHECK(!lb.Evaluate(nullptr, &lr, ljp));
  }
  // LiDAR blocks read the compact view
  for (size_t l = 0; l < L; ++l) {
    HipLidarBlock lb(&buf, l);
    Dest d(3);
    double* jp[1] = {d.v.data()};
    double r = 0;
    CHECK(lb.Evaluate(nullptr, &r, jp) && r == lres[l] && d.Filled(&jl[3 * l]));
    double* none[1] = {nullptr};
    CHECK(lb.Evaluate(nullptr, &r, none) && lb.Evaluate(nullptr, &r, nullptr));
  }
  std::printf("adapter: %zu cases\n%s\n", O, g_fail ? "FAILED" : "ALL OK");
  return g_fail ? 1 : 0;
}

// ---- GPU: compact off against compact on -----------------------------------------------------------------------------
// four images on three camera models (cam_stride 8 > K of the others; the per-observation model switch), rotated
// poses, every image sees every point; image 0 has a constant pose, image 3 is outside the config (constant-pose blocks
// from AddPointToProblem, constant camera); focal length and distortion are refined; a third of the points carry a
// LiDAR plane.  280 observations: more than one 256-thread workgroup, last wavefront partly filled.
static void Scene(Reconstruction* rec, BundleAdjustmentConfig* config) {
  uint64_t st = 12345;
  auto u = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return ((st >> 11) * (1.0 / 9007199254740992.0)) * 2.0 - 1.0; };
  const size_t num_points = 70;
  for (point3D_t p = 1; p <= num_points; ++p) {
    Point3D pt;
    for (double& c : pt.xyz) c = u();
    rec->points3D[p] = pt;
  }
  for (image_t i = 0; i < 4; ++i) {
    Camera cam;
    if (i == 1) { cam.model_id = PCD_CAM_OPENCV; cam.params = {1200.0, 1200.0, 500.0, 500.0, 0.01, -0.002, 1e-4, -1e-4}; }
    else if (i == 2) { cam.model_id = PCD_CAM_PINHOLE; cam.params = {1200.0, 1190.0, 500.0, 500.0}; }
    else { cam.model_id = PCD_CAM_SIMPLE_RADIAL; cam.params = {1200.0, 500.0, 500.0, 0.01}; }
    rec->cameras[i] = cam;
    Image im;
    im.camera_id = i;
    im.tvec[0] = u(); im.tvec[1] = u(); im.tvec[2] = 10;
    for (point3D_t p = 1; p <= num_points; ++p) {
      const Point3D& pt = rec->points3D[p];
      const double X = pt.xyz[0] + im.tvec[0], Y = pt.xyz[1] + im.tvec[1], Z = pt.xyz[2] + im.tvec[2];
      Point2D p2;
      p2.xy[0] = 1200.0 * X / Z + 500.0 + 2.0 * u();
      p2.xy[1] = 1200.0 * Y / Z + 500.0 + 2.0 * u();
      p2.point3D_id = p;
      im.points2D.push_back(p2);
      rec->points3D[p].track.push_back({i, (point2D_t)(p - 1)});
    }
    const double s = i == 3 ? 1.3 : 1.0;                   // the pose outside the config is not normalised by SetUp
    im.qvec[0] = s * 0.999; im.qvec[1] = s * 0.02 * (i + 1); im.qvec[2] = -s * 0.015; im.qvec[3] = s * 0.01 * i;
    rec->images[i] = im;
  }
  for (image_t i = 0; i < 3; ++i) config->AddImage(i);
  config->SetConstantPose(0);
  config->SetConstantTvec(1, {0});
  for (point3D_t p = 1; p <= num_points; ++p) {
    config->AddVariablePoint(p);
    if (p % 3 == 0) {
      LidarPoint lp;
      lp.type = p % 2 ? LidarPointType::Icp : LidarPointType::IcpGround;
      lp.abcd = {0.0, 1.0, 0.0, -(rec->points3D[p].xyz[1] + 0.03 * u())};
      config->AddLidarPoint(p, lp);
    }
  }
}

struct Block { std::unique_ptr<ceres::CostFunction> f; std::vector<double*> params; std::vector<bool> constant; };
struct Result { std::vector<double> r; std::vector<std::vector<double>> j; bool ok = true; };

static Result EvaluateAll(std::vector<Block>& blocks, bool with_jac) {
  Result out;
  for (Block& b : blocks) {
    double r[2] = {0, 0};
    std::vector<std::vector<double>> j(b.params.size());
    std::vector<double*> jp(b.params.size(), nullptr);
    for (size_t k = 0; k < b.params.size(); ++k) {
      j[k].assign((size_t)b.f->num_residuals() * b.f->parameter_block_sizes()[k], -777.0);
      if (!b.constant[k]) jp[k] = j[k].data();             // Ceres passes NULL for constant blocks
    }
    out.ok &= b.f->Evaluate(b.params.data(), r, with_jac ? jp.data() : nullptr);
    for (int k = 0; k < b.f->num_residuals(); ++k) out.r.push_back(r[k]);
    for (auto& v : j) out.j.push_back(std::move(v));
  }
  return out;
}

// bit-identical, entry by entry; reports the first difference by Jacobian block
static bool SameResult(const Result& a, const Result& b, const char* what) {
  bool same = a.ok && b.ok && a.r.size() == b.r.size() && a.j.size() == b.j.size() && SameBits(a.r.data(), b.r.data(), a.r.size());
  if (!same) std::printf("%s: residuals / status differ\n", what);
  for (size_t k = 0; same && k < a.j.size(); ++k)
    if (a.j[k].size() != b.j[k].size() || !SameBits(a.j[k].data(), b.j[k].data(), a.j[k].size())) {
      std::printf("%s: Jacobian block %zu (%zu entries) differs\n", what, k, a.j[k].size());
      for (size_t e = 0; e < a.j[k].size() && e < b.j[k].size(); ++e)
        if (std::memcmp(&a.j[k][e], &b.j[k][e], 8)) std::printf("  [%zu] full %.17g compact %.17g\n", e, a.j[k][e], b.j[k][e]);
      same = false;
    }
  return same;
}

static int Gpu() {
  if (pcd_device_count() < 1) { std::printf("FAIL: no gfx950 device\n"); return 1; }
  unsetenv("COLMAP_PCD_HIP_COMPACT");
  Reconstruction rec;
  BundleAdjustmentConfig config;
  Scene(&rec, &config);
  BundleAdjustmentOptions options;
  options.refine_focal_length = true; options.refine_extra_params = true;
  BundleAdjusterHip ba(options, config);
  ba.SetUp(&rec, BundleAdjusterHip::OptimazePhrase::WholeMap);
  const size_t O = ba.obs_image_.size(), L = ba.lidar_point_.size();
  CHECK(O == 280 && L == 23);
  CHECK(ba.Create(0));
  ShimParameterSource src(&rec);
  HipEvaluation<> cb(&ba, src);
  CHECK(!cb.compact());
  std::vector<Block> blocks;
  size_t n_cpose = 0, n_cam_var = 0, n_cam_const = 0;
  for (size_t o = 0; o < O; ++o) {
    const int im = ba.obs_image_[o], pt = ba.obs_point_[o], cm = ba.image_cam_[im];
    Block b;
    b.f.reset(cb.ReprojectionBlock(o));
    if (!ba.image_const_pose_[im]) {
      b.params = {src.Qvec(ba.image_ids_[im]), src.Tvec(ba.image_ids_[im])};
      b.constant = {false, false};
    } else {
      ++n_cpose;
    }
    b.params.push_back(src.XYZ(ba.point_ids_[pt])); b.constant.push_back(ba.point_const_[pt] != 0);
    b.params.push_back(src.Params(ba.camera_ids_[cm])); b.constant.push_back(!ba.CameraVariable(cm));
    (ba.CameraVariable(cm) ? n_cam_var : n_cam_const) += 1;
    CHECK(b.f->parameter_block_sizes().size() == b.params.size());
    blocks.push_back(std::move(b));
  }
  for (size_t l = 0; l < L; ++l) {
    Block b;
    b.f.reset(cb.LidarBlock(l));
    b.params = {src.XYZ(ba.point_ids_[ba.lidar_point_[l]])};
    b.constant = {false};
    blocks.push_back(std::move(b));
  }
  CHECK(n_cpose == 140 && n_cam_var == 210 && n_cam_const == 70);
  auto both = [&](bool with_jac, const char* what) {
    cb.SetCompact(false);
    cb.PrepareForEvaluation(with_jac, true);
    CHECK(cb.ok());
    const uint64_t full_bytes = cb.buffers().b.bytes_d2h;
    const Result full = EvaluateAll(blocks, with_jac);
    cb.SetCompact(true);
    cb.PrepareForEvaluation(with_jac, true);
    CHECK(cb.ok());
    const Result compact = EvaluateAll(blocks, with_jac);
    CHECK(SameResult(full, compact, what));
    const pcd_ba_blocks_compact& c = cb.buffers().c;
    CHECK(c.cam_stride == 8);
    CHECK(c.bytes_d2h == (with_jac ? 8 * (8 * O + 4 * L) + 16 * 8 * O : 8 * (2 * O + L)));
    CHECK(c.bytes_d2h <= full_bytes);
    std::printf("%s: %zu blocks bit-identical: %s, %llu -> %llu bytes\n", what, blocks.size(), g_fail ? "no" : "yes",
                (unsigned long long)full_bytes, (unsigned long long)c.bytes_d2h);
  };
  both(true, "jacobians");
  both(false, "residuals only");
  cb.PrepareForEvaluation(false, false);                   // still compact: Jacobians asked after a residual-only pass
  CHECK(!EvaluateAll(blocks, true).ok);
  // the solver moves the parameters in place
  rec.images[2].tvec[0] += 0.05; rec.images[1].qvec[2] *= 1.1; rec.points3D[7].xyz[2] -= 0.02; rec.cameras[1].params[0] *= 1.001;
  both(true, "moved state");
  // ---- the recorder route, mode taken from the environment at Finalize ----
  cb.SetCompact(false);
  cb.PrepareForEvaluation(true, true);
  const Result full = EvaluateAll(blocks, true);
  for (int pass = 0; pass < 3; ++pass) {                   // switch set | unset | set, but the setter says no
    if (pass != 1) setenv("COLMAP_PCD_HIP_COMPACT", "1", 1); else unsetenv("COLMAP_PCD_HIP_COMPACT");
    HipBlockRecorder recd;
    if (pass == 2) recd.SetCompact(false);
    std::vector<Block> rb(O + L);
    auto add_obs = [&](size_t o) {
      const int im = ba.obs_image_[o], pt = ba.obs_point_[o], cm = ba.image_cam_[im];
      rb[o].f.reset(recd.AddReprojection(ba.cam_model_[cm], src.Qvec(ba.image_ids_[im]), src.Tvec(ba.image_ids_[im]),
                                         src.XYZ(ba.point_ids_[pt]), src.Params(ba.camera_ids_[cm]), &ba.obs_xy_[2 * o],
                                         ba.image_const_pose_[im] != 0));
    };
    for (size_t o = 0; o < O / 2; ++o) add_obs(o);
    for (size_t l = 0; l < L; ++l)
      rb[O + l].f.reset(recd.AddLidar(src.XYZ(ba.point_ids_[ba.lidar_point_[l]]), &ba.lidar_abcd_[4 * l], ba.lidar_w_[l]));
    for (size_t o = O / 2; o < O; ++o) add_obs(o);
    for (size_t k = 0; k < O + L; ++k) { rb[k].params = blocks[k].params; rb[k].constant = blocks[k].constant; }
    CHECK(recd.Finalize(0, /*cameras_variable=*/true));
    CHECK(recd.compact() == (pass == 0));
    unsetenv("COLMAP_PCD_HIP_COMPACT");                    // read at Finalize, never on the evaluation path
    recd.PrepareForEvaluation(true, true);
    CHECK(recd.ok());
    CHECK(SameResult(full, EvaluateAll(rb, true), pass == 0 ? "recorder, compact" : "recorder, full"));
    CHECK((recd.buffers().c.records != nullptr) == (pass == 0) && (recd.buffers().b.residuals != nullptr) == (pass != 0));
  }
  {   // HipEvaluation reads the environment at construction; only "1" switches the mode on
    setenv("COLMAP_PCD_HIP_COMPACT", "1", 1);
    HipEvaluation<> env_cb(&ba, src);
    CHECK(env_cb.compact());
    setenv("COLMAP_PCD_HIP_COMPACT", "0", 1);
    CHECK(!HipCompactRequested());
    unsetenv("COLMAP_PCD_HIP_COMPACT");
  }
  std::printf("%s\n", g_fail ? "FAILED" : "ALL OK");
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "expand") return Expand(argv[2], argv[3]);
  if (argc == 3 && std::string(argv[1]) == "adapter") return Adapter(argv[2]);
  if (argc == 2 && std::string(argv[1]) == "--gpu") return Gpu();
  std::printf("usage: test_ceres_compact expand <cases> <out> | adapter <cases> | --gpu\n");
  return 2;
}

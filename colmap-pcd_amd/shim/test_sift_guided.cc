// test_sift_guided.cc -- the sequence of src/feature/sift_test.cc:675-760 (TestMatchGuidedSiftFeaturesGPU) through the
// SiftMatchGPU-shaped adapter: MatchGuidedSiftFeaturesGPU (feature/sift.cc:1274-1365) restated on SiftMatchHIP,
// including the calls that pass nullptr and so match the slots' previous contents.
// Usage: test_sift_guided <descriptors file: 2 x 128 bytes of CreateRandomFeatureDescriptors(2)>  (needs a GPU)
#include <cstdio>
#include <cstring>
#include <vector>

#include "sift_match_hip.h"

namespace {

int g_fail = 0;
#define CHECK_EQ(a, b)                                                                            \
  do {                                                                                            \
    const long long _a = (long long)(a), _b = (long long)(b);                                     \
    if (_a != _b) { std::printf("FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, _a, _b); ++g_fail; } \
  } while (0)

struct Keypoint { float x = 0, y = 0, a11 = 1, a12 = 0, a21 = 0, a22 = 1; };   // colmap's FeatureKeypoint (6 floats)
typedef std::vector<unsigned char> Descriptors;                               // [n][128]
struct Match { uint32_t idx1, idx2; };

// MatchGuidedSiftFeaturesGPU for a PLANAR_OR_PANORAMIC geometry with H = I and SiftMatchingOptions() defaults
void MatchGuided(const std::vector<Keypoint>* k1, const std::vector<Keypoint>* k2, const Descriptors* d1,
                 const Descriptors* d2, colmap_hip::SiftMatchHIP* m, std::vector<Match>* out) {
  const int kFeatureShapeNumElems = 4;
  if (d1) {
    m->SetDescriptors(0, (int)(d1->size() / 128), d1->data());
    m->SetFeautreLocation(0, reinterpret_cast<const float*>(k1->data()), kFeatureShapeNumElems);
  }
  if (d2) {
    m->SetDescriptors(1, (int)(d2->size() / 128), d2->data());
    m->SetFeautreLocation(1, reinterpret_cast<const float*>(k2->data()), kFeatureShapeNumElems);
  }
  float H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const int max_num_matches = 32768;
  const float max_error = 4.0f;
  out->resize(max_num_matches);
  const int n = m->GetGuidedSiftMatch(max_num_matches, reinterpret_cast<uint32_t(*)[2]>(out->data()), H, nullptr, 0.7f,
                                      0.8f, max_error * max_error, max_error * max_error, 1);
  if (n < 0) { std::printf("FAIL: GetGuidedSiftMatch returned %d\n", n); ++g_fail; out->clear(); return; }
  out->resize(n);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s descriptors.bin\n", argv[0]); return 2; }
  Descriptors descriptors1(2 * 128);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(descriptors1.data(), 1, descriptors1.size(), f) != descriptors1.size()) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  std::fclose(f);
  Descriptors descriptors2(2 * 128);   // descriptors1.colwise().reverse(): the two rows swapped
  std::memcpy(descriptors2.data(), descriptors1.data() + 128, 128);
  std::memcpy(descriptors2.data() + 128, descriptors1.data(), 128);
  const Descriptors empty_descriptors;

  colmap_hip::SiftMatchHIP m(1000);
  CHECK_EQ(m.VerifyContextGL(), 1);
  std::vector<Keypoint> empty_keypoints, keypoints1(2), keypoints2(2);
  keypoints1[0].x = 1; keypoints1[1].x = 2;
  keypoints2[0].x = 2; keypoints2[1].x = 1;
  std::vector<Match> r;
  auto expect_both = [&](int line) {
    CHECK_EQ(r.size(), 2);
    if (r.size() == 2) {
      CHECK_EQ(r[0].idx1, 0); CHECK_EQ(r[0].idx2, 1); CHECK_EQ(r[1].idx1, 1); CHECK_EQ(r[1].idx2, 0);
    }
    if (g_fail) std::printf("  (step at line %d)\n", line);
  };

  MatchGuided(&keypoints1, &keypoints2, &descriptors1, &descriptors2, &m, &r);
  expect_both(__LINE__);
  MatchGuided(nullptr, nullptr, nullptr, nullptr, &m, &r);   // both slots reused
  expect_both(__LINE__);
  MatchGuided(&keypoints1, nullptr, &descriptors1, nullptr, &m, &r);
  expect_both(__LINE__);
  MatchGuided(nullptr, &keypoints2, nullptr, &descriptors2, &m, &r);
  expect_both(__LINE__);

  keypoints1[0].x = 100;
  MatchGuided(&keypoints1, &keypoints2, &descriptors1, &descriptors2, &m, &r);
  CHECK_EQ(r.size(), 1);
  if (r.size() == 1) { CHECK_EQ(r[0].idx1, 1); CHECK_EQ(r[0].idx2, 0); }

  MatchGuided(&empty_keypoints, &keypoints2, &empty_descriptors, &descriptors2, &m, &r);
  CHECK_EQ(r.size(), 0);
  MatchGuided(&keypoints1, &empty_keypoints, &descriptors1, &empty_descriptors, &m, &r);
  CHECK_EQ(r.size(), 0);
  MatchGuided(&empty_keypoints, &empty_keypoints, &empty_descriptors, &empty_descriptors, &m, &r);
  CHECK_EQ(r.size(), 0);

  // descriptors set again after the locations: the slot's locations are stale, the guided match refuses
  uint32_t buf[4][2];
  float H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  colmap_hip::SiftMatchHIP m2(1000);
  m2.SetDescriptors(0, 2, descriptors1.data());
  m2.SetFeautreLocation(0, reinterpret_cast<const float*>(keypoints1.data()), 4);
  m2.SetDescriptors(1, 2, descriptors2.data());
  m2.SetFeautreLocation(1, reinterpret_cast<const float*>(keypoints2.data()), 4);
  m2.SetDescriptors(0, 2, descriptors1.data());
  CHECK_EQ(m2.GetGuidedSiftMatch(4, buf, H, nullptr), -1);
  // SetFeatureLocation: SiftGPU's 4-float keypoints
  const float keys1[8] = {2, 0, 1, 0, 1, 0, 1, 0};   // (x, y, scale, orientation): points 2 and 1
  m2.SetFeatureLocation(0, keys1);
  CHECK_EQ(m2.GetGuidedSiftMatch(4, buf, H, nullptr), 2);   // point 0 at x 2 <-> set 2's x 1: still within 4 px

  if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

// sift_match_hip.h -- adapter with the interface of lib/SiftGPU's SiftMatchGPU (lib/SiftGPU/SiftGPU.h:268-352)
// as far as the reference uses it (feature/sift.cc:1170-1266 CreateSiftGPUMatcher / MatchSiftFeaturesGPU):
//   SiftMatchHIP m(max_sift); m.gpu_index = i; m.VerifyContextGL(); m.SetMaxSift(n); m.GetMaxSift();
//   m.SetDescriptors(0|1, num, const unsigned char*); m.GetSiftMatch(max_match, buf, distmax, ratiomax, mutual)
// The result is the exact brute-force match set of feature/sift.cc:55-144 (what SiftGPU approximates), in
// ascending index of set 0.  Guided matching as feature/sift.cc:1274-1365 MatchGuidedSiftFeaturesGPU drives it:
//   m.SetDescriptors(i, ...); m.SetFeautreLocation(i, keypoints, 4); m.GetGuidedSiftMatch(max_match, buf, H, F,
//   distmax, ratiomax, hdistmax, fdistmax, mutual)
// returns the exact MatchGuidedSiftFeaturesCPU result (sift.cc:1092-1162; hdistmax / fdistmax are the squared
// thresholds colmap passes).  No CPU fallback: without a gfx950 device VerifyContextGL() returns 0 and
// GetSiftMatch() / GetGuidedSiftMatch() return -1, the value the reference treats as "matching failed"
// (feature/sift.cc:1261-1266, :1356-1361).
#pragma once
#include <cstdint>

#include "../../include/pcdhip.h"

namespace colmap_hip {

class SiftMatchHIP {
 public:
  int gpu_index = 0;
  explicit SiftMatchHIP(int max_sift = 4096) : max_sift_(max_sift) {}
  ~SiftMatchHIP() { pcd_sift_matcher_destroy(m_); }
  SiftMatchHIP(const SiftMatchHIP&) = delete;
  SiftMatchHIP& operator=(const SiftMatchHIP&) = delete;

  int VerifyContextGL() { return Ensure() ? 1 : 0; }
  int CreateContextGL() { return VerifyContextGL(); }
  bool Allocate(int max_sift, int /*mbm*/) { SetMaxSift(max_sift); return Ensure(); }
  void SetMaxSift(int max_sift) {
    max_sift_ = max_sift;
    if (m_) pcd_sift_matcher_set_max_sift(m_, max_sift);
  }
  int GetMaxSift() const { return max_sift_; }
  void SetDescriptors(int index, int num, const unsigned char* descriptors, int /*id*/ = -1) {
    if (Ensure()) ok_ = pcd_sift_matcher_set_descriptors(m_, index, num, descriptors) == PCD_OK;
  }
  int GetSiftMatch(int max_match, uint32_t match_buffer[][2], float distmax = 0.7f, float ratiomax = 0.8f,
                   int mutual_best_match = 1) {
    if (!Ensure() || !ok_) return -1;
    int32_t n = 0;
    if (pcd_sift_matcher_match(m_, max_match, &match_buffer[0][0], distmax, ratiomax, mutual_best_match, &n) != PCD_OK)
      return -1;
    return n;
  }
  // SiftGPU.h:331-335: num locations of the slot's last SetDescriptors, (x, y) at a stride of 2 + gap floats
  void SetFeautreLocation(int index, const float* locations, int gap = 0) {
    if (Ensure()) ok_ = pcd_sift_matcher_set_locations(m_, index, locations, gap) == PCD_OK && ok_;
  }
  // SiftGPU's 4-float keypoint (x, y, scale, orientation)
  void SetFeatureLocation(int index, const float* keys) { SetFeautreLocation(index, keys, 2); }
  // SiftGPU.h:343-352
  int GetGuidedSiftMatch(int max_match, uint32_t match_buffer[][2], float* H, float* F, float distmax = 0.7f,
                         float ratiomax = 0.8f, float hdistmax = 32.0f, float fdistmax = 16.0f,
                         int mutual_best_match = 1) {
    if (!Ensure() || !ok_) return -1;
    int32_t n = 0;
    if (pcd_sift_matcher_match_guided(m_, max_match, &match_buffer[0][0], H, F, distmax, ratiomax, hdistmax, fdistmax,
                                      mutual_best_match, &n) != PCD_OK)
      return -1;
    return n;
  }

 private:
  bool Ensure() {
    if (!m_ && pcd_sift_matcher_create(gpu_index, max_sift_, &m_) != PCD_OK) m_ = nullptr;
    return m_ != nullptr;
  }
  int max_sift_;
  bool ok_ = true;
  pcd_sift_matcher* m_ = nullptr;
};

}  // namespace colmap_hip

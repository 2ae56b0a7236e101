// proj.h -- what the BA unit needs of the depth projector (proj.hip): projecting images whose poses and camera
// parameters are device memory, without a host copy of either.  Internal.
#pragma once
#include "common.h"

namespace pcd {

// The images of a BA handle as the projector takes them.  Host: what lays the buffers out and sizes the grids.
// Device: everything a record's values come from.
struct ProjDeviceImages {
  uint64_t n = 0;
  const uint64_t* width = nullptr;      // host [n]    Camera::Width / Height of the image's camera
  const uint64_t* height = nullptr;
  const int* num_params = nullptr;      // host [n]    K of the image's camera: prm[k] = k < K ? cam_params[off + k] : 0
  const uint32_t* feat_start = nullptr; // host [n+1]  image i's features are rows feat_start[i] .. feat_start[i+1]
  double latch_fx = 0, latch_fy = 0;    // focal lengths of the camera of image 0: a projector not latched yet latches on them
  const double* d_poses = nullptr;      // [n][7] qvec, tvec
  const int* d_image_cam = nullptr;     // [n]
  const int* d_cam_off = nullptr;
  const double* d_cam_params = nullptr;
  const uint8_t* d_select = nullptr;    // [n] or nullptr (all): an unselected image finds nothing
};

// pcd_proj_set_new_images_device for such images, everything enqueued on s, no synchronisation.  Feature g's results
// go to row d_out_row[g] of d_found / d_l6 (nullptr: row g).  The projector's scratch (pinned records, pair counts) is
// in flight until s has been synchronised; proj_collect_pairs then folds the pair counts into pcd_proj_last_pairs.
pcd_status proj_project_device_images(pcd_proj* p, const ProjDeviceImages& in, uint64_t n_feat, const double* d_feat_xy,
                                      const uint32_t* d_out_row, uint8_t* d_found, double* d_l6, hipStream_t s);
uint64_t proj_collect_pairs(pcd_proj* p);
pcd_cloud* proj_cloud(pcd_proj* p);

}  // namespace pcd

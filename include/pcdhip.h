/*
 * pcdhip.h -- C ABI of libpcdhip.so, the MI355X (gfx950) implementation of
 * colmap-pcd's image-to-LiDAR registration hot path.
 *
 * The reference (Wangshihu12/colmap-pcd) has no plugin/FFI API for this
 * path: it is reached through C++ call sites.  Every entry point below names
 * the reference interface it replaces (paths relative to the reference's
 * src/).  C++ adapters with the reference's own signatures live in
 * colmap-pcd_amd/shim/; INTEGRATION.md shows the call-site patch.
 *
 * Conventions
 *   - every function returns a pcd_status (0 = OK) and never throws;
 *   - host pointers unless the name ends in _device; the caller owns all
 *     buffers it passes, the library owns device memory behind the handles;
 *   - a handle is bound to one HIP device and may be used from one thread at
 *     a time; different handles are independent;
 *   - `stream` arguments are hipStream_t passed as void* (NULL = default
 *     stream); _device calls are asynchronous on that stream;
 *   - _device calls are EAGER launches: they grow per-handle scratch, build
 *     per-cloud tables on first use and may synchronise the stream, so they
 *     cannot be recorded into a HIP graph.  A stream that is capturing
 *     (hipStreamBeginCapture, torch.cuda.graph) is refused with
 *     PCD_ERR_UNSUPPORTED before anything is allocated or launched;
 *   - there is NO CPU fallback: without a usable gfx950 device every entry
 *     point that computes returns PCD_ERR_NO_DEVICE.
 */
#ifndef PCDHIP_H_
#define PCDHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCDHIP_VERSION_MAJOR 0
#define PCDHIP_VERSION_MINOR 1

typedef enum {
  PCD_OK = 0,
  PCD_ERR_INVALID = 1,     /* bad argument (null pointer, size mismatch, unknown enum) */
  PCD_ERR_NO_DEVICE = 2,   /* no HIP device / wrong architecture                       */
  PCD_ERR_HIP = 3,         /* a HIP runtime call failed; see pcd_last_error()          */
  PCD_ERR_OOM = 4,
  PCD_ERR_UNSUPPORTED = 5
} pcd_status;

const char* pcd_last_error(void);            /* thread-local message of the last failure */
int pcd_version(void);                       /* major*100 + minor                         */
int pcd_device_count(void);                  /* number of usable gfx950 devices (0 on a CPU box) */

/* ------------------------------------------------------------------------
 * LiDAR cloud index                         replaces lidar/ply.cc:9-57
 *   PointCloudProcess::Initialize -> PointCloudDirectionTrans -> Kdtree::BuildMap
 *   (lidar/kdtree.cc:5-8, pcl::KdTreeFLANN::setInputCloud)
 * --------------------------------------------------------------------- */
typedef struct pcd_cloud pcd_cloud;

typedef enum {
  PCD_LAYOUT_XYZ_NRM = 0,  /* xyz[n][3] floats + nrm[n][3] floats (two arrays)             */
  PCD_LAYOUT_AOS32 = 1     /* lidarpt::Point, lidar/pt_type.h:14-30: x y z pad nx ny nz pad */
} pcd_layout;

typedef struct {
  int32_t device;           /* HIP device ordinal                                           */
  int32_t layout;           /* pcd_layout                                                   */
  int32_t raw_lidar_frame;  /* 1: input rows are in the PLY/LiDAR frame: apply ply.cc:38-54 */
                            /*    (x,y,z)->(-y,-z,x) to position and normal and drop rows   */
                            /*    with a NaN; 0: rows are already transformed and filtered  */
  float cell_size;          /* grid cell edge in metres, 0 = choose from point density      */
  uint32_t index_base;      /* global index of local row i = index_base + i*index_stride:   */
  uint32_t index_stride;    /*    lets N ranks each hold every N-th row of one cloud        */
                            /*    (0 is read as 1).  Requires raw_lidar_frame == 0 if != 1. */
  int32_t reserved[8];
} pcd_cloud_options;

void pcd_cloud_options_default(pcd_cloud_options* o);

/* xyz: n rows (layout XYZ_NRM: 3 floats/row; AOS32: 8 floats/row, nrm ignored). */
pcd_status pcd_cloud_create(const float* xyz, const float* nrm, uint64_t n,
                            const pcd_cloud_options* opts, pcd_cloud** out);
void pcd_cloud_destroy(pcd_cloud* c);

/* rows kept after the NaN filter (index space of every idx returned below) */
uint64_t pcd_cloud_size(const pcd_cloud* c);

typedef struct {
  float cell_size;
  float origin[3];
  int32_t dims[3];           /* fine grid cells per axis                                     */
  int32_t block_dims[3];     /* 4x4x4-cell blocks per axis                                   */
  uint64_t num_indexed;      /* finite points in the grid (Inf rows keep an index, never win) */
  uint64_t occupied_cells;
  double build_ms;
  float bbox_lo[3], bbox_hi[3];   /* tight bounds of the finite rows (meaningful when num_indexed > 0): what    */
                                  /* pcd_nn_refine_device tests queries against, and what a caller uses to send */
                                  /* each query to its home shard                                               */
} pcd_cloud_info;
pcd_status pcd_cloud_get_info(const pcd_cloud* c, pcd_cloud_info* info);

/* copy the transformed / filtered cloud back (tests; GUI display path ply.cc:59-84 wants it) */
pcd_status pcd_cloud_download(const pcd_cloud* c, float* xyz /*[size][3]*/, float* nrm /*[size][3]*/);

/* ------------------------------------------------------------------------
 * One cloud over several devices of this process.
 * What IncrementalMapper::LoadPointcloud / BundleAdjustmentController::LoadPointcloud
 * (sfm/incremental_mapper.cc:194-206, controllers/bundle_adjustment.cc:206-212)
 * would build on a multi-GPU host: the cloud cut into ndev spatially compact
 * shards, one per device; indices everywhere are the post-filter row indices
 * of the WHOLE cloud, and every result equals the single-device one bit for
 * bit (ties -> lowest index, also across shards).
 * Verification status: every test so far has run on hosts with ONE GPU, all
 * shards on device 0.  The code paths that only exist between distinct
 * devices (peer copies of the built-in reduction, per-device streams) are
 * covered by tests/test_sharded_gpu.py::test_shards_on_distinct_devices,
 * which skips itself below two devices -- they have not executed yet.
 * --------------------------------------------------------------------- */
typedef struct pcd_cloud_shards pcd_cloud_shards;
pcd_status pcd_cloud_create_sharded(const float* xyz, const float* nrm, uint64_t n, const pcd_cloud_options* opts,
                                    const int* devices, int ndev, pcd_cloud_shards** out);  /* opts->device unused */
void pcd_cloud_shards_destroy(pcd_cloud_shards* s);
int pcd_cloud_shards_count(const pcd_cloud_shards* s);
uint64_t pcd_cloud_shards_size(const pcd_cloud_shards* s);          /* rows kept after the NaN filter, all shards */
pcd_cloud* pcd_cloud_shards_get(pcd_cloud_shards* s, int shard);    /* borrowed: shard `shard` as a pcd_cloud      */

/* ------------------------------------------------------------------------
 * Normal estimation (radius PCA)      replaces the preparation step of the reference's manual
 *   (README.md "Preparing point cloud": CloudCompare, "calculate normals using radius at 10-20cm");
 *   a cloud whose normals are 0 associates nothing (lidar/ply.cc:101 drops ||n|| < 1e-6).
 * Index space: the handle's post-filter rows.  For every finite row i, with r2 = radius*radius in float:
 *   neighbours  N_i = { finite rows j : ((dx*dx) + dy*dy) + dz*dz <= r2 }, d = p_i - p_j evaluated in float with
 *               separate multiply / add (the arithmetic of the search); i itself and duplicates count, a point at
 *               distance exactly r is inside; count[i] = |N_i| = k;
 *   moments     the float differences widened to double: m = (1/k) sum d, C = (1/k) sum d d^T - m m^T in fp64, every
 *               row's sum in an order fixed by the cloud layout (no atomics: a repeated call is bitwise identical);
 *   normal      unit eigenvector of the smallest eigenvalue of C (cyclic Jacobi in fp64), eigenvalues l0 <= l1 <= l2;
 *               curvature[i] = l0 / (l0 + l1 + l2)  (PCL's surface variation);
 *   no normal   (normal 0 0 0, curvature 0): k < max(min_neighbors, 3) [num_too_few]; l2 == 0 or l1 <= 1e-10 * l2,
 *               i.e. coincident or collinear neighbours [num_degenerate]; rows with an Inf coordinate (count 0);
 *   sign        PCD_NORMALS_ORIENT_VIEWPOINT: n . (viewpoint - p_i) >= 0, in double; viewpoint is given in the handle's
 *               frame, (0,0,0) = the sensor after the raw_lidar_frame swap.  PCD_NORMALS_ORIENT_NONE, or a dot product
 *               of exactly 0: the component of largest magnitude is positive (ties: lowest axis).  Nothing downstream
 *               depends on the sign (lidar/lidar_point.cc:21-37 takes abs, base/cost_functions.h:226-229 squares);
 *   store       the double vector rounded to float replaces the row's normal in the handle: every later search,
 *               association, projection read-out and pcd_cloud_download sees it.  only_missing != 0: rows whose
 *               stored normal has ||n|| >= 1e-6 keep it [num_kept]; their count and curvature are still reported.
 * Limits: radius <= 8 * cell_size of the handle (PCD_ERR_INVALID otherwise: create the handle with a larger
 * cell_size); ONE handle holding the whole cloud -- a shard of pcd_cloud_create_sharded or a handle with
 * index_stride != 1 / index_base != 0 is refused with PCD_ERR_UNSUPPORTED, its neighbourhoods cross handle borders:
 * estimate on one handle, download, then shard.  An empty cloud returns PCD_OK with zero counts.  Where the cloud's
 * largest absolute coordinate times 2e-6 takes a radius of up to 8 cells past 9 cells: PCD_ERR_UNSUPPORTED ("reaches").
 * A refused call of either entry point leaves the stored normals and the outputs as they were.
 * --------------------------------------------------------------------- */
typedef enum { PCD_NORMALS_ORIENT_NONE = 0, PCD_NORMALS_ORIENT_VIEWPOINT = 1 } pcd_normals_orient;
typedef struct {
  float radius;            /* metres, finite and > 0                                        */
  int32_t min_neighbors;   /* >= 0; fewer than max(min_neighbors, 3) neighbours: no normal  */
  int32_t orient;          /* pcd_normals_orient                                            */
  float viewpoint[3];
  int32_t only_missing;
  int32_t reserved[8];
} pcd_normals_options;
typedef struct {
  uint64_t num_estimated, num_too_few, num_degenerate, num_kept;   /* finite rows: the four add up to num_indexed */
  uint64_t pair_tests;       /* distance tests made (candidates staged x queries)            */
  uint32_t max_neighbors;
  double mean_neighbors;     /* over the finite rows                                         */
  double ms;                 /* device time of the pass                                      */
} pcd_normals_info;
void pcd_normals_options_default(pcd_normals_options* o);   /* 0.15, 3, VIEWPOINT, {0,0,0}, 0 */
/* d_count [size] / d_curvature [size]: device outputs, either may be NULL */
pcd_status pcd_cloud_estimate_normals_device(pcd_cloud* c, const pcd_normals_options* opts /*NULL = defaults*/,
                                             uint32_t* d_count, double* d_curvature, void* stream);
/* host outputs; count, curvature and info may be NULL */
pcd_status pcd_cloud_estimate_normals(pcd_cloud* c, const pcd_normals_options* opts, uint32_t* count,
                                      double* curvature, pcd_normals_info* info);

/* ------------------------------------------------------------------------
 * Voxel-grid downsampling      replaces the other half of the manual's preparation step (README.md "Preparing point
 *   cloud": "Downsample the point cloud to 3-5cm resolution") and PointCloudProcess::LoadDownsizedMap
 *   (lidar/ply.cc:59-84, pcl::VoxelGrid at a 1 m leaf for the viewer, ui/model_viewer_widget.cc:774-791).
 * The model is pcl::VoxelGrid with downsample_all_data = true.  PCL sums in float in the order of an unstable
 * std::sort, so bit parity with it does not exist; the contract is this definition.
 * Source: ONE handle holding the whole cloud -- a shard of pcd_cloud_create_sharded or a handle with
 * index_stride != 1 / index_base != 0 is refused with PCD_ERR_UNSUPPORTED, its voxels cross handle borders.  The source
 * handle is not modified.  For every finite row p and leaf l[3] (floats, finite, > 0):
 *   inv_a       1.0f / l_a, in float;
 *   voxel       v_a = (int32) floorf(p_a * inv_a): ONE float multiply, not fused, then floor -- a point at -0.01 with
 *               leaf 0.05 lies in voxel -1;
 *   bounds      min_b_a = floorf(bbox_lo_a * inv_a), max_b_a = floorf(bbox_hi_a * inv_a) from the handle's tight bounds
 *               (multiply and floor are monotone: these are the extreme v_a); d_a = max_b_a - min_b_a + 1;
 *   key         (v_0 - min_b_0) + d_0 ((v_1 - min_b_1) + d_1 (v_2 - min_b_2)) as uint64.  Keys above 2^32 are ordinary
 *               (100 m at a 1 cm leaf is 10^12 voxels; PCL gives up at 2^31);
 *   refused     with PCD_ERR_INVALID and no handle created: |bbox * inv| >= 2^31 on any axis; d_0 d_1 d_2 >= 2^63;
 *   Inf rows    (a non-finite coordinate) belong to no voxel.
 * Output rows are the occupied voxels in ascending key (PCL's output order, x fastest).  For voxel V with rows R(V) in
 * ascending source row, k = |R(V)|:
 *   position    float((sum double(p_j)) / k);
 *   normal      s = sum double(n_j); |s| (fp64 norm) not finite or < 1e-12: (0,0,0); else float(s / |s|)  (PCL's
 *               normal accumulator: sum, then normalise).  Rows with a zero normal add nothing; a cloud without normals
 *               stays without them;
 *   sums        fp64, no atomics, in an order that is a function of k and of the rows' order alone -- never of the launch
 *               geometry or of timing; a repeated call is bitwise identical.  The order: the segment is cut into pieces
 *               of 512 rows from its start; in a piece, lane L of 64 adds rows L, L + 64, ... in sequence; the 64 lane
 *               sums (absent rows are +0.0) are added by a butterfly over the lane offsets 8, 16, 32, 1, 2, 4; the pieces
 *               are added in sequence; +0.0 is added to the total (a sum of zeros is +0.0);
 *   min_points  (>= 0) a voxel with k < min_points is dropped [num_dropped_rows counts its rows]; the survivors keep
 *               their key order.
 * row_voxel[i]: the output row of source row i, 0xFFFFFFFF for Inf rows and for rows of dropped voxels -- the map a
 * caller needs to carry colour or intensity along.
 * *out: an ordinary handle on the source's device (index_base 0, stride 1), rows written device to device, index built
 * as pcd_cloud_create builds it; destroy it with pcd_cloud_destroy.  On any failure *out is NULL.
 * BOTH forms synchronise (the _device form synchronises `stream`): the row count sizes the new handle.  The guards
 * of every _device call apply (a capturing stream: PCD_ERR_UNSUPPORTED before anything is allocated).  An empty source,
 * or one with only Inf rows, returns PCD_OK with an empty handle and zero counts.
 * --------------------------------------------------------------------- */
typedef struct {
  float leaf[3];        /* metres, finite and > 0                                          */
  int32_t min_points;   /* >= 0                                                            */
  float cell_size;      /* of the NEW handle, 0 = auto                                     */
  int32_t reserved[8];
} pcd_voxel_options;

typedef struct {
  uint64_t num_input;        /* finite rows                                                */
  uint64_t num_voxels;       /* occupied, before min_points                                */
  uint64_t num_output;
  uint64_t num_dropped_rows;
  int32_t min_b[3], dims[3]; /* dims saturates at INT32_MAX (d_a can reach 2^32)           */
  uint32_t max_points_per_voxel;
  double ms;                 /* device time without the new handle's index build          */
  double build_ms;
} pcd_voxel_info;

void pcd_voxel_options_default(pcd_voxel_options* o);   /* 0.05 x3, 0, 0 */

pcd_status pcd_cloud_voxel_downsample(pcd_cloud* src, const pcd_voxel_options* opts /*NULL = defaults*/,
                                      uint32_t* row_voxel /*[size(src)] host, may be NULL*/,
                                      pcd_cloud** out, pcd_voxel_info* info /*may be NULL*/);

pcd_status pcd_cloud_voxel_downsample_device(pcd_cloud* src, const pcd_voxel_options* opts,
                                             uint32_t* d_row_voxel /*device, may be NULL*/,
                                             void* stream, pcd_cloud** out, pcd_voxel_info* info);

/* ------------------------------------------------------------------------
 * Nearest neighbour                          replaces lidar/kdtree.cc:10-21
 *   Kdtree::GetClosestPoint  (k = 1 pcl::KdTreeFLANN::nearestKSearch,
 *   FLANN L2_Simple<float> on x,y,z; exact)
 * query = (float)q_xyz (lidar/ply.cc:92).  Ties on the float distance go to
 * the lowest index.  found = 0: empty cloud, non-finite query, or nothing
 * closer than FLT_MAX; idx is then 0xFFFFFFFF and sqdist FLT_MAX.
 * --------------------------------------------------------------------- */
typedef enum {
  PCD_NN_AUTO = 0,        /* PCD_NN_GRID for large batches, PCD_NN_FALLBACK_ONLY for small ones (one launch) */
  PCD_NN_BRUTEFORCE = 1,  /* tiled all-pairs kernel: reference for the others */
  PCD_NN_FALLBACK_ONLY = 2,/* per-wavefront hierarchical search for every query */
  PCD_NN_GRID = 3         /* grid kernels (query sort + brick LDS tiles + exact fallback) whatever the batch size */
} pcd_nn_algo;

pcd_status pcd_nn_query(pcd_cloud* c, const double* q_xyz /*[Q][3]*/, uint64_t Q,
                        uint32_t* idx, float* sqdist, uint8_t* found);
pcd_status pcd_nn_query_algo(pcd_cloud* c, const double* q_xyz, uint64_t Q, int algo,
                             uint32_t* idx, float* sqdist, uint8_t* found);

/* Device-resident form.  keys[i] = (uint64)float_bits(sqdist) << 32 | global_idx,
 * PCD_KEY_NONE when nothing was found.  sqdist is a non-negative float, so the
 * unsigned AND the signed 64-bit order of keys equal the (distance, index)
 * order, and PCD_KEY_NONE is the largest value in both: shards of one cloud
 * combine with an element-wise MIN (RCCL ncclMin on ncclUint64 or ncclInt64). */
#define PCD_KEY_NONE 0x7FFFFFFFFFFFFFFFull
pcd_status pcd_nn_query_device(pcd_cloud* c, const double* d_q_xyz, uint64_t Q, int algo,
                               uint64_t* d_keys, void* stream);

/* Second phase of a search over SHARDS of one cloud (spatially compact shards, one per GPU).
 * d_keys comes in holding the best key found so far for every query (from the query's home shard after a
 * cross-rank MIN; PCD_KEY_NONE = nothing yet) and leaves holding min(incoming, this shard's result).  A query is
 * searched here only if it can still improve: not d_skip[i] (may be NULL; e.g. queries whose home is this shard)
 * and the exact float lower bound of its distance to the shard's bounding box does not exceed its incoming
 * distance (an equal distance is searched: a lower index may hide here).  All other entries are left untouched.
 * The element-wise MIN over ranks of the outputs is the exact single-cloud result, ties included. */
pcd_status pcd_nn_refine_device(pcd_cloud* c, const double* d_q_xyz, uint64_t Q, const uint8_t* d_skip,
                                uint64_t* d_keys, void* stream);

/* ------------------------------------------------------------------------
 * Plane association                          replaces the three serial loops
 *   optim/bundle_adjustment.cc:358-410  BundleAdjustmentConfig::MatchClosestLidarPoint   (PCD_GATE_MAPPER_LOCAL)
 *   sfm/incremental_mapper.cc:1413-1469 IncrementalMapper::AdjustGlobalBundleByLidar     (PCD_GATE_MAPPER_GLOBAL)
 *   controllers/bundle_adjustment.cc:130-185 BundleAdjustmentController::Run             (PCD_GATE_CONTROLLER)
 * each of which does: lidar/ply.cc:90-107 SearchNearestNeiborByKdtree ->
 * lidar/lidar_point.cc:5-50 LidarPoint(l_pt, plane) / Normalize ->
 * classification on the raw normal -> range gate.
 * --------------------------------------------------------------------- */
typedef enum { PCD_GATE_MAPPER_LOCAL = 0, PCD_GATE_MAPPER_GLOBAL = 1, PCD_GATE_CONTROLLER = 2 } pcd_gate_mode;
typedef enum { PCD_LIDAR_NONE = 0, PCD_LIDAR_ICP = 1, PCD_LIDAR_ICP_GROUND = 2 } pcd_lidar_type;
/* OR-ed into gate_mode: bound the search by the gate.  All three call sites drop an association whose
 * point-to-point distance exceeds max_range (mapper) / 2 m (controller), so no neighbour beyond that distance can be
 * recorded; with this flag the search prunes there (exact inside the bound), the set of recorded associations and
 * every field of their rows are identical, and rows with type 0 carry zeros / 0xFFFFFFFF instead of the rejected
 * winner: in bounded mode nn_idx / nn_sqdist are DEFINED ONLY FOR ACCEPTED ASSOCIATIONS (type != 0) -- a query whose
 * gate rejects it reports 0xFFFFFFFF / FLT_MAX, not its true nearest neighbour.  Ignored when keys are passed in.
 * pcd_associate_staged always searches this way (it returns only the recorded associations; the flag is accepted
 * and redundant there); pcd_nn_query* is never bounded. */
#define PCD_GATE_BOUNDED_SEARCH 0x100

typedef struct {
  double* lidar_xyz;   /* [Q][3] LidarPoint::LidarXYZ()  (winner position as doubles)        */
  double* abcd;        /* [Q][4] LidarPoint::LidarABCD() after Normalize()                   */
  uint8_t* type;       /* [Q]    pcd_lidar_type; 0 = the reference records no LidarPoint     */
  double* dist;        /* [Q]    point-to-point distance (SetDist at bundle_adjustment.cc:403) */
  double* angle;       /* [Q]    ComputeAngle (SetAngle at :404)                              */
  double* dist2plane;  /* [Q]    ComputeDist, may be NULL                                     */
  uint32_t* nn_idx;    /* [Q]    winner index, may be NULL                                    */
  float* nn_sqdist;    /* [Q]    may be NULL                                                  */
} pcd_assoc_out;

/* max_range: Q entries (per-point schedule, sfm/incremental_mapper.cc:1159-1163) or
 * one entry broadcast when max_range_count == 1; ignored for PCD_GATE_CONTROLLER. */
pcd_status pcd_associate(pcd_cloud* c, const double* q_xyz, uint64_t Q, const double* max_range,
                         uint64_t max_range_count, int gate_mode, const pcd_assoc_out* out);

/* Staged host form for the call sites (the drop-in's PCIe path): inputs and results live in PINNED host memory
 * owned by the cloud handle, and only the associations the reference would have recorded come back, as one
 * 80-byte record each, in ascending query order:
 *   pcd_assoc_staging   pinned input buffers for Q queries (valid until the next staging call or destroy); the
 *                       caller gathers Point3D::XYZ() / the range schedule straight into them
 *   pcd_associate_staged  H2D (24 B / query) -> search + epilogue -> device-side compaction of type != 0 ->
 *                       D2H of num_hits records; *hits points into pinned memory valid until the next call
 * (pcd_associate with caller-owned pageable arrays of 89 B / query stays for convenience: it is PCIe- and
 * staging-copy-bound, about 10x the device time.) */
typedef struct {
  double lidar_xyz[3];   /* LidarPoint::LidarXYZ()                    */
  double abcd[4];        /* LidarPoint::LidarABCD() after Normalize() */
  double dist, angle;    /* SetDist / SetAngle                        */
  uint32_t query;        /* row of q_xyz this association belongs to  */
  uint8_t type;          /* PCD_LIDAR_ICP | PCD_LIDAR_ICP_GROUND      */
  uint8_t pad[3];
} pcd_assoc_hit;
pcd_status pcd_assoc_staging(pcd_cloud* c, uint64_t Q, double** q_xyz /*[Q][3]*/, double** max_range /*[Q]*/);
pcd_status pcd_associate_staged(pcd_cloud* c, uint64_t Q, uint64_t max_range_count, int gate_mode,
                                const pcd_assoc_hit** hits, uint64_t* num_hits);

/* Device form: every pointer in `out` and d_q_xyz / d_max_range are device
 * pointers.  d_keys_in == NULL: run the search; otherwise use these keys
 * (e.g. after a cross-rank MIN) and skip the search.  On a sharded cloud
 * (index_stride != 1 or index_base != 0) a key whose index this shard does not
 * own yields type 0 here: the owner associates it, or use the payload path. */
pcd_status pcd_associate_device(pcd_cloud* c, const double* d_q_xyz, uint64_t Q, const double* d_max_range,
                                uint64_t max_range_count, int gate_mode, const uint64_t* d_keys_in,
                                const pcd_assoc_out* d_out, void* stream);

/* Sharded clouds: after the MIN over ranks each rank fills winner (xyz, normal)
 * for the keys it owns and zeros elsewhere: d_payload [Q][6] floats as int32 bit
 * patterns, so that a SUM over ranks reassembles them bit-exactly.
 * pcd_associate_from_payload_device then runs the epilogue on any rank. */
pcd_status pcd_nn_winner_payload_device(pcd_cloud* c, const uint64_t* d_keys, uint64_t Q,
                                        int32_t* d_payload, void* stream);
pcd_status pcd_associate_from_payload_device(int device, const double* d_q_xyz, uint64_t Q,
                                             const double* d_max_range, uint64_t max_range_count,
                                             int gate_mode, const uint64_t* d_keys, const int32_t* d_payload,
                                             const pcd_assoc_out* d_out, void* stream);

/* Post-BA outlier filter of the associations       replaces base/reconstruction.cc:771-805
 *   Reconstruction::FilterLidarOutlier: erase[i] = 1 when ||lidar_xyz[i] - points_xyz[i]|| exceeds
 *   max_proj_dist_error (type PCD_LIDAR_PROJ) or max_icp_dist_error (Icp / IcpGround); type 0 rows are
 *   left alone.  Device pointers (the arrays normally still live in HBM after BA). */
#define PCD_LIDAR_PROJ 3   /* LidarPointType::Proj: depth-projection associations (pcd_proj_*) */
pcd_status pcd_filter_lidar_outlier_device(int device, const double* d_points_xyz, const double* d_lidar_xyz,
                                           const uint8_t* d_type, uint64_t n, double max_proj_dist_error,
                                           double max_icp_dist_error, uint8_t* d_erase, void* stream);

/* ------------------------------------------------------------------------
 * Sharded cloud (pcd_cloud_create_sharded above): search and association
 * --------------------------------------------------------------------- */
/* The exchange steps of the sharded search are reductions over the shards' device buffers: buf[s] lives on
 * devices[s]; on return EVERY buf[s] must hold the element-wise result.  A C++ host plugs RCCL here
 * (ncclGroupStart; ncclAllReduce(buf[s], buf[s], count, ncclUint64, ncclMin, comm[s], 0) per shard; ncclGroupEnd),
 * tests an in-process loop.  NULL callbacks (or a NULL pcd_shard_reduce): the library reduces with peer copies to the
 * first shard's device.  All devices are idle (synchronised) when a callback is entered; return 0 for success. */
typedef struct {
  int (*min_u64)(void* user, uint64_t* const* buf, const int* devices, int nshards, uint64_t count);
  int (*sum_i32)(void* user, int32_t* const* buf, const int* devices, int nshards, uint64_t count);
  void* user;
} pcd_shard_reduce;

/* pcd_nn_query / pcd_associate over the shards: home-shard search, MIN over shards, refinement of the queries a foreign
 * shard's bounding box cannot rule out, MIN again (+ the winners' rows from their owners, SUM over shards). */
pcd_status pcd_nn_query_sharded(pcd_cloud_shards* s, const double* q_xyz, uint64_t Q, const pcd_shard_reduce* red,
                                uint32_t* idx, float* sqdist, uint8_t* found);
pcd_status pcd_associate_sharded(pcd_cloud_shards* s, const double* q_xyz, uint64_t Q, const double* max_range,
                                 uint64_t max_range_count, int gate_mode, const pcd_shard_reduce* red,
                                 const pcd_assoc_out* out);

/* ------------------------------------------------------------------------
 * Depth-projection association (LidarPointType::Proj)   replaces lidar/pcd_projection.{h,cc} `PcdProj`
 *   pcd_proj_create          <- PcdProj::PcdProj + BuildSubMap          pcd_projection.h:52, .cc:223-255
 *   pcd_proj_set_new_images  <- both PcdProj::SetNewImage overloads     .cc:13-89, .cc:102-220
 *                               (SearchSubMap .cc:258-297, SearchImageMap .cc:499-559,
 *                                ImageMapProj .cc:305-468, DistortOpenCV .cc:561-594), for a batch of images.
 * The winner of a feature pixel is the LiDAR point with the smallest float camera-frame norm among the points
 * whose splat covers the pixel; equal norms resolve to the point the reference's single-thread walk meets first
 * (submap key order, then cloud row) -- the reference's OpenMP loop is racy there, this is deterministic.
 * The cloud handle must outlive the projector and must hold the whole cloud (no shard).
 * --------------------------------------------------------------------- */
typedef struct pcd_proj pcd_proj;
typedef struct {                 /* lidar/pcd_projection.h:31-47, numeric members */
  double depth_image_scale;      /* 0.2 */
  int32_t max_proj_scale;        /* 10  */
  int32_t min_proj_scale;        /* 2   */
  double min_proj_dist;          /* 2   */
  float submap_length;           /* x, 1.0 */
  float submap_width;            /* z, 1.0 */
  float submap_height;           /* y, 1.0 */
  float choose_meter;            /* 40  */
  double min_lidar_proj_dist;    /* no default in the reference; controllers/incremental_mapper.cc:345 */
} pcd_proj_options;
typedef struct {
  double qvec[4], tvec[3];       /* Image::Qvec (w,x,y,z; used un-normalised as the reference does), Tvec */
  double params[8];              /* fx fy cx cy k1 k2 p1 p2: the reference reads an OPENCV camera
                                    unconditionally (.cc:21, .cc:561-571); zero-fill what a model lacks */
  uint64_t width, height;        /* Camera::Width / Height (full resolution) */
  uint64_t feat_begin, feat_end; /* this image's rows of feat_xy */
} pcd_proj_image;
void pcd_proj_default_options(pcd_proj_options* o);
pcd_status pcd_proj_create(pcd_cloud* cloud, const pcd_proj_options* options, pcd_proj** out);
void pcd_proj_destroy(pcd_proj* p);
uint64_t pcd_proj_num_submaps(const pcd_proj* p);
/* (image, submap) pairs the last call projected, summed over its chunks.  A chunk in which no image has a feature
 * is not culled at all (nobody would read the result) and adds 0, so a featureless batch reports 0. */
uint64_t pcd_proj_last_pairs(const pcd_proj* p);
/* The splat half-width beyond min_proj_dist is a_x*depth+b_x (and y): four function-local `static`s in the
 * reference (.cc:391-397), initialised from the FIRST camera the process projects with and never again.
 * Here they latch per projector on the first image of the first call; set=1 overrides them (coeffs4 = a_x, b_x,
 * a_y, b_y), set=0 reads them back.  *latched (optional) reports whether they are fixed yet. */
pcd_status pcd_proj_scale_coeffs(pcd_proj* p, int set, double* coeffs4, int* latched);
/* Host buffers.  feat_xy: [n_feat][2] full-resolution pixel coordinates (for overload #1 pass the Point2D's that
 * have a 3D point; for #2 every pt_xy).  Any output may be NULL:
 *   found[n_feat]        1 when a LiDAR point was matched (pt_xy.second of overload #2)
 *   lidar_index[n_feat]  cloud row of the winner (0xFFFFFFFF when none), dist[n_feat] its float norm
 *   lidar6[n_feat][6]    overload #1 value: x y z nx ny nz as doubles (zeros when none)
 *   cam_xyz[n_feat][3]   overload #2 value: pixel ray intersected with the winner's plane (zeros when none) */
pcd_status pcd_proj_set_new_images(pcd_proj* p, uint64_t n_images, const pcd_proj_image* images, uint64_t n_feat,
                                   const double* feat_xy, uint8_t* found, uint32_t* lidar_index, float* dist,
                                   double* lidar6, double* cam_xyz);
/* The same call with the features and every output in device memory (each output may be NULL) and all work on
 * `stream`: the same winner rule, coefficient latch, chunking and pcd_proj_last_pairs.  `images` stays a host array
 * (the poses size nothing, but the image sizes lay the buffers out).  Guards as every _device call: NULL / a bad
 * feature range / a zero focal length -> INVALID; no gfx950 -> NO_DEVICE; a capturing stream -> UNSUPPORTED before
 * anything is allocated.  Synchronises `stream` once, at the end (the pair counts of pcd_proj_last_pairs).  The host
 * form is a wrapper over the same launcher. */
pcd_status pcd_proj_set_new_images_device(pcd_proj* p, uint64_t n_images, const pcd_proj_image* images /*host*/,
                                          uint64_t n_feat, const double* d_feat_xy, uint8_t* d_found,
                                          uint32_t* d_lidar_index, float* d_dist, double* d_lidar6, double* d_cam_xyz,
                                          void* stream);

/* search-radius schedule, sfm/incremental_mapper.cc:1159-1163, 1423-1427 */
pcd_status pcd_search_range_schedule(const int32_t* global_opt_num, uint64_t n, double kd_max,
                                     double kd_min, double drop_speed, double* out);

/* ------------------------------------------------------------------------
 * Bundle-adjustment residual / Jacobian evaluation
 *   replaces what ceres::Solve calls per iteration on the problem built by
 *   optim/bundle_adjustment.cc:694-1131: for every residual block
 *   ceres::CostFunction::Evaluate(parameters, residuals, jacobians) of
 *     base/cost_functions.h:49-141   BundleAdjustmentCostFunction<Model>            (variable pose)
 *     base/cost_functions.h:256-370  BundleAdjustmentConstantPoseCostFunction<Model>
 *     base/cost_functions.h:150-241  BundleAdjustmentLidarCostFunction
 *   with base/camera_models.h WorldToImage of the 11 models, followed by the
 *   loss correction (optim/bundle_adjustment.cc:53-68) and the quaternion /
 *   subset manifolds (base/cost_functions.h:610-627).
 * --------------------------------------------------------------------- */
typedef struct pcd_ba pcd_ba;

typedef enum { PCD_LOSS_TRIVIAL = 0, PCD_LOSS_SOFT_L1 = 1, PCD_LOSS_CAUCHY = 2 } pcd_loss_type;

/* model ids = CameraModel::kModelId, base/camera_models.h:187-347 */
typedef enum {
  PCD_CAM_SIMPLE_PINHOLE = 0, PCD_CAM_PINHOLE = 1, PCD_CAM_SIMPLE_RADIAL = 2, PCD_CAM_RADIAL = 3,
  PCD_CAM_OPENCV = 4, PCD_CAM_OPENCV_FISHEYE = 5, PCD_CAM_FULL_OPENCV = 6, PCD_CAM_FOV = 7,
  PCD_CAM_SIMPLE_RADIAL_FISHEYE = 8, PCD_CAM_RADIAL_FISHEYE = 9, PCD_CAM_THIN_PRISM_FISHEYE = 10
} pcd_camera_model;
int pcd_camera_num_params(int model_id);   /* -1 for an unknown id */
/* Parameter groups of a model (base/camera_models.h FocalLengthIdxs / PrincipalPointIdxs / ExtraParamsIdxs):
 * group[k] = 0 focal length, 1 principal point, 2 extra (distortion) parameter, for k < num_params.
 * BundleAdjuster::ParameterizeCameras (optim/bundle_adjustment.cc:1047-1100) holds a group constant unless
 * refine_focal_length / refine_principal_point / refine_extra_params is set. */
pcd_status pcd_camera_param_groups(int model_id, uint8_t* group /*[num_params]*/);

/* Flat problem description (all host pointers, copied at create).
 * It is what BundleAdjuster::SetUp*ByLidar assembles block by block:
 *   cameras  <- Camera::ParamsData()            optim/bundle_adjustment.cc:828
 *   images   <- Image::Qvec()/Tvec()            :825-826   (qw qx qy qz tx ty tz)
 *   points   <- Point3D::XYZ()                  :894
 *   obs      <- one per AddResidualBlock of a reprojection functor :875,:893,:982
 *   lidar    <- one per AddLidarToProblem       :993-1040 (abcd NaN rows must be dropped by the caller
 *               exactly as :1005-1009 does; weight chosen by type :1013-1028)
 * image_const_pose[i] = !refine_extrinsics || HasConstantPose(i) (:831) or the
 * image is outside the config (:967-983): such blocks use the constant-pose functor.
 * image_const_tvec[i] bit k = tvec[k] held constant (SetSubsetManifold :912-915).
 * point_const[p] = ParameterizePoints (:1107-1131).
 * camera_refine = what ParameterizeCameras (:1047-1100) decides: one byte per entry of cam_params, 1 = the
 * parameter is optimised, 0 = held constant (SetParameterBlockConstant for a whole camera, SubsetManifold for
 * part of one).  NULL = all intrinsics constant (this fork's default, ba_refine_* = false,
 * controllers/incremental_mapper.h:156-158): the camera outputs of pcd_ba_out are then zero. */
typedef struct {
  int32_t device;
  int32_t num_cameras;
  const int32_t* cam_model;        /* [C]                        */
  const int32_t* cam_param_offset; /* [C] start in cam_params    */
  const double* cam_params;        /* packed                     */
  uint64_t cam_params_len;
  int32_t num_images;
  const double* poses;             /* [I][7]                     */
  const int32_t* image_camera;     /* [I]                        */
  const uint8_t* image_const_pose; /* [I] or NULL (all variable) */
  const uint8_t* image_const_tvec; /* [I] or NULL                */
  int32_t num_points;
  const double* points;            /* [P][3]                     */
  const uint8_t* point_const;      /* [P] or NULL                */
  uint64_t num_obs;
  const int32_t* obs_image;        /* [O]                        */
  const int32_t* obs_point;        /* [O]                        */
  const double* obs_xy;            /* [O][2]                     */
  uint64_t num_lidar;
  const int32_t* lidar_point;      /* [L]                        */
  const double* lidar_abcd;        /* [L][4]                     */
  const double* lidar_weight;      /* [L]                        */
  int32_t loss_type;               /* pcd_loss_type              */
  double loss_scale;
  const uint8_t* camera_refine;    /* [cam_params_len] or NULL   */
  int32_t reserved[8];
} pcd_ba_desc;

pcd_status pcd_ba_create(const pcd_ba_desc* desc, pcd_ba** out);
void pcd_ba_destroy(pcd_ba* ba);

/* parameter update between iterations (host -> device); NULL keeps the old values */
pcd_status pcd_ba_set_parameters(pcd_ba* ba, const double* poses /*[I][7]*/, const double* points /*[P][3]*/);
/* refined intrinsics: the camera parameter blocks change between iterations too (same layout as desc.cam_params) */
pcd_status pcd_ba_set_camera_parameters(pcd_ba* ba, const double* cam_params /*[cam_params_len]*/);

/* Outputs of one evaluation; every pointer may be NULL (not computed / not copied).
 * Raw blocks are exactly what each CostFunction::Evaluate hands to Ceres
 * (row-major num_residuals x block_size, ambient quaternion size 4):
 *   residuals [2*O + L]   obs blocks first, then lidar blocks
 *   jac_q [O][2][4]  jac_t [O][2][3]  jac_X [O][2][3]   (zero rows for constant-pose blocks)
 *   jac_lidar [L][3]
 *   jac_cam [O][2][PCD_CAM_JAC_STRIDE]   the camera-parameter block (2 x K row-major in the first K columns of
 *             each row, K = pcd_camera_num_params(model), remaining columns zero): what autodiff returns when
 *             refine_focal_length / refine_principal_point / refine_extra_params (optim/bundle_adjustment.h:76-81)
 *             leave the camera block variable; Ceres applies its SubsetManifold for the constant subset itself.
 * Normal-equation blocks use the loss-corrected residuals/Jacobians projected on
 * the manifolds (pose tangent = 3 quaternion-tangent + 3 tvec):
 *   H_img [I][6][6] g_img [I][6]   H_pt [P][3][3] g_pt [P][3]   W [O][6][3] = Jp^T JX */
#define PCD_CAM_JAC_STRIDE 12   /* widest camera model (FULL_OPENCV, THIN_PRISM_FISHEYE) */
typedef struct {
  double* cost;        /* [1]  1/2 sum rho(||r_block||^2).  Fixed-order sums, no atomics: bitwise reproducible
                          run to run.  Requested without H_pt / g_pt it is summed per observation (the cheap
                          LM trial-step pass), with them per track: the two agree up to summation order. */
  double* residuals;
  double* jac_q;
  double* jac_t;
  double* jac_X;
  double* jac_lidar;
  double* H_img;
  double* g_img;
  double* H_pt;
  double* g_pt;
  double* W;
  double* jac_cam;     /* [O][2][PCD_CAM_JAC_STRIDE] d r / d camera params, see above */
  /* Camera blocks of the normal equations (refined intrinsics, desc.camera_refine): loss-corrected, columns of
   * constant parameters zero, S = PCD_CAM_JAC_STRIDE rows / columns per camera (entries >= K zero):
   *   H_cam [C][S][S] = sum Jc^T Jc    g_cam [C][S] = sum Jc^T r      over the observations of the camera's images
   *   E_cam [I][S][6] = sum Jc^T Jp    camera x pose-tangent coupling of each image (an image has one camera)
   *   W_cam [O][S][3] = Jc^T JX        camera x point coupling of each observation
   * Together with H_img, g_img, H_pt, g_pt, W this is the full J^T J / J^T r of the problem in block form. */
  double* H_cam;
  double* g_cam;
  double* E_cam;
  double* W_cam;
} pcd_ba_out;

pcd_status pcd_ba_evaluate(pcd_ba* ba, const pcd_ba_out* out);                 /* host outputs   */

/* Post-BA filters reduced PER TRACK on the device, from the parameters resident after BA:
 *   Reconstruction::FilterPoints3DWithLargeReprojectionError   base/reconstruction.cc:1662-1712
 *   Reconstruction::FilterObservationsWithNegativeDepth        base/reconstruction.cc:837-855
 *   Reconstruction::ComputeMeanReprojectionError               base/reconstruction.cc:906-921
 * A track = all observations of a point in this problem (AddPointToProblem adds the observations from images outside
 * the config too, optim/bundle_adjustment.cc:927-985, so for the points of a BA config that is the whole track).
 * Per point: track shorter than 2 -> deleted; an element whose squared error (normalised quaternion, DBL_MAX behind
 * the camera, base/projection.cc:104-117) exceeds max_reproj_error^2 is erased; if at most one element would survive
 * the point is deleted with all its elements; otherwise Point3D::SetError(sum of sqrt(error) of the kept elements /
 * their number).  Sums run in ascending observation index.  Every pointer may be NULL.  The erase / bookkeeping on
 * the Reconstruction itself stays with the caller. */
typedef struct {
  uint8_t* obs_erase;            /* [O] 1: DeleteObservation (or its point is deleted)                       */
  uint8_t* obs_negative_depth;   /* [O] 1: !HasPointPositiveDepth (depth < eps)                              */
  uint8_t* point_delete;         /* [P] 1: DeletePoint3D                                                     */
  double* point_error;           /* [P] Point3D::Error() after the filter; -1 = HasError() false (deleted)   */
  double* summary;               /* [4] num_filtered (the function's return value), mean reprojection error  */
                                 /*     over the points with an error (0 if none), number of such points,     */
                                 /*     number of observations with negative depth                            */
} pcd_ba_filter_out;
pcd_status pcd_ba_filter_tracks_device(pcd_ba* ba, double max_reproj_error, const pcd_ba_filter_out* d_out, void* stream);
pcd_status pcd_ba_filter_tracks(pcd_ba* ba, double max_reproj_error, const pcd_ba_filter_out* out);   /* host outputs */

/* Reconstruction::FilterPoints3D (base/reconstruction.cc:760-769) on the device: the filter above, then
 * FilterPoints3DWithSmallTriangulationAngle (:1600-1660) on what it left.
 *   Stage 1 is pcd_ba_filter_tracks_device with max_reproj_error: every output has its bits.
 *   Stage 2 runs for every point stage 1 did not delete, on its surviving elements (obs_erase == 0) in ascending
 *   observation index, pairs (i1, i2 < i1) in the reference's loop order.  The projection centre of an image is
 *   ProjectionCenterFromPose (base/pose.cc:164-171) of the handle's CURRENT pose: the normalised quaternion, conjugated,
 *   applied to -tvec (a zero quaternion counts as the identity, as in pcd_ba_observation_errors).  The angle is
 *   CalculateTriangulationAngle (base/triangulation.cc:122-145): squared norms, denominator == 0 gives 0, acos, abs,
 *   min(angle, pi - angle).  The point is kept as soon as one pair reaches DegToRad(min_tri_angle_deg); a NaN angle (the
 *   acos argument outside [-1, 1] by rounding) keeps nothing.
 *   A point stage 2 does not keep is deleted: point_delete = 1, obs_erase = 1 for all its observations, point_error =
 *   -1; summary[0] grows by 1 PER SUCH POINT (the reference counts points here, elements in stage 1), summary[1..2]
 *   lose the point's error, summary[3] is unchanged.  The summary is a fixed-order reduction: a repeated call is
 *   bitwise identical.
 * min_tri_angle_deg <= 0 (or NaN): stage 1 alone.  Every output pointer may be NULL.
 * There is no point-subset argument (FilterPoints3D takes an id set): the call filters every point; a caller who wants
 * a subset masks obs_erase / point_delete before applying them (pcd_ba_remove_observations_device). */
typedef struct {
  double max_reproj_error;     /* as pcd_ba_filter_tracks */
  double min_tri_angle_deg;    /* degrees, converted as DegToRad does; <= 0 keeps every point the first filter kept */
  int32_t reserved[8];
} pcd_ba_filter_opts;
void pcd_ba_filter_opts_default(pcd_ba_filter_opts* opts);   /* 8.0, 1.5: sfm/incremental_mapper.h:131,135 */
pcd_status pcd_ba_filter_points_device(pcd_ba* ba, const pcd_ba_filter_opts* opts, const pcd_ba_filter_out* d_out, void* stream);
pcd_status pcd_ba_filter_points(pcd_ba* ba, const pcd_ba_filter_opts* opts, const pcd_ba_filter_out* out);   /* host outputs */

/* The Ceres route (optim/bundle_adjustment.cc:858-893, :967-983, :1031-1037: every residual block's Evaluate copies
 * its rows): the raw blocks of ALL residual blocks land in PINNED host buffers owned by the handle -- one device pass,
 * then one asynchronous copy per array at the pinned PCIe rate instead of pcd_ba_evaluate's synchronous copies into
 * the caller's pageable memory.  Constant-pose blocks (the reference's BundleAdjustmentConstantPoseCostFunction has
 * no pose parameter blocks) carry no pose Jacobians: jac_q / jac_t hold one row per VARIABLE-pose observation, packed
 * on the device, and pose_row[o] is observation o's row (0xFFFFFFFF: none).  The pointers stay valid until the next
 * pcd_ba_evaluate_blocks / pcd_ba_destroy on the handle. */
typedef struct {
  const double* residuals;   /* [2*O + L]                                                       */
  const double* jac_q;       /* [num_pose_rows][2][4]   NULL when want_jacobians == 0           */
  const double* jac_t;       /* [num_pose_rows][2][3]                                           */
  const double* jac_X;       /* [O][2][3]                                                       */
  const double* jac_lidar;   /* [L][3]                                                          */
  const double* jac_cam;     /* [O][2][PCD_CAM_JAC_STRIDE] or NULL (want_jac_cam == 0)          */
  const uint32_t* pose_row;  /* [O] host array (fixed at pcd_ba_create)                         */
  uint64_t num_pose_rows;
  uint64_t bytes_d2h;        /* bytes that crossed PCIe device -> host in this call             */
} pcd_ba_blocks;
pcd_status pcd_ba_evaluate_blocks(pcd_ba* ba, int want_jacobians, int want_jac_cam, pcd_ba_blocks* out);
/* The same route at 64 B instead of 176 B per reprojection block over PCIe.  With want_jacobians the reprojection
 * blocks arrive as one record of 8 doubles per observation, in the caller's observation order:
 *   records[o] = {r0, r1, M00, M01, M02, M10, M11, M12},   M = d r / d P (2x3 row-major), P = R(q) X + t.
 * Every Jacobian block is M times a factor of the evaluation point alone, which the caller already holds:
 *   jac_t = M     jac_X = M * D(q)     jac_q = M * dPdq(q, X)
 * with D = dP/dX (3x3) and dPdq = dP/dq (3x4) of Ceres' UnitQuaternionRotatePoint polynomial, q taken as it is (not
 * normalised).  shim/ceres_compact.h rebuilds the three blocks in the operation order of the device code, so they are
 * the rows pcd_ba_evaluate_blocks returns.  M of a CONSTANT-POSE block is not zero: the block has no pose Jacobians,
 * but its jac_X is M * D(q of the constant pose).  There is no pose_row: records are not packed.
 * jac_cam rows have cam_stride columns, cam_stride = the largest pcd_camera_num_params over the handle's cameras;
 * columns >= K of a narrower camera are zero.  Otherwise the contract of pcd_ba_evaluate_blocks: one device pass, one
 * asynchronous copy per array into the handle's pinned buffer (shared with pcd_ba_evaluate_blocks), one stream
 * synchronisation; pointers valid until the next pcd_ba_evaluate_blocks* / pcd_ba_destroy on the handle;
 * PCD_ERR_NO_DEVICE without a gfx950.  bytes_d2h = 8 (2 O + L) without Jacobians, else
 * 8 (8 O + 4 L) + (want_jac_cam ? 16 cam_stride O : 0). */
typedef struct {
  const double* residuals;        /* [2*O]  only when want_jacobians == 0, else NULL            */
  const double* records;          /* [O][8] {r0,r1,M row-major 2x3}, only when want_jacobians   */
  const double* lidar_residuals;  /* [L]                                                        */
  const double* jac_lidar;        /* [L][3] or NULL                                             */
  const double* jac_cam;          /* [O][2][cam_stride] or NULL                                 */
  int32_t cam_stride;
  uint64_t bytes_d2h;
} pcd_ba_blocks_compact;
pcd_status pcd_ba_evaluate_blocks_compact(pcd_ba* ba, int want_jacobians, int want_jac_cam,
                                          pcd_ba_blocks_compact* out);
pcd_status pcd_ba_evaluate_device(pcd_ba* ba, const pcd_ba_out* d_out, void* stream);  /* device outputs */
/* Inputs of the post-BA filters, per observation (either pointer may be NULL):
 *   sq_err[o] = CalculateSquaredReprojectionError (base/projection.cc:104-117), DBL_MAX when the point is not
 *               in front of the camera -- what FilterPoints3DWithLargeReprojectionError
 *               (base/reconstruction.cc:1662-1700) and ComputeMeanReprojectionError (:906) consume;
 *   depth[o]  = z of the point in the camera frame -- FilterObservationsWithNegativeDepth (:837-855) deletes
 *               observations with depth < DBL_EPSILON. */
pcd_status pcd_ba_observation_errors(pcd_ba* ba, double* sq_err /*[O]*/, double* depth /*[O]*/);
pcd_status pcd_ba_observation_errors_device(pcd_ba* ba, double* d_sq_err, double* d_depth, void* stream);
/* device-side parameter pointers for zero-copy updates: [I][7] and [P][3] doubles */
pcd_status pcd_ba_device_parameters(pcd_ba* ba, double** d_poses, double** d_points);
/* device -> device parameter update on `stream` (NULL keeps the old values).  Invalidates nothing: a Schur state of the
 * old parameters stays readable, and ordering it against the update is the caller's business.
 * pcd_ba_window_commit_device, which also writes parameters, differs there: it drops the source's Schur state. */
pcd_status pcd_ba_set_parameters_device(pcd_ba* ba, const double* d_poses, const double* d_points, void* stream);

/* Point elimination on the device: one Levenberg-Marquardt step of the normal equations without the
 * per-observation blocks leaving HBM.  Unknowns: the 6-dim pose tangents (3 quaternion-tangent + 3 tvec, the manifold
 * of H_img) of the variable-pose images -- "slots", numbered in ascending image index -- then the 3-dim points.  The
 * step solves (H + D) delta = -g with D on the pose and point diagonals:
 *   PCD_DAMP_MARQUARDT  D_kk = mu * clamp(H_kk, 1e-6, 1e32)   (Ceres' LM form, mu = 1 / radius)
 *   PCD_DAMP_LEVENBERG  D_kk = mu
 * Every non-constant point is eliminated: V_p = H_pt[p] + D_p through a 3x3 Cholesky; a point whose V_p is not
 * numerically positive definite is skipped -- delta 0, no contribution -- and counted.  The test is scale-invariant:
 * V_00 > 0 and Cholesky pivot k > 1e-10 V_kk (the pivots of the unit-diagonal, Jacobi-scaled V exceed 1e-10), so a
 * rank-deficient V_p (one observation and no LiDAR term, or LiDAR terms only, at mu = 0 or a tiny mu) is skipped
 * whatever the rounding of H_pt.  Reduced system:
 *   S_ij  = delta_ij (U_i + D_i) - sum_p sum_{a in p,i; b in p,j} W_a V_p^-1 W_b^T
 *   rhs_i = -g_i + sum_{a in i} W_a V_p(a)^-1 g_p(a)
 * Constant-pose images have no slot; constant-tvec components are inactive (identity rows / columns of S, rhs 0,
 * delta 0); constant points get delta 0.  No atomics, fixed-order sums: bitwise reproducible run to run.
 * Guards of every entry point below, before anything is allocated or launched: no gfx950 device -> NO_DEVICE; a
 * capturing stream -> UNSUPPORTED (as every _device call); a handle with some camera_refine byte set -> UNSUPPORTED
 * (the camera rows are not part of the reduced system).  All scratch is owned by the handle (freed by
 * pcd_ba_destroy); the co-visibility structure is built on the first call and again after an edit dropped it, on the
 * device and on the stream of the call that needs it (the host forms: the legacy stream; build_ms). */
typedef enum { PCD_DAMP_MARQUARDT = 0, PCD_DAMP_LEVENBERG = 1 } pcd_ba_damping;
typedef struct {
  double mu;          /* >= 0 */
  int32_t damping;    /* pcd_ba_damping */
  int32_t reserved[7];
} pcd_ba_schur_opts;
/* every pointer may be NULL (not written); ns = num_slots, n = 6 ns */
typedef struct {
  double* cost;            /* [1] cost at the current parameters (per-track sum, as pcd_ba_evaluate with H_pt) */
  double* S_diag;          /* [ns][6][6]                                                                       */
  double* S_off;           /* [num_pairs][6][6] block (pair_i[q], pair_j[q]), pair_i < pair_j                   */
  double* rhs;             /* [ns][6]                                                                          */
  double* S;               /* [n][n] dense, row-major, both triangles (for a direct Cholesky:                 */
                           /* pcd_ba_schur_solve_cholesky* below reads its lower triangle)                     */
  uint64_t* num_skipped;   /* [1] eliminated points skipped by the pivot test above (V_p numerically singular) */
} pcd_ba_schur_out;
/* Co-visibility structure (host query): image_slot [I] (-1 = constant pose), the number of slots, and the slot pairs
 * i < j that share an eliminated point, ascending (i, j).  Every output may be NULL (size the buffers first). */
pcd_status pcd_ba_schur_structure(pcd_ba* ba, int32_t* image_slot, int32_t* num_slots, uint64_t* num_pairs,
                                  int32_t* pair_i, int32_t* pair_j);
/* Normal-equation pass at the current parameters into handle scratch, then the elimination. */
pcd_status pcd_ba_schur_device(pcd_ba* ba, const pcd_ba_schur_opts* opts, const pcd_ba_schur_out* d_out, void* stream);
pcd_status pcd_ba_schur(pcd_ba* ba, const pcd_ba_schur_opts* opts, const pcd_ba_schur_out* out);   /* host outputs */
/* delta X_p = -V_p^-1 (g_p + sum_{a in p} W_a^T dpose[slot(a)]) from the state of the last Schur call (INVALID
 * without one); d_dpoint [P][3] (0 for constant / skipped points).  d_model_decrease (may be NULL): [1]
 * 1/2 (-delta^T g + delta^T D delta), the decrease of the LM model, summed in a fixed order.  d_dpose may be NULL
 * when ns = 0 (every pose constant). */
pcd_status pcd_ba_schur_back_substitute_device(pcd_ba* ba, const double* d_dpose /*[ns][6]*/, double* d_dpoint,
                                               double* d_model_decrease, void* stream);
/* Candidate parameters: Ceres' QuaternionManifold::Plus on the quaternion, t + dt on the variable tvec components,
 * X + dX on the non-constant points, copies of everything constant.  Reads the handle's current parameters; the
 * outputs may be the handle's own buffers (pcd_ba_device_parameters).  d_dpose may be NULL when ns = 0. */
pcd_status pcd_ba_plus_device(pcd_ba* ba, const double* d_dpose /*[ns][6]*/, const double* d_dpoint /*[P][3]*/,
                              double* d_poses_out /*[I][7]*/, double* d_points_out /*[P][3]*/, void* stream);
typedef struct {
  double build_ms;          /* wall time of the structure build (0: not built yet) */
  uint64_t num_entries;     /* (a, b) observation pairs of all blocks              */
  uint64_t scratch_bytes;   /* device memory the elimination holds in the handle   */
} pcd_ba_schur_info;
pcd_status pcd_ba_schur_stats(pcd_ba* ba, pcd_ba_schur_info* info);
/* The co-visibility structure, built explicitly: sorts, scans and a load-balanced expansion over the
 * handle's own device arrays, no atomics, bitwise the same lists on every build.  Nothing of the size of the
 * observations or the entries crosses PCIe; the stream is synchronised at most twice (the slot and entry counts, which
 * size the entry buffers, then the pair count).  More than 2^32 - 16 entries or blocks -> UNSUPPORTED, decided from
 * the 64-bit count before an entry buffer exists; the handle stays usable for everything else. */
typedef struct {
  double build_ms;                 /* wall time of the build, its synchronisations included (0: already built) */
  int32_t num_slots, num_syncs;    /* stream synchronisations the build made */
  uint64_t num_pairs, num_entries;
} pcd_ba_schur_build_info;
/* builds the structure now, on `stream`, if the handle has none (after pcd_ba_create, or after an edit dropped it) */
pcd_status pcd_ba_schur_build_device(pcd_ba* ba, void* stream, pcd_ba_schur_build_info* info /*may be NULL*/);
/* The structure's lists, device -> host (built first, on the legacy stream, if the handle has none).  Every pointer may
 * be NULL.  With ns = num_slots, nblk = ns + num_pairs: slot_image [ns]; obs_pos [O] image-major position of every
 * observation; blk_start [nblk + 1] (the ns diagonal blocks, then the pair blocks in ascending (i, j)); ent_a, ent_b
 * [num_entries] image-major positions, ascending (a, b) within a block; pair_ij [2 num_pairs]; row_start [ns + 1],
 * row_blk / row_col [ns + 2 num_pairs]: per slot s the transposed (k, s) blocks in ascending k (col = k << 1 | 1), the
 * diagonal block (col = s << 1), the (s, j) blocks in ascending j (col = j << 1). */
typedef struct {
  int32_t* slot_image; uint32_t *obs_pos, *blk_start, *ent_a, *ent_b, *pair_ij, *row_start, *row_blk, *row_col;
} pcd_ba_schur_lists;
pcd_status pcd_ba_schur_structure_lists(pcd_ba* ba, const pcd_ba_schur_lists* out);

/* Reduced camera system on the device: block-sparse preconditioned conjugate gradients on S dpose = rhs of the LAST
 * Schur call on the handle, read from the handle's own S_diag / S_off / rhs (INVALID, with a message that says which,
 * when there is no Schur state or when that call sent one of the three to caller memory).  fp64, no atomics,
 * fixed-order sums: bitwise reproducible.  From x_0 = 0 (no warm start: r_k stays orthogonal to x_k, so the model
 * decrease of pcd_ba_schur_back_substitute_device holds for an inexact step), iteration k = 1, 2, ...:
 *   z = M^-1 r; rho = r.z; p = z + (rho / rho_old) p; w = S p; alpha = rho / (p.w); x += alpha p; r -= alpha w
 * then, with Q_k = -1/2 x.(rhs + r) (= 1/2 x^T S x - x^T rhs):
 *   1. zeta = k (Q_k - Q_{k-1}) / Q_k;  k >= min_iterations and zeta < q_tolerance          -> PCD_PCG_Q_TOLERANCE
 *   2. k >= min_iterations and ||r|| <= r_tolerance ||rhs||                                   -> PCD_PCG_R_TOLERANCE
 *   3. k = max_iterations                                                                     -> PCD_PCG_MAX_ITERATIONS
 * A negative tolerance switches its test off.  ||rhs|| = 0 (and ns = 0): x = 0, PCD_PCG_ZERO_RHS, 0 iterations.
 * p.w <= 0 or a non-finite scalar: PCD_PCG_BREAKDOWN, x is the last finite iterate.
 * Preconditioner: SCHUR_JACOBI = the inverse of every 6x6 diagonal block of S through its Cholesky factor (a block with
 * a non-positive pivot falls back to the identity and is counted; constant-tvec coordinates stay identity), or IDENTITY.
 * Guards as for the other pcd_ba_schur* calls.  The host looks at the device's done flag once per batch of
 * iterations (8, 16, then 32 at a time); nothing else is synchronised. */
typedef enum { PCD_PRECOND_IDENTITY = 0, PCD_PRECOND_SCHUR_JACOBI = 1 } pcd_ba_preconditioner;
typedef enum { PCD_PCG_MAX_ITERATIONS = 0, PCD_PCG_Q_TOLERANCE = 1, PCD_PCG_R_TOLERANCE = 2,
               PCD_PCG_BREAKDOWN = 3, PCD_PCG_ZERO_RHS = 4 } pcd_ba_pcg_termination;
typedef struct {
  int32_t max_iterations, min_iterations;
  int32_t preconditioner;           /* pcd_ba_preconditioner */
  double q_tolerance, r_tolerance;
  int32_t reserved[8];
} pcd_ba_pcg_opts;
typedef struct {
  int32_t iterations, termination;  /* pcd_ba_pcg_termination */
  uint32_t precond_fallbacks;       /* slots whose diagonal block failed its Cholesky */
  double rhs_norm, residual_norm;   /* ||rhs||, ||r|| of the recurrence */
  double q;                         /* Q of the last iteration */
  double step_dot_residual;         /* x.r, 0 up to rounding (diagnostic) */
} pcd_ba_pcg_info;
void pcd_ba_pcg_opts_default(pcd_ba_pcg_opts* opts);   /* 100, 0, SCHUR_JACOBI, 0.1, -1 */
pcd_status pcd_ba_schur_solve_pcg_device(pcd_ba* ba, const pcd_ba_pcg_opts* opts, double* d_dpose /*[ns][6]*/,
                                         pcd_ba_pcg_info* d_info /*device, may be NULL*/, void* stream);
pcd_status pcd_ba_schur_solve_pcg(pcd_ba* ba, const pcd_ba_pcg_opts* opts, double* dpose /*[ns][6] host*/,
                                  pcd_ba_pcg_info* info /*host, may be NULL*/);
/* Direct solve of the reduced camera system on the device: blocked right-looking fp64 Cholesky S = L L^T, then the two
 * triangular solves.  n = 6 ns is padded to n_padded, a multiple of the panel width 96 (16 pose slots), with identity
 * rows / columns and rhs 0, so no kernel has a ragged edge.  Per panel: one launch factors the 96 x 96 diagonal block
 * and solves the rows below against it (every workgroup re-derives the same diagonal factor in the same operation
 * order, so they agree bit for bit; the launch never writes the block it reads: the factor of a diagonal block goes
 * to rows of its own behind the matrix), one launch updates the lower-triangle tiles behind it on the fp64 matrix pipe
 * (v_mfma_f64_16x16x4_f64).  The right-hand side rides along as one more row of the matrix, which makes the panel
 * solve deliver y = L^-1 rhs; L^T x = y then runs panel by panel from the last.  Plain launches only, no atomics, every
 * sum in an order fixed by n: bitwise reproducible.  The host does not synchronise inside the solve.
 *   d_S == NULL && d_rhs == NULL: reads the handle's own S_diag / S_off / rhs of the LAST Schur call (same state guard
 *     and message as the PCG);
 *   both given: d_S [n][n] row-major as pcd_ba_schur_out.S delivers it, of which only the lower triangle is read and
 *     nothing is modified, d_rhs [n];  exactly one of the two: PCD_ERR_INVALID.
 * A pivot that is <= 0 or not finite ends the factorisation at that column: PCD_CHOL_NOT_POSITIVE_DEFINITE,
 * failed_column, and dpose = 0 exactly (the call itself still returns PCD_OK).  The dense scratch
 * ((n_padded + 192) n_padded doubles) belongs to the handle, is allocated on first use (PCD_ERR_OOM when that fails) and
 * counted in pcd_ba_schur_stats.  ns = 0: PCD_OK, status OK, nothing launched.  Guards as for the other pcd_ba_schur*
 * calls; d_dpose may be NULL only when ns = 0.  The host form with S given stages the n^2 doubles of S on the device for
 * the call and frees them again (a hipMalloc / hipFree pair per call, 288 MB at n = 6000): a caller in a loop wants the
 * _device form, or the handle's own blocks, which need no staging. */
typedef enum { PCD_LINEAR_PCG = 0, PCD_LINEAR_CHOLESKY = 1, PCD_LINEAR_PCG_CAM = 2 /* the bordered PCG, below */ } pcd_ba_linear_solver;
typedef enum { PCD_CHOL_OK = 0, PCD_CHOL_NOT_POSITIVE_DEFINITE = 1 } pcd_ba_chol_status;
typedef struct {
  int32_t status;          /* pcd_ba_chol_status */
  int32_t failed_column;   /* first column whose pivot was <= 0 or not finite; -1 when OK */
  int32_t n, n_padded, panels;
  double min_pivot, max_pivot;   /* of L's diagonal, as stored, over the unpadded columns factored so far */
} pcd_ba_chol_info;
pcd_status pcd_ba_schur_solve_cholesky_device(pcd_ba* ba, const double* d_S, const double* d_rhs,
                                              double* d_dpose /*[ns][6]*/,
                                              pcd_ba_chol_info* d_info /*device, may be NULL*/, void* stream);
pcd_status pcd_ba_schur_solve_cholesky(pcd_ba* ba, const double* S, const double* rhs, double* dpose,
                                       pcd_ba_chol_info* info /*may be NULL*/);   /* host pointers */
/* current parameters, device -> host (either pointer may be NULL) */
pcd_status pcd_ba_get_parameters(pcd_ba* ba, double* poses /*[I][7]*/, double* points /*[P][3]*/);

/* Levenberg-Marquardt in the library.  Each iteration: pcd_ba_schur_device at mu = 1 / radius, the PCG above
 * (BREAKDOWN counts as a rejected step), back-substitution, Plus into the handle's parameters (the accepted ones are
 * kept in handle scratch), the cost pass at the candidate, then Ceres' trust-region rule: accept if
 * rho = (cost - candidate_cost) / model_decrease > min_relative_decrease; on success
 * radius = min(max_radius, radius / max(1/3, 1 - (2 rho - 1)^3)) and the decrease factor resets to 2, on failure
 * radius /= factor and the factor doubles.  No Jacobi scaling of the columns.  It stops at max_num_iterations
 * (PCD_SOLVE_MAX_ITERATIONS), when |cost - candidate_cost| <= function_tolerance cost after an accepted step, when
 * the gradient max-norm at the current parameters is <= gradient_tolerance (tested before the step is tried), or when
 * radius < min_radius.  The gradient test is the plain max-norm of g over the active pose coordinates and the
 * non-constant points, NOT Ceres' manifold-projected ||Plus(x, -g) - x||.  A tolerance of 0 switches its test off.
 * One small device-to-host copy per iteration carries the costs, the model decrease, the PCG record and the gradient
 * norm (one more per extra batch when the PCG runs past its first 8 iterations).  On return the handle holds the
 * accepted parameters.
 * linear_solver = PCD_LINEAR_CHOLESKY replaces the PCG by pcd_ba_schur_solve_cholesky_device on the handle's own
 * blocks (an exact step; `linear` is then checked but not used).  There is no second batch: exactly one copy per
 * iteration.  PCD_CHOL_NOT_POSITIVE_DEFINITE counts as a rejected step, as BREAKDOWN does.  In pcd_ba_solve_iteration
 * linear_iterations is then 0 and linear_termination holds the pcd_ba_chol_status; linear_solver_ms covers fill,
 * factorisation and the triangular solves.  Any other value of linear_solver: PCD_ERR_INVALID. */
typedef enum { PCD_SOLVE_MAX_ITERATIONS = 0, PCD_SOLVE_FUNCTION_TOLERANCE = 1, PCD_SOLVE_GRADIENT_TOLERANCE = 2,
               PCD_SOLVE_MIN_RADIUS = 3 } pcd_ba_solve_termination;
typedef struct {
  int32_t max_num_iterations;
  int32_t damping;                  /* pcd_ba_damping */
  double initial_radius, max_radius, min_radius, min_relative_decrease, function_tolerance, gradient_tolerance;
  pcd_ba_pcg_opts linear;
  int32_t linear_solver;            /* pcd_ba_linear_solver; 0 (a zero-filled struct, the defaults) = PCG */
  int32_t refine_intrinsics;        /* 1: solve for the refined camera parameters too (pcd_ba_schur_cam* below);  */
                                    /* 0 (a zero-filled struct, the defaults): a refined handle is refused        */
  int32_t reserved[6];
} pcd_ba_solve_opts;
typedef struct {
  double cost, candidate_cost, model_decrease, relative_decrease;
  double radius;                    /* after the update */
  double gradient_max_norm;         /* at the parameters the iteration started from */
  int32_t accepted, linear_iterations, linear_termination;
  uint64_t num_skipped;
} pcd_ba_solve_iteration;
typedef struct {
  double initial_cost, final_cost;
  int32_t num_iterations, num_accepted;
  int32_t termination;              /* pcd_ba_solve_termination */
  double total_ms, linear_solver_ms;
} pcd_ba_solve_summary;
/* 10, MARQUARDT, 1e4, 1e16, 1e-32, 1e-3, 0, 0, linear = pcd_ba_pcg_opts_default */
void pcd_ba_solve_opts_default(pcd_ba_solve_opts* opts);
pcd_status pcd_ba_solve(pcd_ba* ba, const pcd_ba_solve_opts* opts, pcd_ba_solve_summary* summary,
                        pcd_ba_solve_iteration* iterations /*[max_num_iterations] or NULL*/);

/* Refined intrinsics in the reduced system: the calls above stay refused on a handle with a camera_refine
 * byte set; the calls below, beside them, carry the camera rows.  Camera slots are the cameras with at least one
 * refined parameter, in ascending camera index, ncs of them; each has PCD_CAM_JAC_STRIDE coordinates of which the
 * refined entries below the model's K are active and the others inactive exactly as a constant-tvec coordinate is
 * (identity row and column, right-hand side 0, delta 0).  Reduced unknowns: [6 ns pose tangents | 12 ncs camera
 * coordinates], n = 6 ns + 12 ncs.  With V_p, W_a as above and cam(o) the camera slot of observation o's image:
 *   Wc_p[r] = sum over the observations o of point p with cam(o) = r, ascending o, of W_cam[o]       (12 x 3)
 *   Z_p[r]  = Wc_p[r] V_p^-1                                            (0 for constant and skipped points)
 *   S_cam[r][r'] = delta_rr' (H_cam[r] + D_r) - sum_p Z_p[r] Wc_p[r']^T
 *   B[i][r]      = [cam(image of slot i) = r] E_cam[image] - sum over the eliminated observations e of the image,
 *                  image-major, of Z_pt(e)[r] W_e^T                      (constant-tvec columns zero)
 *   rhs_cam[r]   = -g_cam[r] + sum_p Z_p[r] g_p
 *   S = [[S_pose, B^T], [B, S_cam]],  D_r,kk = the damping of H_cam[r][k][k] on the active coordinates
 *   dX_p = -V_p^-1 (g_p + sum_a W_a^T dpose[slot(a)] + sum_r Wc_p[r]^T dcam[r])
 * and the model decrease gains 1/2 sum over the active camera coordinates of (-dcam g_cam + D dcam^2).  An observation
 * in a constant-pose image has no slot but still couples its camera to its point.  The pose part (S_diag, S_off, rhs)
 * is that of pcd_ba_schur_device, bit for bit.  Two solvers read the bordered system: the direct solve and the
 * bordered PCG (pcd_ba_schur_cam_solve_pcg*).  Camera slots couple
 * every image of a camera, so they are kept dense and few: more than PCD_BA_MAX_CAMERA_SLOTS (for example one refined
 * camera per image) -> PCD_ERR_UNSUPPORTED from every call below and from pcd_ba_solve with refine_intrinsics, before
 * anything is allocated or launched; the handle stays usable.  The other guards (NULL, no device, capturing stream,
 * "no Schur state") are those of the plain calls.  On a handle without camera slots every call below is valid and
 * returns bit for bit what its plain counterpart returns.  No atomics, fixed-order sums: bitwise reproducible. */
#define PCD_BA_MAX_CAMERA_SLOTS 8
/* host query, no device work: camera_slot [C] (-1: no refined parameter), the number of slots, active [ncs][12]
 * (1 = the coordinate is solved for); every output may be NULL */
pcd_status pcd_ba_camera_slots(pcd_ba* ba, int32_t* camera_slot, int32_t* num_slots, uint8_t* active);
/* every pointer may be NULL (not written) */
typedef struct {
  double *cost, *S_diag, *S_off, *rhs;   /* as pcd_ba_schur_out */
  double* B;                             /* [ns][ncs][12][6] */
  double* S_cam;                         /* [ncs][ncs][12][12], both triangles */
  double* rhs_cam;                       /* [ncs][12] */
  double* S;                             /* [n][n] dense, row-major, both triangles */
  uint64_t* num_skipped;
} pcd_ba_schur_cam_out;
/* Normal-equation pass with the camera blocks (pcd_ba_evaluate_device's H_cam, g_cam, E_cam, W_cam) into handle
 * scratch, then the elimination.  B, S_cam and rhs_cam always stay in the handle; the outputs are copies. */
pcd_status pcd_ba_schur_cam_device(pcd_ba* ba, const pcd_ba_schur_opts* opts, const pcd_ba_schur_cam_out* d_out,
                                   void* stream);
pcd_status pcd_ba_schur_cam(pcd_ba* ba, const pcd_ba_schur_opts* opts, const pcd_ba_schur_cam_out* out);   /* host outputs */
/* Direct solve (pcd_ba_schur_solve_cholesky_device's factorisation) of the bordered system from the handle's own blocks
 * of the last pcd_ba_schur_cam* (INVALID without one, or when that call sent S_diag / S_off / rhs to caller memory);
 * d_delta [n] = dpose [ns][6], then dcam [ncs][12] (0 on inactive coordinates; all 0 when the factorisation failed). */
pcd_status pcd_ba_schur_cam_solve_cholesky_device(pcd_ba* ba, double* d_delta, pcd_ba_chol_info* d_info /*may be NULL*/,
                                                  void* stream);
/* Bordered PCG: preconditioned conjugate gradients on the bordered system of the last pcd_ba_schur_cam*, from the
 * handle's own blocks (INVALID as for the direct solve above).  With x = [dpose | dcam], b = [rhs | rhs_cam]:
 *   w_pose[i] = sum over the row list of i of (S block) p_j + sum_r B[i][r]^T p_cam[r]
 *   w_cam[r]  = sum_i B[i][r] p_pose[i] + sum_r' S_cam[r][r'] p_cam[r']
 * Recurrence, pcd_ba_pcg_opts, pcd_ba_pcg_info, terminations, x_0 = 0, the Q / r / max-iteration order, BREAKDOWN and
 * ZERO_RHS are exactly those of pcd_ba_schur_solve_pcg*, with every dot product and norm over the whole vector, poses
 * and cameras (rhs_norm includes rhs_cam); the done flag stays on the device and the host looks at it in batches of 8,
 * 16 and 32 iterations.  PCD_PRECOND_SCHUR_JACOBI: the 6 x 6 pose block inverses and the inverse of every camera slot's
 * 12 x 12 diagonal block S_cam[r][r] through its Cholesky factor (Ceres' SCHUR_JACOBI with the intrinsics as one more
 * parameter block per camera); inactive coordinates stay identity rows / columns of that inverse, exactly; a block with
 * a non-positive or non-finite pivot falls back to the identity and is counted in precond_fallbacks.  fp64, no atomics,
 * every sum in an order fixed by the structure: bitwise repeatable.  Inactive camera coordinates and constant-tvec
 * coordinates of x are exactly 0.  B crosses memory once per iteration; an iteration is four launches.  d_delta [n] has
 * the layout of pcd_ba_schur_cam_solve_cholesky_device.  All scratch belongs to the handle (pcd_ba_schur_stats). */
pcd_status pcd_ba_schur_cam_solve_pcg_device(pcd_ba* ba, const pcd_ba_pcg_opts* opts, double* d_delta /*[n]*/,
                                             pcd_ba_pcg_info* d_info /*device, may be NULL*/, void* stream);
pcd_status pcd_ba_schur_cam_solve_pcg(pcd_ba* ba, const pcd_ba_pcg_opts* opts, double* delta /*host*/,
                                      pcd_ba_pcg_info* info);
/* point steps and model decrease for d_delta [n], from the state of the last pcd_ba_schur_cam* */
pcd_status pcd_ba_schur_cam_back_substitute_device(pcd_ba* ba, const double* d_delta, double* d_dpoint /*[P][3]*/,
                                                   double* d_model_decrease /*[1] or NULL*/, void* stream);
/* pcd_ba_plus_device, and p + dcam on the active camera parameters; constant cameras and parameters are copied bit for
 * bit.  Reads the handle's current parameters; in-place safe.  d_cam_params_out may be NULL (not written). */
pcd_status pcd_ba_plus_cam_device(pcd_ba* ba, const double* d_delta, const double* d_dpoint, double* d_poses_out,
                                  double* d_points_out, double* d_cam_params_out /*[cam_params_len]*/, void* stream);
/* current camera parameters, device -> host */
pcd_status pcd_ba_get_camera_parameters(pcd_ba* ba, double* cam_params /*[cam_params_len] host*/);
/* pcd_ba_solve with refine_intrinsics = 1: each iteration runs pcd_ba_schur_cam_device, the direct solve of the bordered
 * system, the back-substitution, Plus on poses, points and the active camera parameters, and the cost pass; the
 * trust-region rule is unchanged, the gradient max-norm includes g_cam over the active coordinates, the accepted camera
 * parameters are kept beside the accepted poses and points and restored on a rejected step.  On return the handle
 * holds the accepted camera parameters, on the device and in the host mirror pcd_ba_project_lidar_device reads.
 * linear_solver = PCD_LINEAR_PCG_CAM runs the bordered PCG instead (`linear` as for PCD_LINEAR_PCG; BREAKDOWN counts as a
 * rejected step; one small device-to-host copy per iteration and one more per extra PCG batch); without camera slots,
 * or with refine_intrinsics = 0 on an unrefined handle, it is PCD_LINEAR_PCG.
 * refine_intrinsics = 1 with PCD_LINEAR_PCG on a handle that has camera slots -> PCD_ERR_UNSUPPORTED (use
 * PCD_LINEAR_CHOLESKY or PCD_LINEAR_PCG_CAM).  On a handle without camera slots the flag changes nothing. */

/* ------------------------------------------------------------------------
 * Re-association of a handle's LiDAR terms on the device        
 *   the loop of sfm/incremental_mapper.cc:1413-1478 IncrementalMapper::AdjustGlobalBundleByLidar and of
 *   controllers/bundle_adjustment.cc:130-201 BundleAdjustmentController::Run: associate, solve, associate again
 *   with a tighter radius, solve again -- without a host round trip and without rebuilding anything that depends
 *   on the observations alone.
 * pcd_ba_set_lidar_device replaces ALL LiDAR terms of the handle by those of Q device rows:
 *   row q becomes a term iff type[q] != 0 and none of its four abcd values is NaN (the guard of
 *   optim/bundle_adjustment.cc:1005-1009; an Inf passes, as there); its point is d_point[q] (d_point == NULL: q, and
 *   Q must equal num_points), its weight is weight[type[q]] (:1013-1028); terms are numbered in ascending row order.
 *   A point may receive several terms, rows may come in any point order, and the number of terms may grow, shrink,
 *   become 0, or become non-zero on a handle created without terms.
 * Contract: afterwards the handle is indistinguishable from one that pcd_ba_create built from the same description
 *   with lidar_point / lidar_abcd / lidar_weight set to this term list -- every derived array is the one
 *   pcd_ba_create would upload, byte for byte, so every later result on the handle (evaluate, blocks, Schur, solve,
 *   filters) is bit-identical to the fresh handle's.
 * Refused with PCD_ERR_INVALID, the handle left exactly as it was: a d_point entry outside [0, num_points) or a
 *   type above 3 in ANY row (rows of type 0 included), a weight that is not finite for a type some term has,
 *   Q >= 0xFFFFFFF0, d_point == NULL with Q != num_points.  The new layout is built in buffers of its own and
 *   swapped in only on success.
 * Guards: a NULL handle or argument -> INVALID; no gfx950 -> NO_DEVICE; a capturing stream -> UNSUPPORTED before
 *   anything is allocated (as every _device call).
 * The call synchronises `stream` ONCE: the number of terms (read back together with the validation record) sizes
 *   buffers and launch grids, as the row count does in pcd_cloud_voxel_downsample_device.  The rest is enqueued on
 *   `stream`; later work on the handle must be ordered behind it (the same stream, or the legacy stream).
 * What the call invalidates: pointers handed out by an earlier pcd_ba_evaluate_blocks* (the pinned buffer follows the
 *   number of terms) and by pcd_ba_lidar_device; the Schur state of the last call (pcd_ba_schur_solve_* and the
 *   back-substitution return their "no Schur state" PCD_ERR_INVALID until the next Schur call).  The co-visibility
 *   structure and the elimination scratch are kept: they depend on the observations alone.
 * No atomics; no order depends on launch geometry: a repeated call is bitwise identical.
 * --------------------------------------------------------------------- */
pcd_status pcd_ba_set_lidar_device(pcd_ba* ba, uint64_t Q,
    const int32_t* d_point   /* [Q] point of row q; NULL: row q is point q (then Q must equal P) */,
    const uint8_t* d_type    /* [Q] pcd_lidar_type or PCD_LIDAR_PROJ; 0 = no term */,
    const double*  d_abcd    /* [Q][4] */,
    const double*  d_lidar_xyz /* [Q][3] or NULL: kept per term for the outlier filter */,
    const double   weight[4] /* host; by type: [1] Icp, [2] IcpGround, [3] Proj; [0] unused */,
    void* stream, uint64_t* num_terms /* host, may be NULL */);
/* Host copies of the current terms: point [L], abcd [L][4], weight [L], type [L], lidar_xyz [L][3]; every pointer may
 * be NULL (size the arrays with num_terms first).  type and lidar_xyz are zero for terms that came from pcd_ba_create,
 * which knows neither. */
pcd_status pcd_ba_get_lidar(pcd_ba* ba, uint64_t* num_terms, int32_t* point, double* abcd, double* weight,
                            uint8_t* type, double* lidar_xyz);
/* The same arrays as device pointers (every output may be NULL), e.g. for pcd_filter_lidar_outlier_device on the
 * terms (gather the points by d_point first).  Valid until the next pcd_ba_set_lidar_device /
 * pcd_ba_associate_lidar_device / pcd_ba_destroy on the handle. */
pcd_status pcd_ba_lidar_device(pcd_ba* ba, uint64_t* num_terms, const int32_t** d_point, const double** d_abcd,
                               const double** d_weight, const uint8_t** d_type, const double** d_lidar_xyz);

/* One call for "associate this handle's CURRENT points against this cloud and install the terms":
 * pcd_associate_device with the handle's device points [P][3] as the queries, the rows written to scratch owned by the
 * BA handle, then the machinery of pcd_ba_set_lidar_device with row = point and weight = {-, icp_weight,
 * icp_ground_weight, -}.  d_select is applied AFTER a full-P association: the association rows are exactly those of
 * pcd_associate_device on all points, and an unselected row then counts as type 0.  One term per point at most, in
 * ascending point order: what the reference's loops (point-id order, a map keyed by point) produce.
 * Refusals: handle and cloud on different devices -> INVALID; a cloud that is a shard or strided (index_stride != 1 or
 * index_base != 0) -> UNSUPPORTED; otherwise those of pcd_associate_device and pcd_ba_set_lidar_device.  P == 0:
 * PCD_OK with zero counts.  With info the call also waits for its last kernel, to report rebuild_ms. */
typedef struct {
  int32_t gate_mode;            /* pcd_gate_mode, PCD_GATE_BOUNDED_SEARCH may be OR-ed in */
  const double* d_max_range;    /* device, [P] or [1]; ignored for PCD_GATE_CONTROLLER */
  uint64_t max_range_count;
  const uint8_t* d_select;      /* device [P] or NULL: which points are queries (the mapper's variable points; the controller: all) */
  double icp_weight, icp_ground_weight;
  int32_t reserved[8];
} pcd_ba_assoc_opts;
typedef struct {
  uint64_t num_queries;         /* selected points (P without d_select) */
  uint64_t num_terms, num_icp, num_icp_ground;
  double assoc_ms, rebuild_ms;  /* device time of the association and of the rebuild (its one synchronisation included) */
} pcd_ba_assoc_info;
void pcd_ba_assoc_opts_default(pcd_ba_assoc_opts* opts);   /* MAPPER_GLOBAL, NULL, 0, NULL, 100, 1000 (shim/ba_problem.h:71-72) */
pcd_status pcd_ba_associate_lidar_device(pcd_ba* ba, pcd_cloud* cloud, const pcd_ba_assoc_opts* opts,
                                         void* stream, pcd_ba_assoc_info* info /* host, may be NULL */);

/* ------------------------------------------------------------------------
 * Depth-projection (Proj) terms installed on a live handle        
 *   the short-track route of the local bundle adjustment, sfm/incremental_mapper.cc:1109-1165: Project2Image
 *   (PcdProj::SetNewImage on the images of the track), then optim/bundle_adjustment.cc:288-350
 *   BundleAdjustmentConfig::MatchVariablePoint2LidarPoint; long tracks take MatchClosestLidarPoint, and both feed one
 *   term list.  One call: project the handle's images at their CURRENT poses, pick per track, associate the
 *   nearest-neighbour points, install.
 * Images.  Image i is projected iff d_image_select is NULL or d_image_select[i] != 0.  Its pose is the handle's current
 *   poses[i], read on the device.  Its parameters are prm[k] = k < K ? cam_params[off + k] : 0 for k < 8 (K the
 *   parameter count of its camera's model): the reference reads an OPENCV camera unconditionally.  Width and height are
 *   cam_width / cam_height of its camera.  Its features are its observations in ascending observation index.  The
 *   focal-length check of pcd_proj_set_new_images (params[0] != 0 && params[1] != 0) runs over all cameras of the handle,
 *   on a host mirror of the camera parameters that pcd_ba_create and pcd_ba_set_camera_parameters keep.  A projector
 *   that has not latched its splat coefficients yet latches on the camera of image 0.
 * Candidates of a point of mode PCD_BA_POINT_PROJ: its observations in ascending observation index; an observation is
 *   a candidate when its image is selected and its feature found a winner; of several such observations of the point
 *   in one image only the one with the lowest index counts (std::map::insert, pcd_projection.cc:79).
 * Pick.  With X the point and c = (x y z nx ny nz) the candidate's winner, in double, left to right, without FMA:
 *   v = X - c.xyz; dot = v0 nx + v1 ny + v2 nz; nn = sqrt(nx nx + ny ny + nz nz); vn = sqrt(v0 v0 + v1 v1 + v2 v2);
 *   the candidate with the smallest fabs(dot / (nn * vn)) wins; the comparison is strict < starting from 360, so ties go
 *   to the lowest observation index and a NaN (zero normal, X on the LiDAR point) never wins.
 * Row of the point: with a winner, type PCD_LIDAR_PROJ, lidar_xyz = c.xyz, abcd = (n / sqrt(nx nx + ny ny + nz nz),
 *   0 - a x - b y - c z) (lidar_point.cc:39-50); without one, type 0.  A NaN in abcd drops the row by the rule of
 *   pcd_ba_set_lidar_device.
 * Points of mode PCD_BA_POINT_NN: their row is exactly that of pcd_associate_device on ALL the handle's points against
 *   the projector's cloud (a full-P association, then masked, as pcd_ba_associate_lidar_device defines it), with
 *   gate_mode / d_max_range.  The association does not run at all when d_point_mode is NULL.  Mode 0: no term.
 * Install: the machinery of pcd_ba_set_lidar_device with row = point and weight = {-, icp_weight, icp_ground_weight,
 *   proj_weight}: at most one term per point, in ascending point order; afterwards the handle is bit-identical to one
 *   pcd_ba_create built with this term list.  The same invalidations and the same single synchronisation of `stream`
 *   (with info the call also waits for its last kernel).  A repeated call is bitwise identical.
 * Refused with the handle exactly as it was: NULL opts / cam_width / cam_height / handle / projector, a mode above 2 in
 *   any row, a zero focal length, handle and projector on different devices -> INVALID; a capturing stream ->
 *   UNSUPPORTED before anything is allocated; otherwise the refusals of pcd_associate_device (when d_point_mode is
 *   given) and pcd_ba_set_lidar_device.  num_points == 0: PCD_OK with zero counts; no observations: zero terms.
 * Scratch belongs to the handle and the projector and only grows.
 * --------------------------------------------------------------------- */
#define PCD_BA_POINT_NONE 0
#define PCD_BA_POINT_PROJ 1
#define PCD_BA_POINT_NN   2
typedef struct {
  const uint64_t* cam_width;        /* host [num_cameras]  Camera::Width()  -- the handle does not know image sizes */
  const uint64_t* cam_height;       /* host [num_cameras] */
  const uint8_t* d_image_select;    /* device [I] or NULL (all): the images that are projected
                                       (lidar_searched_image_ids_; Project2Image's pair-count test stays with the caller) */
  const uint8_t* d_point_mode;      /* device [P] or NULL (= every point PROJ): 0 no term, 1 PCD_BA_POINT_PROJ, 2 PCD_BA_POINT_NN */
  int32_t gate_mode;                /* for mode-2 points, as pcd_ba_assoc_opts */
  const double* d_max_range; uint64_t max_range_count;
  double proj_weight, icp_weight, icp_ground_weight;   /* defaults 1, 100, 1000 */
  int32_t reserved[8];
} pcd_ba_proj_opts;
typedef struct {
  uint64_t num_images, num_features, num_found;     /* selected images, their observations, those with a winner */
  uint64_t num_terms, num_proj, num_icp, num_icp_ground, pairs;   /* pairs: pcd_proj_last_pairs of this call */
  double proj_ms, assoc_ms, rebuild_ms;
} pcd_ba_proj_info;
void pcd_ba_proj_opts_default(pcd_ba_proj_opts* opts);   /* NULLs, MAPPER_LOCAL, 1, 100, 1000 */
pcd_status pcd_ba_project_lidar_device(pcd_ba* ba, pcd_proj* proj, const pcd_ba_proj_opts* opts, void* stream,
                                       pcd_ba_proj_info* info /* host, may be NULL */);

/* ------------------------------------------------------------------------
 * Observations and points dropped from a live handle on the device        
 *   the "adjust, filter, adjust" of controllers/incremental_mapper.cc:150-199 IterativeGlobalRefinement and of the
 *   local round, sfm/incremental_mapper.cc:1190-1211: the flags of pcd_ba_filter_points_device (or any others) applied
 *   to the handle without a host round trip and without a second pcd_ba_create.
 * Observation o is kept iff !d_obs_erase[o] && !d_point_delete[obs_point[o]]; LiDAR term l is kept iff
 *   !d_point_delete[lidar_point[l]].  Any non-zero byte counts as 1.  Kept rows keep their relative order.  P, I, C, the
 *   parameters currently on the device, the constness masks, the refine mask and the loss are unchanged.  A deleted
 *   point stays as a row without a residual block, so point ids remain stable for the caller; nothing constrains its
 *   coordinates any more: they are meaningless from then on (a solve leaves them where they are).
 * Contract (that of pcd_ba_set_lidar_device): afterwards the handle is indistinguishable from one pcd_ba_create built
 *   from the same description with obs_* and lidar_* compacted this way -- every derived array is the one pcd_ba_create
 *   would upload, byte for byte, so every later result on the handle (evaluate, both block routes, the filters, the
 *   Schur structure and blocks, both solves, associate_lidar / project_lidar, get_lidar with its type / lidar_xyz meta)
 *   is bit-identical to the fresh handle's.
 * d_obs_map, if given, receives the new index of every old observation, 0xFFFFFFFF for a dropped one.
 * Both flag pointers NULL is a valid call that changes nothing and invalidates nothing (d_obs_map is not written).
 * Guards, the handle exactly as it was: a NULL handle -> INVALID; no gfx950 -> NO_DEVICE; a capturing stream ->
 *   UNSUPPORTED before anything is allocated.  The flags cannot be invalid; a failed allocation is the only other
 *   failure, and every buffer is reserved before the first kernel; the new layout is built in buffers of its own and
 *   swapped in at the end.
 * The call synchronises `stream` ONCE, to read O(I) bytes: the counts and the image bounds.  The rest is enqueued on
 *   `stream`; later work on the handle must be ordered behind it.  info does not add a wait: rebuild_ms is the device
 *   time up to that synchronisation (every pass but the image-major fill, which is enqueued behind it).
 * What the call invalidates: pointers handed out by an earlier pcd_ba_evaluate_blocks* and pcd_ba_lidar_device; the
 *   Schur state of the last call AND the co-visibility structure, which depends on the observations: the next Schur
 *   call builds it as on a fresh handle.  Scratch only shrinks and is kept.
 * No atomics; no order depends on launch geometry: a repeated call is bitwise identical.
 * --------------------------------------------------------------------- */
typedef struct {
  uint64_t num_obs, num_obs_removed;      /* after / removed */
  uint64_t num_lidar, num_lidar_removed;
  uint64_t num_points_emptied;            /* points that had observations before and have none now */
  double rebuild_ms;                      /* device time up to the call's one synchronisation */
} pcd_ba_remove_info;
pcd_status pcd_ba_remove_observations_device(pcd_ba* ba,
    const uint8_t* d_obs_erase     /* [O] != 0: drop; NULL: none */,
    const uint8_t* d_point_delete  /* [P] != 0: drop all observations AND all LiDAR terms of the point; NULL: none */,
    uint32_t* d_obs_map            /* [O before] or NULL: new index of every old observation, 0xFFFFFFFF = dropped */,
    void* stream, pcd_ba_remove_info* info /* host, may be NULL */);

/* ------------------------------------------------------------------------
 * Observations and points added to a live handle on the device            
 *   the growing half of controllers/incremental_mapper.cc:157-198: CompleteAndMergeTracks and Retriangulate between
 *   the adjustments.  A completed track is an addition; a retriangulated point is a new point with its rows; a merge
 *   (MergePoints3D) is pcd_ba_remove_observations_device of two points followed by the addition of one.
 * Contract (that of pcd_ba_set_lidar_device and pcd_ba_remove_observations_device): afterwards the handle is
 *   indistinguishable from one pcd_ba_create built from a description with
 *     points      = the handle's current device points followed by d_new_points (ids P .. P + num_new_points - 1),
 *     obs_*       = the handle's rows followed by the new rows in the order given (ids O .. O + num_new_obs - 1; old
 *                   observation indices do not change, so there is no map),
 *     point_const = (only if the handle has one) extended by zeros: new points are variable,
 *   and everything else unchanged: I, C, the poses as they are on the device, cameras, masks, refine mask, loss, the
 *   LiDAR terms with their type / lidar_xyz meta.  Every derived array is the one pcd_ba_create would upload, byte for
 *   byte, so every later result is bit-identical to the fresh handle's.  New points carry no LiDAR term until the next
 *   pcd_ba_associate_lidar_device / pcd_ba_project_lidar_device / pcd_ba_set_lidar_device.
 * Arrays of the caller's with one entry per point (d_max_range, d_point_mode, the select masks of the associate /
 *   project options, point_delete flags, parameter uploads) must have the new length from then on.
 * Rows are validated ON THE DEVICE: obs_image in [0, I), obs_point in [0, P + num_new_points).  The verdict travels with
 *   the counts in the call's one status record; on a bad row the call returns PCD_ERR_INVALID and nothing has changed:
 *   the new layout is built in buffers of its own and swapped in only after the record says OK.
 * Guards, the handle exactly as it was: a NULL handle -> INVALID; no gfx950 -> NO_DEVICE; a capturing stream ->
 *   UNSUPPORTED before anything is allocated; a count with a NULL array -> INVALID; O + num_new_obs >= 0xFFFFFFF0 or
 *   P + num_new_points > INT32_MAX -> INVALID from the counts alone.  num_new_obs == 0 && num_new_points == 0 is a valid
 *   call that changes nothing and invalidates nothing.  Every buffer whose size follows from the counts is reserved before
 *   the first kernel; the sliced-ELL copies, whose size depends on the rows, are reserved behind the synchronisation and
 *   ahead of the swap.  A failed allocation leaves the handle intact.
 * The call synchronises `stream` ONCE, to read O(I) bytes: the verdict, the counts and the image bounds.  The two fill
 *   kernels are enqueued behind that read; later work on the handle must be ordered behind `stream`.  rebuild_ms is the
 *   device time up to the synchronisation.
 * What a successful call invalidates: pointers handed out by pcd_ba_evaluate_blocks*, pcd_ba_lidar_device and (when
 *   points were added) pcd_ba_device_parameters; the Schur state of the last call and the co-visibility structure.
 * No atomics; no order depends on launch geometry: a repeated call is bitwise identical.
 * --------------------------------------------------------------------- */
typedef struct {
  uint64_t num_obs, num_obs_added;         /* after / added */
  uint64_t num_points, num_points_added;
  uint64_t num_pose_rows;                  /* observations on variable-pose images, after */
  double rebuild_ms;                       /* device time up to the call's one synchronisation */
} pcd_ba_add_info;
pcd_status pcd_ba_add_observations_device(pcd_ba* ba,
    const double* d_new_points   /* [num_new_points][3] or NULL when 0: they get ids P .. P+num_new_points-1 */,
    uint64_t num_new_points,
    const int32_t* d_obs_image, const int32_t* d_obs_point, const double* d_obs_xy /* [num_new_obs] ([..][2]) */,
    uint64_t num_new_obs, void* stream, pcd_ba_add_info* info /* host, may be NULL */);
/* host arrays: uploads them and calls the device form on the null stream */
pcd_status pcd_ba_add_observations(pcd_ba* ba, const double* new_points, uint64_t num_new_points,
                                   const int32_t* obs_image, const int32_t* obs_point, const double* obs_xy,
                                   uint64_t num_new_obs, pcd_ba_add_info* info /* may be NULL */);

/* ------------------------------------------------------------------------
 * The sphere window of a global round: a second handle derived on the device   
 *   the selection of sfm/incremental_mapper.cc:1347-1408 (IncrementalMapper::AdjustGlobalBundleByLidar) and of
 *   optim/bundle_adjustment.cc:694-806 (AddImageInSphereToProblem): a sphere of ba_spherical_search_radius around the
 *   newest image's projection centre; images outside get a constant pose; only points seen from inside take part, with
 *   ALL their observations and their LiDAR terms.
 * pcd_ba_window_create_device derives that sub-problem from a live handle as a NEW handle; src is only read.
 * Selection, in the reference's arithmetic (fp64, no FMA, sums left to right; the stored quaternion is NOT normalised):
 *   R = Eigen's Quaterniond(w, x, y, z).toRotationMatrix():
 *     tx=2x ty=2y tz=2z  twx=tx*w twy=ty*w twz=tz*w  txx=tx*x txy=ty*x txz=tz*x  tyy=ty*y tyz=tz*y  tzz=tz*z
 *     R00=1-(tyy+tzz) R01=txy-twz R02=txz+twy  R10=txy+twz R11=1-(txx+tzz) R12=tyz-twx  R20=txz-twy R21=tyz+twx R22=1-(txx+tyy)
 *   c_k = -((R0k*t0 + R1k*t1) + R2k*t2);  dist = sqrt((dx*dx + dy*dy) + dz*dz);  image i is IN iff dist <= radius.
 *   With d_image_set the caller names the "in" images instead (any non-zero byte).
 *   Point p is ACTIVE iff one of its observations lies on an "in" image.
 *   Observation o of src is in the window iff active[obs_point[o]]; LiDAR term l iff active[lidar_point[l]];
 *   image_const_pose' = src's mask | !in | d_extra_const_pose.
 * Contract (that of the edits above): the window is indistinguishable from a handle pcd_ba_create builds from src's
 *   cameras, image_const_tvec / point_const / camera_refine and loss, src's parameters as they are on the device now,
 *   image_const_pose = image_const_pose' (always an array), and obs_* / lidar_* compacted as above in their old order
 *   (terms keep their type / lidar_xyz meta).  I, P and C are unchanged: image and point indices mean the same in both
 *   handles; an inactive point is a row without a residual block.  Every derived array is the fresh handle's byte for
 *   byte, so every later call on the window is bit-identical to the fresh handle's.
 * The window owns all its buffers: the handles are destroyed in either order, and nothing of src -- results, handed-out
 *   pointers, Schur state, structure -- changes.
 * Guards, before anything is allocated or launched: NULL src / opts / window -> INVALID; no gfx950 -> NO_DEVICE; a
 *   capturing stream -> UNSUPPORTED; exactly one of center_image >= 0 and d_image_set must be given, center_image < I,
 *   radius >= 0 and not NaN (+inf: every image is in) -> INVALID otherwise.  A failed allocation leaves *window NULL.
 *   A window without an active point (O == 0, L == 0) is a valid handle.
 * The call synchronises `stream` ONCE, to read O(I) bytes (the counts and the image bounds); the image-major fill is
 *   enqueued behind it.  No atomics, nothing depends on launch geometry: a repeated call gives the same bytes.
 * pcd_ba_window_commit_device copies the window's poses and points over src's, device to device on `stream` (exact: the
 *   window's constant poses and inactive points never moved), and, when the window refines intrinsics, its camera
 *   parameters with the host mirror.  It drops src's Schur state of the last call (it belongs to the old parameters);
 *   the co-visibility structure stays.  INVALID: a NULL handle, different devices, differing I, P or cam_params_len.
 * --------------------------------------------------------------------- */
typedef struct {
  int32_t center_image;              /* image whose projection centre is the sphere's; -1: use d_image_set */
  double  radius;                    /* ba_spherical_search_radius; image i is in iff dist(c_i, c_center) <= radius */
  const uint8_t* d_image_set;        /* device [I] or NULL: the images that are "in", given by the caller instead of a
                                        sphere (center_image must be -1 then; radius ignored) */
  const uint8_t* d_extra_const_pose; /* device [I] or NULL: OR-ed into the pose constness
                                        (fix_existing_images :1323-1329, first_image_fixed_frames :1341-1345) */
  int32_t reserved[8];
} pcd_ba_window_opts;
typedef struct {
  uint64_t num_images_in, num_points_active;
  uint64_t num_obs, num_lidar, num_pose_rows;   /* of the window */
  double build_ms;                               /* device time up to the call's one synchronisation */
} pcd_ba_window_info;
void pcd_ba_window_opts_default(pcd_ba_window_opts* o);   /* -1, 40.0, NULL, NULL */
pcd_status pcd_ba_window_create_device(pcd_ba* src, const pcd_ba_window_opts* opts,
    uint8_t* d_image_in      /* [I] or NULL, out */,
    uint8_t* d_point_active  /* [P] or NULL, out */,
    uint32_t* d_obs_map      /* [O of src] or NULL, out: row in the window, 0xFFFFFFFF = not in it */,
    void* stream, pcd_ba** window, pcd_ba_window_info* info /* host, may be NULL */);
pcd_status pcd_ba_window_commit_device(pcd_ba* window, pcd_ba* src, void* stream);

/* ------------------------------------------------------------------------
 * The local round on a live handle: FindLocalBundle and the local sub-problem   
 *   IncrementalMapper::FindLocalBundle (sfm/incremental_mapper.cc:1747-1914) picks the images of the local bundle;
 *   AdjustLocalBundle (:1004-1213) with AddImageToProblem / AddPointToProblem / ParameterizePoints
 *   (optim/bundle_adjustment.cc:814-985, 1107-1131) makes their sub-problem.
 * pcd_ba_local_bundle_device: the selection, fp64 without FMA, one operation at a time.
 *   n         = the rows of `image` (NumPoints3D).
 *   shared[j] = the pairs (row of `image`, row of j) on the same point, j != image (per ROW, as the reference counts: a
 *               point `image` sees through two rows counts twice); shared[image] = 0.
 *   Candidates: the images with shared > 0, by shared descending, TIES BY IMAGE INDEX ASCENDING (a chosen deviation: the
 *               reference's tie order is what std::sort makes of an unordered_map's iteration order).
 *   num_eff   = min(num_images - 1, #candidates).  #candidates == num_eff: the bundle is the candidates in that order, no
 *               angle is computed and d_tri_angle is -1 everywhere (:1798-1803).
 *   Otherwise tri[j] = Percentile(75) (util/math.h:231-246) of CalculateTriangulationAngles (base/triangulation.cc:147-181)
 *               between ProjectionCenter(image), ProjectionCenter(j) -- the NORMALISED quaternion, as the filter's
 *               centres, not the sphere window's -- and the point of EVERY row of `image` (the test at :1861 is against
 *               the image's own set: all n rows enter, a duplicated row twice).  idx = (int)std::round(0.75 * (n - 1)),
 *               halves away from zero; the result is the idx-th smallest angle, A NaN ANGLE ORDERING BEHIND EVERY NUMBER
 *               (a chosen deviation: nth_element over NaN is unspecified).  d_tri_angle[j] holds it for every candidate
 *               with (double)shared[j] >= 0.1 * n (the loosest pass's bound; below it no pass reads an angle), else -1.
 *   Passes:   thresholds (m / d, f * n), m = min_tri_angle_deg * DegToRad, (d, f) = (1, .6) (1.5, .6) (2, .5) (2.5, .4)
 *               (3, .3) (4, .2) (5, .1) (6, .1).  A pass visits the candidates in order; one with (double)shared < f * n
 *               ends the pass; an unused one with tri >= m / d is appended; the pass stops at num_eff.  Then the bundle is
 *               filled up with the unused candidates in order (:1895-1911).
 *   Outputs: d_bundle in selection order with -1 behind the last, d_num, d_image_set = 1 for `image` and the bundle.
 *   The device form does not synchronise; no floating-point atomics (the integer LDS histograms of the percentile's
 *   radix select are exact), nothing depends on the launch geometry: a repeated call gives the same bytes.
 *   Guards, before anything is allocated or launched: NULL ba / opts / d_bundle / d_num / d_image_set -> INVALID; no
 *   gfx950 -> NO_DEVICE; a capturing stream -> UNSUPPORTED; image outside [0, I), num_images < 2, min_tri_angle_deg
 *   negative or NaN -> INVALID.  An image without a row is valid: num = 0 and only `image` is in the set.
 * pcd_ba_local_window_create_device: the sub-problem as a second handle; src is only read.  With in = d_image_set != 0
 *   and V = the variable flags (d_point_variable != 0, or, with `image`: observed by `image` and track length <=
 *   max_track_length):
 *   row o stays iff in[obs_image[o]] || V[obs_point[o]]  (rows on "in" images: AddImageToProblem; the outside rows of
 *               variable points: the constant-pose blocks of AddPointToProblem);
 *   kept[p]   = the rows of p that stay; a point with kept == 0 is a row without a residual block;
 *   point_const'[p] = src's || (0 < kept[p] < track length of p)  (ParameterizePoints :1110-1121; a non-variable point
 *               whose whole track lies on "in" images stays variable, as in the reference);
 *   LiDAR term l stays iff V[lidar_point[l]] (the reference installs terms for variable points only);
 *   image_const_pose' = src's | !in | d_extra_const_pose.
 *   Cameras, image_const_tvec, camera_refine, the loss and I / P / C are the source's.  SetConstantCamera for a camera
 *   with images outside the bundle (:1064-1080) stays with the caller.
 *   Contract: the sphere window's, word for word -- the window is byte for byte the handle pcd_ba_create builds from
 *   the compacted description (image_const_pose and point_const always arrays); the source, its Schur state and
 *   structure are untouched; ONE synchronisation, to read O(I) bytes; no floating-point atomics; a repeated call gives
 *   the same bytes.  pcd_ba_window_commit_device carries a local window back unchanged (the new constant points and the
 *   outside poses never move: the copy is exact).  num_points_fixed counts the points the rule above made constant
 *   (0 < kept < length on a point the source does not hold constant).
 *   Guards: as for the sphere window (NULL src / opts / window -> INVALID, NO_DEVICE, UNSUPPORTED), d_image_set NULL ->
 *   INVALID, exactly one of d_point_variable and image >= 0, image < I.
 * --------------------------------------------------------------------- */
typedef struct {
  int32_t image;              /* the newly registered image; must have a variable or constant pose, any */
  int32_t num_images;         /* local_ba_num_images (6): at most num_images - 1 other images */
  double  min_tri_angle_deg;  /* local_ba_min_tri_angle (6.0) */
  int32_t reserved[8];
} pcd_ba_local_bundle_opts;
void pcd_ba_local_bundle_opts_default(pcd_ba_local_bundle_opts* o);   /* -1, 6, 6.0 */
pcd_status pcd_ba_local_bundle_device(pcd_ba* ba, const pcd_ba_local_bundle_opts* opts,
    int32_t* d_bundle    /* [num_images - 1], selection order, -1 behind the last */,
    int32_t* d_num       /* [1] */,
    uint8_t* d_image_set /* [I]: 1 for `image` and the bundle */,
    uint32_t* d_shared   /* [I] or NULL */, double* d_tri_angle /* [I] or NULL */, void* stream);
/* host form: null stream, waits.  bundle [num_images - 1], num [1]; shared / tri_angle [I] or NULL */
pcd_status pcd_ba_local_bundle(pcd_ba* ba, const pcd_ba_local_bundle_opts* opts, int32_t* bundle, int32_t* num,
                               uint32_t* shared, double* tri_angle);
typedef struct {
  const uint8_t* d_image_set;        /* device [I], required: `image` and its bundle (what the call above wrote) */
  const uint8_t* d_point_variable;   /* device [P] or NULL: the caller's point3D_ids after its track-length rule */
  int32_t image;                     /* used when d_point_variable is NULL (-1 otherwise): variable = observed by
                                        `image` and track length <= max_track_length */
  uint32_t max_track_length;         /* kMaxTrackLength: 1000 with LiDAR constraints (:1113), 15 without (:1129) */
  const uint8_t* d_extra_const_pose; /* device [I] or NULL (:1049-1062, :1084-1100) */
  int32_t reserved[8];
} pcd_ba_local_window_opts;
typedef struct {
  uint64_t num_images_in, num_points_variable, num_points_fixed;
  uint64_t num_obs, num_lidar, num_pose_rows;   /* of the window */
  double build_ms;                               /* device time up to the call's one synchronisation */
} pcd_ba_local_window_info;
void pcd_ba_local_window_opts_default(pcd_ba_local_window_opts* o);   /* NULL, NULL, -1, 1000, NULL */
pcd_status pcd_ba_local_window_create_device(pcd_ba* src, const pcd_ba_local_window_opts* opts,
    uint8_t* d_point_variable_out /* [P] or NULL, out: V */,
    uint32_t* d_obs_map           /* [O of src] or NULL, out: row in the window, 0xFFFFFFFF = not in it */,
    void* stream, pcd_ba** window, pcd_ba_local_window_info* info /* host, may be NULL */);

/* ------------------------------------------------------------------------
 * Exact SIFT descriptor matching (stretch row a19)
 *   replaces feature/sift.cc:1041-1054 MatchSiftFeaturesCPUBruteForce =
 *     feature/sift.cc:171-204 ComputeSiftDistanceMatrix (int32 dot of uint8 x 128) +
 *     feature/sift.cc:55-144  FindBestMatches[OneWay]BruteForce (ratio / distance tests, cross check)
 *   -- the exact result the reference's GPU path approximates with lib/SiftGPU SiftMatchGPU::GetSiftMatch
 *   (lib/SiftGPU/SiftGPU.h:268-352).  Defaults of SiftMatchingOptions (feature/sift.h:121-137):
 *   max_ratio 0.8, max_distance 0.7, cross_check 1.
 * desc: [n][128] uint8 row-major.  matches: [min(n1, ...)<= n1][2] = (point2D_idx1, point2D_idx2) in
 * ascending idx1, exactly the order of the reference's FeatureMatches vector.
 * --------------------------------------------------------------------- */
pcd_status pcd_sift_match(int device, const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float max_ratio,
                          float max_distance, int cross_check, uint32_t* matches /*[n1][2]*/, int32_t* num_matches);
/* device form: m12 [n1] / m21 [n2] receive the one-way results (-1 = none) as well */
pcd_status pcd_sift_match_device(int device, const uint8_t* d_desc1, int n1, const uint8_t* d_desc2, int n2,
                                 float max_ratio, float max_distance, int cross_check, int32_t* d_m12,
                                 int32_t* d_m21, uint32_t* d_matches, int32_t* d_num_matches, void* stream);

/* Many image pairs in one call: replaces feature/matching.cc:798 SiftFeatureMatcher::Match(image_pairs), which
 * ExhaustiveFeatureMatcher::Run (:902-960) calls once per block of up to block_size^2 pairs and whose workers
 * (:358-380 CPU, :403-440 GPU) run MatchSiftFeaturesCPU / MatchSiftFeaturesGPU pair by pair.
 * All descriptors live in one arena of 128-byte rows: image i owns rows [first_row[i], first_row[i+1]).
 * `pairs` is n_pairs x {image1, image2}.  Per pair the result is exactly pcd_sift_match(image1, image2).
 * Device form: first_row / pairs / match_offset are HOST arrays (read before the call returns), d_arena,
 * d_matches and d_counts device memory.  Pair p's list goes to d_matches + 2 * match_offset[p] and must have
 * room for n(image1) matches; d_counts[p] = its length.  Three launches per sub-batch of pairs (scores,
 * finalize, cross check + compaction) on `stream`; the call does not wait for them.
 * Host form: uploads the arena, returns the lists back to back in `matches` (list p =
 * matches[2 * list_offset[p] .. 2 * list_offset[p + 1])); PCD_ERR_INVALID if they exceed matches_capacity
 * (counted in matches; list_offset is still filled so the caller can size the buffer and call again). */
pcd_status pcd_sift_match_batch_device(int device, const uint8_t* d_arena, const uint64_t* first_row /*[n_images+1]*/,
                                       int n_images, const uint32_t* pairs /*[n_pairs][2]*/, int n_pairs,
                                       float max_ratio, float max_distance, int cross_check, uint32_t* d_matches,
                                       const uint64_t* match_offset /*[n_pairs]*/, int32_t* d_counts /*[n_pairs]*/,
                                       void* stream);
pcd_status pcd_sift_match_batch(int device, const uint8_t* arena, const uint64_t* first_row /*[n_images+1]*/, int n_images,
                                const uint32_t* pairs /*[n_pairs][2]*/, int n_pairs, float max_ratio, float max_distance,
                                int cross_check, uint32_t* matches, uint64_t matches_capacity,
                                uint64_t* list_offset /*[n_pairs+1]*/);

/* Matcher object with the shape of lib/SiftGPU's SiftMatchGPU (lib/SiftGPU/SiftGPU.h:268-352) as the reference
 * drives it in feature/sift.cc:1227-1266 MatchSiftFeaturesGPU: two descriptor slots stay on the device, so
 * matching image i against many j uploads i once.  set_descriptors clips num to max_sift like
 * SiftMatchGPU::SetDescriptors; match = GetSiftMatch(max_match, match_buffer, distmax, ratiomax,
 * mutual_best_match) and returns the exact brute-force result (see above). */
typedef struct pcd_sift_matcher pcd_sift_matcher;
pcd_status pcd_sift_matcher_create(int device, int max_sift, pcd_sift_matcher** out);
void pcd_sift_matcher_destroy(pcd_sift_matcher* m);
pcd_status pcd_sift_matcher_set_max_sift(pcd_sift_matcher* m, int max_sift);
pcd_status pcd_sift_matcher_set_descriptors(pcd_sift_matcher* m, int index /*0|1*/, int num, const uint8_t* desc);
pcd_status pcd_sift_matcher_match(pcd_sift_matcher* m, int max_match, uint32_t* matches /*[max_match][2]*/,
                                  float distmax, float ratiomax, int mutual_best_match, int32_t* num_matches);

/* Guided matching: replaces feature/sift.cc:1092-1162 MatchGuidedSiftFeaturesCPU (the specification) and
 * :1274-1365 MatchGuidedSiftFeaturesGPU (lib/SiftGPU/SiftGPU.h:331-352 SetFeautreLocation / GetGuidedSiftMatch),
 * which feature/matching.cc:459-580 Guided{CPU,GPU}FeatureMatcher run once per verified image pair.
 * The result is the brute-force match set of sift.cc:55-144 on the distance matrix of sift.cc:171-204 with every
 * pair the geometric filter rejects scored 0 -- exactly the same as leaving the pair out of both scans.
 * loc: [n][2] float32 (x, y).  H / F: row-major float 3x3 (colmap passes Eigen::RowMajor .data()) or NULL; the
 * filter, one IEEE float32 operation at a time in this order (no FMA):
 *   H: h_i = (H[i][0] x1 + H[i][1] y1) + H[i][2]; r = (h0/h2 - x2)^2 + (h1/h2 - y2)^2; rejected iff r > h_max_residual
 *   F: a_i = (F[i][0] x1 + F[i][1] y1) + F[i][2]; b_j = (F[0][j] x2 + F[1][j] y2) + F[2][j];
 *      e = (x2 a0 + y2 a1) + a2; rejected iff (e e) / (((a0 a0 + a1 a1) + b0 b0) + b1 b1) > f_max_residual
 * (a NaN residual is kept, an infinite one rejected).  With both matrices a pair is rejected if either test rejects
 * it; with neither the result is exactly pcd_sift_match.  colmap passes max_error^2 for both thresholds
 * (sift.cc:1346-1353).  The device form follows pcd_sift_match_device (H / F are host pointers, read before the call
 * returns). */
pcd_status pcd_sift_match_guided(int device, const uint8_t* desc1, const float* loc1 /*[n1][2]*/, int n1,
                                 const uint8_t* desc2, const float* loc2 /*[n2][2]*/, int n2,
                                 const float* H /*row-major 3x3 or NULL*/, const float* F /*row-major 3x3 or NULL*/,
                                 float h_max_residual, float f_max_residual, float max_ratio, float max_distance,
                                 int cross_check, uint32_t* matches /*[n1][2]*/, int32_t* num_matches);
pcd_status pcd_sift_match_guided_device(int device, const uint8_t* d_desc1, const float* d_loc1, int n1,
                                        const uint8_t* d_desc2, const float* d_loc2, int n2, const float* H,
                                        const float* F, float h_max_residual, float f_max_residual, float max_ratio,
                                        float max_distance, int cross_check, int32_t* d_m12, int32_t* d_m21,
                                        uint32_t* d_matches, int32_t* d_num_matches, void* stream);

/* Guided batch: matching.cc:523-575 GuidedSiftGPUFeatureMatcher's per-pair loop in one launch set.  Arguments as
 * pcd_sift_match_batch[_device], plus a location arena ([rows][2] float32, indexed by the same first_row) and one
 * guide per pair; the thresholds are shared.  Per pair the result equals pcd_sift_match_guided with that pair's
 * matrices; a pair of mode PCD_SIFT_GUIDE_NONE equals pcd_sift_match. */
typedef enum { PCD_SIFT_GUIDE_NONE = 0, PCD_SIFT_GUIDE_H = 1, PCD_SIFT_GUIDE_F = 2, PCD_SIFT_GUIDE_HF = 3 } pcd_sift_guide_mode;
typedef struct {
  int32_t mode;   /* pcd_sift_guide_mode */
  float H[9];     /* row-major, read iff mode & PCD_SIFT_GUIDE_H */
  float F[9];     /* row-major, read iff mode & PCD_SIFT_GUIDE_F */
} pcd_sift_guide;
pcd_status pcd_sift_match_guided_batch_device(int device, const uint8_t* d_arena, const float* d_locs,
                                              const uint64_t* first_row /*[n_images+1]*/, int n_images,
                                              const uint32_t* pairs /*[n_pairs][2]*/, int n_pairs,
                                              const pcd_sift_guide* guides /*[n_pairs], host*/, float h_max_residual,
                                              float f_max_residual, float max_ratio, float max_distance,
                                              int cross_check, uint32_t* d_matches,
                                              const uint64_t* match_offset /*[n_pairs]*/,
                                              int32_t* d_counts /*[n_pairs]*/, void* stream);
pcd_status pcd_sift_match_guided_batch(int device, const uint8_t* arena, const float* locs /*[rows][2]*/,
                                       const uint64_t* first_row /*[n_images+1]*/, int n_images,
                                       const uint32_t* pairs /*[n_pairs][2]*/, int n_pairs,
                                       const pcd_sift_guide* guides /*[n_pairs]*/, float h_max_residual,
                                       float f_max_residual, float max_ratio, float max_distance, int cross_check,
                                       uint32_t* matches, uint64_t matches_capacity,
                                       uint64_t* list_offset /*[n_pairs+1]*/);

/* Matcher slots with locations (SiftMatchGPU::SetFeautreLocation, SiftGPU.h:331-335): reads n locations of slot
 * `index` (n = the count of its last set_descriptors, clipped to max_sift) at a stride of 2 + gap floats.
 * match_guided = GetGuidedSiftMatch (SiftGPU.h:343-352); hdistmax / fdistmax are the squared thresholds.  A slot
 * whose descriptors were set again after its locations makes it return PCD_ERR_INVALID; calling again without new
 * descriptors or locations reuses the slots (sift_test.cc:715-740). */
pcd_status pcd_sift_matcher_set_locations(pcd_sift_matcher* m, int index /*0|1*/, const float* loc, int gap);
pcd_status pcd_sift_matcher_match_guided(pcd_sift_matcher* m, int max_match, uint32_t* matches /*[max_match][2]*/,
                                         const float* H, const float* F, float distmax, float ratiomax,
                                         float hdistmax, float fdistmax, int mutual_best_match, int32_t* num_matches);

/* ------------------------------------------------------------------------
 * Profiling hooks used by bench.py (HIP events on the launch stream)
 * --------------------------------------------------------------------- */
typedef struct {
  char name[48];
  uint64_t launches;
  double total_ms;
} pcd_kernel_time;
pcd_status pcd_profile_enable(int on);
pcd_status pcd_profile_only(const char* scope);   /* time just this scope (NULL / "": all): two HIP events per timed
                                                      scope cost a few microseconds of stream time each */
pcd_status pcd_profile_reset(void);
/* fills up to cap entries, returns the number of distinct kernels in *count (syncs the device) */
pcd_status pcd_profile_get(pcd_kernel_time* entries, int cap, int* count);

/* Not declared here on purpose: the tuning hooks bench.py / tools / tests use (pcd_nn_set_tuning, pcd_nn_set_search,
 * pcd_nn_set_schedule(0 | 1): the brick kernel's work schedule, 1 = static rounds alone; pcd_nn_schedule_params and
 * pcd_nn_last_wave_records: its constants and the per-wavefront records of a statistics pass with bit 4;
 * pcd_nn_last_fb_wave_records: the same records of the fallback walk, bit 16;
 * pcd_nn_set_bookkeeping, pcd_sift_set_tuning(int nchunk, uint64_t batch_partials_int4): column chunks per stripe walk
 * and partial results per sub-batch in 16-byte units) set PROCESS-GLOBAL state -- they are for experiments on one
 * handle at a time, not part of the ABI, and the thread-safety statement at the top of this header does not cover
 * them. */

/* statistics of the last pcd_nn_query*(…, PCD_NN_AUTO) call on this handle */
typedef struct {
  uint64_t queries;
  uint64_t brick_groups;        /* wavefront work items of the brick kernel                 */
  uint64_t staged_points;       /* sum over groups of points staged through LDS             */
  uint64_t fallback_queries;    /* queries finished by the exact hierarchical kernel        */
  uint64_t fallback_points;     /* points scanned by that kernel                            */
  uint64_t pair_evals;          /* distance evaluations, both kernels                       */
} pcd_nn_stats;
pcd_status pcd_nn_last_stats(pcd_cloud* c, pcd_nn_stats* s);   /* syncs */

#ifdef __cplusplus
}
#endif
#endif /* PCDHIP_H_ */

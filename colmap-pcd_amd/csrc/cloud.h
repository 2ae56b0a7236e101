// cloud.h -- device-resident LiDAR cloud index (replaces PointCloudProcess +
// Kdtree of the reference: lidar/ply.cc:9-57, lidar/kdtree.cc:5-8).
//
// HBM layout (all hipMalloc'ed on one device):
//   pts4 [n]   float4 {x,y,z,0}     original (post-NaN-filter) row order  -- epilogue gathers, brute force
//   pn8  [n]   2 x float4 {x,y,z,0, nx,ny,nz,0}  original order           -- epilogue gathers: a winner's point AND
//                                   normal in ONE 32-byte record (one cache line instead of a line of pts4 and one of nrm4)
//   sorted [m] float4 {x,y,z,bits(global_idx)}  finite rows in cell-sorted order (x fastest):
//              one 16-B record per lane per load; a row of cells along x is one contiguous range
//   cell_start [ncells+1] uint32    exclusive prefix of per-cell counts
//   blk_aabb [records][8] float     the AABB tree of the exact fallback: a 64-ary tree over the OCCUPIED nodes of the
//                                   4x4x4 pyramid over the grid, 32 B per record, {lo.xyz, hi.x | hi.y, hi.z, bits(first),
//                                   bits(count)}.  A LEAF is a sub-block of 2x2x2 cells -- an x-range of 2 cells of ONE
//                                   quad row, i.e. one contiguous point range -- and first / count are that range in
//                                   `sorted`; an INNER node's first / count are the range of its children's records in
//                                   this array.  Only nodes that hold a point have a record; the children of a node are
//                                   contiguous, in ascending order of their position ci + 4 cj + 16 ck inside the node's
//                                   4x4x4 lattice (the walk breaks ties towards the lowest lane: the order is part of
//                                   the result's definition).  Levels are stored top down, each level's nodes in the
//                                   order of their parents, so the upper levels of the whole cloud are a few hundred KB
//                                   at the front of the array (workload M: 99 k records, 3 MB; the dense lattice the
//                                   records are compacted from is 4.7 M nodes, 151 MB, and lives only during the build).
//                                   The walk starts at a virtual top whose children are the records of the first level
//                                   with <= 64 lattice nodes (PyramidParams below).
//                                   An expansion tests up to 64 children with the exact float bound; a leaf is scanned.
#pragma once
#include <memory>

#include "common.h"

namespace pcd {

constexpr int kSortedSpare = 16;  // records behind the last point of `sorted` (copies of it): range reads may overrun
constexpr int kBlockCells = 4;  // cells per block edge (blocks carry tight AABBs for the exact fallback)

struct GridParams {
  float origin[3];
  float h, inv_h;
  int dims[3];    // cells
  int qdims[2];   // (dims[1]+1)/2, (dims[2]+1)/2: 2x2 (y,z) cell quads, see grid.h cell_index
  int bdims[3];   // blocks of kBlockCells^3 cells
  float slack;    // metres: bound on binning rounding, see nn.hip
};

// 64-ary AABB tree over the occupied nodes of the pyramid: level 0 = leaves (2x2x2-cell sub-blocks), level k+1 = 4x4x4
// nodes of level k, up to the first level with at most 64 lattice nodes (level nlev-2); level nlev-1 is a VIRTUAL top
// whose children are the occupied nodes of level nlev-2 in the order of their flat lattice index: the records
// root_first .. root_first + root_count - 1 of blk_aabb (root_count = 0: a cloud without a finite point).
constexpr int kMaxPyrLevels = 10;
struct PyramidParams {
  int nlev;                       // >= 2
  uint32_t root_first, root_count;
  int seed_dims[3];               // lattice of the fallback's seed table: 8x8x8-cell cubes (nn.hip fb_seed_table)
};
// an inner node's child range travels through the walk's stack as first | (count - 1) << 26
constexpr uint32_t kMaxPyrRecords = 1u << 26;

struct QueryScratch;                          // scratch.h
void free_query_scratch(QueryScratch* s);     // nn.hip

// ownership of a global index by a shard: local row or 0xFFFFFFFFFFFFFFFF
struct ShardIndex {
  uint32_t base, stride;
  uint64_t n;
  const uint32_t* g2l;   // NULL: base / stride arithmetic
  uint64_t g2l_n;
};
__device__ __forceinline__ uint64_t shard_local_row(const ShardIndex& si, uint32_t gi) {
  if (si.g2l) {
    const uint32_t l = gi < si.g2l_n ? si.g2l[gi] : 0xFFFFFFFFu;
    return l == 0xFFFFFFFFu ? ~0ull : (uint64_t)l;
  }
  if (gi < si.base || (gi - si.base) % si.stride != 0) return ~0ull;
  const uint64_t li = (uint64_t)(gi - si.base) / si.stride;
  return li < si.n ? li : ~0ull;
}

}  // namespace pcd

struct pcd_cloud {
  int device = 0;
  uint64_t n = 0;  // rows kept
  uint64_t m = 0;  // finite rows indexed in the grid
  uint32_t index_base = 0, index_stride = 1;
  // shards with an arbitrary row -> global index map (pcd_cloud_create_sharded): global index of local row i, and the
  // inverse over the whole cloud (0xFFFFFFFF = not a row of this shard).  Empty: global = index_base + i * index_stride.
  pcd::DevBuf<uint32_t> row_index, g2l;
  uint64_t g2l_n = 0;
  pcd::DevBuf<float4> pts4, pn8, sorted;   // pn8: 2 float4 per row
  pcd::DevBuf<uint32_t> cell_start;
  pcd::DevBuf<float> blk_aabb;
  pcd::GridParams grid{};
  pcd::PyramidParams pyr{};
  uint64_t ncells = 0, nblocks = 0, occupied = 0;
  float bb_lo[3] = {0, 0, 0}, bb_hi[3] = {0, 0, 0};   // tight bounds of the finite rows (valid when m > 0)
  double build_ms = 0;
  pcd::QueryScratch* scratch = nullptr;
  pcd::ShardIndex shard_index() const { return pcd::ShardIndex{index_base, index_stride, n, g2l.p, g2l_n}; }
};

namespace pcd {
// owner of a handle under construction: a failure path destroys it by returning; success hands it out with release()
struct CloudDeleter {
  void operator()(pcd_cloud* c) const { pcd_cloud_destroy(c); }
};
using CloudPtr = std::unique_ptr<pcd_cloud, CloudDeleter>;

// pcd_cloud_create with an explicit global index per row (row_index[n], host; NULL = index_base / index_stride) over
// a cloud of global_n rows in total
pcd_status cloud_create_indexed(const float* xyz, const float* nrm, uint64_t n, const pcd_cloud_options* opts,
                                const uint32_t* row_index, uint64_t global_n, pcd_cloud** out);
// A handle whose rows are produced on the device (voxel.hip): cloud_alloc_rows gives a handle on `device` with pts4 /
// pn8 allocated for n rows (index_base 0, stride 1) and no index; the caller writes every row of both arrays on stream
// s, then cloud_build_index builds the index.
pcd_status cloud_alloc_rows(int device, uint64_t n, CloudPtr& out);
// The index of a handle whose pts4 holds its n rows: bounds, cell size, cell table, sorted records, pyramid records
// (the stages are in cloud.hip).  pcd_cloud_create runs it after its row transform.  It synchronises s, and build_ms
// is its wall time.
pcd_status cloud_build_index(pcd_cloud* c, float cell_size, hipStream_t s);
// Refusal (PCD_ERR_UNSUPPORTED) of a shard or a strided handle by a pass over the neighbourhood of every row: `what`
// names the pass, `parts` what would cross handle borders, `verb` what to do on one handle instead.
inline pcd_status require_whole_cloud(const pcd_cloud* c, const char* what, const char* parts, const char* verb) {
  if (c->row_index.p || c->g2l.p || c->index_stride != 1 || c->index_base != 0) {
    set_error("%s needs ONE handle holding the whole cloud: %s of a shard (pcd_cloud_create_sharded, index_stride / "
              "index_base) cross handle borders; %s on one handle, download, then shard", what, parts, verb);
    return PCD_ERR_UNSUPPORTED;
  }
  return PCD_OK;
}
}

// cloud.hip -- build of the device-resident cloud index.
// Reference behaviour restated: lidar/ply.cc:33-57 (axis swap, NaN-row filter,
// order preserved); lidar/kdtree.cc:5-8 (index over x,y,z of every kept row).
// Host side: cloud_create_indexed (upload, row transform) and cloud_build_index, the driver of the build's six stages.
#include <chrono>
#include <cmath>

#include "cloud.h"
#include "grid.h"
#include "prim.h"

namespace pcd {

// ------------------------------------------------------------- kernels ----
// ply.cc:38-54: p' = (-y,-z,x), n' = (-ny,-nz,nx); row dropped if any of the six is NaN.
__global__ void k_flag_rows(const float* __restrict__ xyz, const float* __restrict__ nrm, uint64_t n, int layout,
                            uint32_t* __restrict__ keep) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = layout == PCD_LAYOUT_AOS32 ? xyz + 8 * i : xyz + 3 * i;
  const float* q = layout == PCD_LAYOUT_AOS32 ? xyz + 8 * i + 4 : nrm + 3 * i;
  bool bad = isnan(p[0]) || isnan(p[1]) || isnan(p[2]) || isnan(q[0]) || isnan(q[1]) || isnan(q[2]);
  keep[i] = bad ? 0u : 1u;
}

__global__ void k_compact_rows(const float* __restrict__ xyz, const float* __restrict__ nrm, uint64_t n, int layout,
                               int raw_frame, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                               float4* __restrict__ pts4, float4* __restrict__ pn8) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t dst = (uint32_t)i;
  if (raw_frame) {
    if (!keep[i]) return;
    dst = pos[i];
  }
  const float* p = layout == PCD_LAYOUT_AOS32 ? xyz + 8 * i : xyz + 3 * i;
  const float* q = layout == PCD_LAYOUT_AOS32 ? xyz + 8 * i + 4 : nrm + 3 * i;
  float4 a, b;
  if (raw_frame) {
    a = make_float4(-p[1], -p[2], p[0], 0.f);
    b = make_float4(-q[1], -q[2], q[0], 0.f);
  } else {
    a = make_float4(p[0], p[1], p[2], 0.f);
    b = make_float4(q[0], q[1], q[2], 0.f);
  }
  pts4[dst] = a;
  pn8[2 * (size_t)dst] = a;
  pn8[2 * (size_t)dst + 1] = b;
}

__device__ inline int f2ord(float f) {
  int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ inline float ord2f(int i) {
  int j = i >= 0 ? i : i ^ 0x7fffffff;
#ifdef __HIP_DEVICE_COMPILE__
  return __int_as_float(j);
#else
  float f;
  std::memcpy(&f, &j, 4);
  return f;
#endif
}

// bbox of rows with three finite coordinates; bb[0..2] = min (ordered ints), bb[3..5] = max, bb[6] = count
__global__ void k_bbox(const float4* __restrict__ pts4, uint64_t n, int* __restrict__ bb,
                       unsigned long long* __restrict__ cnt) {
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  unsigned c = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    float4 p = pts4[i];
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
      int o[3] = {f2ord(p.x), f2ord(p.y), f2ord(p.z)};
      for (int d = 0; d < 3; ++d) {
        lo[d] = min(lo[d], o[d]);
        hi[d] = max(hi[d], o[d]);
      }
      ++c;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    for (int d = 0; d < 3; ++d) {
      lo[d] = min(lo[d], __shfl_xor(lo[d], off));
      hi[d] = max(hi[d], __shfl_xor(hi[d], off));
    }
    c += __shfl_xor(c, off);
  }
  if ((threadIdx.x & 63) == 0) {
    for (int d = 0; d < 3; ++d) {
      atomicMin(&bb[d], lo[d]);
      atomicMax(&bb[3 + d], hi[d]);
    }
    atomicAdd(cnt, (unsigned long long)c);
  }
}

// per-cell histogram; non-finite rows are skipped (they keep an index but can never win, see nn.hip)
__global__ void k_cell_hist(const float4* __restrict__ pts4, uint64_t n, GridParams g, uint32_t* __restrict__ count) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 p = pts4[i];
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return;
  atomicAdd(&count[cell_of(g, p.x, p.y, p.z)], 1u);
}

__global__ void k_count_nonzero(const uint32_t* __restrict__ count, uint64_t ncells, unsigned long long* __restrict__ out) {
  unsigned c = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < ncells; i += (uint64_t)gridDim.x * blockDim.x)
    c += count[i] != 0;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// sort keys: cell id for finite rows, 0xFFFFFFFF for the rest (sorted to the tail, never referenced)
__global__ void k_cell_keys(const float4* __restrict__ pts4, uint64_t n, GridParams g, uint32_t* __restrict__ keys,
                            uint32_t* __restrict__ vals) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 p = pts4[i];
  bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  keys[i] = fin ? cell_of(g, p.x, p.y, p.z) : 0xFFFFFFFFu;
  vals[i] = (uint32_t)i;
}

__global__ void k_gather_sorted(const float4* __restrict__ pts4, const uint32_t* __restrict__ order, uint64_t m,
                                uint32_t index_base, uint32_t index_stride, const uint32_t* __restrict__ row_index,
                                float4* __restrict__ sorted) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= m + kSortedSpare) return;
  // rows m .. m+15 repeat the last record: the brick kernel reads ranges in groups of 4 records and may run up to
  // 3 records past the end of the last range (brick_kernel.h); a repeated real point cannot change a minimum
  uint32_t src = order[i < m ? i : m - 1];
  float4 p = pts4[src];
  p.w = __uint_as_float(row_index ? row_index[src] : index_base + src * index_stride);
  sorted[i] = p;
}

// Pyramid level 0 = LEAVES: every sub-block of 2x2x2 cells (half a quad row of two x-cells: ONE contiguous point
// range) with its tight box and its range, {lo.xyz, hi.x | hi.y, hi.z, bits(first point), bits(count)}.  One wavefront
// per leaf.  (Round 2 had 4x4x4-cell blocks as level 0 with 8 sub-block records each: a far query then paid one walk
// step per BLOCK of the shell between its true distance and the blocks' looser bounds; with the sub-blocks as the
// children of a 64-ary node one step tests 64 of them.)
__global__ void k_leaf_aabb(const float4* __restrict__ sorted, const uint32_t* __restrict__ cell_start, GridParams g,
                            int sdx, int sdy, int sdz, float* __restrict__ aabb) {
  const int lane = threadIdx.x & 63;
  const uint64_t id = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  if (id >= (uint64_t)sdx * sdy * sdz) return;
  const int sx = (int)(id % sdx), sy = (int)((id / sdx) % sdy), sz = (int)(id / ((uint64_t)sdx * sdy));
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int cx0 = min(2 * sx, g.dims[0]), cx1 = min(cx0 + 2, g.dims[0]);
  const uint64_t rowbase = quad_row_base(g, sy, sz);
  const uint32_t s = cell_start[rowbase + 4 * cx0], e = cell_start[rowbase + 4 * cx1];
  for (uint32_t i = s + lane; i < e; i += 64) {
    const float4 p = sorted[i];
    lo[0] = fminf(lo[0], p.x); hi[0] = fmaxf(hi[0], p.x);
    lo[1] = fminf(lo[1], p.y); hi[1] = fmaxf(hi[1], p.y);
    lo[2] = fminf(lo[2], p.z); hi[2] = fmaxf(hi[2], p.z);
  }
  if (s != e)
    for (int off = 32; off > 0; off >>= 1)
      for (int d = 0; d < 3; ++d) {
        lo[d] = fminf(lo[d], __shfl_xor(lo[d], off));
        hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off));
      }
  if (lane == 0) {
    float* o = aabb + 8 * id;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2];
    o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
    o[6] = __uint_as_float(s); o[7] = __uint_as_float(e - s);
  }
}

// pyramid level k+1 from level k: union of the <= 64 children boxes (empty = {+inf, -inf})
__global__ void k_pyramid_level(float* __restrict__ aabb, uint32_t off_child, int cdx, int cdy, int cdz,
                                uint32_t off_parent, int pdx, int pdy, int pdz) {
  const uint64_t id = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (id >= (uint64_t)pdx * pdy * pdz) return;
  const int px = (int)(id % pdx), py = (int)((id / pdx) % pdy), pz = (int)(id / ((uint64_t)pdx * pdy));
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = 0; k < 4; ++k)
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i < 4; ++i) {
        const int cx = 4 * px + i, cy = 4 * py + j, cz = 4 * pz + k;
        if (cx >= cdx || cy >= cdy || cz >= cdz) continue;
        const float* a = aabb + 8 * ((uint64_t)off_child + ((uint64_t)cz * cdy + cy) * cdx + cx);
        for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], a[d]); hi[d] = fmaxf(hi[d], a[3 + d]); }
      }
  float* o = aabb + 8 * ((uint64_t)off_parent + id);
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2]; o[6] = 0.f; o[7] = 0.f;
}

// ---- compaction of the dense pyramid to its occupied nodes (cloud.h: blk_aabb) ----
// The dense levels above are a scaffold: the walk reads a 64-ary tree over the nodes that hold a point, built from the
// top down.  A level's occupied nodes are kept as a list of their flat lattice indices in the order of their records;
// per parent of the list a 64-bit mask of its occupied children (a wavefront's ballot, lane = ci + 4 cj + 16 ck), the
// scan of the masks' popcounts over the list = the first child record of every parent, and a child's record index =
// that + popcount(mask below its lane).  So the children of a node are contiguous and in lane order, and the
// children of consecutive parents follow each other.
__device__ __forceinline__ bool node_occupied(const float* __restrict__ dense, uint64_t id) {
  return dense[8 * id] <= dense[8 * id + 3];   // (an empty node's box is {+inf, -inf})
}

__global__ void k_count_occupied(const float* __restrict__ dense, uint64_t first, uint64_t n,
                                 unsigned long long* __restrict__ out) {
  unsigned c = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    c += node_occupied(dense, first + i) ? 1u : 0u;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// the children of the virtual top: the occupied nodes of the top real level (<= 64 nodes) by flat index; one wavefront
__global__ void k_top_list(const float* __restrict__ dense, uint32_t off_top, uint32_t ntop, uint32_t* __restrict__ list) {
  const uint32_t lane = threadIdx.x;
  const bool occ = lane < ntop && node_occupied(dense, (uint64_t)off_top + lane);
  const unsigned long long mask = __ballot(occ);
  if (occ) list[__popcll(mask & ((1ull << lane) - 1))] = lane;
}

// one wavefront per parent of `list`: the lane's child (flat index on the child level) and the mask of occupied children
__device__ __forceinline__ unsigned long long child_mask(const float* __restrict__ dense, uint32_t parent, int pdx, int pdy,
                                                         uint32_t off_child, int cdx, int cdy, int cdz, int lane,
                                                         uint32_t* child) {
  const int px = (int)(parent % (uint32_t)pdx), py = (int)((parent / (uint32_t)pdx) % (uint32_t)pdy),
            pz = (int)(parent / ((uint32_t)pdx * (uint32_t)pdy));
  const int cx = 4 * px + (lane & 3), cy = 4 * py + ((lane >> 2) & 3), cz = 4 * pz + (lane >> 4);
  const bool in = cx < cdx && cy < cdy && cz < cdz;
  *child = in ? (uint32_t)(((uint64_t)cz * cdy + cy) * cdx + cx) : 0u;
  return __ballot(in && node_occupied(dense, (uint64_t)off_child + *child));
}

__global__ void k_child_count(const float* __restrict__ dense, const uint32_t* __restrict__ list, uint32_t np, int pdx,
                              int pdy, uint32_t off_child, int cdx, int cdy, int cdz, uint32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const uint64_t k = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  if (k >= np) return;
  uint32_t child;
  const unsigned long long mask = child_mask(dense, list[k], pdx, pdy, off_child, cdx, cdy, cdz, lane, &child);
  if (lane == 0) count[k] = (uint32_t)__popcll(mask);
}

// the parents' records {box, first child record, children} and the list of the child level
__global__ void k_emit_children(const float* __restrict__ dense, const uint32_t* __restrict__ list, uint32_t np,
                                uint32_t off_parent, int pdx, int pdy, uint32_t off_child, int cdx, int cdy, int cdz,
                                const uint32_t* __restrict__ first, uint32_t base_parent, uint32_t base_child,
                                uint32_t* __restrict__ child_list, float* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const uint64_t k = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  if (k >= np) return;
  const uint32_t parent = list[k];
  uint32_t child;
  const unsigned long long mask = child_mask(dense, parent, pdx, pdy, off_child, cdx, cdy, cdz, lane, &child);
  const uint32_t f = first[k];
  if ((mask >> lane) & 1) child_list[f + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = child;
  if (lane == 0) {
    const float* a = dense + 8 * ((uint64_t)off_parent + parent);
    float* o = rec + 8 * ((uint64_t)base_parent + k);
    for (int d = 0; d < 6; ++d) o[d] = a[d];
    o[6] = __uint_as_float(base_child + f); o[7] = __uint_as_float((uint32_t)__popcll(mask));
  }
}

__global__ void k_emit_leaves(const float4* __restrict__ dense_leaves, const uint32_t* __restrict__ list, uint32_t n,
                              float4* __restrict__ rec) {
  const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint64_t src = list[k];
  rec[2 * k] = dense_leaves[2 * src];
  rec[2 * k + 1] = dense_leaves[2 * src + 1];
}

// ------------------------------------------------------------ host side ----
static void set_dims(GridParams& g, const float lo[3], const float hi[3], float h) {
  g.h = h;
  g.inv_h = 1.0f / h;
  float ext = 0.f;
  for (int d = 0; d < 3; ++d) {
    g.origin[d] = lo[d];
    double e = (double)hi[d] - (double)lo[d];
    long c = (long)std::floor(e / h) + 1;
    if (c < 1) c = 1;
    g.dims[d] = (int)c;
    g.bdims[d] = (g.dims[d] + kBlockCells - 1) / kBlockCells;
    ext = std::fmax(ext, (float)e);
    ext = std::fmax(ext, std::fmax(std::fabs(lo[d]), std::fabs(hi[d])));
  }
  g.qdims[0] = (g.dims[1] + 1) / 2;
  g.qdims[1] = (g.dims[2] + 1) / 2;
  // bound on |true coordinate - nominal cell face| caused by float binning (see nn.hip "slack")
  g.slack = ext * 9.6e-7f + 1e-30f;
}

// cell table entries (quad-row order pads odd y / z extents with empty cells)
static uint64_t num_cells(const GridParams& g) { return (uint64_t)g.dims[0] * g.qdims[0] * g.qdims[1] * 4u; }

constexpr uint64_t kMaxCells = 1ull << 26;
constexpr double kTargetOcc = 24.0;  // mean points per occupied cell

// ---- the index build, stage by stage (cloud_build_index is the driver).  The stages allocate and free their scratch in
// a fixed order: what hipMalloc hands out next, to the handle's arrays and the query scratch too, depends on it ----
// the dense levels of the pyramid: a scaffold of one build (151 MB for workload M, 98 % of it empty nodes)
struct Lattice {
  int nreal = 1;                  // real levels (level 0 = leaves)
  int dims[kMaxPyrLevels][3];
  uint32_t off[kMaxPyrLevels] = {};   // node offset of each level in `nodes`
  DevBuf<float> nodes;            // 8 floats per node, the record layout of blk_aabb
  uint64_t count(int l) const { return (uint64_t)dims[l][0] * dims[l][1] * dims[l][2]; }
};

// bounds (k_bbox): reads pts4; writes c->m, bb_lo, bb_hi (zeros without a finite row)
static pcd_status index_bounds(pcd_cloud* c, DevBuf<int>& bb, DevBuf<unsigned long long>& cnt, hipStream_t s) {
  const uint64_t n = c->n;
  PCD_TRY(bb.reserve(6));
  PCD_TRY(cnt.reserve(2));
  int init[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
  PCD_HIP_TRY(hipMemcpyAsync(bb.p, init, sizeof init, hipMemcpyHostToDevice, s));
  PCD_HIP_TRY(hipMemsetAsync(cnt.p, 0, 2 * sizeof(unsigned long long), s));
  if (n)
    hipLaunchKernelGGL(k_bbox, dim3(std::min<unsigned>(div_up(n, 256), 2048)), dim3(256), 0, s, c->pts4.p, n, bb.p, cnt.p);
  int hb[6];
  unsigned long long hc[2];
  PCD_HIP_TRY(hipMemcpyAsync(hb, bb.p, sizeof hb, hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipMemcpyAsync(hc, cnt.p, sizeof hc, hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipStreamSynchronize(s));
  c->m = hc[0];
  for (int d = 0; d < 3; ++d) { c->bb_lo[d] = c->m ? ord2f(hb[d]) : 0.f; c->bb_hi[d] = c->m ? ord2f(hb[3 + d]) : 0.f; }
  return PCD_OK;
}

// histogram of the finite rows over the cells of c->grid into count[0 .. cells], the number of occupied cells into
// *occupied (host): enqueued on s, so *occupied is valid after the caller's next synchronisation
static pcd_status cell_histogram(const pcd_cloud* c, uint32_t* count, unsigned long long* d_cnt,
                                 unsigned long long* occupied, hipStream_t s) {
  const uint64_t n = c->n, nc = num_cells(c->grid);
  PCD_HIP_TRY(hipMemsetAsync(count, 0, (nc + 1) * sizeof(uint32_t), s));
  PCD_HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), s));
  if (n) hipLaunchKernelGGL(k_cell_hist, dim3(div_up(n, 256)), dim3(256), 0, s, c->pts4.p, n, c->grid, count);
  hipLaunchKernelGGL(k_count_nonzero, dim3(std::min<unsigned>(div_up(nc, 256), 4096)), dim3(256), 0, s, count, nc, d_cnt);
  PCD_HIP_TRY(hipMemcpyAsync(occupied, d_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  return PCD_OK;
}

// cell size: the user's value (raised to the cell budget), or up to six rounds towards kTargetOcc points per occupied
// cell.  Reads m and the bounds; sets h.  The rounds use c->grid and c->cell_start as their scratch.
static pcd_status choose_cell_size(pcd_cloud* c, float user_h, DevBuf<unsigned long long>& cnt, hipStream_t s, float& h) {
  const float *lo = c->bb_lo, *hi = c->bb_hi;
  const double ext[3] = {(double)hi[0] - lo[0], (double)hi[1] - lo[1], (double)hi[2] - lo[2]};
  const double maxext = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
  // the smallest cell whose grid over the bounds stays within kMaxCells
  double hb = std::cbrt((ext[0] + 1e-3) * (ext[1] + 1e-3) * (ext[2] + 1e-3) / (double)kMaxCells);
  for (int it = 0; it < 64; ++it) {
    double cells = (std::floor(ext[0] / hb) + 1) * (std::floor(ext[1] / hb) + 1) * (std::floor(ext[2] / hb) + 1);
    if (cells <= (double)kMaxCells) break;
    hb *= 1.05;
  }
  const double hmin = std::fmax(hb, 1e-6 * std::fmax(maxext, 1e-3));
  if (c->m == 0 || maxext <= 0) {
    h = user_h > 0 ? user_h : 1.0f;
  } else if (user_h > 0) {
    h = (float)std::fmax((double)user_h, hmin);
  } else {
    // start from a surface-like guess and refine with measured occupancy
    double hguess = std::sqrt(kTargetOcc * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2] + 1e-6) / (double)c->m);
    h = (float)std::fmin(std::fmax(hguess, hmin), std::fmax(maxext, hmin));
    for (int it = 0; it < 6; ++it) {
      set_dims(c->grid, lo, hi, h);
      PCD_TRY(c->cell_start.reserve(num_cells(c->grid) + 1));
      unsigned long long occupied = 0;
      PCD_TRY(cell_histogram(c, c->cell_start.p, cnt.p, &occupied, s));
      PCD_HIP_TRY(hipStreamSynchronize(s));
      double occ = (double)c->m / (double)std::max<unsigned long long>(occupied, 1);
      if (occ > 0.75 * kTargetOcc && occ < 1.5 * kTargetOcc) break;
      // occupancy ~ h^2 on surfaces, h^3 in volumes: use exponent 2.5
      double hn = h * std::pow(kTargetOcc / occ, 1.0 / 2.5);
      hn = std::fmin(std::fmax(hn, hmin), std::fmax(maxext, hmin));
      if (std::fabs(hn - h) < 1e-3 * h) break;
      h = (float)hn;
    }
  }
  return PCD_OK;
}

// cell table: the grid at cell size h, the budget check, the final histogram and its exclusive scan.  Writes c->grid,
// ncells, nblocks, cell_start, occupied.
static pcd_status build_cell_table(pcd_cloud* c, float h, DevBuf<unsigned long long>& cnt, hipStream_t s) {
  set_dims(c->grid, c->bb_lo, c->bb_hi, h);
  c->ncells = num_cells(c->grid);
  c->nblocks = (uint64_t)c->grid.bdims[0] * c->grid.bdims[1] * c->grid.bdims[2];
  if (c->ncells > kMaxCells * 2) {
    set_error("grid of %llu cells exceeds the budget", (unsigned long long)c->ncells);
    return PCD_ERR_UNSUPPORTED;
  }
  PCD_TRY(c->cell_start.reserve(c->ncells + 1));
  DevBuf<uint32_t> counts;
  PCD_TRY(counts.reserve(c->ncells + 1));
  unsigned long long occupied = 0;
  PCD_TRY(cell_histogram(c, counts.p, cnt.p, &occupied, s));
  DevBuf<char> tmp;
  PCD_TRY(exclusive_sum(tmp, counts.p, c->cell_start.p, 0u, c->ncells + 1, s));
  PCD_HIP_TRY(hipStreamSynchronize(s));
  c->occupied = occupied;
  return PCD_OK;
}

// sorted records: rows by cell (the stable radix sort keeps the original order inside a cell), gathered with their
// global index.  Reads pts4, grid, m; writes c->sorted.
static pcd_status sort_rows(pcd_cloud* c, hipStream_t s) {
  const uint64_t n = c->n;
  PCD_TRY(c->sorted.reserve(c->m + kSortedSpare));   // spare records, see k_gather_sorted
  if (n == 0) return PCD_OK;
  DevBuf<uint32_t> k0, k1, v0, v1;
  PCD_TRY(k0.reserve(n)); PCD_TRY(k1.reserve(n)); PCD_TRY(v0.reserve(n)); PCD_TRY(v1.reserve(n));
  hipLaunchKernelGGL(k_cell_keys, dim3(div_up(n, 256)), dim3(256), 0, s, c->pts4.p, n, c->grid, k0.p, v0.p);
  DevBuf<char> tmp;
  PCD_TRY(sort_pairs(tmp, k0.p, k1.p, v0.p, v1.p, n, 0, 32, s));
  if (c->m)
    hipLaunchKernelGGL(k_gather_sorted, dim3(div_up(c->m + kSortedSpare, 256)), dim3(256), 0, s, c->pts4.p, v1.p, c->m,
                       c->index_base, c->index_stride, c->row_index.p, c->sorted.p);
  PCD_HIP_TRY(hipStreamSynchronize(s));   // the keys go out of scope
  return PCD_OK;
}

// lattice: leaves (2x2x2-cell sub-blocks: tight box + point range) and the coarser levels, dense.  Reads sorted,
// cell_start, grid; writes L, c->pyr.nlev and c->pyr.seed_dims.  Enqueues only.
static pcd_status build_lattice(pcd_cloud* c, Lattice& L, hipStream_t s) {
  const GridParams& g = c->grid;
  L.dims[0][0] = (g.dims[0] + 1) / 2; L.dims[0][1] = g.qdims[0]; L.dims[0][2] = g.qdims[1];
  const uint64_t nleaves = L.count(0);
  uint64_t total_nodes = nleaves;
  // real levels until one has at most 64 nodes; above it sits a VIRTUAL top whose children are ALL nodes of that level,
  // one per lane (k_nn_fallback): for workload M's grid that is 5 x 2 x 5 = 50 nodes -- the walk starts there instead of
  // expanding a root of 1 and a level of 4 nodes first (two expansions and two pops less per query)
  while (L.nreal < kMaxPyrLevels - 1) {
    if (L.count(L.nreal - 1) <= 64) break;
    for (int d = 0; d < 3; ++d) L.dims[L.nreal][d] = (L.dims[L.nreal - 1][d] + 3) / 4;
    L.off[L.nreal] = (uint32_t)total_nodes;
    total_nodes += L.count(L.nreal);
    L.nreal++;
  }
  if (L.count(L.nreal - 1) > 64) {
    set_error("grid too large for %d pyramid levels", kMaxPyrLevels);
    return PCD_ERR_UNSUPPORTED;
  }
  for (int d = 0; d < 3; ++d) c->pyr.seed_dims[d] = (g.dims[d] + 7) / 8;   // (cell >> 3 for every cell of the grid)
  c->pyr.nlev = L.nreal + 1;   // + the virtual top
  PCD_TRY(L.nodes.reserve(8 * total_nodes));
  hipLaunchKernelGGL(k_leaf_aabb, dim3(div_up(nleaves * 64, 256)), dim3(256), 0, s, c->sorted.p, c->cell_start.p, g,
                     L.dims[0][0], L.dims[0][1], L.dims[0][2], L.nodes.p);
  for (int l = 1; l < L.nreal; ++l) {
    const int *cd = L.dims[l - 1], *pd = L.dims[l];
    hipLaunchKernelGGL(k_pyramid_level, dim3(div_up(L.count(l), 256)), dim3(256), 0, s, L.nodes.p, L.off[l - 1], cd[0],
                       cd[1], cd[2], L.off[l], pd[0], pd[1], pd[2]);
  }
  return PCD_OK;
}

// tree: the records of the occupied nodes (cloud.h), top down, children contiguous and in lane order.  Reads L; writes
// c->blk_aabb, c->pyr.root_first and root_count.
static pcd_status compact_tree(pcd_cloud* c, const Lattice& L, hipStream_t s) {
  const int nreal = L.nreal;
  const float* dense = L.nodes.p;
  DevBuf<unsigned long long> occ;
  unsigned long long hocc[kMaxPyrLevels] = {};
  PCD_TRY(occ.reserve(kMaxPyrLevels));
  PCD_HIP_TRY(hipMemsetAsync(occ.p, 0, kMaxPyrLevels * sizeof(unsigned long long), s));
  for (int l = 0; l < nreal; ++l)
    hipLaunchKernelGGL(k_count_occupied, dim3(std::min<unsigned>(div_up(L.count(l), 256), 4096)), dim3(256), 0, s,
                       dense, (uint64_t)L.off[l], L.count(l), occ.p + l);
  PCD_HIP_TRY(hipMemcpyAsync(hocc, occ.p, nreal * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipStreamSynchronize(s));
  uint64_t base[kMaxPyrLevels], total_rec = 0, max_level = 1;
  for (int l = nreal - 1; l >= 0; --l) {
    base[l] = total_rec;
    total_rec += hocc[l];
    max_level = std::max<uint64_t>(max_level, hocc[l]);
  }
  if (total_rec >= kMaxPyrRecords) {   // (cannot happen within the cell budget: the lattice itself has fewer nodes)
    set_error("%llu pyramid records exceed the walk's range encoding", (unsigned long long)total_rec);
    return PCD_ERR_UNSUPPORTED;
  }
  c->pyr.root_first = (uint32_t)base[nreal - 1];
  c->pyr.root_count = (uint32_t)hocc[nreal - 1];
  PCD_TRY(c->blk_aabb.reserve(8 * std::max<uint64_t>(total_rec, 1)));
  if (total_rec == 0) {   // one record that is never a child: defined bytes for the walk's clamped load
    PCD_HIP_TRY(hipMemsetAsync(c->blk_aabb.p, 0, 8 * sizeof(float), s));
    return PCD_OK;
  }
  DevBuf<uint32_t> list_a, list_b, nchild, first;
  DevBuf<char> tmp;
  PCD_TRY(list_a.reserve(max_level)); PCD_TRY(list_b.reserve(max_level));
  PCD_TRY(nchild.reserve(max_level)); PCD_TRY(first.reserve(max_level));
  uint32_t *cur = list_a.p, *nxt = list_b.p;
  hipLaunchKernelGGL(k_top_list, dim3(1), dim3(64), 0, s, dense, L.off[nreal - 1], (uint32_t)L.count(nreal - 1), cur);
  for (int l = nreal - 1; l >= 1; --l) {
    const uint32_t np = (uint32_t)hocc[l];
    const int *cd = L.dims[l - 1], *pd = L.dims[l];
    hipLaunchKernelGGL(k_child_count, dim3(div_up((uint64_t)np * 64, 256)), dim3(256), 0, s, dense, cur, np, pd[0], pd[1],
                       L.off[l - 1], cd[0], cd[1], cd[2], nchild.p);
    PCD_TRY(exclusive_sum(tmp, nchild.p, first.p, 0u, np, s));
    hipLaunchKernelGGL(k_emit_children, dim3(div_up((uint64_t)np * 64, 256)), dim3(256), 0, s, dense, cur, np, L.off[l],
                       pd[0], pd[1], L.off[l - 1], cd[0], cd[1], cd[2], first.p, (uint32_t)base[l], (uint32_t)base[l - 1],
                       nxt, c->blk_aabb.p);
    std::swap(cur, nxt);
  }
  hipLaunchKernelGGL(k_emit_leaves, dim3(div_up(hocc[0], 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(dense),
                     cur, (uint32_t)hocc[0], reinterpret_cast<float4*>(c->blk_aabb.p + 8 * base[0]));
  PCD_HIP_TRY(hipStreamSynchronize(s));   // the lists go out of scope
  return PCD_OK;
}

// the rows of a handle: n, pts4 and pn8 (never empty allocations: kernels and the walk may form their addresses)
static pcd_status reserve_rows(pcd_cloud* c, uint64_t n) {
  PCD_REQUIRE(n < 0xFFFFFFF0ull, "more than 2^32 rows");
  c->n = n;
  PCD_TRY(c->pts4.reserve(std::max<uint64_t>(n, 1)));
  PCD_TRY(c->pn8.reserve(2 * std::max<uint64_t>(n, 1)));
  return PCD_OK;
}

pcd_status cloud_alloc_rows(int device, uint64_t n, CloudPtr& out) {
  out.reset(new pcd_cloud());
  out->device = device;
  return reserve_rows(out.get(), n);
}

pcd_status cloud_build_index(pcd_cloud* c, float cell_size, hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  DevBuf<int> bb;                   // device results of the bounds pass ...
  DevBuf<unsigned long long> cnt;   // ... and of the histograms: freed last
  Lattice L;                        // lives to the end of the build and no longer
  float h = 0.f;
  PCD_TRY(index_bounds(c, bb, cnt, s));
  PCD_TRY(choose_cell_size(c, cell_size, cnt, s, h));
  PCD_TRY(build_cell_table(c, h, cnt, s));
  PCD_TRY(sort_rows(c, s));
  PCD_TRY(build_lattice(c, L, s));
  PCD_TRY(compact_tree(c, L, s));
  PCD_HIP_TRY(hipStreamSynchronize(s));   // the scaffold and the scratch go out of scope
  PCD_HIP_TRY(hipGetLastError());
  c->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" {

void pcd_cloud_options_default(pcd_cloud_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->layout = PCD_LAYOUT_XYZ_NRM;
  o->raw_lidar_frame = 1;
  o->index_stride = 1;
}

pcd_status pcd_cloud_create(const float* xyz, const float* nrm, uint64_t n, const pcd_cloud_options* opts,
                            pcd_cloud** out) {
  return pcd::guard([&]() -> pcd_status {
  return pcd::cloud_create_indexed(xyz, nrm, n, opts, nullptr, 0, out);
  });
}

}  // extern "C"

__global__ static void k_fill_g2l(const uint32_t* __restrict__ row_index, uint64_t n, uint32_t* __restrict__ g2l) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i < n) g2l[row_index[i]] = (uint32_t)i;
}

pcd_status pcd::cloud_create_indexed(const float* xyz, const float* nrm, uint64_t n, const pcd_cloud_options* opts,
                                     const uint32_t* row_index, uint64_t global_n, pcd_cloud** out) {
  PCD_REQUIRE(out, "out is null");
  *out = nullptr;
  pcd_cloud_options o;
  if (opts) o = *opts; else pcd_cloud_options_default(&o);
  PCD_REQUIRE(o.layout == PCD_LAYOUT_XYZ_NRM || o.layout == PCD_LAYOUT_AOS32, "unknown layout");
  PCD_REQUIRE(n == 0 || xyz, "xyz is null");
  PCD_REQUIRE(n == 0 || o.layout == PCD_LAYOUT_AOS32 || nrm, "nrm is null");
  PCD_REQUIRE(n < 0xFFFFFFF0ull, "more than 2^32 rows");
  if (o.index_stride == 0) o.index_stride = 1;
  PCD_REQUIRE(!(o.raw_lidar_frame && (o.index_stride != 1 || o.index_base != 0)),
              "sharded clouds (index_stride/base) need raw_lidar_frame = 0");
  PCD_REQUIRE(o.cell_size >= 0 && std::isfinite(o.cell_size), "cell_size");
  PCD_TRY(require_device(o.device));

  const auto t0 = std::chrono::steady_clock::now();
  CloudPtr c(new pcd_cloud());   // destroyed by every failing return below
  c->device = o.device;
  c->index_base = o.index_base;
  c->index_stride = o.index_stride;
  hipStream_t s = nullptr;
  if (row_index) {
    PCD_REQUIRE(!o.raw_lidar_frame, "indexed shards need raw_lidar_frame = 0");
    PCD_TRY(c->row_index.reserve(std::max<uint64_t>(n, 1)));
    PCD_TRY(c->g2l.reserve(std::max<uint64_t>(global_n, 1)));
    c->g2l_n = global_n;
    if (n) PCD_HIP_TRY(hipMemcpy(c->row_index.p, row_index, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    PCD_HIP_TRY(hipMemset(c->g2l.p, 0xFF, std::max<uint64_t>(global_n, 1) * sizeof(uint32_t)));
    if (n) hipLaunchKernelGGL(k_fill_g2l, dim3(div_up(n, 256)), dim3(256), 0, s, c->row_index.p, n, c->g2l.p);
  }

  const size_t row = o.layout == PCD_LAYOUT_AOS32 ? 8 : 3;
  DevBuf<float> d_xyz, d_nrm;
  DevBuf<uint32_t> keep, pos;
  PCD_TRY(d_xyz.reserve(std::max<size_t>(n * row, 1)));
  PCD_TRY(d_nrm.reserve(std::max<size_t>(n * 3, 1)));
  if (n) {
    PCD_HIP_TRY(hipMemcpy(d_xyz.p, xyz, n * row * sizeof(float), hipMemcpyHostToDevice));
    if (o.layout == PCD_LAYOUT_XYZ_NRM) PCD_HIP_TRY(hipMemcpy(d_nrm.p, nrm, n * 3 * sizeof(float), hipMemcpyHostToDevice));
  }
  uint64_t kept = n;
  if (o.raw_lidar_frame && n) {
    PCD_TRY(keep.reserve(n)); PCD_TRY(pos.reserve(n));
    hipLaunchKernelGGL(k_flag_rows, dim3(div_up(n, 256)), dim3(256), 0, s, d_xyz.p, d_nrm.p, n, o.layout, keep.p);
    DevBuf<char> tmp;
    PCD_TRY(exclusive_sum(tmp, keep.p, pos.p, 0u, n, s));
    uint32_t lastp = 0, lastk = 0;
    PCD_HIP_TRY(hipMemcpy(&lastp, pos.p + (n - 1), 4, hipMemcpyDeviceToHost));
    PCD_HIP_TRY(hipMemcpy(&lastk, keep.p + (n - 1), 4, hipMemcpyDeviceToHost));
    kept = (uint64_t)lastp + lastk;
  }
  PCD_TRY(reserve_rows(c.get(), kept));
  if (n)
    hipLaunchKernelGGL(k_compact_rows, dim3(div_up(n, 256)), dim3(256), 0, s, d_xyz.p, d_nrm.p, n, o.layout,
                       o.raw_lidar_frame, keep.p, pos.p, c->pts4.p, c->pn8.p);
  if (hipStreamSynchronize(s) != hipSuccess) { set_error("row transform failed"); return PCD_ERR_HIP; }
  PCD_TRY(cloud_build_index(c.get(), o.cell_size, s));
  c->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = c.release();
  return PCD_OK;
}

extern "C" {

void pcd_cloud_destroy(pcd_cloud* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  pcd::free_query_scratch(c->scratch);
  delete c;
}

uint64_t pcd_cloud_size(const pcd_cloud* c) { return c ? c->n : 0; }

pcd_status pcd_cloud_get_info(const pcd_cloud* c, pcd_cloud_info* info) {
  PCD_REQUIRE(c && info, "null pointer");
  info->cell_size = c->grid.h;
  for (int d = 0; d < 3; ++d) {
    info->origin[d] = c->grid.origin[d];
    info->dims[d] = c->grid.dims[d];
    info->block_dims[d] = c->grid.bdims[d];
  }
  info->num_indexed = c->m;
  info->occupied_cells = c->occupied;
  info->build_ms = c->build_ms;
  for (int d = 0; d < 3; ++d) { info->bbox_lo[d] = c->bb_lo[d]; info->bbox_hi[d] = c->bb_hi[d]; }
  return PCD_OK;
}

pcd_status pcd_cloud_download(const pcd_cloud* c, float* xyz, float* nrm) {
  return pcd::guard([&]() -> pcd_status {
  PCD_REQUIRE(c, "null cloud");
  PCD_HIP_TRY(hipSetDevice(c->device));
  std::vector<float4> h(2 * c->n);
  if (xyz && c->n) {
    PCD_HIP_TRY(hipMemcpy(h.data(), c->pts4.p, c->n * sizeof(float4), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < c->n; ++i) { xyz[3 * i] = h[i].x; xyz[3 * i + 1] = h[i].y; xyz[3 * i + 2] = h[i].z; }
  }
  if (nrm && c->n) {
    PCD_HIP_TRY(hipMemcpy(h.data(), c->pn8.p, 2 * c->n * sizeof(float4), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < c->n; ++i) { nrm[3 * i] = h[2 * i + 1].x; nrm[3 * i + 1] = h[2 * i + 1].y; nrm[3 * i + 2] = h[2 * i + 1].z; }
  }
  return PCD_OK;
  });
}

}  // extern "C"

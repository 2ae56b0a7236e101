// nn.hip -- exact nearest neighbour of 3D feature points in the LiDAR cloud.
//
// Replaces lidar/kdtree.cc:10-21 (Kdtree::GetClosestPoint -> pcl::KdTreeFLANN
// nearestKSearch, k = 1) as called from lidar/ply.cc:90-107.  Arithmetic is
// FLANN's L2_Simple<float> on (x,y,z): ((dx*dx) + dy*dy) + dz*dz in float32
// with separate multiplies and adds (this file is compiled with
// -ffp-contract=off), query = (float)double (ply.cc:92).  Result = the
// minimum of key = float_bits(d) << 32 | index over all points, i.e. ties on
// the float distance go to the lowest index; a point only counts if
// d < FLT_MAX (FLANN's initial worst distance).
//
// Three search kernels, all with lanes = cloud points and wave-uniform queries, each
// finishing with a per-wavefront min-reduction of packed keys (around them k_prepare<MODE>, k_finalize_keys and the
// bookkeeping kernels described below; the host driver at the end strings them together, one path per call: choose_path):
//   k_nn_bruteforce  all pairs; LDS-tiled; reference for the other two.
//   k_nn_brick_clip  one wavefront per group of <= G queries that fall into
//                    the same brick of 2^3 grid cells: the brick's own cells, then
//                    the parts of the cell rows of the brick grown by 2 cells that
//                    the queries' balls touch are streamed through LDS tiles
//                    (16-B records, coalesced row ranges) and every query of
//                    the group is compared with every staged point.  A query
//                    is final when its best distance is provably smaller than
//                    its distance to the boundary of the region
//                    (brick_clip_kernel.h; the shared machinery: brick_kernel.h).
//   k_nn_fallback    one wavefront per remaining query: depth-first, nearest-first
//                    descent of the 64-ary pyramid of tight AABBs over the grid
//                    (level 0 = leaves of 2x2x2 cells, one contiguous point range each;
//                    a virtual top over the first level with <= 64 nodes), the 64
//                    children of a node one per lane, pruned with the exact float
//                    lower bound.  Exact for any query position, also outside the grid.  The walk starts
//                    from min(incoming key, key of the query's SEED): the exact nearest cloud point of the centre
//                    of the query's 8x8x8-cell cube (a table built once per cloud, fb_seed_table).
// Query bookkeeping in front of k_nn_brick_clip: a two-level counting sort on the brick id
// (k_bk_slots, k_bk_colscan, k_bk_scatter, k_bk_count, k_bk_emit) that starts from the
// caller's double queries and yields the float records, the initial keys, the brick-sorted
// query records and the work items; queries with no cloud point in their brick's halo go
// straight to the fallback list.  Grids beyond the counting sort's limits take a radix sort
// on the brick id instead (k_brick_keys, rocPRIM, k_brick_tile_count, k_brick_emit).
//
// Exactness of the pruning (float distances, not real ones):
//   * AABB bound: lb = l2_simple3(q, clamp(q, lo, hi)) with lo/hi the actual
//     float min/max of the block's points.  Rounding is monotone, so for every
//     point p of the block fl_dist(q,p) >= lb; a block is skipped only if
//     lb > best (strictly: an equal-distance point with a lower index may hide
//     in it).
//   * region bound: margin = min distance from q to the faces of the
//     brick's cell range (float).  A point binned outside the range can lie at
//     most `slack` inside it because of float rounding in the binning
//     (grid.slack = 9.6e-7 * max(extent, |coord|) >= 4 roundings of 2^-24),
//     and its float distance is >= true^2 * (1 - 2.4e-7); a second slack covers
//     the rounding of the margin itself.  A result is final
//     iff best < (margin - 2 slack)^2 * (1 - 1e-5), margin > 2 slack
//     (brick_clip_kernel.h proven_bound_f).
//   * seed: the seed is a point of this cloud and its key is computed with the walk's own arithmetic
//     (l2_simple3 on the float query, make_key with the point's global index), so min(best, seed key) is the key
//     of a real candidate -- exactly what a leaf scan that met the point would have left.  The walk's pruning only
//     ever compares bounds with the current best, whatever produced it, so no bound argument is needed: the result
//     is the minimum over the cloud as before.  Ties: a point at the seed's distance with a lower index lies in a
//     block with lb <= best, which is not skipped.
#include <atomic>
#include <cfloat>

#include "cloud.h"
#include "grid.h"
#include "prim.h"
#include "scratch.h"

namespace pcd {

void free_query_scratch(QueryScratch* s) { delete s; }

constexpr uint64_t kKeyInit = (uint64_t)0x7F7FFFFFu << 32;  // (FLT_MAX, idx 0): nothing with d >= FLT_MAX beats it
// Batches up to this size skip the grid path (query sort + brick kernel + list squeeze + fallback = 8 launches with the
// counting-sort bookkeeping; 13 with the radix sort at the time of the measurement) and go straight to the
// per-wavefront hierarchical search, one launch: measured on a 2 M-point cloud (tools/nn_latency.py), 20 k queries take
// 99 us that way against 190 us, 100 k queries 290 against 329.
constexpr uint64_t kSmallBatch = 65536;

// ------------------------------------------------------------ brick math ---
struct BrickParams {
  int B, R;        // brick edge in cells (y, z), halo in cells
  int Bx;          // brick length along x in cells (the rows of the region run along x)
  int nb[3];       // bricks per axis
  uint32_t nbricks;
};

// The geometry k_nn_brick_clip is written for.  Others were measured and not adopted: x-long bricks (Bx = 2B, 3B, 4B:
// fewer, fuller groups but a longer region per query) on workload M 0.638 / 0.698 / 0.768 ms against 0.633 ms for
// cubes (profiles/r02_nn_config_sweeps.txt); x-long bricks of 3 and 4 cells with the in-kernel clip 0.529 / 0.551 ms
// against 0.509 (profiles/r04_nn_experiments.txt).
constexpr int kBrickCells = 2, kBrickCellsX = 2, kBrickHalo = 2;

static BrickParams make_bricks(const GridParams& g) {
  BrickParams b;
  b.B = kBrickCells; b.R = kBrickHalo; b.Bx = kBrickCellsX;
  uint64_t n = 1;
  for (int d = 0; d < 3; ++d) {
    const int e = d == 0 ? b.Bx : b.B;
    b.nb[d] = (g.dims[d] + e - 1) / e;
    n *= (uint64_t)b.nb[d];
  }
  b.nbricks = (uint32_t)n;
  return b;
}

// keys still at their initial value (kKeyInit, or a bound with the impossible index) mean "nothing found".  Every
// kernel that writes a FINAL key writes it in this form (the brick kernels for the queries they prove, the pyramid walk
// for all of its queries, the prepare kernels for the queries no search kernel touches): no separate pass over the keys.
__device__ __forceinline__ uint64_t finalized_key(uint64_t k) {
  return (k == kKeyInit || (uint32_t)k == 0xFFFFFFFFu) ? PCD_KEY_NONE : k;
}

// ------------------------------------------------------- query preparation --
// ply.cc:92: feature_point.getVector3fMap() = point_3d.cast<float>()
// One __device__ function per prepare flavour: the record qf4[i] is returned, the query's initial key goes to *key.
// Shared by the stand-alone k_prepare<MODE> and by k_bk_slots, which does the preparation itself on the counting-sort
// path: the arithmetic lives here only.
__device__ __forceinline__ float4 prepare_plain(const double* __restrict__ q, uint64_t i, uint64_t* key) {
  float x = (float)q[3 * i], y = (float)q[3 * i + 1], z = (float)q[3 * i + 2];
  bool ok = isfinite(x) && isfinite(y) && isfinite(z);
  *key = ok ? kKeyInit : PCD_KEY_NONE;   // a query no search kernel touches leaves with its final key
  return make_float4(x, y, z, ok ? 1.f : 0.f);
}

// pcd_nn_refine_device: the keys come in with another shard's results.  A query stays active only if this shard
// can still improve it: lower bound of the float distance to the shard's tight bounding box <= incoming distance
// (monotone rounding: fl_dist(q, p) >= fl_dist(q, clamp(q, lo, hi)) for every p in the box; equality is kept --
// a lower index at the same distance may live here).  Inactive queries get w = 0 and no kernel touches their key.
struct BoxF { float lox, loy, loz, hix, hiy, hiz; };
// *key: in = the incoming key, out = the key the search starts from (inactive: the incoming key in its final form)
__device__ __forceinline__ float4 prepare_refine(const double* __restrict__ q, uint64_t i, const uint8_t* __restrict__ skip,
                                                 const BoxF& bx, uint64_t* key) {
  float x = (float)q[3 * i], y = (float)q[3 * i + 1], z = (float)q[3 * i + 2];
  bool ok = isfinite(x) && isfinite(y) && isfinite(z) && !(skip && skip[i]);
  uint64_t k = *key;
  if (k == PCD_KEY_NONE) k = kKeyInit;
  if (ok) {
    const float px = fminf(fmaxf(x, bx.lox), bx.hix), py = fminf(fmaxf(y, bx.loy), bx.hiy), pz = fminf(fmaxf(z, bx.loz), bx.hiz);
    ok = l2_simple3(x, y, z, px, py, pz) <= __uint_as_float((uint32_t)(k >> 32));
  }
  *key = ok ? k : finalized_key(k);   // inactive: the key it came with, in its final form
  return make_float4(x, y, z, ok ? 1.f : 0.f);
}

// Gate-bounded search (the association entry points): the three call sites reject an association whose point-to-point
// distance exceeds max_search_range (mapper) or 2 m (controller), so a query needs no neighbour farther than that.
// The search starts from key = (bound, index 0xFFFFFFFF) instead of (FLT_MAX, 0): every candidate at or inside the
// bound beats it, everything beyond is pruned by the same exact float bounds as ever, and a key that still carries
// the impossible index at the end means "nothing within the gate" (-> PCD_KEY_NONE, type 0, as the reference's gate
// decides).  bound = float >= (R + e)^2 (1 + 1e-5), e = the query's float rounding (bounded_init_key): the float distance of any point that passes the double-precision gate
// is below it.  NaN range: the reference's `dist > range` is false, nothing is rejected -> unbounded.
// (x, y, z): the query in double.  The gate compares R with the DOUBLE distance |double(p_float) - q_double|
// (lidar_point.cc:27-30), the search minimises the FLOAT distance |p_float - float(q)|: the two differ by up to
// |q_double - float(q)| <= 0.5 ulp per axis -- millimetres for coordinates of kilometres -- plus the rounding of the
// float arithmetic (relative 2e-7, inside the 1e-5 factor).  e = (|x| + |y| + |z|) 2^-23 bounds the first term twice
// over, so every point the gate accepts has a float distance below (R + e)^2 (1 + 1e-5).  (Found by tools/nn_fuzz.py:
// a cloud 8 km from the origin, 11 of 150 000 associations with double distance 0.3899 < R = 0.39 < float distance.)
__device__ __forceinline__ uint64_t bounded_init_key(double R, double x, double y, double z) {
  uint64_t k = kKeyInit;
  if (R == R) {   // not NaN
    const double e = (fabs(x) + fabs(y) + fabs(z)) * (1.0 / 8388608.0);
    const double Rb = (R < 0.0 ? 0.0 : R) + e;
    const double b = Rb * Rb * (1.0 + 1e-5);
    float bf = (float)b;
    if ((double)bf < b) bf = nextafterf(bf, INFINITY);
    if (bf < FLT_MAX) k = ((uint64_t)__float_as_uint(bf) << 32) | 0xFFFFFFFFull;
  }
  return k;
}
__device__ __forceinline__ float4 prepare_bounded(const double* __restrict__ q, uint64_t i,
                                                  const double* __restrict__ max_range, uint64_t mr_count,
                                                  double fixed_range, uint64_t* key) {
  float x = (float)q[3 * i], y = (float)q[3 * i + 1], z = (float)q[3 * i + 2];
  bool ok = isfinite(x) && isfinite(y) && isfinite(z);
  *key = ok ? bounded_init_key(max_range ? max_range[mr_count == 1 ? 0 : i] : fixed_range, q[3 * i], q[3 * i + 1], q[3 * i + 2])
            : PCD_KEY_NONE;
  return make_float4(x, y, z, ok ? 1.f : 0.f);
}

// which prepare flavour a call uses, and its inputs (host and device; NnCall: the two together, as the entry points
// hand them to the driver)
enum { kPrepPlain = 0, kPrepRefine = 1, kPrepBounded = 2 };
struct PrepArgs {
  const double* q;             // the caller's queries, 3 doubles each
  const uint8_t* skip;         // refine: queries to leave alone (may be null)
  BoxF box;                    // refine: the shard's tight bounding box
  const double* max_range;     // gate-bounded: 1 or Q ranges, or null: fixed_range
  uint64_t mr_count;
  double fixed_range;
};
struct NnCall { int prep; PrepArgs pa; };
template <int MODE>
__device__ __forceinline__ float4 prepare_query(const PrepArgs& a, uint64_t i, uint64_t* key) {
  if (MODE == kPrepRefine) return prepare_refine(a.q, i, a.skip, a.box, key);
  if (MODE == kPrepBounded) return prepare_bounded(a.q, i, a.max_range, a.mr_count, a.fixed_range, key);
  return prepare_plain(a.q, i, key);
}
// the stand-alone prepare pass of every path whose first search kernel does not prepare the queries itself
template <int MODE>
__global__ void k_prepare(PrepArgs pa, uint64_t Q, float4* __restrict__ qf4, uint64_t* __restrict__ keys) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= Q) return;
  uint64_t k = MODE == kPrepRefine ? keys[i] : 0;   // refine: the key the query comes with
  qf4[i] = prepare_query<MODE>(pa, i, &k);
  keys[i] = k;
}
// the prepare flavour of a call as a template argument: f(std::integral_constant<int, MODE>)
template <class F>
static void with_prep_mode(int mode, F&& f) {
  if (mode == kPrepBounded) f(std::integral_constant<int, kPrepBounded>{});
  else if (mode == kPrepRefine) f(std::integral_constant<int, kPrepRefine>{});
  else f(std::integral_constant<int, kPrepPlain>{});
}

__global__ void k_finalize_keys(uint64_t* __restrict__ keys, uint64_t Q) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const uint64_t k = keys[i];
  if (finalized_key(k) != k) keys[i] = PCD_KEY_NONE;
}

__global__ void k_unpack_keys(const uint64_t* __restrict__ keys, uint64_t Q, uint32_t* __restrict__ idx,
                              float* __restrict__ sq, uint8_t* __restrict__ found) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= Q) return;
  uint64_t k = keys[i];
  bool f = k != PCD_KEY_NONE;
  idx[i] = f ? (uint32_t)k : 0xFFFFFFFFu;
  sq[i] = f ? __uint_as_float((uint32_t)(k >> 32)) : FLT_MAX;
  found[i] = f ? 1 : 0;
}

// ------------------------------------------------------------ brute force ---
// thread = query, the cloud chunk of blockIdx.y is streamed through a 1024-point LDS tile
// (broadcast reads), chunks are combined with atomicMin on the packed key.
__global__ __launch_bounds__(256) void k_nn_bruteforce(const float4* __restrict__ pts4, uint64_t n,
                                                        uint32_t index_base, uint32_t index_stride,
                                                        const uint32_t* __restrict__ row_index,
                                                        const float4* __restrict__ qf4, uint64_t Q,
                                                        uint64_t chunk, uint64_t* __restrict__ keys) {
  __shared__ float4 tile[1024];
  const uint64_t qi = blockIdx.x * (uint64_t)256 + threadIdx.x;
  float4 q = qi < Q ? qf4[qi] : make_float4(0, 0, 0, 0);
  uint64_t best = kKeyInit;
  const uint64_t beg = (uint64_t)blockIdx.y * chunk;
  const uint64_t end = beg + chunk < n ? beg + chunk : n;
  for (uint64_t t0 = beg; t0 < end; t0 += 1024) {
    const int tn = (int)(end - t0 < 1024 ? end - t0 : 1024);
    __syncthreads();
    for (int j = threadIdx.x; j < tn; j += 256) {
      float4 p = pts4[t0 + j];
      p.w = __uint_as_float(row_index ? row_index[t0 + j] : index_base + (uint32_t)(t0 + j) * index_stride);
      tile[j] = p;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < tn; ++j) {
      float4 p = tile[j];
      float d = l2_simple3(q.x, q.y, q.z, p.x, p.y, p.z);
      uint64_t k = make_key(d, __float_as_uint(p.w));
      best = k < best ? k : best;
    }
  }
  if (qi < Q && q.w != 0.f && best < kKeyInit) atomicMin((unsigned long long*)&keys[qi], (unsigned long long)best);
}

// ------------------------------------------------------ brick bookkeeping ---
// O(Q), independent of the number of bricks: queries are sorted by brick id (rocPRIM radix sort of (brick, query)
// pairs over the bits the brick count needs), runs of equal bricks are cut into work items of <= G queries with
// two scans over the sorted keys, and one kernel writes the item records and the brick-sorted query records.
// Keys: brick id | nbricks = finite query outside the grid (-> exact fallback) | nbricks + 1 = not finite (skipped).
__global__ void k_brick_keys(const float4* __restrict__ qf4, uint64_t Q, GridParams g, BrickParams b,
                             uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const float4 q = qf4[i];
  uint32_t bid = b.nbricks + 1u;
  if (q.w != 0.f) {
    const int cx = cell_coord_raw(q.x, g.origin[0], g.inv_h, g.dims[0]);
    const int cy = cell_coord_raw(q.y, g.origin[1], g.inv_h, g.dims[1]);
    const int cz = cell_coord_raw(q.z, g.origin[2], g.inv_h, g.dims[2]);
    const bool in = cx >= 0 && cx < g.dims[0] && cy >= 0 && cy < g.dims[1] && cz >= 0 && cz < g.dims[2];
    bid = in ? (uint32_t)(((uint64_t)(cz / b.B) * b.nb[1] + (cy / b.B)) * b.nb[0] + (cx / b.Bx)) : b.nbricks;
  }
  keys[i] = bid;
  vals[i] = (uint32_t)i;
}

// ---- work items from the sorted keys: two launches (count per tile, then offsets + emit) -------------------------
// A work item starts at sorted position j when its key is a brick id and (j - start of j's run of equal keys) is a
// multiple of G.  A tile = 1024 consecutive positions handled by one workgroup (4 per thread).
constexpr uint32_t kBkTile = 1024;

__device__ __forceinline__ uint32_t wave_scan_max_u32(uint32_t v) { return ~wave_scan_min_u32(~v); }   // inclusive

// per thread: keys of its 4 positions, start of each position's run, item flags; returns the tile's item count
// through *tile_items (valid in every thread).  s_* : LDS scratch of the workgroup.
template <int G>
__device__ __forceinline__ void brick_tile(const uint32_t* __restrict__ keys, uint32_t Q, uint32_t nbricks,
                                           uint32_t tile, uint32_t (&key)[4], uint32_t (&excl_items)[4],
                                           bool (&flag)[4], uint32_t* tile_items, uint32_t* s_wave /*[8]*/,
                                           uint32_t* s_left /*[1]*/) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t j0 = tile * kBkTile + tid * 4;
  const uint32_t tile_start = tile * kBkTile;
  uint32_t prev = j0 > 0 && j0 - 1 < Q ? keys[j0 - 1] : 0xFFFFFFFFu;
  uint32_t hp[4];   // position of the run head at or before each element, 0 = none seen yet in this thread
  uint32_t run = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t j = j0 + k;
    key[k] = j < Q ? keys[j] : 0xFFFFFFFFu;
    const bool head = j < Q && (j == 0 || key[k] != prev);
    run = head ? j : run;
    hp[k] = run;
    prev = key[k];
  }
  // run start carried in from the threads to the left (max-scan of the last head position per thread)
  const uint32_t inc = wave_scan_max_u32(run);
  if (lane == 63) s_wave[wave] = inc;
  // the run that crosses the tile's left edge starts before the tile: first position with that key (sorted array)
  if (tid == 0) {
    uint32_t left = tile_start;
    if (tile_start > 0 && tile_start < Q && keys[tile_start - 1] == keys[tile_start]) {
      const uint32_t k0 = keys[tile_start];
      uint32_t lo = 0, hi = tile_start;   // first index in [0, tile_start] with keys[idx] >= k0 (== k0)
      while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < k0) lo = mid + 1; else hi = mid; }
      left = lo;
    }
    s_left[0] = left;
  }
  __syncthreads();
  const uint32_t up = __shfl_up(inc, 1);
  uint32_t carry = lane == 0 ? 0u : up;     // exclusive within the wave
  for (uint32_t w = 0; w < wave; ++w) carry = max(carry, s_wave[w]);
  const uint32_t left = s_left[0];
  uint32_t cnt = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t j = j0 + k;
    uint32_t rs = max(hp[k], carry);
    // no head at or before j inside this tile (rs == 0 cannot be a real head unless tile 0, where left == 0 too)
    if (rs == 0 || rs < tile_start) rs = left;
    flag[k] = j < Q && key[k] < nbricks && ((j - rs) % (uint32_t)G) == 0u;
    excl_items[k] = cnt;
    cnt += flag[k] ? 1u : 0u;
  }
  // exclusive sum-scan of the per-thread item counts over the workgroup
  const uint32_t sinc = wave_scan_add_u32(cnt);
  __syncthreads();                        // s_wave is reused
  if (lane == 63) s_wave[wave] = sinc;
  __syncthreads();
  uint32_t base = sinc - cnt, total = 0;
  for (uint32_t w = 0; w < 4; ++w) { if (w < wave) base += s_wave[w]; total += s_wave[w]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) excl_items[k] += base;
  *tile_items = total;
}

template <int G>
__global__ __launch_bounds__(256) void k_brick_tile_count(const uint32_t* __restrict__ keys, uint32_t Q, uint32_t nbricks,
                                                          uint32_t* __restrict__ tile_items) {
  __shared__ uint32_t s_wave[8], s_left[1];
  uint32_t key[4], ex[4], total;
  bool flag[4];
  brick_tile<G>(keys, Q, nbricks, blockIdx.x, key, ex, flag, &total, s_wave, s_left);
  if (threadIdx.x == 0) tile_items[blockIdx.x] = total;
}

template <int G>
__global__ __launch_bounds__(256) void k_brick_emit(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    const uint32_t* __restrict__ tile_items, const float4* __restrict__ qf4,
                                                    const uint64_t* __restrict__ keys_in, uint32_t Q, uint32_t nbricks,
                                                    uint32_t nb0, uint32_t nb1, uint4* __restrict__ items,
                                                    float4* __restrict__ qsorted, uint64_t* __restrict__ ksorted,
                                                    uint32_t* __restrict__ fb_list, NnCounters* __restrict__ ctr) {
  __shared__ uint32_t s_wave[8], s_left[1], s_off[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // items of the tiles to the left: fixed-order strided sums (few hundred values)
  uint32_t part = 0;
  for (uint32_t t = tid; t < blockIdx.x; t += 256) part += tile_items[t];
  part = wave_scan_add_u32(part);
  if (lane == 63) s_off[wave] = part;
  __syncthreads();
  const uint32_t tile_off = s_off[0] + s_off[1] + s_off[2] + s_off[3];
  __syncthreads();
  uint32_t key[4], ex[4], total;
  bool flag[4];
  brick_tile<G>(keys, Q, nbricks, blockIdx.x, key, ex, flag, &total, s_wave, s_left);
  const uint32_t j0 = blockIdx.x * kBkTile + tid * 4;
  // the four positions of a thread: all loads of a stage are issued before any is used (the dependent chain
  // vals -> qf4 / keys_in would otherwise be walked four times in a row)
  uint32_t v[4];
  float4 q[4];
  uint64_t kin[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = j0 + k < Q ? vals[j0 + k] : 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = j0 + k < Q && key[k] < nbricks;
    q[k] = in ? qf4[v[k]] : make_float4(0.f, 0.f, 0.f, 0.f);
    // the key the query came with (a plain query comes with kKeyInit: no gather)
    kin[k] = (in && keys_in) ? keys_in[v[k]] : kKeyInit;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t j = j0 + k;
    if (j >= Q) break;
    if (key[k] < nbricks) {
      q[k].w = __uint_as_float(v[k]);          // brick-sorted query record {x, y, z, bits(query id)}
      qsorted[j] = q[k];
      ksorted[j] = kin[k];
      if (j + 1 == Q || keys[j + 1] >= nbricks) ctr->n_in_grid = j + 1;   // in-grid queries sort first
      if (flag[k]) {
        uint32_t cnt = 1;
        while (cnt < (uint32_t)G && j + cnt < Q && keys[j + cnt] == key[k]) ++cnt;
        // item record {first query, brick x, brick y, brick z | count << 28}: the brick kernel needs no divisions
        const uint32_t bx = key[k] % nb0, by = (key[k] / nb0) % nb1, bz = key[k] / (nb0 * nb1);
        items[tile_off + ex[k]] = make_uint4(j, bx, by, bz | (cnt << 28));
      }
    } else if (key[k] == nbricks) {
      fb_list[atomicAdd(&ctr->fb_count, 1u)] = v[k];   // outside the grid: straight to the exact fallback
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) ctr->nitems = tile_off + total;
}

// ------------------------------------------- brick bookkeeping, counting sort ---
// Five short launches instead of the radix sort's seven (round 2: 0.17 ms at Q = 1 M, three Onesweep digit passes at
// ~29 us each whatever the size), and nothing in front of them: the first one reads the caller's double queries itself
// (no stand-alone prepare pass) and the counters clean themselves (no memset, see take_counters).  Per cloud and brick
// geometry, once: one bit for every brick whose halo region holds at least one cloud point (k_brick_occupied +
// k_brick_bitmap); a query in a brick without the bit has nothing within the halo and goes straight to the exact
// fallback -- which is where the brick kernel would have sent it after walking an empty region.  Per batch a two-level
// counting sort on the brick id:
//   k_bk_slots<MODE>  at most 256 workgroups, each with a contiguous RANGE of rounds x 4096 queries.  Per query: the
//                 prepare flavour MODE (prepare_query: float record qf4[i] and initial key keys[i], as k_prepare<MODE>
//                 writes them on the other paths), then the sort key (brick id) or "fallback" (outside the grid /
//                 brick with an empty halo region: those are appended to the chunked fallback list here).  The LDS
//                 histogram of the COARSE keys (id >> shift, at most 4096 buckets) is left as one row of a
//                 [ranges][buckets] matrix -- no global atomics.  One thread clears the counters of the NEXT call.
//   k_bk_colscan  the matrix column by column, in place: queries of the bucket in the ranges before this one; the
//                 bucket totals.
//   k_bk_scatter  the same ranges: every workgroup scans the (at most 4096) bucket totals into bucket starts itself,
//                 adds its row of the matrix and has its private cursor per bucket in LDS; every query takes its place
//                 with one returning LDS atomic and is written as ONE 8-byte {fine key, query id} pair.
//   k_bk_count    one workgroup per coarse bucket: queries per FINE key (low bits) in LDS -> the bucket's item count.
//   k_bk_emit     one workgroup per coarse bucket: the same counting sort again, now with the item base known (sum
//                 of the item counts to the left: items stay in brick order, which the XCD-aware walk of k_nn_brick_clip
//                 is worth 0.04 ms for), then the brick-sorted query records, their incoming keys and the work
//                 items (G queries of one brick each).  LDS sized by the call's fine keys (dynamic), a thread's first
//                 two pairs kept in registers between the two passes.
// (No workgroup waits for another one: every hand-over is a kernel boundary.  A look-back over per-bucket descriptors
//  needs agent-scope release / acquire to cross the XCDs' L2s -- with relaxed polling the descriptors never arrived --
//  and at that price was slower than one more launch.)
// Measured at Q = 1 M on the 10 M-point cloud (profiles/bk_fused_bench_lines.txt; scope nn_brick_bookkeeping, which now
// holds the preparation too): 0.0925 ms, against 0.0953 + 0.0175 (nn_prepare) + the 64-byte memset's launch before.
// By item: fused prepare + no memset 0.1049; + histogram matrix, LDS cursors and 8-byte pairs 0.0945; + dynamic LDS and
// held pairs in k_bk_emit 0.0925.  Step 1.349 -> 1.330 ms.
// Queries of one brick arrive in any order (LDS atomics): WHICH queries share a work item varies from run to run, every
// query's result does not.
constexpr uint32_t kSlotFallback = 0xFFFFFFFEu;   // query: finite, but outside the grid or in a brick without a slot
constexpr uint32_t kSlotSkip = 0xFFFFFFFFu;       // query: not finite
constexpr uint32_t kBkMaxRanges = 256;   // workgroups of k_bk_slots / k_bk_scatter: rows of the histogram matrix
constexpr uint32_t kBkMaxCoarse = 4096, kBkMaxFine = 4096, kBkTileQ = 4096;   // 2^24 bricks: every grid of the 2^26-cell budget

// one thread per brick: does the halo region (whole quad rows, as the brick kernel's boundary table has them) hold any point?
__global__ void k_brick_occupied(GridParams g, BrickParams b, const uint32_t* __restrict__ cell_start,
                                 uint32_t* __restrict__ flag) {
  const uint32_t bid = blockIdx.x * blockDim.x + threadIdx.x;
  if (bid >= b.nbricks) return;
  const int bx = (int)(bid % (uint32_t)b.nb[0]), by = (int)((bid / (uint32_t)b.nb[0]) % (uint32_t)b.nb[1]),
            bz = (int)(bid / ((uint32_t)b.nb[0] * (uint32_t)b.nb[1]));
  const int x0 = max(bx * b.Bx - b.R, 0), x1 = min(bx * b.Bx + b.Bx + b.R, g.dims[0]);
  const int y0 = max(by * b.B - b.R, 0), y1 = min(by * b.B + b.B + b.R, g.dims[1]);
  const int z0 = max(bz * b.B - b.R, 0), z1 = min(bz * b.B + b.B + b.R, g.dims[2]);
  uint32_t any = 0;
  if (x0 < x1 && y0 < y1 && z0 < z1)
    for (int zq = z0 >> 1; zq < (z1 + 1) >> 1; ++zq)
      for (int yq = y0 >> 1; yq < (y1 + 1) >> 1; ++yq) {
        const uint64_t rb = quad_row_base(g, yq, zq);
        any |= cell_start[rb + 4 * (uint64_t)x1] - cell_start[rb + 4 * (uint64_t)x0];
      }
  flag[bid] = any ? 1u : 0u;
}
// 1 bit per brick: the halo region holds a point (32 bricks per thread; 580 KB for workload M's 4.65 M bricks, cache
// resident -- a 4-byte slot per brick made the per-query lookup a 128 MB gather)
__global__ void k_brick_bitmap(const uint32_t* __restrict__ flag, uint32_t nbricks, uint32_t* __restrict__ bits) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32u >= nbricks) return;
  uint32_t m = 0;
  for (uint32_t k = 0; k < 32u && w * 32u + k < nbricks; ++k) m |= (flag[w * 32u + k] ? 1u : 0u) << k;
  bits[w] = m;
}

// block-wide exclusive scan of one value per thread (NW wavefronts); returns the exclusive prefix, *total in every thread
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w /*[NW]*/, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_scan_add_u32(v);
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (uint32_t w = 0; w < (uint32_t)NW; ++w) { if (w < wave) base += s_w[w]; tot += s_w[w]; }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

template <int MODE>   // the call's prepare flavour, a template parameter for the reason given at k_nn_fallback<FUSED>
__global__ __launch_bounds__(1024) void k_bk_slots(PrepArgs pa, uint32_t Q, uint32_t rounds, GridParams g, BrickParams b,
                                                   const uint32_t* __restrict__ brick_slot, uint32_t shift, uint32_t ncoarse,
                                                   float4* __restrict__ qf4, uint64_t* __restrict__ keys,
                                                   uint32_t* __restrict__ qslot, uint32_t* __restrict__ hmat,
                                                   uint32_t* __restrict__ fb_list, NnCounters* __restrict__ ctr,
                                                   NnCounters* __restrict__ ctr_next) {
  // few, large workgroups (at most kBkMaxRanges): each owns a contiguous RANGE of `rounds` x 4096 queries and leaves its
  // LDS histogram as one row of the [ranges][ncoarse] matrix
  __shared__ uint32_t s_h[kBkMaxCoarse], s_w[16], s_base;
  // the counters of the NEXT grid-path call: every user of that block (the call before this one) has finished
  static_assert(sizeof(NnCounters) / 4 <= 1024, "one thread per word of the block");
  if (blockIdx.x == 0 && threadIdx.x < sizeof(NnCounters) / 4) reinterpret_cast<uint32_t*>(ctr_next)[threadIdx.x] = 0;
  for (uint32_t c = threadIdx.x; c < ncoarse; c += 1024) s_h[c] = 0;
  __syncthreads();
  // rounds of 4 queries per thread: the fallback queries of a round are counted over the WORKGROUP and placed with one
  // global atomic (a chunk per wavefront, as the brick kernel does it, was one same-address returning atomic per
  // wavefront of this short kernel: 4096 of them, ~40 of its 54 us)
  for (uint32_t rr = 0; rr < rounds; ++rr) {
    const uint64_t r0 = ((uint64_t)blockIdx.x * rounds + rr) * kBkTileQ;   // (64 bits: Q may be close to 2^32)
    if (r0 >= Q) break;
    uint32_t sv[4], nfb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t i = r0 + k * 1024u + threadIdx.x;
      uint32_t s = kSlotSkip;
      if (i < Q) {
        // the caller's double query -> float record and initial key (what k_prepare<MODE> does elsewhere)
        uint64_t key = MODE == kPrepRefine ? keys[i] : 0;
        const float4 q = prepare_query<MODE>(pa, i, &key);
        qf4[i] = q;
        keys[i] = key;
        if (q.w != 0.f) {
          const int cx = cell_coord_raw(q.x, g.origin[0], g.inv_h, g.dims[0]);
          const int cy = cell_coord_raw(q.y, g.origin[1], g.inv_h, g.dims[1]);
          const int cz = cell_coord_raw(q.z, g.origin[2], g.inv_h, g.dims[2]);
          const bool in = cx >= 0 && cx < g.dims[0] && cy >= 0 && cy < g.dims[1] && cz >= 0 && cz < g.dims[2];
          s = kSlotFallback;
          if (in) {
            const uint32_t bid = (uint32_t)(((uint64_t)(cz / b.B) * b.nb[1] + (cy / b.B)) * b.nb[0] + (cx / b.Bx));
            if ((brick_slot[bid >> 5] >> (bid & 31u)) & 1u) { s = bid; atomicAdd(&s_h[bid >> shift], 1u); }
          }
        }
        qslot[i] = s;
      }
      sv[k] = s;
      nfb += s == kSlotFallback ? 1u : 0u;
    }
    uint32_t total;
    uint32_t pos = block_excl_scan<16>(nfb, s_w, &total);
    if (total) {   // workgroup-uniform
      if (threadIdx.x == 0) s_base = atomicAdd(&ctr->fb_count, total);
      __syncthreads();
      pos += s_base;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (sv[k] == kSlotFallback) fb_list[pos++] = (uint32_t)r0 + k * 1024u + threadIdx.x;
      __syncthreads();   // s_base is rewritten in the next round
    }
  }
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < ncoarse; c += 1024) hmat[(size_t)blockIdx.x * ncoarse + c] = s_h[c];   // zeros too
}

// Column scan of the histogram matrix, in place: hmat[r][c] becomes the number of bucket c's queries in the ranges
// before r, ctot[c] the bucket's total.  One workgroup per 64 buckets (a lane each), its 16 wavefronts share the ranges:
// partial sums, their scan through LDS, then the prefixes.
__global__ __launch_bounds__(1024) void k_bk_colscan(uint32_t* __restrict__ hmat, uint32_t nranges, uint32_t ncoarse,
                                                     uint32_t* __restrict__ ctot) {
  __shared__ uint32_t s_p[16][64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, c = blockIdx.x * 64u + lane;
  const uint32_t per = (nranges + 15u) / 16u, ra = min(w * per, nranges), rb = min(ra + per, nranges);
  uint32_t sum = 0;
  if (c < ncoarse)
    for (uint32_t r = ra; r < rb; ++r) sum += hmat[(size_t)r * ncoarse + c];
  s_p[w][lane] = sum;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) { const uint32_t v = s_p[k][lane]; base += k < w ? v : 0u; tot += v; }
  if (c >= ncoarse) return;
  if (w == 0) ctot[c] = tot;
  for (uint32_t r = ra; r < rb; ++r) {
    const uint32_t v = hmat[(size_t)r * ncoarse + c];
    hmat[(size_t)r * ncoarse + c] = base;
    base += v;
  }
}

__global__ __launch_bounds__(1024) void k_bk_scatter(const uint32_t* __restrict__ qslot, uint32_t Q, uint32_t rounds,
                                                     uint32_t shift, uint32_t ncoarse, const uint32_t* __restrict__ ctot,
                                                     const uint32_t* __restrict__ hmat, uint32_t* __restrict__ cstart,
                                                     uint2* __restrict__ ppair, NnCounters* __restrict__ ctr) {
  __shared__ uint32_t s_cur[kBkMaxCoarse], s_w[16];
  // cursors of this range: bucket start (every workgroup scans the at most 4096 bucket totals itself; workgroup 0
  // keeps the result) + the bucket's queries in the ranges before this one (k_bk_colscan)
  {
    const uint32_t per = (ncoarse + 1023u) / 1024u, c0 = threadIdx.x * per;   // per <= 4
    uint32_t h[4] = {0, 0, 0, 0}, sum = 0;
    for (uint32_t k = 0; k < per && c0 + k < ncoarse; ++k) { h[k] = ctot[c0 + k]; sum += h[k]; }
    uint32_t total;
    uint32_t base = block_excl_scan<16>(sum, s_w, &total);
    for (uint32_t k = 0; k < per && c0 + k < ncoarse; ++k) {
      s_cur[c0 + k] = base + hmat[(size_t)blockIdx.x * ncoarse + c0 + k];
      if (blockIdx.x == 0) cstart[c0 + k] = base;
      base += h[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { cstart[ncoarse] = total; ctr->n_in_grid = total; }
  }
  __syncthreads();
  // every query of the range: one returning LDS atomic on its bucket's cursor, one 8-byte store {fine key, query id}
  const uint32_t mask = (1u << shift) - 1u;
  for (uint32_t rr = 0; rr < rounds; ++rr) {
    const uint64_t r0 = ((uint64_t)blockIdx.x * rounds + rr) * kBkTileQ;
    if (r0 >= Q) break;
    uint32_t sl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t i = r0 + k * 1024u + threadIdx.x;
      sl[k] = i < Q ? qslot[i] : kSlotSkip;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (sl[k] < kSlotFallback) {
        const uint32_t p = atomicAdd(&s_cur[sl[k] >> shift], 1u);
        ppair[p] = make_uint2(sl[k] & mask, (uint32_t)r0 + k * 1024u + threadIdx.x);
      }
  }
}

// work items of every coarse bucket: one workgroup per bucket counts the bucket's queries per fine key in LDS
template <int G>
__global__ __launch_bounds__(256) void k_bk_count(uint32_t shift, const uint32_t* __restrict__ cstart,
                                                  const uint2* __restrict__ ppair, uint32_t* __restrict__ bitems) {
  __shared__ uint32_t s_cnt[kBkMaxFine], s_w[4];
  const uint32_t nfine = 1u << shift, mask = nfine - 1u;
  const uint32_t beg = cstart[blockIdx.x], end = cstart[blockIdx.x + 1];
  if (beg == end) { if (threadIdx.x == 0) bitems[blockIdx.x] = 0; return; }
  for (uint32_t f = threadIdx.x; f < nfine; f += 256) s_cnt[f] = 0;
  __syncthreads();
  for (uint32_t p = beg + threadIdx.x; p < end; p += 256) atomicAdd(&s_cnt[ppair[p].x & mask], 1u);
  __syncthreads();
  uint32_t ai = 0;
  for (uint32_t f = threadIdx.x; f < nfine; f += 256) ai += (s_cnt[f] + G - 1) / G;
  uint32_t ti;
  (void)block_excl_scan<4>(ai, s_w, &ti);
  if (threadIdx.x == 0) bitems[blockIdx.x] = ti;
}

template <int G>
__global__ __launch_bounds__(256) void k_bk_emit(const float4* __restrict__ qf4, const uint64_t* __restrict__ keys_in,
                                                 GridParams g, BrickParams b, uint32_t shift,
                                                 const uint32_t* __restrict__ cstart, const uint2* __restrict__ ppair,
                                                 const uint32_t* __restrict__ bitems, uint4* __restrict__ items, float4* __restrict__ qsorted,
                                                 uint64_t* __restrict__ ksorted, NnCounters* __restrict__ ctr) {
  // per fine key: start of its queries / items inside the bucket (nfine + 1 entries: the count of key f is
  // s_off[f + 1] - s_off[f]) and the running rank.  Dynamic LDS, 12 B per fine key of THIS call: 24 KB at the 2048 fine
  // keys of a 4.65 M-brick grid (six workgroups per CU), 48 KB at the maximum of 4096
  extern __shared__ uint32_t s_dyn[];
  __shared__ uint32_t s_w[4];
  const uint32_t nfine = 1u << shift, mask = nfine - 1u;
  uint32_t *s_off = s_dyn, *s_ioff = s_off + nfine + 1, *s_cur = s_ioff + nfine + 1;
  const uint32_t beg = cstart[blockIdx.x], end = cstart[blockIdx.x + 1];
  // item base = items of all buckets to the left, in bucket order = brick order (the XCD-aware walk of k_nn_brick_clip
  // depends on it): summed from k_bk_count's per-bucket totals -- no atomics, no waiting on other workgroups
  uint32_t acc = 0;
  for (uint32_t c = threadIdx.x; c < blockIdx.x; c += 256) acc += bitems[c];
  uint32_t ibase;
  (void)block_excl_scan<4>(acc, s_w, &ibase);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) ctr->nitems = ibase + bitems[blockIdx.x];
  if (beg == end) return;
  for (uint32_t f = threadIdx.x; f < nfine; f += 256) s_cur[f] = 0;
  __syncthreads();
  // a thread's first kBkHeld entries stay in registers from the counting pass to the placement pass (a bucket of the
  // 1 M-query workload holds ~440 entries: all of them); larger buckets read the rest twice
  constexpr uint32_t kBkHeld = 2;
  uint2 held[kBkHeld];
#pragma unroll
  for (uint32_t k = 0; k < kBkHeld; ++k) {
    const uint32_t p = beg + threadIdx.x + k * 256u;
    held[k] = p < end ? ppair[p] : make_uint2(0u, 0u);
  }
#pragma unroll
  for (uint32_t k = 0; k < kBkHeld; ++k)
    if (beg + threadIdx.x + k * 256u < end) atomicAdd(&s_cur[held[k].x & mask], 1u);   // counts
  for (uint32_t p = beg + threadIdx.x + kBkHeld * 256u; p < end; p += 256) atomicAdd(&s_cur[ppair[p].x & mask], 1u);
  __syncthreads();
  // exclusive prefixes of the query counts and of the item counts over the bucket's fine keys
  const uint32_t per = (nfine + 255u) / 256u, f0 = threadIdx.x * per;
  {
    uint32_t aq = 0, ai = 0;
    for (uint32_t f = f0; f < min(f0 + per, nfine); ++f) { aq += s_cur[f]; ai += (s_cur[f] + G - 1) / G; }
    uint32_t tq, ti;
    uint32_t bq = block_excl_scan<4>(aq, s_w, &tq);
    uint32_t bi = block_excl_scan<4>(ai, s_w, &ti);
    for (uint32_t f = f0; f < min(f0 + per, nfine); ++f) {
      const uint32_t c = s_cur[f];
      s_off[f] = bq; s_ioff[f] = bi; bq += c; bi += (c + G - 1) / G;
      s_cur[f] = 0;                     // becomes the running rank
    }
    if (threadIdx.x == 255) { s_off[nfine] = tq; s_ioff[nfine] = ti; }
    __syncthreads();
  }
  auto place = [&](const uint2 e) {
    const uint32_t f = e.x & mask, i = e.y;
    const uint32_t r = atomicAdd(&s_cur[f], 1u);
    float4 q = qf4[i];
    const uint32_t pos = beg + s_off[f] + r;
    if (r % (uint32_t)G == 0u) {   // first query of a work item: G consecutive positions of one brick
      const int cx = cell_coord_raw(q.x, g.origin[0], g.inv_h, g.dims[0]);
      const int cy = cell_coord_raw(q.y, g.origin[1], g.inv_h, g.dims[1]);
      const int cz = cell_coord_raw(q.z, g.origin[2], g.inv_h, g.dims[2]);
      const uint32_t left = s_off[f + 1] - s_off[f] - r;
      items[ibase + s_ioff[f] + r / (uint32_t)G] =
          make_uint4(pos, (uint32_t)(cx / b.Bx), (uint32_t)(cy / b.B),
                     (uint32_t)(cz / b.B) | ((left < (uint32_t)G ? left : (uint32_t)G) << 28));
    }
    q.w = __uint_as_float(i);
    qsorted[pos] = q;
    ksorted[pos] = keys_in ? keys_in[i] : kKeyInit;
  };
#pragma unroll
  for (uint32_t k = 0; k < kBkHeld; ++k)
    if (beg + threadIdx.x + k * 256u < end) place(held[k]);
  for (uint32_t p = beg + threadIdx.x + kBkHeld * 256u; p < end; p += 256) place(ppair[p]);
}

// ------------------------------------------------------------ brick kernel ---
}  // namespace pcd
#include "brick_kernel.h"
#include "brick_clip_kernel.h"
namespace pcd {

// The brick kernel fills the fallback list in per-wavefront chunks (brick_kernel.h kFbChunk); the unused slots of
// the chunks keep 0xFFFFFFFF.  One pass squeezes them out (wave-aggregated atomics: the order of the dense list is
// not deterministic, the per-query results do not depend on it) so that k_nn_fallback gets an evenly filled list.
constexpr uint32_t kFbcThreads = 1024, kFbcPer = 4;   // 4096 list slots per workgroup
__global__ __launch_bounds__(1024) void k_fb_compact(const uint32_t* __restrict__ list,
                                                     const uint32_t* __restrict__ count_ptr,
                                                     uint32_t* __restrict__ dense, uint32_t* __restrict__ dense_count) {
  // one atomic per WORKGROUP of 4096 slots: same-address device-scope atomics serialise at ~10 ns each on this part
  // (one per wavefront of 64 slots made this pass 45 us for a 390 k-slot list)
  __shared__ uint32_t s_wave[16], s_base;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t n = *count_ptr;
  const uint32_t e0 = (blockIdx.x * kFbcThreads + tid) * kFbcPer;
  if (blockIdx.x * kFbcThreads * kFbcPer >= n) return;   // whole workgroup past the end
  uint32_t v[kFbcPer], cnt = 0;
  if (e0 + kFbcPer <= n) {
    const uint4 q = *reinterpret_cast<const uint4*>(list + e0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kFbcPer; ++k) v[k] = e0 + k < n ? list[e0 + k] : 0xFFFFFFFFu;
  }
#pragma unroll
  for (uint32_t k = 0; k < kFbcPer; ++k) cnt += v[k] != 0xFFFFFFFFu ? 1u : 0u;
  const uint32_t inc = wave_scan_add_u32(cnt);
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (uint32_t w = 0; w < kFbcThreads / 64; ++w) { before += w < wave ? s_wave[w] : 0u; total += s_wave[w]; }
  if (tid == 0) s_base = total ? atomicAdd(dense_count, total) : 0u;
  __syncthreads();
  uint32_t pos = s_base + before + inc - cnt;
#pragma unroll
  for (uint32_t k = 0; k < kFbcPer; ++k)
    if (v[k] != 0xFFFFFFFFu) dense[pos++] = v[k];
}

// --------------------------------------------------------- exact fallback ---
struct FbFused {   // inputs of k_nn_fallback<1 / 2> (the kernel as the only launch of a call)
  const double* q;
  const double* max_range;
  uint64_t mr_count;
  double fixed_range;
};

// One wavefront per query walks the 64-ary AABB tree over the occupied nodes of the grid's pyramid (level 0 = 2x2x2-cell
// leaves carrying their point range, level k+1 = 4x4x4 nodes of level k carrying the range of their children's records,
// cloud.h): the up to 64 children of the current node sit one per lane in the order of their records (= of their
// position in the node's 4x4x4 lattice), each lane computes the exact float lower bound of its child, and the wave
// descends into the nearest child whose bound does not exceed the best distance so far (depth first, nearest first,
// ties to the lowest lane).
// Every skipped subtree has bound > best, so the result is the exact minimum of the packed keys.
// FUSED: 0 = queries from qf4, keys in and out raw (the grid path's second stage; refining), 1 / 2 = the kernel is the
// only launch of the call (plain / gate-bounded).  A template parameter, not a run-time mode: with the mode tested at
// run time the grid path's instance compiled differently and ran 17 % slower (0.365 -> 0.425 ms on workload M).
// One wavefront per workgroup: a workgroup's LDS (and its place in the CU's workgroup count) goes back only when its
// LAST walk ends, and the walks differ widely in length (12.8 steps on average, up to ~80 on workload M) -- with four
// walks per workgroup the wavefronts of a workgroup were finished for 27 % of its life, with one every walk gives back
// everything it holds when it ends (256 / 128 / 64 threads: 0.173 / 0.163 / 0.159 ms on workload M,
// profiles/fb_release_probe.txt).  At most 80 SGPRs: a SIMD's scalar registers admit an eighth wavefront only up to
// there (MI355X: 800 / (allocation + 16)), the walk's uniform state took 94-96 without the bound, and the bound costs
// one VGPR (0.159 -> 0.152 ms).
// dynamic LDS of a workgroup: its walk's stack, one entry per level that pushes
constexpr size_t fb_stack_bytes(int nlev) { return (size_t)(nlev - 2) * (64 * 4 + 64 * 4 + 8); }
static_assert(fb_stack_bytes(kMaxPyrLevels) <= 64 * 1024, "the deepest pyramid's stack fits a workgroup's LDS");
template <int FUSED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_sgpr(80)))
void k_nn_fallback(GridParams g, PyramidParams py, const float4* __restrict__ sorted,
                   const uint32_t* __restrict__ cell_start, const float* __restrict__ aabb,
                   const float4* __restrict__ seeds, const float4* __restrict__ qf4,
                   const uint32_t* __restrict__ list,  // NULL: queries 0..count-1
                   const uint32_t* __restrict__ count_ptr, uint32_t count_imm, uint64_t* __restrict__ keys,
                   NnCounters* __restrict__ ctr, int collect_stats, FbFused fu,
                   unsigned long long* __restrict__ wave_rec) {
  // the stack: levels 2 .. nlev - 1 push (a level-1 node's children are leaves).  Per lane the child's bound and its
  // own child range as first | (count - 1) << 26 (cloud.h kMaxPyrRecords), per level the mask of the children still
  // to visit.  Dynamic LDS of nlev - 2 levels (fb_stack_bytes; none for a two-level pyramid, which never pushes):
  // the levels a cloud's pyramid does not have would only keep other workgroups off the CU (kMaxPyrLevels - 2 = 8
  // levels for four walks were 16 KB a workgroup, workload M's pyramid pushes at three)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_stack[];
  const int lane = threadIdx.x;
  const int nst = py.nlev - 2;   // levels of the stack
  float* const s_lb = reinterpret_cast<float*>(s_stack);                                        // [nst][64]
  uint32_t* const s_rng = reinterpret_cast<uint32_t*>(s_stack) + (size_t)nst * 64;               // [nst][64]
  unsigned long long* const s_mask = reinterpret_cast<unsigned long long*>(s_stack + (size_t)nst * 512);   // [nst]
  const uint32_t count = count_ptr ? *count_ptr : count_imm;
  const int top = py.nlev - 1;  // >= 1
  const bool probe = (collect_stats & 16) != 0;   // (uniform) a pass that keeps per-wavefront records
  const unsigned long long t_start = probe ? wall_clock64() : 0ull;
  unsigned long long st_pts = 0, st_q = 0, st_steps = 0, st_leaves = 0;
  uint32_t st_max_steps = 0, st_max_leaves = 0;
  for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
    const uint32_t qi = list ? list[e] : e;
    float qx, qy, qz;
    uint64_t best;
    if (FUSED == 0) {
      const float4 q = qf4[qi];
      if (q.w == 0.f) continue;  // not finite: stays "not found"
      qx = q.x; qy = q.y; qz = q.z;
      best = keys[qi];  // kKeyInit or the brick kernel's tentative result
    } else {
      // one-launch form (small batches): the query is converted here and the key leaves finalised -- no prepare
      // kernel in front, no finalize kernel behind (lidar/ply.cc:92: feature_point = point_3d.cast<float>())
      qx = (float)fu.q[3 * (size_t)qi]; qy = (float)fu.q[3 * (size_t)qi + 1]; qz = (float)fu.q[3 * (size_t)qi + 2];
      if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
        if (lane == 0) keys[qi] = PCD_KEY_NONE;
        continue;
      }
      best = FUSED == 2 ? bounded_init_key(fu.max_range ? fu.max_range[fu.mr_count == 1 ? 0 : qi] : fu.fixed_range,
                                             fu.q[3 * (size_t)qi], fu.q[3 * (size_t)qi + 1], fu.q[3 * (size_t)qi + 2])
                          : kKeyInit;
    }
    {
      // seed bound (fb_seed_table): the point of the query's 8x8x8-cell cube -- of the nearest cube for a query
      // outside the grid -- as a candidate before the walk.  Far outliers no longer start from kKeyInit, and the first
      // leaves the walk meets are pruned against a distance near the true one (tools/fb_walk_sim.py).  The load
      // does not depend on the first expansion's and goes out beside it.
      const int sx = cell_coord(qx, g.origin[0], g.inv_h, g.dims[0]) >> 3;
      const int sy = cell_coord(qy, g.origin[1], g.inv_h, g.dims[1]) >> 3;
      const int sz = cell_coord(qz, g.origin[2], g.inv_h, g.dims[2]) >> 3;
      const float4 sp = seeds[((size_t)sz * py.seed_dims[1] + sy) * py.seed_dims[0] + sx];
      const uint64_t sk = make_key(l2_simple3(qx, qy, qz, sp.x, sp.y, sp.z), __float_as_uint(sp.w));
      best = sk < best ? sk : best;
    }
    // The state of the level being iterated lives in REGISTERS (the children's bounds one per lane, the mask of the
    // children still to visit in an SGPR pair, the children's ranges one per lane); the LDS arrays are a stack touched
    // only when the walk descends (push) or comes back (pop).  Before, every iteration went through LDS for the mask and the node -- a
    // write -> read round trip in the walk's dependent chain, and most iterations are leaves of ONE level-1 node.
    // The keys are compared as doubles (brick_kernel.h: one v_min_f64 instead of a 64-bit compare + two selects).
    double lane_best = __builtin_bit_cast(double, best);
    float best_d = __uint_as_float((uint32_t)(best >> 32));
    int lev = top;                 // the children of a node of level `lev` are being iterated
    float cur_lb;
    unsigned long long cur_m;
    uint32_t rs = 0, rn = 0;       // the lane's child's range: points of `sorted` (lev == 1) or records of its children
    uint32_t q_steps = 0, q_leaves = 0;
    // the children of the node are the records cf .. cf + cn - 1 (uniform: the virtual top's from the kernel arguments,
    // a child's from the lane that holds it).  ONE memory round trip per expansion: the child's two 16-byte loads are
    // unconditional on a clamped index -- the lanes past the last child re-read its record, a line a live lane fetches
    // anyway -- and the bound is selected afterwards (under `if (live)` the compiler split them into a first pair of
    // dwords, the test, and a second, dependent pair of loads): the walk is a chain of such steps.
#define PCD_FB_EXPAND(cf, cn)                                                                                         \
    {                                                                                                                 \
      const uint32_t cn_ = (cn);                                                                                      \
      const uint32_t last = cn_ ? cn_ - 1u : 0u; /* (no children: a cloud without a finite point) */                  \
      const uint32_t id = (cf) + ((uint32_t)lane < last ? (uint32_t)lane : last);                                     \
      const float4 lo = *reinterpret_cast<const float4*>(aabb + 8 * (size_t)id);     /* lo.x lo.y lo.z hi.x */        \
      const float4 hi = *reinterpret_cast<const float4*>(aabb + 8 * (size_t)id + 4); /* hi.y hi.z first count */      \
      /* clamp(q, lo, hi) = the median of the three for lo <= hi: ONE v_med3_f32 (fminf(fmaxf()) costs two ops + */     \
      /* three canonicalising v_max x, x, x); every record holds a point, so its box is not inverted */                \
      const float px = __builtin_amdgcn_fmed3f(qx, lo.x, lo.w), pyc = __builtin_amdgcn_fmed3f(qy, lo.y, hi.x),        \
                  pz = __builtin_amdgcn_fmed3f(qz, lo.z, hi.y);                                                       \
      const float lbv = l2_simple3(qx, qy, qz, px, pyc, pz);                                                          \
      cur_lb = (uint32_t)lane < cn_ ? lbv : INFINITY;                                                                 \
      rs = __float_as_uint(hi.z); rn = __float_as_uint(hi.w);                                                         \
      cur_m = __ballot(cur_lb <= best_d);                                                                             \
    }
    PCD_FB_EXPAND(py.root_first, py.root_count);
    while (true) {
      ++q_steps;
      unsigned long long m = cur_m & __ballot(cur_lb <= best_d);
      if (m == 0) {
        if (lev == top) break;
        ++lev;   // pop
        cur_lb = s_lb[(lev - 2) * 64 + lane];
        const uint32_t pr = s_rng[(lev - 2) * 64 + lane];
        rs = pr & (kMaxPyrRecords - 1u); rn = (pr >> 26) + 1u;
        const unsigned long long pm = s_mask[lev - 2];
        cur_m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(pm >> 32)) << 32) |
                (uint32_t)__builtin_amdgcn_readfirstlane((int)pm);
        continue;
      }
      const int sl = wave_argmin_u32(__float_as_uint(cur_lb), m);  // nearest remaining child (lb >= 0: bit order)
      m &= ~(1ull << sl);
      cur_m = m;
      if (lev == 1) {
        // the child is a LEAF (cloud.h: a sub-block of 2x2x2 cells, one contiguous point range with a tight box): scan
        // it, 128 points per trip with the loads issued back to back (clamped indices, no branches around the loads: a
        // re-read is harmless), then tighten the bound -- the other leaves of the node are tested against it
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)rs, sl), n0 = (uint32_t)__builtin_amdgcn_readlane((int)rn, sl);
        for (uint32_t base = 0; base < n0; base += 128) {
          float4 p[2];
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const uint32_t gi = base + k * 64 + lane;
            p[k] = sorted[s0 + (gi < n0 ? gi : n0 - 1)];
          }
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const float d = l2_simple3(qx, qy, qz, p[k].x, p[k].y, p[k].z);
            lane_best = min_key_f64(lane_best, __builtin_bit_cast(double, make_key(d, __float_as_uint(p[k].w))));
          }
        }
        st_pts += n0;
        ++q_leaves;
        best = wave_min_u64(__builtin_bit_cast(uint64_t, lane_best));
        best_d = __uint_as_float((uint32_t)(best >> 32));
        // The node's OTHER leaves that still pass the tightened bound: all of them in one batch -- four leaves' loads in
        // flight at a time, no reduction in between.  They would each be scanned anyway (a leaf on a tilted surface has a
        // fat box: a far query at distance d finds ~d / 0.1 m leaves whose box is nearer than d although none of their
        // points is -- 129 leaf scans in the longest walk of workload M, one walk step each before); the rare leaf that
        // a batch neighbour would have ruled out costs one load.
        unsigned long long mb = m & __ballot(cur_lb <= best_d);
        if (mb) {
          cur_m = m & ~mb;
          while (mb) {
            // four leaves per trip, one 64-point load each (a leaf holds ~50 points; the rare longer one loops)
            uint32_t a[4], c[4];
            uint32_t cmax = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int r = mb ? __ffsll((long long)mb) - 1 : -1;
              mb &= mb - 1;   // (0 stays 0)
              a[k] = r >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)rs, r) : a[0];
              c[k] = r >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)rn, r) : 0u;
              cmax = c[k] > cmax ? c[k] : cmax;
              st_pts += c[k];
              q_leaves += r >= 0 ? 1 : 0;
            }
            for (uint32_t base = 0; base < cmax; base += 64) {
              float4 p[4];
              const uint32_t gi = base + lane;
#pragma unroll
              for (int k = 0; k < 4; ++k) p[k] = sorted[a[k] + (gi < c[k] ? gi : (c[k] ? c[k] - 1 : 0u))];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const float d = l2_simple3(qx, qy, qz, p[k].x, p[k].y, p[k].z);
                lane_best = min_key_f64(lane_best, __builtin_bit_cast(double, make_key(d, __float_as_uint(p[k].w))));
              }
            }
          }
          best = wave_min_u64(__builtin_bit_cast(uint64_t, lane_best));
          best_d = __uint_as_float((uint32_t)(best >> 32));
        }
      } else {
        // push the level, descend into child `sl`: its children's records are named by its own
        s_lb[(lev - 2) * 64 + lane] = cur_lb;
        s_rng[(lev - 2) * 64 + lane] = rs | ((rn - 1u) << 26);   // (lanes past the last child hold its copy: rn >= 1)
        if (lane == 0) s_mask[lev - 2] = cur_m;
        const uint32_t cf = (uint32_t)__builtin_amdgcn_readlane((int)rs, sl), cn = (uint32_t)__builtin_amdgcn_readlane((int)rn, sl);
        --lev;
        PCD_FB_EXPAND(cf, cn);
      }
    }
#undef PCD_FB_EXPAND
    if (lane == 0) keys[qi] = finalized_key(best);   // the walk is exact: whatever it ends with is final
    st_q += 1;
    st_steps += q_steps; st_leaves += q_leaves;
    st_max_steps = q_steps > st_max_steps ? q_steps : st_max_steps;
    st_max_leaves = q_leaves > st_max_leaves ? q_leaves : st_max_leaves;
  }
  if (probe && lane == 0) {
    unsigned long long* const rec = wave_rec + 3u * blockIdx.x;
    rec[0] = t_start; rec[1] = wall_clock64(); rec[2] = st_steps;
  }
  // (uniform) statistics passes only: one set of global atomics per wavefront.  Same-address atomics serialise at
  // ~10 ns each, so a pass over the whole grid of 65 k wavefronts takes ~3 ms instead of 0.15; the plain kernel pays nothing
  if ((collect_stats & 1) && lane == 0 && st_q) {
    atomicAdd(&ctr->fallback_points, st_pts);
    atomicAdd(&ctr->pair_evals, st_pts);
    atomicAdd(&ctr->fallback_queries, st_q);
    atomicAdd(&ctr->fb_steps, st_steps); atomicAdd(&ctr->fb_leaves, st_leaves);
    atomicMax(&ctr->fb_max_steps, st_max_steps); atomicMax(&ctr->fb_max_leaves, st_max_leaves);
  }
}

// ------------------------------------------------------------- host driver ---
// k_nn_fallback's grid: up to 65536 wavefronts (= workgroups), i.e. one or two queries per wavefront for lists up to 128 k
// and the hardware's workgroup dispatch as the load balancer (query costs spread 1:4).  With four wavefronts per workgroup,
// 2048 / 4096 / 16384 / 65536 workgroups: 0.384 / 0.387 / 0.368 / 0.369 ms at workload M, 0.136 / 0.125 / 0.126 / 0.125 ms
// on an eighth of it.
constexpr unsigned g_fb_max_blocks = 65536;
// where k_nn_fallback finds its queries: prepared records (FUSED == 0) or the caller's doubles (FUSED != 0); the
// queries list[0 .. *list_count), or without a list 0 .. n - 1 (n: an upper bound when the list's length is on the device)
struct FbQueries {
  const float4* qf4;
  FbFused fused;
  const uint32_t *list, *list_count;
};
template <int FUSED>
static pcd_status launch_fallback(const pcd_cloud* c, const float4* seeds, const FbQueries& src, uint64_t n, uint64_t* keys,
                                  NnCounters* ctr, int collect_stats, hipStream_t s) {
  const unsigned blocks = (unsigned)std::min<uint64_t>(n, g_fb_max_blocks);
  QueryScratch* sc = c->scratch;   // (the callers' scratch_of(c))
  if (collect_stats & 16) {   // a pass that keeps {start, end, steps} of every wavefront
    PCD_TRY(sc->fb_rec.reserve(3 * (size_t)blocks));
    sc->fb_rec_n = blocks;
  }
  hipLaunchKernelGGL(k_nn_fallback<FUSED>, dim3(blocks), dim3(64), fb_stack_bytes(c->pyr.nlev),
                     s, c->grid, c->pyr, c->sorted.p, c->cell_start.p, c->blk_aabb.p, seeds, src.qf4, src.list,
                     src.list_count, src.list_count ? 0u : (uint32_t)n, keys, ctr, collect_stats, src.fused, sc->fb_rec.p);
  return PCD_OK;
}
// process-global tuning state (pcd_nn_set_*: experiments and tests, not part of the stable ABI): independent atomic
// switches, each read once at the top of a call
static std::atomic<int> g_collect_stats{0};
#ifdef PCD_ABLATE   // occupancy experiments (tools/nn_ablate.py): workgroups of the brick kernels per CU
static const int g_brick_blocks_per_cu = std::getenv("PCD_BRICK_BLOCKS") ? std::atoi(std::getenv("PCD_BRICK_BLOCKS")) : PCD_BRICK_MINWAVES;
#else
constexpr int g_brick_blocks_per_cu = PCD_BRICK_MINWAVES;
#endif
// first stage of the grid path: 0 = the clipped brick kernel (brick_clip_kernel.h), 1 = the same kernel with the clip
// switched off (A/B timing and tests: it then stages the whole region; results identical)
static std::atomic<int> g_nn_kernel{0};
static std::atomic<int> g_bk_sort{0};   // 1: force the radix-sort bookkeeping (A/B timing, tests)
// how the brick kernel's items are spread over its wavefronts: 0 = static rounds, then chunks from a cursor per block
// class (brick_clip_kernel.h), 1 = the static strided schedule alone (A/B timing and tests; results identical)
static std::atomic<int> g_nn_schedule{0};

// slot table of the cloud (built on first use)
static pcd_status brick_slots(pcd_cloud* c, QueryScratch* sc, const BrickParams& b, hipStream_t s) {
  if (sc->bk_slot.p && sc->bk_nslots == b.nbricks) return PCD_OK;
  PCD_TRY(sc->bk_slot.reserve((size_t)b.nbricks / 32 + 1));
  DevBuf<uint32_t> flag;
  PCD_TRY(flag.reserve((size_t)b.nbricks + 1));
  hipLaunchKernelGGL(k_brick_occupied, dim3(div_up(b.nbricks, 256)), dim3(256), 0, s, c->grid, b, c->cell_start.p, flag.p);
  hipLaunchKernelGGL(k_brick_bitmap, dim3(div_up(div_up(b.nbricks, 32), 256)), dim3(256), 0, s, flag.p, b.nbricks, sc->bk_slot.p);
  PCD_HIP_TRY(hipStreamSynchronize(s));   // one-off per cloud; `flag` goes out of scope
  sc->bk_nslots = b.nbricks;
  return PCD_OK;
}

// Seed table of k_nn_fallback (per cloud, built once, on first use like the slot table): for every cube of 8x8x8 cells
// (py.seed_dims; = the level-1 nodes of the pyramid) the record {x, y, z, bits(global index)} of the exact nearest cloud
// point to the cube's centre, found by the library's own exact search (k_nn_fallback over the centres, every seed still
// the sentinel {+inf, +inf, +inf, 0}: its key (inf, 0) is above kKeyInit and changes no minimum).  74 k cubes for
// workload M's grid: a fallback batch of far queries, about a millisecond.
__global__ void k_seed_init(GridParams g, int sdx, int sdy, int sdz, float4* __restrict__ seeds, float4* __restrict__ qf4,
                            uint64_t* __restrict__ keys) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= (uint64_t)sdx * sdy * sdz) return;
  const int x = (int)(i % sdx), y = (int)((i / sdx) % sdy), z = (int)(i / ((uint64_t)sdx * sdy));
  seeds[i] = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
  // the centre of the cube's part inside the grid (any position would do: the seed only has to be a real point)
  const float cx = 0.5f * (float)(8 * x + min(8 * x + 8, g.dims[0])), cy = 0.5f * (float)(8 * y + min(8 * y + 8, g.dims[1])),
              cz = 0.5f * (float)(8 * z + min(8 * z + 8, g.dims[2]));
  qf4[i] = make_float4(g.origin[0] + cx * g.h, g.origin[1] + cy * g.h, g.origin[2] + cz * g.h, 1.f);
  keys[i] = kKeyInit;
}
__global__ void k_seed_gather(const uint64_t* __restrict__ keys, uint64_t n, ShardIndex si, const float4* __restrict__ pts4,
                              float4* __restrict__ seeds) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  const uint64_t row = k == PCD_KEY_NONE ? ~0ull : shard_local_row(si, (uint32_t)k);
  if (row == ~0ull) return;   // nothing found (distances beyond FLT_MAX): the sentinel stays
  const float4 p = pts4[row];
  seeds[i] = make_float4(p.x, p.y, p.z, __uint_as_float((uint32_t)k));
}
static pcd_status fb_seed_table(pcd_cloud* c, QueryScratch* sc, hipStream_t s) {
  if (sc->fb_seed_ok) return PCD_OK;
  const PyramidParams& py = c->pyr;
  const uint64_t n = (uint64_t)py.seed_dims[0] * py.seed_dims[1] * py.seed_dims[2];
  DevBuf<float4> qf4;
  DevBuf<uint64_t> keys;
  DevBuf<float4>& seeds = sc->fb_seed;
  PCD_TRY(seeds.reserve(n));
  PCD_TRY(qf4.reserve(n));
  PCD_TRY(keys.reserve(n));
  hipLaunchKernelGGL(k_seed_init, dim3(div_up(n, 256)), dim3(256), 0, s, c->grid, py.seed_dims[0], py.seed_dims[1],
                     py.seed_dims[2], seeds.p, qf4.p, keys.p);
  PCD_TRY(launch_fallback<0>(c, seeds.p, {qf4.p}, n, keys.p, nullptr, 0, s));
  hipLaunchKernelGGL(k_seed_gather, dim3(div_up(n, 256)), dim3(256), 0, s, keys.p, n, c->shard_index(), c->pts4.p, seeds.p);
  PCD_HIP_TRY(hipGetLastError());
  PCD_HIP_TRY(hipStreamSynchronize(s));   // one-off per cloud; qf4 / keys go out of scope
  sc->fb_seed_ok = true;
  return PCD_OK;
}

// The counters: two blocks, zeroed once when they are allocated.  Grid-path calls with the counting-sort bookkeeping
// use them alternately and need no memset of their own: k_bk_slots of call n clears the block call n + 1 will use (its
// last users, the kernels of call n - 1, finished before call n started on the stream).  sc->ctr_cur is the block of
// the last call (pcd_nn_last_stats reads it); every other path clears and uses that block with its own memset (the
// one-launch walk only when it collects statistics: nothing else reads its counters).
// sc->ctr_next_clean is false from the start of a counting-sort call until all of its launches went through
// (counters_left_clean): a call that failed part-way makes the next one fall back to the memset.
static pcd_status counters_ready(QueryScratch* sc, hipStream_t s) {
  if (sc->counters.p) return PCD_OK;
  PCD_TRY(sc->counters.reserve(2));
  PCD_HIP_TRY(hipMemsetAsync(sc->counters.p, 0, 2 * sizeof(NnCounters), s));
  sc->ctr_cur = 0;
  sc->ctr_next_clean = true;
  return PCD_OK;
}
// hands a path its block (*ctr; *ctr_next: the block of the next alternating call), cleared where the path needs it
enum class CtrUse { kAlternate, kClear, kClearForStats };
static pcd_status take_counters(QueryScratch* sc, CtrUse use, int collect_stats, hipStream_t s, NnCounters** ctr,
                                NnCounters** ctr_next = nullptr) {
  PCD_TRY(counters_ready(sc, s));
  const bool clean = use == CtrUse::kAlternate ? sc->ctr_next_clean : use == CtrUse::kClearForStats && !collect_stats;
  if (use == CtrUse::kAlternate) {
    sc->ctr_cur = 1 - sc->ctr_cur;
    sc->ctr_next_clean = false;
  }
  *ctr = sc->counters.p + sc->ctr_cur;
  if (ctr_next) *ctr_next = sc->counters.p + (1 - sc->ctr_cur);
  if (!clean) PCD_HIP_TRY(hipMemsetAsync(*ctr, 0, sizeof(NnCounters), s));
  return PCD_OK;
}
static void counters_left_clean(QueryScratch* sc) { sc->ctr_next_clean = true; }

static void launch_prepare(const NnCall& call, uint64_t Q, float4* qf4, uint64_t* d_keys, hipStream_t s) {
  ScopedKernelTimer t("nn_prepare", s);
  with_prep_mode(call.prep, [&](auto mode) {
    hipLaunchKernelGGL(k_prepare<decltype(mode)::value>, dim3(div_up(Q, 256)), dim3(256), 0, s, call.pa, Q, qf4, d_keys);
  });
}
static void launch_finalize(uint64_t Q, uint64_t* d_keys, hipStream_t s) {
  ScopedKernelTimer t("nn_finalize", s);
  hipLaunchKernelGGL(k_finalize_keys, dim3(div_up(Q, 256)), dim3(256), 0, s, d_keys, Q);
}
static void launch_bruteforce(const pcd_cloud* c, const float4* qf4, uint64_t Q, uint64_t* d_keys, hipStream_t s) {
  ScopedKernelTimer t("nn_bruteforce", s);
  // enough chunks to fill the chip even for few queries
  const unsigned qblocks = div_up(Q, 256);
  unsigned chunks = std::max(1u, std::min<unsigned>(div_up(c->n, 4096), 2048u / std::max(1u, qblocks)));
  chunks = std::min(chunks, 65535u);
  const uint64_t chunk = ((c->n + chunks - 1) / chunks + 1023) / 1024 * 1024;
  chunks = div_up(c->n, chunk);
  hipLaunchKernelGGL(k_nn_bruteforce, dim3(qblocks, chunks), dim3(256), 0, s, c->pts4.p, c->n, c->index_base,
                     c->index_stride, c->row_index.p, qf4, Q, chunk, d_keys);
}

// The grid path: query bookkeeping, brick kernel, exact fallback for what is left.  The counting-sort bookkeeping does
// the preparation in its first kernel; the radix-sort bookkeeping runs the stand-alone prepare kernel first.
constexpr int kGroup = 8;   // queries per work item of the brick kernel (brick_clip_kernel.h is written for 8)
static pcd_status run_grid(pcd_cloud* c, QueryScratch* sc, uint64_t Q, uint64_t* d_keys, hipStream_t s, const NnCall& call) {
  const uint64_t* carried_keys = call.prep != kPrepPlain ? d_keys : nullptr;   // refine, gate-bounded: the keys the queries come with matter
  const GridParams& g = c->grid;
  const int nn_kernel = g_nn_kernel.load(), bk_sort = g_bk_sort.load(), collect_stats = g_collect_stats.load();
  const int nn_schedule = g_nn_schedule.load();
  const BrickParams b = make_bricks(g);
  PCD_TRY(sc->qsorted.reserve(Q));
  PCD_TRY(sc->ksorted.reserve(Q));
  // fallback list: one slot per query + the chunk slack of every wavefront of the brick kernel (brick_kernel.h)
  // A wavefront leaves a chunk when the next item's unproven queries (<= 8) do not fit: at most 7 of 64 slots stay
  // unused per chunk, so the reserved slots are <= used * 64 / 57 + one chunk per wavefront, used <= Q.
  const size_t fb_cap = Q + Q / 8 + 8 + (size_t)256 * g_brick_blocks_per_cu * 4 * kFbChunk +
                        (size_t)2048 * 4 * 64;   // + the last chunk of every wavefront of k_bk_emit
  PCD_TRY(sc->fb_list.reserve(fb_cap));   // no memset: every reserved slot is written (a query id or the sentinel)
  PCD_TRY(sc->bk_keys.reserve(2 * Q));
  PCD_TRY(sc->bk_vals.reserve(2 * Q));
  PCD_TRY(sc->bk_item.reserve(div_up(Q, kBkTile) + 1));
  PCD_TRY(sc->items.reserve(Q + 1));
  PCD_TRY(counters_ready(sc, s));   // (the one-off work of a cloud's first call, in this order)
  PCD_TRY(brick_slots(c, sc, b, s));
  // sort key = brick id: coarse key = id >> shift (at most 4096 buckets), fine key = the low bits (at most 4096)
  uint32_t shift = 8;
  while ((((uint64_t)b.nbricks + (1u << shift) - 1) >> shift) > 2304 && shift < 16) ++shift;
  const uint32_t ncoarse = std::max<uint32_t>(1u, (uint32_t)(((uint64_t)b.nbricks + (1u << shift) - 1) >> shift));
  const bool counting = (1u << shift) <= kBkMaxFine && ncoarse <= kBkMaxCoarse && bk_sort == 0;
  NnCounters *ctr, *ctr_next;
  PCD_TRY(take_counters(sc, counting ? CtrUse::kAlternate : CtrUse::kClear, collect_stats, s, &ctr, &ctr_next));
  if (counting) {
    ScopedKernelTimer t("nn_brick_bookkeeping", s);
    // bucket totals | bucket starts | items per bucket; the histogram matrix [ranges][ncoarse] (<= 256 x 4096 entries);
    // every entry that is read is written by the call itself: nothing to zero
    const uint32_t nrounds = div_up(Q, kBkTileQ), rounds = div_up(nrounds, kBkMaxRanges), nranges = div_up(nrounds, rounds);
    PCD_TRY(sc->bk_chist.reserve(3 * (size_t)kBkMaxCoarse + 3));
    PCD_TRY(sc->bk_hmat.reserve((size_t)nranges * ncoarse));
    uint32_t *ctot = sc->bk_chist.p, *cstart = ctot + kBkMaxCoarse + 1, *bitems = cstart + kBkMaxCoarse + 1;
    uint32_t* qslot = sc->bk_keys.p;
    uint2* ppair = reinterpret_cast<uint2*>(sc->bk_vals.p);   // 2 Q words: Q {fine key, query id} pairs
    with_prep_mode(call.prep, [&](auto mode) {
      hipLaunchKernelGGL(k_bk_slots<decltype(mode)::value>, dim3(nranges), dim3(1024), 0, s, call.pa, (uint32_t)Q, rounds,
                         g, b, sc->bk_slot.p, shift, ncoarse, sc->qf4.p, d_keys, qslot, sc->bk_hmat.p, sc->fb_list.p, ctr,
                         ctr_next);
    });
    hipLaunchKernelGGL(k_bk_colscan, dim3(div_up(ncoarse, 64)), dim3(1024), 0, s, sc->bk_hmat.p, nranges, ncoarse, ctot);
    hipLaunchKernelGGL(k_bk_scatter, dim3(nranges), dim3(1024), 0, s, qslot, (uint32_t)Q, rounds, shift, ncoarse, ctot,
                       sc->bk_hmat.p, cstart, ppair, ctr);
    hipLaunchKernelGGL(k_bk_count<kGroup>, dim3(ncoarse), dim3(256), 0, s, shift, cstart, ppair, bitems);
    hipLaunchKernelGGL(k_bk_emit<kGroup>, dim3(ncoarse), dim3(256), (3u * (1u << shift) + 2u) * sizeof(uint32_t), s,
                       sc->qf4.p, carried_keys, g, b, shift, cstart, ppair, bitems, sc->items.p, sc->qsorted.p, sc->ksorted.p, ctr);
  } else {
    // (grids with more than 8 M occupied bricks: the radix-sort bookkeeping of round 2)
    launch_prepare(call, Q, sc->qf4.p, d_keys, s);
    ScopedKernelTimer t("nn_brick_bookkeeping", s);
    uint32_t *k0 = sc->bk_keys.p, *k1 = sc->bk_keys.p + Q, *v0 = sc->bk_vals.p, *v1 = sc->bk_vals.p + Q;
    hipLaunchKernelGGL(k_brick_keys, dim3(div_up(Q, 256)), dim3(256), 0, s, sc->qf4.p, Q, g, b, k0, v0);
    unsigned end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) <= (uint64_t)b.nbricks + 1) ++end_bit;
#ifndef PCD_SORT_MERGE_LIMIT
#define PCD_SORT_MERGE_LIMIT 262144
#endif
    // rocPRIM's default takes its merge sort up to 2^20 items: Onesweep above 256 k
    using SortCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                               rocprim::default_config, PCD_SORT_MERGE_LIMIT>;
    PCD_TRY(sort_pairs<SortCfg>(sc->tmp, k0, k1, v0, v1, (unsigned)Q, 0u, end_bit, s));
    const unsigned ntiles = div_up(Q, kBkTile);
    hipLaunchKernelGGL(k_brick_tile_count<kGroup>, dim3(ntiles), dim3(256), 0, s, k1, (uint32_t)Q, b.nbricks, sc->bk_item.p);
    hipLaunchKernelGGL(k_brick_emit<kGroup>, dim3(ntiles), dim3(256), 0, s, k1, v1, sc->bk_item.p, sc->qf4.p, carried_keys,
                       (uint32_t)Q, b.nbricks, (uint32_t)b.nb[0], (uint32_t)b.nb[1], sc->items.p, sc->qsorted.p,
                       sc->ksorted.p, sc->fb_list.p, ctr);
  }
  {
    ScopedKernelTimer t("nn_brick", s);
    const unsigned blocks = (unsigned)std::min<uint64_t>(div_up(div_up(Q, kGroup), 4) + 1, 256 * (uint64_t)g_brick_blocks_per_cu);
    // flags: 1 statistics, 2 clip off, 4 per-wavefront records (statistics passes only), 8 static schedule
    int fl = (collect_stats & ~(2 | 4 | 8)) | (nn_kernel == 1 ? 2 : 0) | (nn_schedule == 1 ? 8 : 0);
    if ((collect_stats & 5) == 5) {
      PCD_TRY(sc->wave_rec.reserve(3 * (size_t)blocks * 4));
      sc->wave_rec_n = blocks * 4;
      fl |= 4;
    } else {
      sc->wave_rec_n = 0;
    }
    hipLaunchKernelGGL(k_nn_brick_clip, dim3(blocks), dim3(256), 0, s, g, c->sorted.p, c->cell_start.p, sc->qsorted.p,
                       sc->ksorted.p, sc->items.p, ctr, d_keys, sc->fb_list.p, &ctr->fb_count, fl, sc->wave_rec.p);
  }
  {
    ScopedKernelTimer t("nn_fallback", s);
    PCD_TRY(sc->fb_dense.reserve(Q));
    hipLaunchKernelGGL(k_fb_compact, dim3(div_up(fb_cap, kFbcThreads * kFbcPer)), dim3(kFbcThreads), 0, s, sc->fb_list.p,
                       &ctr->fb_count, sc->fb_dense.p, &ctr->pad[0]);
    PCD_TRY(launch_fallback<0>(c, sc->fb_seed.p, {sc->qf4.p, {}, sc->fb_dense.p, &ctr->pad[0]}, Q, d_keys, ctr, collect_stats, s));
  }
  PCD_HIP_TRY(hipGetLastError());
  if (counting) counters_left_clean(sc);   // every launch went through: k_bk_slots has left the other block clean
  return PCD_OK;
}

// The one place that decides which way a call goes.  kOneLaunch: k_nn_fallback converts the queries itself and writes
// finalised keys, so the per-call latency of a small batch (and of PCD_NN_FALLBACK_ONLY) is one kernel instead of
// prepare + memset + search; refining another shard's keys, the keys come in, so the prepare kernel stays (kPrepareWalk).
enum class NnPath { kEmptyCloud, kBruteForce, kOneLaunch, kPrepareWalk, kGrid };
static pcd_status choose_path(bool empty_cloud, int algo, uint64_t Q, int prep, NnPath* path) {
  const NnPath walk = prep == kPrepRefine ? NnPath::kPrepareWalk : NnPath::kOneLaunch;
  if (empty_cloud) *path = NnPath::kEmptyCloud;   // whatever the algo
  else if (algo == PCD_NN_BRUTEFORCE) *path = NnPath::kBruteForce;
  else if (algo == PCD_NN_FALLBACK_ONLY) *path = walk;
  else if (algo == PCD_NN_AUTO) *path = Q <= kSmallBatch ? walk : NnPath::kGrid;
  else if (algo == PCD_NN_GRID) *path = NnPath::kGrid;
  else {
    set_error("unknown nn algo %d", algo);
    return PCD_ERR_INVALID;
  }
  return PCD_OK;
}

static pcd_status nn_device(pcd_cloud* c, const NnCall& call, uint64_t Q, int algo, uint64_t* d_keys, hipStream_t s) {
  QueryScratch* sc = scratch_of(c);
  if (Q == 0) return PCD_OK;
  PCD_REQUIRE(Q < 0xFFFFFFF0ull, "more than 2^32 queries in one call");
  sc->wave_rec_n = sc->fb_rec_n = 0;   // (a statistics pass sets them: the grid path / the fallback walk)
  NnPath path;
  PCD_TRY(choose_path(c->m == 0, algo, Q, call.prep, &path));
  const int collect_stats = g_collect_stats.load();
  NnCounters* ctr;
  switch (path) {
    case NnPath::kEmptyCloud:   // nothing to search: the prepare kernel's keys are all there is
    case NnPath::kBruteForce:
      PCD_TRY(sc->qf4.reserve(Q));
      launch_prepare(call, Q, sc->qf4.p, d_keys, s);
      if (path == NnPath::kBruteForce) launch_bruteforce(c, sc->qf4.p, Q, d_keys, s);
      launch_finalize(Q, d_keys, s);   // raw keys left behind: the brute-force kernel's atomicMin, an empty cloud
      break;
    case NnPath::kOneLaunch: {
      PCD_TRY(fb_seed_table(c, sc, s));
      PCD_TRY(take_counters(sc, CtrUse::kClearForStats, collect_stats, s, &ctr));
      ScopedKernelTimer t("nn_fallback", s);
      const FbQueries src{nullptr, FbFused{call.pa.q, call.pa.max_range, call.pa.mr_count, call.pa.fixed_range}};
      if (call.prep == kPrepBounded) PCD_TRY(launch_fallback<2>(c, sc->fb_seed.p, src, Q, d_keys, ctr, collect_stats, s));
      else PCD_TRY(launch_fallback<1>(c, sc->fb_seed.p, src, Q, d_keys, ctr, collect_stats, s));
      break;
    }
    case NnPath::kPrepareWalk: {
      PCD_TRY(fb_seed_table(c, sc, s));
      PCD_TRY(sc->qf4.reserve(Q));
      launch_prepare(call, Q, sc->qf4.p, d_keys, s);
      PCD_TRY(take_counters(sc, CtrUse::kClear, collect_stats, s, &ctr));
      ScopedKernelTimer t("nn_fallback", s);
      PCD_TRY(launch_fallback<0>(c, sc->fb_seed.p, {sc->qf4.p}, Q, d_keys, ctr, collect_stats, s));
      break;
    }
    case NnPath::kGrid:
      PCD_TRY(fb_seed_table(c, sc, s));
      PCD_TRY(sc->qf4.reserve(Q));
      PCD_TRY(run_grid(c, sc, Q, d_keys, s, call));
      break;
  }
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

// the entry points' description of a call: the flavour and what it reads
static NnCall make_call(int prep, const pcd_cloud* c, const double* d_q, const uint8_t* d_skip = nullptr,
                        const double* d_max_range = nullptr, uint64_t mr_count = 0, double fixed_range = 0.0) {
  const BoxF box{c->bb_lo[0], c->bb_lo[1], c->bb_lo[2], c->bb_hi[0], c->bb_hi[1], c->bb_hi[2]};
  return {prep, {d_q, d_skip, box, d_max_range, mr_count, fixed_range}};
}

pcd_status nn_query_device_internal(pcd_cloud* c, const double* d_q, uint64_t Q, int algo, uint64_t* d_keys,
                                    hipStream_t s) {
  return nn_device(c, make_call(kPrepPlain, c, d_q), Q, algo, d_keys, s);
}
// bounded by the association gate: d_max_range (1 or Q entries) or, when NULL, fixed_range
pcd_status nn_query_bounded_internal(pcd_cloud* c, const double* d_q, uint64_t Q, const double* d_max_range,
                                     uint64_t mr_count, double fixed_range, uint64_t* d_keys, hipStream_t s) {
  return nn_device(c, make_call(kPrepBounded, c, d_q, nullptr, d_max_range, mr_count, fixed_range), Q, PCD_NN_AUTO, d_keys, s);
}

}  // namespace pcd

using namespace pcd;

extern "C" {

pcd_status pcd_nn_query_device(pcd_cloud* c, const double* d_q_xyz, uint64_t Q, int algo, uint64_t* d_keys,
                               void* stream) {
  PCD_REQUIRE(c, "null cloud");
  PCD_REQUIRE(Q == 0 || (d_q_xyz && d_keys), "null pointer");
  PCD_REFUSE_CAPTURE(stream);
  PCD_HIP_TRY(hipSetDevice(c->device));
  return nn_device(c, make_call(kPrepPlain, c, d_q_xyz), Q, algo, d_keys, (hipStream_t)stream);
}

pcd_status pcd_nn_refine_device(pcd_cloud* c, const double* d_q_xyz, uint64_t Q, const uint8_t* d_skip,
                                uint64_t* d_keys, void* stream) {
  PCD_REQUIRE(c, "null cloud");
  PCD_REQUIRE(Q == 0 || (d_q_xyz && d_keys), "null pointer");
  PCD_REFUSE_CAPTURE(stream);
  PCD_HIP_TRY(hipSetDevice(c->device));
  return nn_device(c, make_call(kPrepRefine, c, d_q_xyz, d_skip), Q, PCD_NN_AUTO, d_keys, (hipStream_t)stream);
}

pcd_status pcd_nn_query_algo(pcd_cloud* c, const double* q_xyz, uint64_t Q, int algo, uint32_t* idx, float* sqdist,
                             uint8_t* found) {
  PCD_REQUIRE(c, "null cloud");
  PCD_REQUIRE(Q == 0 || (q_xyz && idx && sqdist && found), "null pointer");
  if (Q == 0) return PCD_OK;
  PCD_HIP_TRY(hipSetDevice(c->device));
  QueryScratch* sc = scratch_of(c);
  hipStream_t s = nullptr;
  PCD_TRY(sc->d_q.reserve(3 * Q));
  PCD_TRY(sc->keys.reserve(Q));
  PCD_TRY(sc->d_idx.reserve(Q));
  PCD_TRY(sc->d_sq.reserve(Q));
  PCD_TRY(sc->d_found.reserve(Q));
  PCD_HIP_TRY(hipMemcpyAsync(sc->d_q.p, q_xyz, 3 * Q * sizeof(double), hipMemcpyHostToDevice, s));
  PCD_TRY(nn_device(c, make_call(kPrepPlain, c, sc->d_q.p), Q, algo, sc->keys.p, s));
  hipLaunchKernelGGL(k_unpack_keys, dim3(div_up(Q, 256)), dim3(256), 0, s, sc->keys.p, Q, sc->d_idx.p, sc->d_sq.p,
                     sc->d_found.p);
  PCD_HIP_TRY(hipMemcpyAsync(idx, sc->d_idx.p, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipMemcpyAsync(sqdist, sc->d_sq.p, Q * sizeof(float), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipMemcpyAsync(found, sc->d_found.p, Q * sizeof(uint8_t), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipStreamSynchronize(s));
  return PCD_OK;
}

pcd_status pcd_nn_query(pcd_cloud* c, const double* q_xyz, uint64_t Q, uint32_t* idx, float* sqdist, uint8_t* found) {
  return pcd_nn_query_algo(c, q_xyz, Q, PCD_NN_AUTO, idx, sqdist, found);
}

pcd_status pcd_nn_last_stats(pcd_cloud* c, pcd_nn_stats* st) {
  PCD_REQUIRE(c && st, "null pointer");
  std::memset(st, 0, sizeof *st);
  if (!c->scratch || !c->scratch->counters.p) return PCD_OK;
  PCD_HIP_TRY(hipSetDevice(c->device));
  PCD_HIP_TRY(hipDeviceSynchronize());
  NnCounters h;
  PCD_HIP_TRY(hipMemcpy(&h, c->scratch->counters.p + c->scratch->ctr_cur, sizeof h, hipMemcpyDeviceToHost));
  st->brick_groups = h.brick_groups;
  st->staged_points = h.staged_points;
  st->fallback_queries = h.fallback_queries;
  st->fallback_points = h.fallback_points;
  st->pair_evals = h.pair_evals;
  static const bool print_walks = std::getenv("PCD_FB_STATS") != nullptr;   // read once per process
  if (print_walks)
    std::fprintf(stderr, "[pcd] fallback walk: %llu queries, %.1f steps / %.1f leaf scans per query, max %u / %u\n",
                 (unsigned long long)h.fallback_queries, h.fallback_queries ? (double)h.fb_steps / h.fallback_queries : 0.0,
                 h.fallback_queries ? (double)h.fb_leaves / h.fallback_queries : 0.0, h.fb_max_steps, h.fb_max_leaves);
  return PCD_OK;
}

/* tuning hook: which kernel serves the grid path's first stage (g_nn_kernel above).  Negative: leave it as it is. */
pcd_status pcd_nn_set_search(int kernel) {
  if (kernel < 0) return PCD_OK;
  PCD_REQUIRE(kernel <= 1, "kernel must be 0 (clipped brick kernel) or 1 (the same with the clip off); there is no separate "
                           "whole-region kernel: the clip-off switch, pcd_nn_set_search(1), is the A/B reference");
  g_nn_kernel = kernel;
  return PCD_OK;
}

/* tuning hook: the brick kernel's work schedule (g_nn_schedule above).  Negative: leave it as it is. */
pcd_status pcd_nn_set_schedule(int schedule) {
  if (schedule < 0) return PCD_OK;
  PCD_REQUIRE(schedule <= 1, "schedule must be 0 (static rounds + dynamic chunks) or 1 (static)");
  g_nn_schedule = schedule;
  return PCD_OK;
}

/* tools / tests: the compile-time constants of schedule 0 -- static share of the rounds in percent, items per chunk */
pcd_status pcd_nn_schedule_params(int* static_pct, int* chunk) {
  PCD_REQUIRE(static_pct && chunk, "null pointer");
  *static_pct = (int)kSchedStaticPct;
  *chunk = (int)kSchedChunk;
  return PCD_OK;
}

/* tools / tests: the records of the last grid-path call of a statistics pass with bit 4 -- {start, end, items} per
   wavefront of the brick kernel, wall_clock64 ticks -- and the call's number of work items.  Fills up to cap_waves
   records; *nwaves = wavefronts launched (0: the last call kept no records).  Syncs. */
pcd_status pcd_nn_last_wave_records(pcd_cloud* c, uint64_t* records, uint64_t cap_waves, uint64_t* nwaves, uint64_t* nitems) {
  PCD_REQUIRE(c && nwaves && nitems, "null pointer");
  *nwaves = *nitems = 0;
  if (!c->scratch || !c->scratch->counters.p) return PCD_OK;
  QueryScratch* sc = c->scratch;
  PCD_HIP_TRY(hipSetDevice(c->device));
  PCD_HIP_TRY(hipDeviceSynchronize());
  NnCounters h;
  PCD_HIP_TRY(hipMemcpy(&h, sc->counters.p + sc->ctr_cur, sizeof h, hipMemcpyDeviceToHost));
  *nitems = h.nitems;
  *nwaves = sc->wave_rec_n;
  const uint64_t n = std::min<uint64_t>(cap_waves, sc->wave_rec_n);
  if (n && records) PCD_HIP_TRY(hipMemcpy(records, sc->wave_rec.p, n * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return PCD_OK;
}

/* tools / tests: the same for k_nn_fallback, from the last call of a statistics pass with bit 16 -- {start, end, walk
   steps} per wavefront, in the order blockIdx.x * waves_per_block + wave.  Syncs. */
pcd_status pcd_nn_last_fb_wave_records(pcd_cloud* c, uint64_t* records, uint64_t cap_waves, uint64_t* nwaves,
                                       uint64_t* waves_per_block) {
  PCD_REQUIRE(c && nwaves && waves_per_block, "null pointer");
  *nwaves = 0;
  *waves_per_block = 1;
  if (!c->scratch) return PCD_OK;
  QueryScratch* sc = c->scratch;
  PCD_HIP_TRY(hipSetDevice(c->device));
  PCD_HIP_TRY(hipDeviceSynchronize());
  *nwaves = sc->fb_rec_n;
  const uint64_t n = std::min<uint64_t>(cap_waves, sc->fb_rec_n);
  if (n && records) PCD_HIP_TRY(hipMemcpy(records, sc->fb_rec.p, n * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return PCD_OK;
}

pcd_status pcd_nn_set_bookkeeping(int radix_sort) {
  g_bk_sort = radix_sort ? 1 : 0;
  return PCD_OK;
}

/* tuning hook (not part of the stable ABI; used by bench.py and tests): the statistics switch.  The brick geometry is
   fixed (kBrickCells / kBrickHalo); brick_cells = 0 and halo_cells < 0 mean "as it is".  A refused call changes nothing. */
pcd_status pcd_nn_set_tuning(int brick_cells, int halo_cells, int collect_stats) {
  if ((brick_cells != 0 && brick_cells != kBrickCells) || (halo_cells >= 0 && halo_cells != kBrickHalo)) {
    set_error("pcd_nn_set_tuning: the brick geometry is fixed at %d cells with a halo of %d (asked for %d / %d)",
              kBrickCells, kBrickHalo, brick_cells, halo_cells);
    return PCD_ERR_UNSUPPORTED;
  }
#ifdef PCD_ABLATE
  g_collect_stats = collect_stats;
#else
  g_collect_stats = collect_stats & 21;   // (4 / 16: per-wavefront records of the brick kernel / of the fallback walk) the ablation bits exist only in -DPCD_ABLATE builds
#endif
  return PCD_OK;
}

}  // extern "C"

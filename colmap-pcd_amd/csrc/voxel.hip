// voxel.hip -- voxel-grid downsampling of a cloud handle into a new handle (pcd_cloud_voxel_downsample, definition in
// include/pcdhip.h).  Reference behaviour restated: pcl::VoxelGrid with downsample_all_data = true, as
// PointCloudProcess::LoadDownsizedMap runs it (lidar/ply.cc:59-84); the sums are fp64 in a fixed order instead of
// PCL's float sums in the order of an unstable sort.
//
// Passes:  k_voxel_keys (64-bit key per row, Inf rows last)  ->  rocprim stable radix sort of (key, row) over the bits
// the key range needs  ->  k_voxel_heads + inclusive scan (voxel id of every sorted row)  ->  k_voxel_segments (segment
// starts)  ->  k_voxel_keep + ONE exclusive scan of packed {kept, long} flags (output row and place in the list of long
// voxels)  ->  one host synchronisation (the counts size the new handle)  ->  k_voxel_reduce_short / k_voxel_reduce_long
// (the sums and the epilogue, writing the new handle's pts4 / pn8)  ->  k_voxel_map (row_voxel)  ->  the index build.
//
// The order of a voxel's sum (pcdhip.h) on 64 VIRTUAL lanes: row e of a piece of 512 sits on virtual lane e % 64, a
// lane adds its rows e, e + 64, ... in sequence, the lanes are added by a butterfly over the offsets 8, 16, 32, 1, 2, 4,
// the pieces in sequence.  Two kernels realise it:
//   long   (k > 32)   one wavefront per voxel, virtual lane = lane;
//   short  (k <= 32)  8 lanes per voxel, lane g holds the virtual lanes g + 8 j: the offsets 8, 16, 32 are adds between
//                     the lane's own registers (j ^ 1, j ^ 2, j ^ 4), the offsets 1, 2, 4 three DPP steps inside the
//                     group -- at a 3-5 cm leaf most voxels hold a handful of rows and a wavefront serves 8 of them.
// Absent rows are +0.0, which changes no sum but the sign of a zero one; the epilogue adds +0.0 to every total so both
// kernels give the same bits for the same rows.
#include <cmath>

#include "cloud.h"
#include "prim.h"

namespace pcd {

constexpr int kVxGroup = 8;                  // lanes per voxel in the short kernel
constexpr int kVxShortMax = 32;              // longest segment of the short kernel: 4 rows per lane keep it at 8 wavefronts
                                             // per SIMD; longer ones are worth a wavefront of their own
constexpr int kVxStride = 8;                 // rows per lane and piece
constexpr int kVxPiece = 64 * kVxStride;     // rows per piece

struct VoxelParams {
  float inv[3];
  long long min_b[3];
  unsigned long long d0, d1;
  unsigned long long inf_key;   // d0 d1 d2: above every voxel's key
};

// ------------------------------------------------------------- kernels ----
__global__ void k_voxel_keys(const float4* __restrict__ pn8, uint64_t n, VoxelParams P,
                             unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pn8[2 * i];
  unsigned long long key = P.inf_key;
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    // one float multiply (the build has -ffp-contract=off), then floor; inside the handle's bounds, so 0 <= c_a < d_a
    const long long c0 = (long long)(int)floorf(p.x * P.inv[0]) - P.min_b[0];
    const long long c1 = (long long)(int)floorf(p.y * P.inv[1]) - P.min_b[1];
    const long long c2 = (long long)(int)floorf(p.z * P.inv[2]) - P.min_b[2];
    key = (unsigned long long)c0 + P.d0 * ((unsigned long long)c1 + P.d1 * (unsigned long long)c2);
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

__global__ void k_voxel_heads(const unsigned long long* __restrict__ keys, uint64_t m, uint32_t* __restrict__ flag) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// seg[v] = first sorted row of voxel v, seg[nv] = m; cnt[0] = nv.  vid1 = inclusive scan of the head flags = voxel id + 1
__global__ void k_voxel_segments(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ vid1, uint64_t m,
                                 uint32_t* __restrict__ seg, unsigned long long* __restrict__ cnt) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t v1 = vid1[i];
  if (flag[i]) seg[v1 - 1] = (uint32_t)i;
  if (i == m - 1) {
    seg[v1] = (uint32_t)m;
    cnt[0] = v1;
  }
}

// kl[v] = kept | long << 32 for v < nv, 0 up to m (the scan runs over m + 1 entries: nv is not on the host yet);
// cnt[1] += rows of dropped voxels, cnt[2] = max rows per voxel (integer atomics: the result has no order)
__global__ void k_voxel_keep(const uint32_t* __restrict__ seg, uint64_t m, uint32_t min_points,
                             unsigned long long* __restrict__ kl, unsigned long long* __restrict__ cnt) {
  const uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const unsigned long long nv = cnt[0];
  unsigned long long dropped = 0;
  uint32_t maxc = 0;
  if (v <= m) {
    unsigned long long f = 0;
    if (v < nv) {
      const uint32_t c = seg[v + 1] - seg[v];
      const bool keep = c >= min_points;
      f = (keep ? 1ull : 0ull) | ((keep && c > (uint32_t)kVxShortMax) ? 1ull << 32 : 0ull);
      dropped = keep ? 0 : c;
      maxc = c;
    }
    kl[v] = f;
  }
  for (int off = 32; off > 0; off >>= 1) {
    dropped += __shfl_xor(dropped, off);
    maxc = max(maxc, (uint32_t)__shfl_xor((int)maxc, off));
  }
  if ((threadIdx.x & 63) == 0) {
    if (dropped) atomicAdd(&cnt[1], dropped);
    // (millions of wavefronts on one address: only those that can still raise the maximum go to the atomic unit)
    if (maxc > __hip_atomic_load(&cnt[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&cnt[2], (unsigned long long)maxc);
  }
}

__global__ void k_voxel_long_list(const unsigned long long* __restrict__ kl, const unsigned long long* __restrict__ pos,
                                  uint64_t nv, uint32_t* __restrict__ long_list) {
  const uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (v >= nv) return;
  if (kl[v] >> 32) long_list[pos[v] >> 32] = (uint32_t)v;
}

// the epilogue of one voxel: divide, normalise, round, write row o of the new handle
__device__ __forceinline__ void voxel_emit(uint32_t o, uint32_t k, const double* __restrict__ s,
                                           float4* __restrict__ pts4, float4* __restrict__ pn8) {
  const double kk = (double)k;
  const double px = s[0] + 0.0, py = s[1] + 0.0, pz = s[2] + 0.0;
  const double nx = s[3] + 0.0, ny = s[4] + 0.0, nz = s[5] + 0.0;
  const float4 p = make_float4((float)(px / kk), (float)(py / kk), (float)(pz / kk), 0.f);
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (isfinite(len) && !(len < 1e-12)) q = make_float4((float)(nx / len), (float)(ny / len), (float)(nz / len), 0.f);
  pts4[o] = p;
  pn8[2 * (size_t)o] = p;
  pn8[2 * (size_t)o + 1] = q;
}

// x + (x of the lane the DPP control names), both halves of the double moved by one v_mov_dpp each
template <int kCtrl>
__device__ __forceinline__ double dpp_add(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), kCtrl, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), kCtrl, 0xF, 0xF, false);
  return x + __hiloint2double(hi, lo);
}
constexpr int kDppXor1 = 0xB1;          // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;          // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;   // lane i <-> 7 - i of each 8: after the quad steps every lane of a quad holds the
                                        // quad's sum, so the mirror brings the OTHER quad's sum, as offset 4 would
constexpr int kDppRor8 = 0x128;         // row_ror:8, lane i <-> i ^ 8 of each row of 16
// x + x of lane ^ 16: ds_swizzle in bit mode (and 0x1F, or 0, xor 0x10), the crossbar without an LDS access
__device__ __forceinline__ double swizzle_xor16_add(double x) {
  const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), 0x401F);
  const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), 0x401F);
  return x + __hiloint2double(hi, lo);
}

// kJ rows per lane: segments of up to 8 kJ rows.  Every lane of the wavefront runs this (idle groups with k = 0).
template <int kJ>
__device__ __forceinline__ void voxel_short_sums(const float4* __restrict__ pn8, const uint32_t* __restrict__ vals,
                                                 uint32_t s, uint32_t k, int g, double* __restrict__ sum) {
  float4 P[kJ], N[kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) {
    const uint32_t e = (uint32_t)(g + kVxGroup * j);
    P[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    N[j] = P[j];
    if (e < k) {
      const size_t row = vals[s + e];
      P[j] = pn8[2 * row];
      N[j] = pn8[2 * row + 1];
    }
  }
  double a[6][kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) {
    a[0][j] = (double)P[j].x; a[1][j] = (double)P[j].y; a[2][j] = (double)P[j].z;
    a[3][j] = (double)N[j].x; a[4][j] = (double)N[j].y; a[5][j] = (double)N[j].z;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    // offsets 8, 16, 32 of the butterfly: virtual lanes g + 8 j and g + 8 (j ^ w) are registers of this lane
#pragma unroll
    for (int w = 1; w < kJ; w <<= 1)
#pragma unroll
      for (int j = 0; j < kJ; j += 2 * w) a[c][j] = a[c][j] + a[c][j + w];
    double x = a[c][0];
    x = dpp_add<kDppXor1>(x);
    x = dpp_add<kDppXor2>(x);
    x = dpp_add<kDppHalfMirror>(x);
    sum[c] = x;
  }
}

__global__ __launch_bounds__(256) void k_voxel_reduce_short(const float4* __restrict__ pn8,
                                                            const uint32_t* __restrict__ vals,
                                                            const uint32_t* __restrict__ seg,
                                                            const unsigned long long* __restrict__ kl,
                                                            const unsigned long long* __restrict__ pos, uint64_t nv,
                                                            float4* __restrict__ out_pts4, float4* __restrict__ out_pn8) {
  const uint64_t v = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kVxGroup;
  const int g = threadIdx.x & (kVxGroup - 1);
  uint32_t s = 0, k = 0, o = 0;
  if (v < nv && kl[v] == 1ull) {   // kept and not long
    s = seg[v];
    k = seg[v + 1] - s;
    o = (uint32_t)pos[v];
  }
  // no lane leaves before the DPP steps: their sources must be active.  The branch is on a wavefront-wide maximum.
  uint32_t kmax = k;
  for (int off = 32; off >= kVxGroup; off >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, off));
  kmax = __builtin_amdgcn_readfirstlane(kmax);
  double sum[6];
  if (kmax <= 1 * kVxGroup) voxel_short_sums<1>(pn8, vals, s, k, g, sum);
  else if (kmax <= 2 * kVxGroup) voxel_short_sums<2>(pn8, vals, s, k, g, sum);
  else voxel_short_sums<4>(pn8, vals, s, k, g, sum);
  static_assert(kVxShortMax == 4 * kVxGroup, "the widest tier covers the short kernel's longest segment");
  if (g == 0 && k) voxel_emit(o, k, sum, out_pts4, out_pn8);
}

__global__ __launch_bounds__(256) void k_voxel_reduce_long(const float4* __restrict__ pn8,
                                                           const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ seg,
                                                           const unsigned long long* __restrict__ pos,
                                                           const uint32_t* __restrict__ long_list, uint64_t nlong,
                                                           float4* __restrict__ out_pts4, float4* __restrict__ out_pn8) {
  const uint64_t w = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (w >= nlong) return;   // (a whole wavefront)
  const uint32_t v = long_list[w];
  const uint32_t s = seg[v], k = seg[v + 1] - s;
  double total[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t base = 0; base < k; base += kVxPiece) {
    float4 P[kVxStride], N[kVxStride];
#pragma unroll
    for (int t = 0; t < kVxStride; ++t) {
      const uint32_t e = base + 64u * t + lane;
      P[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      N[t] = P[t];
      if (e < k) {
        const size_t row = vals[s + e];
        P[t] = pn8[2 * row];
        N[t] = pn8[2 * row + 1];
      }
    }
    double a[6] = {(double)P[0].x, (double)P[0].y, (double)P[0].z, (double)N[0].x, (double)N[0].y, (double)N[0].z};
#pragma unroll
    for (int t = 1; t < kVxStride; ++t) {
      a[0] = a[0] + (double)P[t].x; a[1] = a[1] + (double)P[t].y; a[2] = a[2] + (double)P[t].z;
      a[3] = a[3] + (double)N[t].x; a[4] = a[4] + (double)N[t].y; a[5] = a[5] + (double)N[t].z;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double x = a[c];
      x = dpp_add<kDppRor8>(x);
      x = swizzle_xor16_add(x);
      x = x + __shfl_xor(x, 32);
      x = dpp_add<kDppXor1>(x);
      x = dpp_add<kDppXor2>(x);
      x = dpp_add<kDppHalfMirror>(x);
      total[c] = base == 0 ? x : total[c] + x;
    }
  }
  if (lane == 0) voxel_emit((uint32_t)pos[v], k, total, out_pts4, out_pn8);
}

// row_voxel through the permutation: sorted row i < m belongs to voxel vid1[i] - 1; the rest are Inf rows
__global__ void k_voxel_map(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ vid1,
                            const unsigned long long* __restrict__ kl, const unsigned long long* __restrict__ pos,
                            uint64_t n, uint64_t m, uint32_t* __restrict__ row_voxel) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t r = 0xFFFFFFFFu;
  if (i < m) {
    const uint32_t v = vid1[i] - 1;
    if (kl[v] & 1ull) r = (uint32_t)pos[v];
  }
  row_voxel[vals[i]] = r;
}

// ------------------------------------------------------------ host side ----
// Guards of both entry points; fills `o` with the options in force.
static pcd_status voxel_guards(const pcd_cloud* src, const pcd_voxel_options* opts, pcd_cloud** out,
                               pcd_voxel_options& o) {
  if (out) *out = nullptr;
  PCD_TRY(require_any_device());
  PCD_REQUIRE(src, "null cloud");
  PCD_REQUIRE(out, "out is null");
  if (opts) o = *opts; else pcd_voxel_options_default(&o);
  for (int d = 0; d < 3; ++d) PCD_REQUIRE(std::isfinite(o.leaf[d]) && o.leaf[d] > 0.f, "leaf must be finite and positive");
  PCD_REQUIRE(o.min_points >= 0, "min_points < 0");
  PCD_REQUIRE(o.cell_size >= 0 && std::isfinite(o.cell_size), "cell_size");
  PCD_TRY(require_device(src->device));
  return PCD_OK;
}

// the key space of the source's bounds at this leaf, or PCD_ERR_INVALID
static pcd_status voxel_params(const pcd_cloud* src, const pcd_voxel_options& o, VoxelParams& P, pcd_voxel_info& vi,
                               int* key_bits) {
  unsigned __int128 total = 1;
  unsigned long long d[3];
  for (int a = 0; a < 3; ++a) {
    const float inv = 1.0f / o.leaf[a];
    const float lo = src->bb_lo[a] * inv, hi = src->bb_hi[a] * inv;   // (no contraction: one float multiply each)
    if (!(std::fabs(lo) < 2147483648.0f) || !(std::fabs(hi) < 2147483648.0f)) {
      set_error("leaf %g on axis %d: voxel coordinates of the bounds [%g, %g] leave the int32 range", (double)o.leaf[a], a,
                (double)src->bb_lo[a], (double)src->bb_hi[a]);
      return PCD_ERR_INVALID;
    }
    const long long min_b = (long long)std::floor(lo), max_b = (long long)std::floor(hi);
    P.inv[a] = inv;
    P.min_b[a] = min_b;
    d[a] = (unsigned long long)(max_b - min_b + 1);
    total *= d[a];
    if (total >> 63) {
      set_error("leaf (%g, %g, %g): the voxel grid over the bounds has 2^63 voxels or more", (double)o.leaf[0],
                (double)o.leaf[1], (double)o.leaf[2]);
      return PCD_ERR_INVALID;
    }
    vi.min_b[a] = (int32_t)min_b;
    vi.dims[a] = (int32_t)std::min<unsigned long long>(d[a], 0x7FFFFFFFull);
  }
  P.d0 = d[0];
  P.d1 = d[1];
  P.inf_key = (unsigned long long)total;
  int bits = 1;
  while (bits < 64 && (P.inf_key >> bits)) ++bits;
  *key_bits = bits;
  return PCD_OK;
}

// The device passes on stream s.  d_row_voxel may be NULL.  c receives the new handle; it is complete only on PCD_OK.
static pcd_status voxel_device(pcd_cloud* src, const pcd_voxel_options& o, uint32_t* d_row_voxel, hipStream_t s,
                               CloudPtr& c, pcd_voxel_info* info) {
  pcd_voxel_info vi;
  std::memset(&vi, 0, sizeof vi);
  PCD_HIP_TRY(hipSetDevice(src->device));
  const uint64_t n = src->n, m = src->m;
  VoxelParams P{};
  int key_bits = 1;
  if (m) PCD_TRY(voxel_params(src, o, P, vi, &key_bits));

  EventPair ev;
  PCD_TRY(ev.create());
  (void)ev.start(s);

  // everything between the two events; returns with c allocated and its rows written (asynchronously)
  auto passes = [&]() -> pcd_status {
    if (m == 0) {
      if (d_row_voxel && n) PCD_HIP_TRY(hipMemsetAsync(d_row_voxel, 0xFF, n * sizeof(uint32_t), s));   // no row has a voxel
      return cloud_alloc_rows(src->device, 0, c);
    }
    // One allocation for the scratch of the call (a dozen hipMalloc / hipFree pairs cost more than the passes), so the
    // rocPRIM operations are bound here, before their arrays exist: a size query (storage == nullptr) reads no pointer
    unsigned long long *k0 = nullptr, *k1 = nullptr, *kl = nullptr, *pos = nullptr, *cnt = nullptr;
    uint32_t *v0 = nullptr, *v1 = nullptr, *flag = nullptr, *vid1 = nullptr, *seg = nullptr, *long_list = nullptr;
    auto sort = [&](void* t, size_t& b) { return sort_pairs_at(t, b, k0, k1, v0, v1, n, 0, key_bits, s); };
    auto scan_heads = [&](void* t, size_t& b) { return inclusive_sum_at(t, b, flag, vid1, m, s); };
    auto scan_keep = [&](void* t, size_t& b) { return exclusive_sum_at(t, b, kl, pos, 0ull, m + 1, s); };
    size_t tb = 0, tb1 = 0, tb2 = 0;   // temporary storage: the largest of the three
    PCD_HIP_TRY(sort(nullptr, tb));
    PCD_HIP_TRY(scan_heads(nullptr, tb1));
    PCD_HIP_TRY(scan_keep(nullptr, tb2));
    tb = std::max(tb, std::max(tb1, tb2));
    size_t bytes = 0;
    auto carve = [&](size_t count, size_t elem) { const size_t at = bytes; bytes += (count * elem + 255) & ~(size_t)255; return at; };
    const size_t o_k0 = carve(n, 8), o_k1 = carve(n, 8), o_kl = carve(m + 1, 8), o_pos = carve(m + 1, 8), o_cnt = carve(4, 8);
    const size_t o_v0 = carve(n, 4), o_v1 = carve(n, 4), o_flag = carve(m, 4), o_vid1 = carve(m, 4), o_seg = carve(m + 2, 4);
    const size_t o_long = carve(m / (kVxShortMax + 1) + 1, 4), o_tmp = carve(tb, 1);
    DevBuf<char> arena;
    PCD_TRY(arena.reserve(bytes));
    auto u64 = [&](size_t at) { return reinterpret_cast<unsigned long long*>(arena.p + at); };
    auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t*>(arena.p + at); };
    k0 = u64(o_k0); k1 = u64(o_k1); kl = u64(o_kl); pos = u64(o_pos); cnt = u64(o_cnt);
    v0 = u32(o_v0); v1 = u32(o_v1); flag = u32(o_flag); vid1 = u32(o_vid1); seg = u32(o_seg); long_list = u32(o_long);
    char* const tmp = arena.p + o_tmp;
    PCD_HIP_TRY(hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned long long), s));
    {
      ScopedKernelTimer tm("k_voxel_keys", s);
      hipLaunchKernelGGL(k_voxel_keys, dim3(div_up(n, 256)), dim3(256), 0, s, src->pn8.p, n, P, k0, v0);
    }
    {
      ScopedKernelTimer tm("voxel_sort", s);
      PCD_HIP_TRY(sort(tmp, tb));
    }
    unsigned long long hc[4] = {0, 0, 0, 0}, hpos = 0;
    {
      ScopedKernelTimer tm("voxel_heads", s);
      hipLaunchKernelGGL(k_voxel_heads, dim3(div_up(m, 256)), dim3(256), 0, s, k1, m, flag);
      PCD_HIP_TRY(scan_heads(tmp, tb));
      hipLaunchKernelGGL(k_voxel_segments, dim3(div_up(m, 256)), dim3(256), 0, s, flag, vid1, m, seg, cnt);
      hipLaunchKernelGGL(k_voxel_keep, dim3(div_up(m + 1, 256)), dim3(256), 0, s, seg, m, (uint32_t)o.min_points,
                         kl, cnt);
      PCD_HIP_TRY(scan_keep(tmp, tb));
      PCD_HIP_TRY(hipMemcpyAsync(hc, cnt, sizeof hc, hipMemcpyDeviceToHost, s));
      PCD_HIP_TRY(hipMemcpyAsync(&hpos, pos + m, sizeof hpos, hipMemcpyDeviceToHost, s));
    }
    PCD_HIP_TRY(hipStreamSynchronize(s));   // the row count sizes the new handle
    const uint64_t nv = hc[0], nout = hpos & 0xFFFFFFFFull, nlong = hpos >> 32;
    vi.num_voxels = nv;
    vi.num_output = nout;
    vi.num_dropped_rows = hc[1];
    vi.max_points_per_voxel = (uint32_t)hc[2];
    PCD_TRY(cloud_alloc_rows(src->device, nout, c));
    {
      ScopedKernelTimer tm("k_voxel_reduce", s);
      if (nlong) {
        hipLaunchKernelGGL(k_voxel_long_list, dim3(div_up(nv, 256)), dim3(256), 0, s, kl, pos, nv, long_list);
        hipLaunchKernelGGL(k_voxel_reduce_long, dim3(div_up(nlong * 64, 256)), dim3(256), 0, s, src->pn8.p, v1, seg,
                           pos, long_list, nlong, c->pts4.p, c->pn8.p);
      }
      if (nout > nlong)
        hipLaunchKernelGGL(k_voxel_reduce_short, dim3(div_up(nv * kVxGroup, 256)), dim3(256), 0, s, src->pn8.p, v1,
                           seg, kl, pos, nv, c->pts4.p, c->pn8.p);
    }
    if (d_row_voxel) {
      ScopedKernelTimer tm("k_voxel_map", s);
      hipLaunchKernelGGL(k_voxel_map, dim3(div_up(n, 256)), dim3(256), 0, s, v1, vid1, kl, pos, n, m, d_row_voxel);
    }
    PCD_HIP_TRY(hipGetLastError());
    PCD_HIP_TRY(hipStreamSynchronize(s));   // the scratch of this call goes out of scope
    return PCD_OK;
  };
  const pcd_status st = passes();
  float ms = 0.f;
  const hipError_t es = ev.stop_and_wait(s, &ms);
  PCD_TRY(st);
  if (es != hipSuccess) { set_error("voxel passes failed: %s", hipGetErrorString(es)); return PCD_ERR_HIP; }
  {
    ScopedKernelTimer tm("voxel_build", s);
    PCD_TRY(cloud_build_index(c.get(), o.cell_size, s));
  }
  vi.num_input = m;
  vi.ms = (double)ms;
  vi.build_ms = c->build_ms;
  if (info) *info = vi;
  return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" {

void pcd_voxel_options_default(pcd_voxel_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->leaf[0] = o->leaf[1] = o->leaf[2] = 0.05f;
}

pcd_status pcd_cloud_voxel_downsample_device(pcd_cloud* src, const pcd_voxel_options* opts, uint32_t* d_row_voxel,
                                             void* stream, pcd_cloud** out, pcd_voxel_info* info) {
  return pcd::guard([&]() -> pcd_status {
    pcd_voxel_options o;
    PCD_TRY(voxel_guards(src, opts, out, o));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_cloud_voxel_downsample_device"));
    PCD_TRY(require_whole_cloud(src, "voxel downsampling", "the voxels", "downsample"));
    CloudPtr c;
    PCD_TRY(voxel_device(src, o, d_row_voxel, (hipStream_t)stream, c, info));
    *out = c.release();
    return PCD_OK;
  });
}

pcd_status pcd_cloud_voxel_downsample(pcd_cloud* src, const pcd_voxel_options* opts, uint32_t* row_voxel,
                                      pcd_cloud** out, pcd_voxel_info* info) {
  return pcd::guard([&]() -> pcd_status {
    pcd_voxel_options o;
    PCD_TRY(voxel_guards(src, opts, out, o));
    PCD_TRY(require_whole_cloud(src, "voxel downsampling", "the voxels", "downsample"));
    PCD_HIP_TRY(hipSetDevice(src->device));
    DevBuf<uint32_t> d_map;
    const bool want = row_voxel && src->n;
    if (want) PCD_TRY(d_map.reserve(src->n));
    CloudPtr c;
    PCD_TRY(voxel_device(src, o, want ? d_map.p : nullptr, nullptr, c, info));
    if (want && hipMemcpy(row_voxel, d_map.p, src->n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("copy of row_voxel failed");
      return PCD_ERR_HIP;
    }
    *out = c.release();
    return PCD_OK;
  });
}

}  // extern "C"

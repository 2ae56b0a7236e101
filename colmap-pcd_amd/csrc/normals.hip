// normals.hip -- radius-PCA normal estimation over the cloud grid (pcd_cloud_estimate_normals*, definition in pcdhip.h).
//
// The brick kernel of the search (brick_kernel.h) with the roles swapped: a work item is one 64-query pass over a
// LEAF of the pyramid (2x2x2 cells = an x-range of two cells of ONE quad row, i.e. one contiguous range of the
// cell-sorted cloud).  The leaf's own points are the QUERIES, one per lane; the candidates are the leaf grown by R
// cells, R = floor((r (1 + 1e-5) + 2 slack) / h) + 1: a neighbour's float distance is <= r2, so its true distance is
// below r (1 + 1e-5), and both points sit at most `slack` outside their nominal cells (grid.slack, nn.hip), which puts
// the neighbour's cell at most R cells from the query's on every axis.  Rounded to whole quads in (y,z) that region is
// (1 + 2 ceil(R/2))^2 <= 121 quad rows (R <= 9 for r <= 8 h) with one contiguous x-range each.
//   * range table: lanes hold rows r and r + 64 (start in the concatenation of the UNPADDED ranges, source - start);
//     a slot finds its range with a 7-step binary search over those registers (ds_bpermute, no memory access: the
//     compiler has no reason to drain the DMAs in flight).  The 4-slot padding of the search kernels would stage
//     real neighbouring points twice, harmless for a minimum, wrong for a sum -- hence unpadded ranges;
//   * staging: 256-point tiles through LDS with global_load_lds_dwordx4, double-buffered under a counted
//     s_waitcnt vmcnt(4), per wavefront (no workgroup barrier in the pass loop).  A wavefront spends 24 VALU
//     instructions, 12 of them fp64, per staged point; the 16 bytes it stages per point come from L2 (neighbouring
//     passes stage the same rows), so sharing tiles between the wavefronts of a brick would save traffic that is two
//     orders of magnitude below the VALU time, and a leaf with one pass occupies one wavefront, not four;
//   * per pair: every lane reads the staged point at the SAME LDS address (a broadcast, no bank conflict) into
//     VGPRs -- never SGPR operands, which halve the VALU rate --, l2_simple3's 8 float operations + one
//     compare, then under the lane mask (differences selected to 0 outside: x + 0 = x exactly) the count, 3 first and
//     6 second moments in fp64.  The second moments use v_fma_f64: the product of two widened floats is exact in
//     double, so fma(d, d, s) IS round(s + d * d), bit for bit the separate multiply and add;
//   * epilogue per lane: covariance, cyclic Jacobi in fp64, the degenerate rules, orientation, stores through the
//     global row in sorted[].w; the info counters are block sums written per block and added up by one more launch
//     (integers: any order gives the same totals).
#include <cmath>

#include "cloud.h"
#include "grid.h"
#include "prim.h"
#include "scratch.h"

namespace pcd {

constexpr int kNrTile = 256;       // points per LDS tile buffer, two buffers per wavefront: 4 DMA instructions each
constexpr int kNrMaxReach = 9;     // cells: r <= 8 h plus the binning slack
constexpr int kNrFields = 8;       // per-block partial sums: estimated, too few, degenerate, kept, sum k, pair tests, max k, -

struct NormalsParams {
  float r2;
  int R, Rq;          // reach in cells / in quads
  int min_k;          // max(min_neighbors, 3)
  int orient, only_missing;
  float vp[3];
  int sdx, sdy, sdz;  // leaves per axis
};

__device__ __forceinline__ void nr_lds_dma16(const float4* gsrc, float4* lds_wave_base) {
  // LDS destination = wave-uniform base + lane * 16 (the hardware adds the lane offset)
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
typedef float nr_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t nr_lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
__device__ __forceinline__ unsigned long long nr_wave_add_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// point range of the leaf's own cells
__device__ __forceinline__ void nr_leaf_range(const GridParams& g, const uint32_t* __restrict__ cell_start, int sx,
                                              int sy, int sz, uint32_t& s, uint32_t& e) {
  const int cx0 = min(2 * sx, g.dims[0]), cx1 = min(cx0 + 2, g.dims[0]);
  const uint64_t rowbase = quad_row_base(g, sy, sz);
  s = cell_start[rowbase + 4 * (uint64_t)cx0];
  e = cell_start[rowbase + 4 * (uint64_t)cx1];
}

// 64-query passes of every leaf (entry nleaves = 0: the exclusive scan then ends with the total)
__global__ void k_normals_passes(GridParams g, const uint32_t* __restrict__ cell_start, int sdx, int sdy, int sdz,
                                 uint32_t* __restrict__ npass) {
  const uint64_t id = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t nleaves = (uint64_t)sdx * sdy * sdz;
  if (id > nleaves) return;
  uint32_t v = 0;
  if (id < nleaves) {
    uint32_t s, e;
    nr_leaf_range(g, cell_start, (int)(id % sdx), (int)((id / sdx) % sdy), (int)(id / ((uint64_t)sdx * sdy)), s, e);
    v = (e - s + 63u) >> 6;
  }
  npass[id] = v;
}

__global__ void k_normals_items(const uint32_t* __restrict__ npass, const uint32_t* __restrict__ off, uint64_t nleaves,
                                uint2* __restrict__ items) {
  const uint64_t id = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (id >= nleaves) return;
  const uint32_t n = npass[id], o = off[id];
  for (uint32_t p = 0; p < n; ++p) items[o + p] = make_uint2((uint32_t)id, p);
}

// rows that are not in the grid (an Inf coordinate): no neighbours, no normal
__global__ void k_normals_unindexed(const float4* __restrict__ pts4, uint64_t n, int only_missing, float4* pn8,
                                    uint32_t* __restrict__ d_count, double* __restrict__ d_curv) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts4[i];
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) return;
  if (d_count) d_count[i] = 0u;
  if (d_curv) d_curv[i] = 0.0;
  if (only_missing) {
    const float4 o = pn8[2 * i + 1];
    const double a = (double)o.x, b = (double)o.y, c = (double)o.z;
    if (sqrt(a * a + b * b + c * c) >= 1e-6) return;
  }
  pn8[2 * i + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// one Jacobi rotation of the pair (p,q) of a symmetric 3x3 (r = the third index) and of the eigenvector columns
#define PCD_NR_ROT2(X, Y)                    \
  {                                          \
    const double x_ = X, y_ = Y;             \
    X = x_ - sn * (y_ + tau * x_);           \
    Y = y_ + sn * (x_ - tau * y_);           \
  }
#define PCD_NR_JACOBI(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                      \
  if (apq != 0.0) {                                                                              \
    const double theta = (aqq - app) / (2.0 * apq);                                              \
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));    \
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs, tau = sn / (1.0 + cs);               \
    const double h_ = t * apq;                                                                   \
    app -= h_;                                                                                   \
    aqq += h_;                                                                                   \
    apq = 0.0;                                                                                   \
    PCD_NR_ROT2(arp, arq) PCD_NR_ROT2(v0p, v0q) PCD_NR_ROT2(v1p, v1q) PCD_NR_ROT2(v2p, v2q)      \
  }

struct NrMoments {
  uint32_t k;
  double sx, sy, sz, sxx, sxy, sxz, syy, syz, szz;
};

// one staged point against the lane's query
__device__ __forceinline__ void nr_accumulate(const nr_f32x4 p, float qx, float qy, float qz, float r2, NrMoments& m) {
  float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
  float d2 = dx * dx;
  d2 = d2 + dy * dy;
  d2 = d2 + dz * dz;
  const bool in = d2 <= r2;
  dx = in ? dx : 0.f;   // (a select, not a multiplication by 0 / 1: an overflowed difference must not become a NaN)
  dy = in ? dy : 0.f;
  dz = in ? dz : 0.f;
  m.k += in ? 1u : 0u;
  const double x = (double)dx, y = (double)dy, z = (double)dz;
  m.sx += x;
  m.sy += y;
  m.sz += z;
  m.sxx = __builtin_fma(x, x, m.sxx);
  m.sxy = __builtin_fma(x, y, m.sxy);
  m.sxz = __builtin_fma(x, z, m.sxz);
  m.syy = __builtin_fma(y, y, m.syy);
  m.syz = __builtin_fma(y, z, m.syz);
  m.szz = __builtin_fma(z, z, m.szz);
}

__global__ __launch_bounds__(256) void k_normals_brick(GridParams g, NormalsParams P, const float4* __restrict__ sorted,
                                                       const uint32_t* __restrict__ cell_start,
                                                       const uint2* __restrict__ items, uint32_t nitems, float4* pn8,
                                                       uint32_t* __restrict__ d_count, double* __restrict__ d_curv,
                                                       unsigned long long* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float4 s_tile[4][2][kNrTile];
  __shared__ unsigned long long s_part[4][kNrFields];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t item = blockIdx.x * 4u + (uint32_t)wave;
  unsigned long long st_est = 0, st_few = 0, st_deg = 0, st_kept = 0, st_k = 0, st_pairs = 0;
  uint32_t st_max = 0;

  if (item < nitems) {   // wave-uniform
    const uint2 it = items[item];
    const uint32_t leaf = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.x);
    const uint32_t pass = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.y);
    const int sx = (int)(leaf % (uint32_t)P.sdx), sy = (int)((leaf / (uint32_t)P.sdx) % (uint32_t)P.sdy),
              sz = (int)(leaf / ((uint32_t)P.sdx * (uint32_t)P.sdy));
    // ---- the lane's query ----
    uint32_t qs, qe;
    nr_leaf_range(g, cell_start, sx, sy, sz, qs, qe);
    const uint32_t q0 = qs + 64u * pass;            // < qe: the item exists
    const uint32_t nq = min(64u, qe - q0);
    const bool valid = (uint32_t)lane < nq;
    const float4 q = sorted[q0 + (valid ? (uint32_t)lane : nq - 1u)];

    // ---- range table: quad rows of the leaf grown by R cells, lanes hold rows `lane` and `lane + 64` ----
    const int cx0 = max(2 * sx - P.R, 0), cx1 = min(2 * sx + 2 + P.R, g.dims[0]);
    const int yq0 = max(sy - P.Rq, 0), yq1 = min(sy + P.Rq, g.qdims[0] - 1);
    const int zq0 = max(sz - P.Rq, 0), zq1 = min(sz + P.Rq, g.qdims[1] - 1);
    const int ny = yq1 - yq0 + 1, nrows = ny * (zq1 - zq0 + 1);   // <= 121
    uint32_t lenA = 0, lenB = 0, startA = 0, startB = 0;
    {
      const int ra = lane < nrows ? lane : nrows - 1;
      const uint64_t rb = quad_row_base(g, yq0 + ra % ny, zq0 + ra / ny);
      startA = cell_start[rb + 4 * (uint64_t)cx0];
      const uint32_t e = cell_start[rb + 4 * (uint64_t)cx1];
      lenA = lane < nrows ? e - startA : 0u;
    }
    if (nrows > 64) {   // wave-uniform
      const int r2nd = lane + 64 < nrows ? lane + 64 : nrows - 1;
      const uint64_t rb = quad_row_base(g, yq0 + r2nd % ny, zq0 + r2nd / ny);
      startB = cell_start[rb + 4 * (uint64_t)cx0];
      const uint32_t e = cell_start[rb + 4 * (uint64_t)cx1];
      lenB = lane + 64 < nrows ? e - startB : 0u;
    }
    const uint32_t incA = wave_scan_add_u32(lenA);
    const uint32_t TA = (uint32_t)__builtin_amdgcn_readlane((int)incA, 63);
    const uint32_t incB = wave_scan_add_u32(lenB);
    const uint32_t T = TA + (uint32_t)__builtin_amdgcn_readlane((int)incB, 63);   // >= nq: the leaf itself is inside
    const uint32_t offA = incA - lenA, offB = TA + incB - lenB;   // rows past the last: T, which no slot reaches
    const uint32_t deltaA = startA - offA, deltaB = startB - offB;
    const uint32_t offB0 = (uint32_t)__builtin_amdgcn_readlane((int)offB, 0);

    // source record of slot s < T: the last range that starts at or before s (empty ranges share their start with
    // the next one: the last one wins)
    auto slot_source = [&](uint32_t s) -> uint32_t {
      uint32_t r = offB0 <= s ? 64u : 0u;
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) {
        const uint32_t cand = r + (uint32_t)step;
        const uint32_t oa = (uint32_t)__shfl((int)offA, (int)(cand & 63u));
        const uint32_t ob = (uint32_t)__shfl((int)offB, (int)(cand & 63u));
        r = (cand >= 64u ? ob : oa) <= s ? cand : r;
      }
      const uint32_t da = (uint32_t)__shfl((int)deltaA, (int)(r & 63u));
      const uint32_t db = (uint32_t)__shfl((int)deltaB, (int)(r & 63u));
      return s + (r >= 64u ? db : da);
    };
    // the 4 DMAs of tile t (always 4 instructions, so that the wait below can count them: slots past T re-read the
    // last record into LDS slots the pass loop never reads)
    auto issue_tile = [&](int t) {
      float4* buf = s_tile[wave][t & 1];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t s = min((uint32_t)t * kNrTile + 64u * k + (uint32_t)lane, T - 1u);
        nr_lds_dma16(sorted + slot_source(s), buf + 64 * k);
      }
    };

    float r2v;   // in a VGPR: an SGPR operand would halve the rate of the compare
    asm volatile("v_mov_b32 %0, %1" : "=v"(r2v) : "s"(P.r2));
    NrMoments mo;
    mo.k = 0;
    mo.sx = mo.sy = mo.sz = mo.sxx = mo.sxy = mo.sxz = mo.syy = mo.syz = mo.szz = 0.0;
    const int ntiles = (int)((T + kNrTile - 1) / kNrTile);
    issue_tile(0);
    for (int t = 0; t < ntiles; ++t) {
      if (t + 1 < ntiles) {
        issue_tile(t + 1);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // tile t landed, the 4 DMAs of tile t + 1 still in flight
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_wave_barrier();
      const int cnt = (int)min((uint32_t)kNrTile, T - (uint32_t)t * kNrTile);
      const uint32_t base = nr_lds_addr(s_tile[wave][t & 1]);
      for (int j = 0; j < cnt; j += 4) {
        // inline asm: for an ordinary LDS load the compiler would first drain the DMAs of tile t + 1 (it cannot
        // tell the two buffers apart).  All lanes read the same address: a broadcast.
        nr_f32x4 p0, p1, p2, p3;
        const uint32_t rd = base + 16u * (uint32_t)j;
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\t"
                     "ds_read_b128 %2, %4 offset:32\n\tds_read_b128 %3, %4 offset:48\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3)
                     : "v"(rd)
                     : "memory");
        nr_accumulate(p0, q.x, q.y, q.z, r2v, mo);
        if (j + 1 < cnt) nr_accumulate(p1, q.x, q.y, q.z, r2v, mo);   // (wave-uniform tails)
        if (j + 2 < cnt) nr_accumulate(p2, q.x, q.y, q.z, r2v, mo);
        if (j + 3 < cnt) nr_accumulate(p3, q.x, q.y, q.z, r2v, mo);
      }
      // (the reads of this buffer have returned -- waited inside the asm block -- before tile t + 2's DMAs)
    }
    st_pairs = lane == 0 ? (unsigned long long)T * nq : 0ull;

    // ---- epilogue: covariance, eigen-solve, rules, orientation, stores ----
    if (valid) {
      const uint32_t gi = __float_as_uint(q.w);
      const uint32_t k = mo.k;
      double nx = 0.0, ny_ = 0.0, nz = 0.0, curv = 0.0;
      bool has = false;
      if (k < (uint32_t)P.min_k) {
        st_few = 1;
      } else {
        const double kk = (double)k;
        const double mx = mo.sx / kk, my = mo.sy / kk, mz = mo.sz / kk;
        double a00 = mo.sxx / kk - mx * mx, a01 = mo.sxy / kk - mx * my, a02 = mo.sxz / kk - mx * mz;
        double a11 = mo.syy / kk - my * my, a12 = mo.syz / kk - my * mz, a22 = mo.szz / kk - mz * mz;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
        for (int sweep = 0; sweep < 20; ++sweep) {
          const double off = fabs(a01) + fabs(a02) + fabs(a12);
          if (off == 0.0 || off <= 1e-26 * (fabs(a00) + fabs(a11) + fabs(a22))) break;
          PCD_NR_JACOBI(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
          PCD_NR_JACOBI(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
          PCD_NR_JACOBI(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
        }
        int i0 = 0;
        double l0 = a00;
        if (a11 < l0) { l0 = a11; i0 = 1; }
        if (a22 < l0) { l0 = a22; i0 = 2; }
        const double l2 = fmax(a00, fmax(a11, a22));
        const double l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
        if (l2 == 0.0 || l1 <= 1e-10 * l2) {
          st_deg = 1;
        } else {
          has = true;
          curv = l0 / ((l0 + l1) + l2);
          nx = i0 == 0 ? v00 : (i0 == 1 ? v01 : v02);
          ny_ = i0 == 0 ? v10 : (i0 == 1 ? v11 : v12);
          nz = i0 == 0 ? v20 : (i0 == 1 ? v21 : v22);
          const double inv = 1.0 / sqrt((nx * nx + ny_ * ny_) + nz * nz);
          nx *= inv; ny_ *= inv; nz *= inv;
          const double wx = (double)P.vp[0] - (double)q.x, wy = (double)P.vp[1] - (double)q.y,
                       wz = (double)P.vp[2] - (double)q.z;
          const double dot = (nx * wx + ny_ * wy) + nz * wz;
          bool flip;
          if (P.orient == PCD_NORMALS_ORIENT_VIEWPOINT && dot != 0.0) {
            flip = dot < 0.0;
          } else {
            double big = nx;
            if (fabs(ny_) > fabs(big)) big = ny_;
            if (fabs(nz) > fabs(big)) big = nz;
            flip = big < 0.0;
          }
          if (flip) { nx = -nx; ny_ = -ny_; nz = -nz; }
        }
      }
      bool keep = false;
      if (P.only_missing) {
        const float4 o = pn8[2 * (size_t)gi + 1];
        const double a = (double)o.x, b = (double)o.y, c = (double)o.z;
        keep = sqrt(a * a + b * b + c * c) >= 1e-6;
      }
      if (keep) {
        st_kept = 1; st_few = 0; st_deg = 0;
      } else {
        pn8[2 * (size_t)gi + 1] = make_float4((float)nx, (float)ny_, (float)nz, 0.f);
        st_est = has ? 1 : 0;
      }
      if (d_count) d_count[gi] = k;
      if (d_curv) d_curv[gi] = curv;
      st_k = k;
      st_max = k;
    }
  }

  // ---- block sums of the counters ----
  st_est = nr_wave_add_u64(st_est); st_few = nr_wave_add_u64(st_few); st_deg = nr_wave_add_u64(st_deg);
  st_kept = nr_wave_add_u64(st_kept); st_k = nr_wave_add_u64(st_k); st_pairs = nr_wave_add_u64(st_pairs);
  for (int off = 32; off > 0; off >>= 1) st_max = max(st_max, (uint32_t)__shfl_xor((int)st_max, off));
  if (lane == 0) {
    unsigned long long* o = s_part[wave];
    o[0] = st_est; o[1] = st_few; o[2] = st_deg; o[3] = st_kept; o[4] = st_k; o[5] = st_pairs; o[6] = st_max; o[7] = 0;
  }
  __syncthreads();
  if (threadIdx.x < kNrFields) {
    const int f = threadIdx.x;
    unsigned long long v = s_part[0][f];
    for (int w = 1; w < 4; ++w) v = f == 6 ? max(v, s_part[w][f]) : v + s_part[w][f];
    part[(size_t)blockIdx.x * kNrFields + f] = v;
  }
}

// totals of the per-block partials: out[f] = sum (f == 6: max) over the blocks
__global__ __launch_bounds__(256) void k_normals_totals(const unsigned long long* __restrict__ part, uint32_t nblocks,
                                                        unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_v[256][kNrFields];
  unsigned long long v[kNrFields];
  for (int f = 0; f < kNrFields; ++f) v[f] = 0;
  for (uint32_t b = threadIdx.x; b < nblocks; b += 256)
    for (int f = 0; f < kNrFields; ++f) {
      const unsigned long long x = part[(size_t)b * kNrFields + f];
      v[f] = f == 6 ? max(v[f], x) : v[f] + x;
    }
  for (int f = 0; f < kNrFields; ++f) s_v[threadIdx.x][f] = v[f];
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half)
      for (int f = 0; f < kNrFields; ++f) {
        const unsigned long long x = s_v[threadIdx.x + half][f];
        s_v[threadIdx.x][f] = f == 6 ? max(s_v[threadIdx.x][f], x) : s_v[threadIdx.x][f] + x;
      }
    __syncthreads();
  }
  if (threadIdx.x < kNrFields) out[threadIdx.x] = s_v[0][threadIdx.x];
}

// ------------------------------------------------------------ host side ----
// Guards of both entry points, in the order pcdhip.h lists them; fills `o` with the options in force.
static pcd_status normals_guards(const pcd_cloud* c, const pcd_normals_options* opts, pcd_normals_options& o) {
  PCD_TRY(require_any_device());
  PCD_REQUIRE(c, "null cloud");
  if (opts) o = *opts; else pcd_normals_options_default(&o);
  PCD_REQUIRE(std::isfinite(o.radius) && o.radius > 0.f, "radius must be finite and positive");
  PCD_REQUIRE(o.min_neighbors >= 0, "min_neighbors < 0");
  PCD_REQUIRE(o.orient == PCD_NORMALS_ORIENT_NONE || o.orient == PCD_NORMALS_ORIENT_VIEWPOINT, "unknown orient");
  PCD_REQUIRE(std::isfinite(o.viewpoint[0]) && std::isfinite(o.viewpoint[1]) && std::isfinite(o.viewpoint[2]),
              "viewpoint is not finite");
  PCD_TRY(require_device(c->device));
  if (o.radius > 8.0f * c->grid.h) {
    set_error("radius %g is %.3g cells of the handle's grid (cell_size %g); at most 8: create the handle with a "
              "larger cell_size", (double)o.radius, (double)o.radius / (double)c->grid.h, (double)c->grid.h);
    return PCD_ERR_INVALID;
  }
  return PCD_OK;
}

// totals land in sc->nr_part[0 .. kNrFields) (device); *have_totals = 0: nothing ran, all counters are 0
static pcd_status normals_device(pcd_cloud* c, const pcd_normals_options& o, uint32_t* d_count, double* d_curv,
                                 hipStream_t s, int* have_totals) {
  *have_totals = 0;
  if (c->n == 0) return PCD_OK;
  QueryScratch* sc = scratch_of(c);
  const GridParams& g = c->grid;
  // the reach is checked before the first launch: a refused call leaves the handle and the outputs as they were
  NormalsParams P;
  P.r2 = o.radius * o.radius;
  const double reach = (double)o.radius * (1.0 + 1e-5) + 2.0 * (double)g.slack;
  P.R = (int)std::floor(reach / (double)g.h) + 1;
  if (c->m != 0 && P.R > kNrMaxReach) {   // (radius <= 8 h was checked: only the slack could bring this about)
    set_error("radius %g reaches %d cells of %g", (double)o.radius, P.R, (double)g.h);
    return PCD_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(k_normals_unindexed, dim3(div_up(c->n, 256)), dim3(256), 0, s, c->pts4.p, c->n, o.only_missing,
                     c->pn8.p, d_count, d_curv);
  if (c->m == 0) {
    PCD_HIP_TRY(hipGetLastError());
    return PCD_OK;
  }
  P.Rq = (P.R + 1) / 2;
  P.min_k = std::max(o.min_neighbors, 3);
  P.orient = o.orient;
  P.only_missing = o.only_missing != 0;
  for (int d = 0; d < 3; ++d) P.vp[d] = o.viewpoint[d];
  P.sdx = (g.dims[0] + 1) / 2; P.sdy = g.qdims[0]; P.sdz = g.qdims[1];
  const uint64_t nleaves = (uint64_t)P.sdx * P.sdy * P.sdz;

  uint32_t nitems = 0;
  {
    ScopedKernelTimer tm("normals_items", s);
    PCD_TRY(sc->nr_pass.reserve(nleaves + 1));
    PCD_TRY(sc->nr_off.reserve(nleaves + 1));
    hipLaunchKernelGGL(k_normals_passes, dim3(div_up(nleaves + 1, 256)), dim3(256), 0, s, g, c->cell_start.p, P.sdx,
                       P.sdy, P.sdz, sc->nr_pass.p);
    PCD_TRY(exclusive_sum(sc->nr_tmp, sc->nr_pass.p, sc->nr_off.p, 0u, nleaves + 1, s));
    PCD_HIP_TRY(hipMemcpyAsync(&nitems, sc->nr_off.p + nleaves, sizeof nitems, hipMemcpyDeviceToHost, s));
    PCD_HIP_TRY(hipStreamSynchronize(s));
    PCD_TRY(sc->nr_items.reserve(nitems));
    hipLaunchKernelGGL(k_normals_items, dim3(div_up(nleaves, 256)), dim3(256), 0, s, sc->nr_pass.p, sc->nr_off.p,
                       nleaves, sc->nr_items.p);
  }
  const uint32_t nblocks = div_up(nitems, 4);
  PCD_TRY(sc->nr_part.reserve((size_t)kNrFields * ((size_t)nblocks + 1)));
  {
    ScopedKernelTimer tm("k_normals_brick", s);
    hipLaunchKernelGGL(k_normals_brick, dim3(nblocks), dim3(256), 0, s, g, P, c->sorted.p, c->cell_start.p,
                       sc->nr_items.p, nitems, c->pn8.p, d_count, d_curv, sc->nr_part.p + kNrFields);
  }
  hipLaunchKernelGGL(k_normals_totals, dim3(1), dim3(256), 0, s, sc->nr_part.p + kNrFields, nblocks, sc->nr_part.p);
  PCD_HIP_TRY(hipGetLastError());
  *have_totals = 1;
  return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" {

void pcd_normals_options_default(pcd_normals_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->radius = 0.15f;
  o->min_neighbors = 3;
  o->orient = PCD_NORMALS_ORIENT_VIEWPOINT;
}

pcd_status pcd_cloud_estimate_normals_device(pcd_cloud* c, const pcd_normals_options* opts, uint32_t* d_count,
                                             double* d_curvature, void* stream) {
  return pcd::guard([&]() -> pcd_status {
    pcd_normals_options o;
    PCD_TRY(normals_guards(c, opts, o));
    PCD_TRY(refuse_capture((hipStream_t)stream, "pcd_cloud_estimate_normals_device"));
    PCD_TRY(require_whole_cloud(c, "normal estimation", "the neighbourhoods", "estimate"));
    int have = 0;
    return normals_device(c, o, d_count, d_curvature, (hipStream_t)stream, &have);
  });
}

pcd_status pcd_cloud_estimate_normals(pcd_cloud* c, const pcd_normals_options* opts, uint32_t* count,
                                      double* curvature, pcd_normals_info* info) {
  return pcd::guard([&]() -> pcd_status {
    pcd_normals_options o;
    PCD_TRY(normals_guards(c, opts, o));
    PCD_TRY(require_whole_cloud(c, "normal estimation", "the neighbourhoods", "estimate"));
    if (info) std::memset(info, 0, sizeof *info);
    if (c->n == 0) return PCD_OK;
    QueryScratch* sc = scratch_of(c);
    hipStream_t s = nullptr;
    PCD_TRY(sc->nr_count.reserve(c->n));
    PCD_TRY(sc->nr_curv.reserve(c->n));
    EventPair ev;
    PCD_TRY(ev.create());
    (void)ev.start(s);
    int have = 0;
    const pcd_status st = normals_device(c, o, sc->nr_count.p, sc->nr_curv.p, s, &have);
    float ms = 0.f;
    const hipError_t es = ev.stop_and_wait(s, &ms);
    PCD_TRY(st);
    PCD_HIP_TRY(es);
    if (count) PCD_HIP_TRY(hipMemcpy(count, sc->nr_count.p, c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (curvature) PCD_HIP_TRY(hipMemcpy(curvature, sc->nr_curv.p, c->n * sizeof(double), hipMemcpyDeviceToHost));
    if (info) {
      unsigned long long t[kNrFields] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (have) PCD_HIP_TRY(hipMemcpy(t, sc->nr_part.p, sizeof t, hipMemcpyDeviceToHost));
      info->num_estimated = t[0];
      info->num_too_few = t[1];
      info->num_degenerate = t[2];
      info->num_kept = t[3];
      info->pair_tests = t[5];
      info->max_neighbors = (uint32_t)t[6];
      info->mean_neighbors = c->m ? (double)t[4] / (double)c->m : 0.0;
      info->ms = (double)ms;
    }
    return PCD_OK;
  });
}

}  // extern "C"

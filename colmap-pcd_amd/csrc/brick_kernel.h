// brick_kernel.h -- the machinery the brick kernels of the NN search share (included by nn.hip in front of
// brick_clip_kernel.h, whose k_nn_brick_clip is the first stage of the grid path).
//
// One wavefront per work item = (brick of 2x2x2 cells, <= 8 queries whose home cell lies in it).  The quad rows
// (grid.h: 2x2 cells in (y,z), contiguous along x) of the brick grown by 2 cells are contiguous ranges of the
// cell-sorted cloud -- 9 ranges; the part of their concatenation a kernel stages is streamed through two
// 256-point LDS tiles per wavefront.  What lives here:
//   * staging is LDS-DMA (global_load_lds_dwordx4: one 16-B record per lane, no VGPR round trip): lds_dma16,
//     lds_dma16_off;
//   * compare: lanes = staged points (ds_read_b128), the queries are wave-uniform (held in VGPRs: an SGPR operand
//     halves the VALU rate on gfx950), every point is tested against every query with FLANN's float arithmetic,
//     per-lane running minima of the packed (distance, index) keys (one v_min_f64 each): PCD_CMP_PAIR,
//     compare_point4 / compare_point2 / compare_query1, compare_tile;
//   * one transposed butterfly reduces all 8 per-lane minima at once (reduce-scatter over
//     xor 32/16/8, then xor 4/2/1), instead of 8 separate wavefront reductions: wave_min8_key;
//   * the build knobs, the timing-only ablation masks and the work item record (item_count, PCD_UNI).
// The kernel itself -- the tile loop, its counted waits, the software pipeline over the items, the region bound that
// decides whether a query is final -- is in brick_clip_kernel.h.
#pragma once
#include <type_traits>

namespace pcd {

// build-time knobs (tools/nn_tune.sh sweeps them): points per LDS tile buffer (two buffers per
// wavefront) and the wavefronts per SIMD the register allocator must leave room for
#ifndef PCD_KTILE
#define PCD_KTILE 256
#endif
#ifndef PCD_BRICK_MINWAVES
#define PCD_BRICK_MINWAVES 4
#endif
constexpr int kTile = PCD_KTILE;
constexpr int kFbChunk = 64;   // fallback-list slots a wavefront reserves per atomic (>= queries per item)
static_assert(kTile == 256, "a tile is 4 DMA instructions (128/192-point tiles were measured slower and removed)");
// timing-only ablations (results are then wrong): compiled in only with -DPCD_ABLATE (tools/nn_ablate.py builds
// such a variant); in the shipped library the masks are 0 and every `flags & kAblate*` folds away.
#ifdef PCD_ABLATE
constexpr int kAblateCompare = 0x100, kAblateReduce = 0x400, kAblateFallback = 0x800, kAblateTiles = 0x1000,
              kAblateNoDma = 0x4000, kAblateNoLdsRead = 0x8000;
#else
constexpr int kAblateCompare = 0, kAblateReduce = 0, kAblateFallback = 0, kAblateTiles = 0, kAblateNoDma = 0,
              kAblateNoLdsRead = 0;
#endif

__device__ __forceinline__ void lds_dma16(const float4* gsrc, float4* lds_wave_base) {
  // LDS destination = wave-uniform base + lane * 16 (hardware adds the lane offset)
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// the same with a compile-time byte offset on the source address (instruction k of a 4-slot group).  The
// instruction offset is added to the LDS address as well as to the source address (LDS address = M0 base +
// instruction offset + lane * 16): callers take it off the base again.
template <int OFF>
__device__ __forceinline__ void lds_dma16_off(const float4* gsrc, float4* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, OFF, 0);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return b < a ? b : a; }

// All-lanes minimum of 8 per-lane packed keys at once (the keys as f64, see compare_point: v_min_f64 on them
// is the lexicographic (distance, index) minimum; none of them is a NaN pattern here).  Returns, in every lane,
// the minimum of value index ((lane>>5)&1)*4 + ((lane>>4)&1)*2 + ((lane>>3)&1).
// A reduce-scatter: each stage halves the number of values a lane still carries.  The first two stages are the
// gfx950 lane-swap instructions: v_permlane32_swap exchanges lanes 32..63 of one register with lanes 0..31 of
// another, so after swapping the registers of values i and 4+i the lane-wise minimum of the pair IS "value i over
// both halves" in lanes 0..31 and "value 4+i over both halves" in lanes 32..63 -- 2 swaps + 1 v_min_f64 per pair
// where select + ds_bpermute + 64-bit compare/select took 13 instructions; v_permlane16_swap does the same for
// the 16-lane rows.  The remaining 8-lane groups are folded with DPP moves (row_ror:8 with a select, then
// row_half_mirror, quad_perm xor 2, quad_perm xor 1).
__device__ __forceinline__ double min_key_f64(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_update_dpp(0u, (uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = __builtin_amdgcn_update_dpp(0u, (uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
template <int ROW>  // 32 or 16: min over the swapped pair (x keeps the even rows' value, y the odd rows')
__device__ __forceinline__ double swap_min_f64(double x, double y) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  const uint64_t ux = __builtin_bit_cast(uint64_t, x), uy = __builtin_bit_cast(uint64_t, y);
  u32x2 lo, hi;
  if (ROW == 32) {
    lo = __builtin_amdgcn_permlane32_swap((uint32_t)ux, (uint32_t)uy, false, false);
    hi = __builtin_amdgcn_permlane32_swap((uint32_t)(ux >> 32), (uint32_t)(uy >> 32), false, false);
  } else {
    lo = __builtin_amdgcn_permlane16_swap((uint32_t)ux, (uint32_t)uy, false, false);
    hi = __builtin_amdgcn_permlane16_swap((uint32_t)(ux >> 32), (uint32_t)(uy >> 32), false, false);
  }
  return min_key_f64(__builtin_bit_cast(double, ((uint64_t)hi.x << 32) | lo.x),
                     __builtin_bit_cast(double, ((uint64_t)hi.y << 32) | lo.y));
}
__device__ __forceinline__ double wave_min8_key(const double (&v)[8]) {
  const int lane = threadIdx.x & 63;
  double a[4], b2[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = swap_min_f64<32>(v[i], v[4 + i]);   // lanes 0..31: value i, 32..63: value 4+i
#pragma unroll
  for (int i = 0; i < 2; ++i) b2[i] = swap_min_f64<16>(a[i], a[2 + i]);  // even rows: a[i], odd rows: a[2+i]
  const bool up = lane & 8;
  const double keep = up ? b2[1] : b2[0], send = up ? b2[0] : b2[1];
  double c = min_key_f64(keep, dpp_f64<0x128>(send));   // row_ror:8 = lane ^ 8 inside a row of 16
  c = min_key_f64(c, dpp_f64<0x141>(c));                // row_half_mirror: lane <- 7 - lane inside each 8
  c = min_key_f64(c, dpp_f64<0x4E>(c));                 // quad_perm [2,3,0,1]
  c = min_key_f64(c, dpp_f64<0xB1>(c));                 // quad_perm [1,0,3,2]
  return c;
}

// One staged point against NQ wave-uniform queries: 8 scalar f32 ops (FLANN's ((dx*dx) + dy*dy) + dz*dz, no FMA)
// + ONE v_min_f64 on the packed (distance, index) key per query.  The key float_bits(d) << 32 | index of a
// non-negative, non-NaN float d is a positive finite (or denormal: d == 0) double whose numeric order is the
// unsigned order of its bits, so the f64 minimum is exactly the lexicographic (distance, index) minimum that
// v_cmp_lt_u64 + 2 v_cndmask computed before -- in one half-rate instruction instead of three (measured on
// gfx950, tools/ubench/valu_rate.hip: v_cmp_lt_u64 4.2, v_min_f64 4.2, v_mul/v_fma_f32 2.4 cycles per wave64
// instruction).  Inline asm: llvm's fmin would canonicalise both operands first (IEEE mode), two more f64 ops.
// f64 denormals are never flushed on gfx9 compute kernels (only the f32 mode is configurable).
// Measured alternatives that did NOT help: packed v_pk_add/mul_f32 (half rate on gfx950), 32-bit lexicographic
// compares instead of the 64-bit one, more wavefronts per SIMD (5, 6, 8: within 3 %).
// Hand-scheduled form.  hipcc builds each 64-bit key with an extra v_mov (the index into the low half of a fresh
// register pair) and folds the wave-uniform queries into the subtractions as SGPR operands, which run at HALF rate
// on gfx950 (tools/ubench/valu_rate2.hip: v_sub_f32 v,v 1.03 ns, s,v 1.75 ns per wave64 instruction); so the
// queries are copied to VGPRs once per item and one staged point is compared with 4 queries per asm block:
// per (point, query) pair 3 v_sub + 3 v_mul + 2 v_add + 1 v_min_f64 = 9 VALU instructions, plus one v_mov per
// block that parks the point's index in the low half of the key pair v[120:121]; the last v_add writes the
// distance straight into its high half.  Two queries are interleaved so that no instruction waits for its
// predecessor.  Same IEEE operations in the same order as l2_simple3 (grid.h): results are bit-identical.
// v118..v127 are scratch of the block (clobbers): the kernel stays within 128 VGPRs = 4 wavefronts per SIMD.
#define PCD_CMP_PAIR(A, B)                                                                         \
  "v_sub_f32 v122, %[qx" #A "], %[px]\n\tv_sub_f32 v125, %[qx" #B "], %[px]\n\t"                       \
  "v_sub_f32 v123, %[qy" #A "], %[py]\n\tv_sub_f32 v126, %[qy" #B "], %[py]\n\t"                       \
  "v_sub_f32 v124, %[qz" #A "], %[pz]\n\tv_sub_f32 v127, %[qz" #B "], %[pz]\n\t"                       \
  "v_mul_f32 v122, v122, v122\n\tv_mul_f32 v125, v125, v125\n\t"                                     \
  "v_mul_f32 v123, v123, v123\n\tv_mul_f32 v126, v126, v126\n\t"                                     \
  "v_mul_f32 v124, v124, v124\n\tv_mul_f32 v127, v127, v127\n\t"                                     \
  "v_add_f32 v122, v122, v123\n\tv_add_f32 v125, v125, v126\n\t"                                     \
  "v_add_f32 v121, v122, v124\n\tv_add_f32 v119, v125, v127\n\t"                                     \
  "v_min_f64 %[b" #A "], %[b" #A "], v[120:121]\n\tv_min_f64 %[b" #B "], %[b" #B "], v[118:119]\n\t"

// one staged point against queries Q0..Q0+3 (whose coordinates are in VGPRs)
__device__ __forceinline__ void compare_point4(const f32x4 p, const float* qx, const float* qy, const float* qz,
                                               double* best) {
  asm("v_mov_b32 v120, %[pw]\n\tv_mov_b32 v118, %[pw]\n\t"
      PCD_CMP_PAIR(0, 1) PCD_CMP_PAIR(2, 3)
      : [b0] "+v"(best[0]), [b1] "+v"(best[1]), [b2] "+v"(best[2]), [b3] "+v"(best[3])
      : [px] "v"(p.x), [py] "v"(p.y), [pz] "v"(p.z), [pw] "v"(p.w),
        [qx0] "v"(qx[0]), [qy0] "v"(qy[0]), [qz0] "v"(qz[0]), [qx1] "v"(qx[1]), [qy1] "v"(qy[1]), [qz1] "v"(qz[1]),
        [qx2] "v"(qx[2]), [qy2] "v"(qy[2]), [qz2] "v"(qz[2]), [qx3] "v"(qx[3]), [qy3] "v"(qy[3]), [qz3] "v"(qz[3])
      : "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
}
__device__ __forceinline__ void compare_point2(const f32x4 p, const float* qx, const float* qy, const float* qz,
                                               double* best) {
  asm("v_mov_b32 v120, %[pw]\n\tv_mov_b32 v118, %[pw]\n\t"
      PCD_CMP_PAIR(0, 1)
      : [b0] "+v"(best[0]), [b1] "+v"(best[1])
      : [px] "v"(p.x), [py] "v"(p.y), [pz] "v"(p.z), [pw] "v"(p.w),
        [qx0] "v"(qx[0]), [qy0] "v"(qy[0]), [qz0] "v"(qz[0]), [qx1] "v"(qx[1]), [qy1] "v"(qy[1]), [qz1] "v"(qz[1])
      : "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
}

// ONE query against TWO staged points (the odd query of a group): the two points' chains interleave the way the two
// queries of PCD_CMP_PAIR do.
__device__ __forceinline__ void compare_query1(const f32x4 pa, const f32x4 pb, const float qx, const float qy,
                                               const float qz, double& best) {
  asm("v_mov_b32 v120, %[aw]\n\tv_mov_b32 v118, %[bw]\n\t"
      "v_sub_f32 v122, %[qx], %[ax]\n\tv_sub_f32 v125, %[qx], %[bx]\n\t"
      "v_sub_f32 v123, %[qy], %[ay]\n\tv_sub_f32 v126, %[qy], %[by]\n\t"
      "v_sub_f32 v124, %[qz], %[az]\n\tv_sub_f32 v127, %[qz], %[bz]\n\t"
      "v_mul_f32 v122, v122, v122\n\tv_mul_f32 v125, v125, v125\n\t"
      "v_mul_f32 v123, v123, v123\n\tv_mul_f32 v126, v126, v126\n\t"
      "v_mul_f32 v124, v124, v124\n\tv_mul_f32 v127, v127, v127\n\t"
      "v_add_f32 v122, v122, v123\n\tv_add_f32 v125, v125, v126\n\t"
      "v_add_f32 v121, v122, v124\n\tv_add_f32 v119, v125, v127\n\t"
      "v_min_f64 %[b], %[b], v[120:121]\n\tv_min_f64 %[b], %[b], v[118:119]\n\t"
      : [b] "+v"(best)
      : [ax] "v"(pa.x), [ay] "v"(pa.y), [az] "v"(pa.z), [aw] "v"(pa.w), [bx] "v"(pb.x), [by] "v"(pb.y), [bz] "v"(pb.z),
        [bw] "v"(pb.w), [qx] "v"(qx), [qy] "v"(qy), [qz] "v"(qz)
      : "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
}

// the lane's 4 staged points of a tile against the first NQ queries of the group: pairs of queries per point, the
// odd query (if any) against pairs of points -- exactly NQ compares per point, no padded query slots
template <int NQ>
__device__ __forceinline__ void compare_tile(const f32x4 (&p)[4], const float (&qx)[8], const float (&qy)[8],
                                             const float (&qz)[8], double (&best)[8]) {
  static_assert(NQ >= 1 && NQ <= 8, "1..8 queries per group");
  constexpr int E = NQ & ~1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (E >= 4) compare_point4(p[k], qx, qy, qz, best);
    if (E == 8) compare_point4(p[k], qx + 4, qy + 4, qz + 4, best + 4);
    if (E == 2 || E == 6) compare_point2(p[k], qx + (E - 2), qy + (E - 2), qz + (E - 2), best + (E - 2));
  }
  if (NQ & 1) {
    compare_query1(p[0], p[1], qx[NQ - 1], qy[NQ - 1], qz[NQ - 1], best[NQ - 1]);
    compare_query1(p[2], p[3], qx[NQ - 1], qy[NQ - 1], qz[NQ - 1], best[NQ - 1]);
  }
}

// item record: {first query, brick x, brick y, brick z | count << 28}
__device__ __forceinline__ int item_count(const uint4 it) { return (int)(it.w >> 28); }
// item records are read through uniform (scalar) indices: they land in SGPRs instead of 12 VGPRs
#define PCD_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))

}  // namespace pcd

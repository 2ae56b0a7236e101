// sift.hip -- exact brute-force SIFT descriptor matching on the matrix cores.
//
// Replaces feature/sift.cc:171-204 (ComputeSiftDistanceMatrix: int32 dot products of uint8 x 128
// descriptors), :55-107 (FindBestMatchesOneWayBruteForce: best / second best per row, acos + distance
// and ratio tests) and :109-144 (FindBestMatchesBruteForce: cross check) -- the exact specification that
// SiftGPU's MultiplyDescriptor / RowMatch / ColMatch kernels (lib/SiftGPU/ProgramCU.cu:1408-1795) and the
// CPU brute-force matcher implement.  This is the one dense contraction of the path, hence MFMA:
//
//   S[i][j] = sum_k a[i][k] b[j][k]   (uint8 inputs, exact int32)
//           = sum_k (a-128)(b-128) + 128 (sum_k a[i][k] + sum_k b[j][k]) - 128*128*128
// so the bytes are re-centred to int8 (a ^ 0x80) and fed to v_mfma_i32_32x32x32_i8 (K = 32 per
// instruction, int32 accumulate: exact), the row-sum correction is added in the epilogue.
//
// Scores kernels (k_sift_scores_stripe / k_sift_scores_batch, guided: k_sift_guided_stripe / k_sift_guided_batch, all
// around sift_rows below): a persistent row-stripe walk of ONE direction -- lane = row of the row set, so a row's running
// (best, second, argbest) is three registers that live for the whole walk.  The other direction (best row per column)
// is the same walk with the two sets exchanged: every tile is multiplied twice, nothing else is done twice.
// Per column chunk and row one int4 {best, second, arg, 0} with true scores goes to a partial buffer (part12 / part21);
// k_sift_finalize merges the chunks' partials in ascending order (ties -> first index, as the reference's ascending
// strict-> scan), applies acos / max_distance / max_ratio; the cross check and the ordered compaction follow.
// Guided matching (H / F filter): per keypoint and pair one record of six floats (k_sift_guide_prep); the walk stages the
// column records beside the descriptors and leaves a rejected pair out of the row's top-2.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "prim.h"

namespace pcd {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// test / fuzzing knobs (pcd_sift_set_tuning; 0 = the library's choice): column chunks per stripe walk, partial results
// per sub-batch in int4 elements (16-byte units).  Atomics read once per call: no environment lookups on the call path.
static std::atomic<int> g_sift_nchunk{0};
static std::atomic<uint64_t> g_sift_batch_partials{0};

constexpr int kSiftTile = 128;
constexpr int kSiftConst = 128 * 128 * 128;
#ifndef PCD_SIFT_WGS
#define PCD_SIFT_WGS 2
#endif
#ifndef PCD_SIFT_ABLATE   // timing-only variants (tools/sift_ablate.sh; results are wrong): 1 no scan, 2 no slow path,
#define PCD_SIFT_ABLATE 0 // 4 no fetch / store of further tiles, 8 no barrier, 16 no MFMA
#endif

// ---- preparation: the re-centred, padded copy the walks read ------------------------------------------------------
// Every image (descriptor set) is copied ONCE per call into scratch with its bytes re-centred (x ^ 0x80) and its rows
// padded with zero descriptors to a multiple of 128, next to one constant per row: cc = 128 sum(row) - 128^3 (a padding
// row: -128^3, i.e. true score 0 against anything).  The walks then stage column tiles with LDS-DMA (no registers, no
// VALU, no bounds tests) and read their row fragments unconditionally.
struct SiftImageDev {
  const uint8_t* src;   // the image's descriptors (n x 128 bytes)
  uint32_t n;           // descriptors
  uint32_t prow;        // first row of the image in the padded copy (a multiple of 128)
};

// one workgroup per 128-row tile: thread (row = tid >> 1, half = tid & 1) moves 64 bytes
__device__ __forceinline__ void sift_prep_tile(const SiftImageDev im, int tile, uint8_t* __restrict__ xa,
                                               int* __restrict__ cc) {
  const uint32_t row = (uint32_t)tile * kSiftTile + (threadIdx.x >> 1), h = threadIdx.x & 1;
  if ((uint32_t)tile * kSiftTile >= im.n) return;   // (the grid is sized for the largest image; an empty one has no tiles)
  uint4 v[4];
  unsigned s = 0;
  if (row < im.n) {
    const uint4* p = reinterpret_cast<const uint4*>(im.src + (size_t)row * 128 + h * 64);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = p[c];
      const unsigned w[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) s += (w[k] & 0xFF) + ((w[k] >> 8) & 0xFF) + ((w[k] >> 16) & 0xFF) + (w[k] >> 24);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = make_uint4(0, 0, 0, 0);
  }
  s += __shfl_xor(s, 1);
  uint4* q = reinterpret_cast<uint4*>(xa + (size_t)(im.prow + row) * 128 + h * 64);
#pragma unroll
  for (int c = 0; c < 4; ++c)
    q[c] = make_uint4(v[c].x ^ 0x80808080u, v[c].y ^ 0x80808080u, v[c].z ^ 0x80808080u, v[c].w ^ 0x80808080u);
  if (h == 0) cc[im.prow + row] = 128 * (int)s - kSiftConst;
}

__global__ __launch_bounds__(256) void k_sift_prep_pair(SiftImageDev a, SiftImageDev b, uint8_t* __restrict__ xa,
                                                        int* __restrict__ cc) {
  sift_prep_tile(blockIdx.y == 0 ? a : b, blockIdx.x, xa, cc);
}
__global__ __launch_bounds__(256) void k_sift_prep_images(const SiftImageDev* __restrict__ images,
                                                          uint8_t* __restrict__ xa, int* __restrict__ cc) {
  sift_prep_tile(images[blockIdx.y], blockIdx.x, xa, cc);
}

// running (best, second, argbest) with the reference's update rule: strictly greater replaces the best
__device__ __forceinline__ void top2_update(int v, int idx, int& best, int& second, int& arg) {
  second = max(second, min(v, best));
  const bool gt = v > best;
  arg = gt ? idx : arg;
  best = max(best, v);
}
// merge another triple; on equal best the lower index wins (= first in an ascending scan)
__device__ __forceinline__ void top2_merge(int b2, int s2, int a2, int& best, int& second, int& arg) {
  const int nsecond = max(max(second, s2), min(best, b2));
  const bool take = (b2 > best) || (b2 == best && (unsigned)a2 < (unsigned)arg);
  arg = take ? a2 : arg;
  best = max(best, b2);
  second = nsecond;
}

// ---- persistent row-stripe walk, ONE direction per walk, lane = row (round 4) -------------------------------------
// Workgroup (by, chunk) owns the 512-row stripe `by` of the ROW set and walks `ct` 128-descriptor tiles of the COLUMN
// set.  Tiles are staged with LDS-DMA from the prepared copy (k_sift_prep_*), double-buffered, one barrier per tile; a
// wavefront owns 128 rows and every 32-column block of a tile: 16 MFMAs per block, in two halves of 2 row tiles x 4
// k-steps into TWO accumulator sets -- one half is multiplied while the other is scanned.
//
// The product is taken TRANSPOSED, D = B A^T (the staged column fragment is the MFMA's first operand), so that in the
// result layout a LANE is a ROW of the row set (lane & 31; the two lane halves hold columns 4 apart) and a REGISTER is a
// column of the block.  The row's running (best, second, argbest) is then three registers per lane and row tile that live
// for the whole walk, and a register of scores concerns them only if SOME lane's score beats its row's running second
// best: one v_cmp (eight issued back to back into SGPR pairs) + one scalar test per 64 scores, the fast path the
// fall-through.  With k columns seen the chance that a given row's pair changes is 2 / k, so after the first tiles almost
// every register takes the fast path.  Round 3 kept both directions' top-2 up to date for every score of ONE product
// (6 half-rate VALU per score against 8 MFMAs per 64 x 32 block: 0.17 of the dense i8 peak, bound by the scan); here the
// other direction (best row per column) is the same walk with the two sets exchanged: every tile is multiplied twice,
// as in rounds 1-2, but nothing else is done twice and a walk costs little more than its MFMAs.
//   * 512 rows per stripe: a staged tile (16 KB) feeds 256 MFMAs -- at 128 rows per stripe the walks of one 50-image
//     block pulled 157 GB through L2 (6 TB/s at the speed reached: the bound); LDS reads per block: 4 KB of column
//     fragments + 4 KB of constants for 16 MFMAs;
//   * the row set's fragments of the wavefront's 128 rows stay in registers for the whole walk (64 VGPRs);
//   * the first MFMA of a chain takes the COLUMN constants 128 sum(col) - 128^3 as its C operand (16 registers read from
//     LDS once per block, 4 consecutive columns per 16-byte read: no VALU); the row constant 128 sum(row) is one register
//     per lane and row tile and never added inside the walk -- the running values are kept relative to it;
//   * the staged tile is swizzled (16-byte chunk q of row r at position q ^ (r & 7): the DMA's lane -> source mapping
//     does it) so that the fragment reads of 32 rows at one k-chunk spread over all banks;
//   * the slow path (some lane beats its second best) is six VALU on the whole register, harmless for the lanes that do
//     not: arg <- (v > best ? code : arg), second <- med3(best, second, v), best <- max(best, v); code = 16 x column
//     block sequence number + register, wave-uniform; the column index is decoded once at the end of the walk.  The
//     masks of later registers of a group of eight are taken against the second best as it was before the earlier ones
//     were absorbed: a superset of the lanes that still beat it;
//   * strict "greater" in ascending column order inside a lane = the reference's rule (sift.cc:72-83: the first of equal
//     scores keeps the best place); the lane halves and the chunks are merged with top2_merge (equal best: lower index).
// part [nchunk][n1] int4 {best, second, arg, 0} with true scores.
constexpr int kSiftWaveRows = 64;            // rows of a wavefront (2 MFMA row tiles)
constexpr int kSiftWaves = 8;                         // wavefronts of a workgroup
constexpr int kSiftStripe = kSiftWaves * kSiftWaveRows;   // rows of a stripe (workgroup)

template <int OFF>
__device__ __forceinline__ void sift_dma16(const uint8_t* gsrc, uint8_t* lds_wave_base) {
  // LDS destination = wave-uniform base + OFF + lane * 16; source = gsrc + OFF (the offset counts on both sides)
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, OFF, 0);
}
__device__ __forceinline__ void sift_dma4(const int* gsrc, int* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}
__device__ __forceinline__ uint32_t sift_lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

struct SiftFrag { v4i fb[4], cq[4]; };   // one column block: 4 k-chunks of the staged descriptors, 16 column constants
template <int BLK>
__device__ __forceinline__ void sift_read_frag(SiftFrag& f, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t cc_a) {
  asm volatile("ds_read_b128 %0, %8 offset:%c12\n\tds_read_b128 %1, %9 offset:%c12\n\t"
               "ds_read_b128 %4, %13 offset:%c14\n\tds_read_b128 %5, %13 offset:%c15\n\t"
               "ds_read_b128 %2, %10 offset:%c12\n\tds_read_b128 %3, %11 offset:%c12\n\t"
               "ds_read_b128 %6, %13 offset:%c16\n\tds_read_b128 %7, %13 offset:%c17"
               : "=&v"(f.fb[0]), "=&v"(f.fb[1]), "=&v"(f.fb[2]), "=&v"(f.fb[3]), "=&v"(f.cq[0]), "=&v"(f.cq[1]), "=&v"(f.cq[2]), "=&v"(f.cq[3])
               : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "n"(BLK * 4096), "v"(cc_a), "n"(BLK * 128), "n"(BLK * 128 + 32),
                 "n"(BLK * 128 + 64), "n"(BLK * 128 + 96)
               : "memory");
}

// ---- guided matching (feature/sift.cc:1092-1162 MatchGuidedSiftFeaturesCPU): the filter inside the walk ------------
// Per keypoint and pair one record of kSiftRecComps floats, built by k_sift_guide_prep in tile-major SoA layout
// (record of row r of a side: rec[(r >> 7) * kSiftRecTile + comp * 128 + (r & 127)]), so a column tile's records are
// one contiguous kSiftRecTile block that LDS-DMA stages next to the descriptors.
//   set 1: {a0, a1, a2, a0*a0 + a1*a1, h0/h2, h1/h2}   a_i = (F[i][0] x1 + F[i][1] y1) + F[i][2], h_i likewise with H
//   set 2: {x2, y2, b0*b0, b1*b1, x2, y2}               b_j = (F[0][j] x2 + F[1][j] y2) + F[2][j]
// The per-pair remainder, in the order of the reference's float Eigen code (every operation one IEEE float op; the
// library is built with -ffp-contract=off):
//   H: d0 = h0/h2 - x2, d1 = h1/h2 - y2, rejected iff d0*d0 + d1*d1 > h_max_residual
//   F: e = (x2*a0 + y2*a1) + a2, rejected iff (e*e) / (((a0*a0 + a1*a1) + b0*b0) + b1*b1) > f_max_residual
// A rejected pair's score is 0 (sift.cc:193-196), and a 0 never becomes a best or second best of the strict-> scan:
// rejecting = leaving the column out of the row's top-2.  The walk folds that into the register test:
// ballot(score > thr && passes).  (A NaN residual passes, as NaN > t is false in the reference.)
enum { kSiftGuideH = 1, kSiftGuideF = 2 };
constexpr int kSiftRecComps = 6;
constexpr int kSiftRecTile = kSiftRecComps * kSiftTile;   // floats per 128-row tile of records

struct SiftGuidePairDev {
  const float* loc1;   // [n1][2] locations of set 1 / set 2 (device)
  const float* loc2;
  uint32_t n1, n2;
  uint64_t rec1, rec2; // float offsets of the two sides' records
  int32_t mode;        // kSiftGuideH | kSiftGuideF (0: no filter)
  float H[9], F[9];    // row-major
};

// what a walk needs: its row side's and column side's records (first row of each image), which of them is set 1
struct SiftGuideWalk {
  const float* rrec;
  const float* crec;
  int mode;
  bool rows_set1;
  float th, tf;
};

// LDS of the guided walk's staged column records (double-buffered, one kSiftRecTile block per tile)
__device__ __forceinline__ float* sift_guide_lds() {
  __shared__ __attribute__((aligned(16))) float sG[2][kSiftRecTile];
  return &sG[0][0];
}

// comps 0 .. N - 1 (counted from the one at byte offset OFF) of the lane's 4 consecutive columns
template <int OFF, int N>
__device__ __forceinline__ void sift_read_rec(float4 (&r)[N], uint32_t a) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f t[N];
#pragma unroll
  for (int c = 0; c < N; ++c)
    asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(t[c]) : "v"(a), "n"(OFF + c * kSiftTile * 4) : "memory");
  // the reads have landed (tied to the registers, as in sift_read_frag)
  if constexpr (N == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]) :: "memory");
  else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]) :: "memory");
#pragma unroll
  for (int c = 0; c < N; ++c) r[c] = make_float4(t[c][0], t[c][1], t[c][2], t[c][3]);
}

// xr / ccr: the row image in the prepared copy (its first row) and its constants; xc / ccc: the column image
// GUIDED: the walk of the guided kernels (gw: its records and thresholds); the unguided instantiation ignores gw
template <bool GUIDED>
__device__ __forceinline__ void sift_rows(const uint8_t* __restrict__ xr, const int* __restrict__ ccr, int n1,
                                          const uint8_t* __restrict__ xc, const int* __restrict__ ccc, int nbx,
                                          int4* __restrict__ part, int ct_per_chunk, const int chunk, const int by,
                                          const SiftGuideWalk& gw) {
  __shared__ __attribute__((aligned(16))) uint8_t sB[2][kSiftTile * 128];
  __shared__ __attribute__((aligned(16))) int sCc[2][kSiftTile];
  const int row0 = by * kSiftStripe;
  const int bx0 = chunk * ct_per_chunk, bx1 = min(bx0 + ct_per_chunk, nbx);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  if (bx0 >= bx1) return;
  const bool active = row0 + wave * kSiftWaveRows < n1;   // wave-uniform: a wavefront without rows only stages

  // staging: wavefront w moves 128 / kSiftWaves rows of a tile, 8 rows per instruction: lane L of instruction j fills
  // position L & 7 of tile row 8 (kDma w + j) + (L >> 3) (r = its place in the 32-row block), which holds chunk
  // (L & 7) ^ swz(r) of the descriptor;
  // wavefronts 0 / 1 move the tile's 128 constants.  swz(r) = (bit 4, bit 3, bit 1) of r: ds_read_b128 serves the lanes
  // {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of a half together (MI355X LDS banking), and over each of these sets
  // (row parity, chunk ^ swz(row)) takes 16 different values = all 64 banks once.
  constexpr int kDma = 16 / kSiftWaves;   // DMA instructions per wavefront and tile (8 rows each)
  uint32_t goff[kDma];
#pragma unroll
  for (int j = 0; j < kDma; ++j) {
    const int row = wave * (8 * kDma) + 8 * j + (lane >> 3), r = row & 31;
    goff[j] = (uint32_t)row * 128u + (uint32_t)(((lane & 7) ^ (((r >> 2) & 6) | ((r >> 1) & 1))) * 16);
  }
  auto issue = [&](int bx, int buf) {
    if (PCD_SIFT_ABLATE & 4) return;
    const uint8_t* g = xc + (size_t)bx * (kSiftTile * 128);   // wave-uniform base + 32-bit lane offsets
    uint8_t* l = sB[buf] + wave * (1024 * kDma);
#pragma unroll
    for (int j = 0; j < kDma; ++j) sift_dma16<0>(g + goff[j], l + 1024 * j);
    if (wave < 2) sift_dma4(ccc + (size_t)bx * kSiftTile + wave * 64 + lane, &sCc[buf][wave * 64]);
    if constexpr (GUIDED) {   // the column records: 3 x 1 KB, wavefronts 2 .. 4
      if (wave >= 2 && wave < 2 + kSiftRecTile * 4 / 1024) {
        const uint8_t* gr = reinterpret_cast<const uint8_t*>(gw.crec + (size_t)bx * kSiftRecTile) + (wave - 2) * 1024 + lane * 16;
        sift_dma16<0>(gr, reinterpret_cast<uint8_t*>(sift_guide_lds() + buf * kSiftRecTile) + (wave - 2) * 1024);
      }
    }
  };
  issue(bx0, 0);

  // the wavefront's row fragments and row constants (rows past n1 are padding or another image's rows: never written)
  v4i fa[2][4];
  int rowc[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const size_t r = (size_t)row0 + wave * kSiftWaveRows + nt * 32 + lr;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const uint4 v = *reinterpret_cast<const uint4*>(xr + r * 128 + kk * 32 + lh * 16);
      fa[nt][kk] = v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
    }
    rowc[nt] = ccr[r] + kSiftConst;
  }
  // guided: the rows' records (rows past n1: zeros; their results are never written)
  float rrec[2][kSiftRecComps];
  if constexpr (GUIDED) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int r = row0 + wave * kSiftWaveRows + nt * 32 + lr;
#pragma unroll
      for (int c = 0; c < kSiftRecComps; ++c)
        rrec[nt][c] = r < n1 ? gw.rrec[(size_t)(r >> 7) * kSiftRecTile + c * kSiftTile + (r & 127)] : 0.f;
    }
  }
  // running state per row tile, relative to the row constant: true score 0 = -rowc, code -1 = "no column" (sift.cc:66-68)
  int m1[2], m2[2], arg[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) { m1[nt] = -rowc[nt]; m2[nt] = -rowc[nt]; arg[nt] = -1; }

  // fragment addresses inside a tile buffer: row lr of a block, k-chunk 2 kk + lh at position (2 kk + lh) ^ swz(lr)
  uint32_t foff[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    foff[kk] = (uint32_t)lr * 128u + (uint32_t)(((2 * kk + lh) ^ (((lr >> 2) & 6) | ((lr >> 1) & 1))) * 16);
  const uint32_t sB_base = sift_lds_addr(&sB[0][0]), sCc_base = sift_lds_addr(&sCc[0][0]) + (uint32_t)lh * 16u;

  // thr: what a score has to beat to matter -- the lane's own second best, or the second best of the row's other lane
  // half minus one (refreshed once per tile): a score below the other half's second best is below the row's final one.
  int thr[2] = {m2[0], m2[1]};
  auto slow = [&](const int v, const int j, const int code_s) {
    // volatile: the instructions must stay behind the branch (they are cheap enough to be if-converted)
    int code;   // (a v_cndmask cannot take an SGPR next to VCC: the code goes through a VGPR)
    asm volatile("v_mov_b32 %[c], %[code]\n\t"
                 "v_cmp_gt_i32 vcc, %[v], %[b]\n\t"
                 "v_cndmask_b32 %[a], %[a], %[c], vcc\n\t"
                 "v_med3_i32 %[s], %[b], %[s], %[v]\n\t"
                 "v_max_i32 %[b], %[b], %[v]\n\t"
                 "v_max_i32 %[t], %[t], %[s]"
                 : [b] "+v"(m1[j]), [s] "+v"(m2[j]), [a] "+v"(arg[j]), [t] "+v"(thr[j]), [c] "=&v"(code)
                 : [v] "v"(v), [code] "s"(code_s)
                 : "vcc");
  };
  // guided: per group of 4 registers (4 consecutive columns of the lane half), which lanes' pairs pass the filter
  const uint32_t sG_base = GUIDED ? sift_lds_addr(sift_guide_lds()) + (uint32_t)lh * 16u : 0u;
  auto guide_pass = [&](bool (&pass)[2][4], const uint32_t g_a, auto off_tag) {
    constexpr int OFF = decltype(off_tag)::value;   // byte offset of the group's columns in the records' comp 0
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) pass[j][i] = true;
    if (gw.mode & kSiftGuideH) {
      float4 c[2];
      sift_read_rec<OFF + 4 * kSiftTile * 4, 2>(c, g_a);
      const float cx[4] = {c[0].x, c[0].y, c[0].z, c[0].w}, cy[4] = {c[1].x, c[1].y, c[1].z, c[1].w};
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d0 = rrec[j][4] - cx[i], d1 = rrec[j][5] - cy[i];   // (the sign of the difference: squared)
          pass[j][i] = !(d0 * d0 + d1 * d1 > gw.th);
        }
    }
    if (gw.mode & kSiftGuideF) {
      float4 c[4];
      sift_read_rec<OFF, 4>(c, g_a);
      const float c0[4] = {c[0].x, c[0].y, c[0].z, c[0].w}, c1[4] = {c[1].x, c[1].y, c[1].z, c[1].w};
      const float c2[4] = {c[2].x, c[2].y, c[2].z, c[2].w}, c3[4] = {c[3].x, c[3].y, c[3].z, c[3].w};
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // set 1 = {a0, a1, a2, a0^2 + a1^2}, set 2 = {x2, y2, b0^2, b1^2}, whichever of them is the row
          const float* r = rrec[j];
          float e, den;
          if (gw.rows_set1) {
            e = (c0[i] * r[0] + c1[i] * r[1]) + r[2];
            den = (r[3] + c2[i]) + c3[i];
          } else {
            e = (r[0] * c0[i] + r[1] * c1[i]) + c2[i];
            den = (c3[i] + r[2]) + r[3];
          }
          pass[j][i] = pass[j][i] && !((e * e) / den > gw.tf);
        }
    }
  };
  auto scan_block = [&](const v16i (&acc)[2], const int seq, auto blk_tag) {
    if (PCD_SIFT_ABLATE & 1) { asm volatile("" ::"v"(acc[0]), "v"(acc[1])); return; }
    const int base = __builtin_amdgcn_readfirstlane(seq * 16);
    if constexpr (GUIDED) {
      // register 4 q + i = column 8 q + 4 lh + i of the block: the records of 4 consecutive columns per group, for both
      // row tiles; every row tile's registers still go in ascending column order
      constexpr int BLK = decltype(blk_tag)::value;
      const uint32_t g_a = sG_base + (uint32_t)(seq >> 2 & 1) * (kSiftRecTile * 4);
      auto group = [&](auto q_tag) {
        constexpr int Q = decltype(q_tag)::value;
        bool pass[2][4];
        guide_pass(pass, g_a, std::integral_constant<int, (BLK * 32 + Q * 8) * 4>{});
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          unsigned long long mk[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) mk[i] = __builtin_amdgcn_ballot_w64(acc[j][4 * Q + i] > thr[j] && pass[j][i]);
#pragma unroll
          for (int k = 0; k < 4; k += 2) {
            if (__builtin_expect((mk[k] | mk[k + 1]) != 0, 0)) {
              if (mk[k]) slow(pass[j][k] ? acc[j][4 * Q + k] : INT_MIN, j, base + 4 * Q + k);
              if (mk[k + 1]) slow(pass[j][k + 1] ? acc[j][4 * Q + k + 1] : INT_MIN, j, base + 4 * Q + k + 1);
            }
          }
        }
      };
      group(std::integral_constant<int, 0>{});
      group(std::integral_constant<int, 1>{});
      group(std::integral_constant<int, 2>{});
      group(std::integral_constant<int, 3>{});
      return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        unsigned long long mk[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (PCD_SIFT_ABLATE & 64) { asm volatile("s_mov_b64 %0, 0" : "=s"(mk[k])); continue; }   // no compares
          mk[k] = __builtin_amdgcn_ballot_w64(acc[j][8 * g + k] > thr[j]);
        }
        if (PCD_SIFT_ABLATE & 32) {   // compares only
#pragma unroll
          for (int k = 0; k < 8; ++k) asm volatile("" ::"s"(mk[k]));
          continue;
        }
        // one scalar test per PAIR of registers (asm goto, which would save the s_cmp behind the s_or, is miscompiled by
        // this hipcc: the asm body is dropped); unlikely: the fast path must be the fall-through
        // (a taken branch costs an instruction refetch)
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
          if (!(PCD_SIFT_ABLATE & 2) && __builtin_expect((mk[k] | mk[k + 1]) != 0, 0)) {
            if (mk[k]) slow(acc[j][8 * g + k], j, base + 8 * g + k);
            if (mk[k + 1]) slow(acc[j][8 * g + k + 1], j, base + 8 * g + k + 1);
          }
        }
      }
  };
  // once per tile: the other lane half's second best (v_permlane32_swap: lanes 32 .. 63 of one copy <-> lanes 0 .. 31 of
  // the other)
  auto share_thr = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const auto sw = __builtin_amdgcn_permlane32_swap((unsigned)m2[j], (unsigned)m2[j], false, false);
      const int other = lh ? (int)sw[0] : (int)sw[1];
      thr[j] = max(thr[j], other - 1);
    }
  };

  v16i acc0[2];
  // fragments of one column block: 4 k-chunks of the staged descriptors + the 16 column constants
  // (inline-asm LDS reads: for an ordinary LDS load hipcc would first drain the DMAs in flight with vmcnt(0))
  auto read_frag = [&](SiftFrag& f, const uint32_t fb_a, const uint32_t cc_a, auto blk_tag) {
    if (PCD_SIFT_ABLATE & 128) {   // fragments read once; opaque "new values" so that the MFMAs stay in the loop
      asm volatile("" : "+v"(f.fb[0]), "+v"(f.fb[1]), "+v"(f.fb[2]), "+v"(f.fb[3]), "+v"(f.cq[0]), "+v"(f.cq[1]), "+v"(f.cq[2]), "+v"(f.cq[3]));
      return;
    }
    sift_read_frag<decltype(blk_tag)::value>(f, fb_a + foff[0], fb_a + foff[1], fb_a + foff[2], fb_a + foff[3], cc_a);
    // the reads have landed (the asm ties the wait to the registers: nothing that uses them moves above it)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f.fb[0]), "+v"(f.fb[1]), "+v"(f.fb[2]), "+v"(f.fb[3]), "+v"(f.cq[0]), "+v"(f.cq[1]), "+v"(f.cq[2]), "+v"(f.cq[3])
                 :: "memory");
  };
  auto mfma_block = [&](v16i (&acc)[2], const SiftFrag& f) {
    // register 4 q + i of the result = column 8 q + 4 lh + i of the block
    v16i cc;
#pragma unroll
    for (int q = 0; q < 4; ++q) { cc[4 * q] = f.cq[q][0]; cc[4 * q + 1] = f.cq[q][1]; cc[4 * q + 2] = f.cq[q][2]; cc[4 * q + 3] = f.cq[q][3]; }
    if (PCD_SIFT_ABLATE & 16) return;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.fb[kk], fa[j][kk], kk == 0 ? cc : acc[j], 0, 0, 0);
  };

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  SiftFrag f;
  if (PCD_SIFT_ABLATE & 128) sift_read_frag<0>(f, sB_base + foff[0], sB_base + foff[1], sB_base + foff[2], sB_base + foff[3], sCc_base);
  for (int bx = bx0; bx < bx1; ++bx) {
    const int t = bx - bx0, buf = t & 1;
    if (bx + 1 < bx1) issue(bx + 1, buf ^ 1);   // the buffer's last readers passed the barrier below
    if (active) {
      share_thr();
      const uint32_t fb_a = sB_base + (uint32_t)buf * (kSiftTile * 128);
      const uint32_t cc_a = sCc_base + (uint32_t)buf * (kSiftTile * 4);
      read_frag(f, fb_a, cc_a, std::integral_constant<int, 0>{});
      mfma_block(acc0, f);
      scan_block(acc0, 4 * t, std::integral_constant<int, 0>{});
      read_frag(f, fb_a, cc_a, std::integral_constant<int, 1>{});
      mfma_block(acc0, f);
      scan_block(acc0, 4 * t + 1, std::integral_constant<int, 1>{});
      read_frag(f, fb_a, cc_a, std::integral_constant<int, 2>{});
      mfma_block(acc0, f);
      scan_block(acc0, 4 * t + 2, std::integral_constant<int, 2>{});
      read_frag(f, fb_a, cc_a, std::integral_constant<int, 3>{});
      mfma_block(acc0, f);
      scan_block(acc0, 4 * t + 3, std::integral_constant<int, 3>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wavefront's part of the next tile has landed
    if (!(PCD_SIFT_ABLATE & 8)) __syncthreads();
  }
  if (!active) return;

  // ---- end of the walk: decode, merge the two lane halves of a row, write the chunk's partial
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    int best = m1[nt] + rowc[nt], second = m2[nt] + rowc[nt], a = -1;
    if (arg[nt] >= 0) {
      const int seq = arg[nt] >> 4, reg = arg[nt] & 15;
      a = (bx0 + (seq >> 2)) * kSiftTile + (seq & 3) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
    }
    const int b2 = __shfl_xor(best, 32), s2 = __shfl_xor(second, 32), a2 = __shfl_xor(a, 32);
    top2_merge(b2, s2, a2, best, second, a);
    const int grow = row0 + wave * kSiftWaveRows + nt * 32 + lr;
    if (lh == 0 && grow < n1) part[(size_t)chunk * n1 + grow] = make_int4(best, second, a, 0);
  }
}

// blockIdx.z = direction: 0 = rows of set 1 over the columns of set 2 (part12), 1 = the sets exchanged (part21).
// ct12 / ct21: column tiles per chunk of the two directions; workgroups past a direction's stripes or chunks leave.
__global__ __launch_bounds__(64 * kSiftWaves, PCD_SIFT_WGS) void k_sift_scores_stripe(const uint8_t* __restrict__ xa,
                                                            const int* __restrict__ cc, uint32_t prow1, int n1,
                                                            uint32_t prow2, int n2, int4* __restrict__ part12,
                                                            int4* __restrict__ part21, int ct12, int ct21) {
  // (one call site: the walk is ~20 KB of code)
  const bool fwd = blockIdx.z == 0;
  const uint32_t pr = fwd ? prow1 : prow2, pc = fwd ? prow2 : prow1;
  const int nr = fwd ? n1 : n2, nc = fwd ? n2 : n1;
  if ((int)blockIdx.y * kSiftStripe >= nr) return;
  sift_rows<false>(xa + (size_t)pr * 128, cc + pr, nr, xa + (size_t)pc * 128, cc + pc, (nc + kSiftTile - 1) / kSiftTile,
                   fwd ? part12 : part21, fwd ? ct12 : ct21, blockIdx.x, blockIdx.y, SiftGuideWalk{});
}

// ---- many image pairs in one launch set (pcd_sift_match_batch_device) ----------------------------------
// All descriptors live in one arena; a pair names two row ranges of it.  blockIdx.z = 2 pair + direction; the grid's
// x / y extents are sized for the largest set of the batch, smaller ones leave early.
struct SiftPairDev {
  uint32_t prow1, n1, prow2, n2; // rows of the two images in the prepared copy, their sizes
  uint64_t part12, part21;       // int4 offsets of the pair's partial results
  uint64_t m12, m21;             // int offsets of the pair's best-match arrays
  uint64_t match;                // offset (in matches) of the pair's output list
};

__global__ __launch_bounds__(64 * kSiftWaves, PCD_SIFT_WGS) void k_sift_scores_batch(const uint8_t* __restrict__ xa,
                                                           const int* __restrict__ cc,
                                                           const SiftPairDev* __restrict__ pairs,
                                                           int4* __restrict__ part12, int4* __restrict__ part21,
                                                           int nchunk) {
  const SiftPairDev pr = pairs[blockIdx.z >> 1];
  const bool fwd = (blockIdx.z & 1) == 0;
  const uint32_t rr = fwd ? pr.prow1 : pr.prow2, rc = fwd ? pr.prow2 : pr.prow1;
  const int nr = (int)(fwd ? pr.n1 : pr.n2), nc = (int)(fwd ? pr.n2 : pr.n1);
  if ((int)blockIdx.y * kSiftStripe >= nr) return;
  const int nb = (nc + kSiftTile - 1) / kSiftTile;   // chunks past the last column tile leave inside sift_rows
  sift_rows<false>(xa + (size_t)rr * 128, cc + rr, nr, xa + (size_t)rc * 128, cc + rc, nb,
                   fwd ? part12 + pr.part12 : part21 + pr.part21, (nb + nchunk - 1) / nchunk, blockIdx.x, blockIdx.y,
                   SiftGuideWalk{});
}

// ---- guided kernels ----
// one workgroup of 128 threads per (128-row tile, side, pair): records of every row of the tile (zeros past n)
__global__ __launch_bounds__(128) void k_sift_guide_prep(const SiftGuidePairDev* __restrict__ guides,
                                                         float* __restrict__ rec) {
  const SiftGuidePairDev& g = guides[blockIdx.z];
  const bool side2 = blockIdx.y == 1;
  const uint32_t n = side2 ? g.n2 : g.n1, tile = blockIdx.x, r = tile * kSiftTile + threadIdx.x;
  if (tile * kSiftTile >= n) return;
  float v[kSiftRecComps] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (r < n) {
    const float* loc = side2 ? g.loc2 : g.loc1;
    const float x = loc[2 * (size_t)r], y = loc[2 * (size_t)r + 1];
    if (!side2) {
      if (g.mode & kSiftGuideF) {
        const float a0 = (g.F[0] * x + g.F[1] * y) + g.F[2];
        const float a1 = (g.F[3] * x + g.F[4] * y) + g.F[5];
        const float a2 = (g.F[6] * x + g.F[7] * y) + g.F[8];
        v[0] = a0; v[1] = a1; v[2] = a2; v[3] = a0 * a0 + a1 * a1;
      }
      if (g.mode & kSiftGuideH) {
        const float h0 = (g.H[0] * x + g.H[1] * y) + g.H[2];
        const float h1 = (g.H[3] * x + g.H[4] * y) + g.H[5];
        const float h2 = (g.H[6] * x + g.H[7] * y) + g.H[8];
        v[4] = h0 / h2; v[5] = h1 / h2;
      }
    } else {
      if (g.mode & kSiftGuideF) {
        const float b0 = (g.F[0] * x + g.F[3] * y) + g.F[6];
        const float b1 = (g.F[1] * x + g.F[4] * y) + g.F[7];
        v[0] = x; v[1] = y; v[2] = b0 * b0; v[3] = b1 * b1;
      }
      v[4] = x; v[5] = y;
    }
  }
  float* out = rec + (side2 ? g.rec2 : g.rec1) + (size_t)tile * kSiftRecTile + threadIdx.x;
#pragma unroll
  for (int c = 0; c < kSiftRecComps; ++c) out[c * kSiftTile] = v[c];
}

// guided form of k_sift_scores_stripe: guide = the pair's entry (mode, record offsets), rec = the records
__global__ __launch_bounds__(64 * kSiftWaves, PCD_SIFT_WGS) void k_sift_guided_stripe(
    const uint8_t* __restrict__ xa, const int* __restrict__ cc, uint32_t prow1, int n1, uint32_t prow2, int n2,
    int4* __restrict__ part12, int4* __restrict__ part21, int ct12, int ct21, const SiftGuidePairDev* __restrict__ guide,
    const float* __restrict__ rec, float th, float tf) {
  const bool fwd = blockIdx.z == 0;
  const uint32_t pr = fwd ? prow1 : prow2, pc = fwd ? prow2 : prow1;
  const int nr = fwd ? n1 : n2, nc = fwd ? n2 : n1;
  if ((int)blockIdx.y * kSiftStripe >= nr) return;
  const float* r1 = rec + guide->rec1;
  const float* r2 = rec + guide->rec2;
  const SiftGuideWalk gw{fwd ? r1 : r2, fwd ? r2 : r1, guide->mode, fwd, th, tf};
  sift_rows<true>(xa + (size_t)pr * 128, cc + pr, nr, xa + (size_t)pc * 128, cc + pc, (nc + kSiftTile - 1) / kSiftTile,
                  fwd ? part12 : part21, fwd ? ct12 : ct21, blockIdx.x, blockIdx.y, gw);
}

// guided form of k_sift_scores_batch: guides [pair] beside pairs [pair] (mode none: the unguided walk's result)
__global__ __launch_bounds__(64 * kSiftWaves, PCD_SIFT_WGS) void k_sift_guided_batch(
    const uint8_t* __restrict__ xa, const int* __restrict__ cc, const SiftPairDev* __restrict__ pairs,
    int4* __restrict__ part12, int4* __restrict__ part21, int nchunk, const SiftGuidePairDev* __restrict__ guides,
    const float* __restrict__ rec, float th, float tf) {
  const SiftPairDev pr = pairs[blockIdx.z >> 1];
  const bool fwd = (blockIdx.z & 1) == 0;
  const uint32_t rr = fwd ? pr.prow1 : pr.prow2, rc = fwd ? pr.prow2 : pr.prow1;
  const int nr = (int)(fwd ? pr.n1 : pr.n2), nc = (int)(fwd ? pr.n2 : pr.n1);
  if ((int)blockIdx.y * kSiftStripe >= nr) return;
  const int nb = (nc + kSiftTile - 1) / kSiftTile;
  const SiftGuidePairDev& g = guides[blockIdx.z >> 1];
  const float* r1 = rec + g.rec1;
  const float* r2 = rec + g.rec2;
  const SiftGuideWalk gw{fwd ? r1 : r2, fwd ? r2 : r1, g.mode, fwd, th, tf};
  sift_rows<true>(xa + (size_t)rr * 128, cc + rr, nr, xa + (size_t)rc * 128, cc + rc, nb,
                  fwd ? part12 + pr.part12 : part21 + pr.part21, (nb + nchunk - 1) / nchunk, blockIdx.x, blockIdx.y, gw);
}

// sift.cc:72-104: merge the per-tile triples in ascending tile order, then the distance / ratio tests.
// One launch for both directions: threads [0, n1) finish set 1 -> 2, threads [n1, n1 + n2) set 2 -> 1.
__device__ __forceinline__ void sift_finalize(const int4* __restrict__ part12, int n1, int nc12,
                                              const int4* __restrict__ part21, int n2, int nc21, float max_ratio,
                                              float max_distance, int* __restrict__ m12, int* __restrict__ m21) {
  // 16 lanes per descriptor: lane p merges chunks p, p + 16, ... in ascending order, then a 4-step butterfly.
  // On equal best scores the lower index wins, which is the earlier chunk (indices ascend with the chunk) --
  // the same winner as the reference's single ascending scan.
  const int g = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, p = threadIdx.x & 15;
  if (g >= n1 + n2) return;
  const bool first = g < n1;
  const int i = first ? g : g - n1;
  const int4* __restrict__ part = first ? part12 : part21;
  const int n = first ? n1 : n2, nc = first ? nc12 : nc21;
  int best = 0, second = 0, arg = -1;
  for (int b = p; b < nc; b += 16) {
    const int4 v = part[(size_t)b * n + i];
    top2_merge(v.x, v.y, v.z, best, second, arg);
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const int b2 = __shfl_xor(best, o), s2 = __shfl_xor(second, o), a2 = __shfl_xor(arg, o);
    top2_merge(b2, s2, a2, best, second, arg);
  }
  if (p != 0) return;
  int m = -1;
  if (arg != -1 && best > 0) {
    const float kDistNorm = 1.0f / (512.0f * 512.0f);
    const float bn = acosf(fminf(kDistNorm * (float)best, 1.0f));
    if (!(bn > max_distance)) {
      const float sn = acosf(fminf(kDistNorm * (float)second, 1.0f));
      if (!(bn >= max_ratio * sn)) m = arg;
    }
  }
  (first ? m12 : m21)[i] = m;
}

// chunks of a walk over nb column tiles cut into nchunk pieces that wrote a partial
__host__ __device__ __forceinline__ int sift_chunks_used(int nb, int nchunk) {
  const int ct = (nb + nchunk - 1) / nchunk;
  return ct > 0 ? (nb + ct - 1) / ct : 0;
}

__global__ __launch_bounds__(256) void k_sift_finalize(const int4* __restrict__ part12, int n1, int nc12,
                                                       const int4* __restrict__ part21, int n2, int nc21,
                                                       float max_ratio, float max_distance, int* __restrict__ m12,
                                                       int* __restrict__ m21) {
  sift_finalize(part12, n1, nc12, part21, n2, nc21, max_ratio, max_distance, m12, m21);
}

__global__ __launch_bounds__(256) void k_sift_finalize_batch(const SiftPairDev* __restrict__ pairs,
                                                             const int4* __restrict__ part12,
                                                             const int4* __restrict__ part21, int nchunk,
                                                             float max_ratio, float max_distance, int* __restrict__ m12,
                                                             int* __restrict__ m21) {
  const SiftPairDev pr = pairs[blockIdx.z];
  const int nb1 = ((int)pr.n1 + kSiftTile - 1) / kSiftTile, nb2 = ((int)pr.n2 + kSiftTile - 1) / kSiftTile;
  sift_finalize(part12 + pr.part12, (int)pr.n1, sift_chunks_used(nb2, nchunk), part21 + pr.part21, (int)pr.n2,
                sift_chunks_used(nb1, nchunk), max_ratio, max_distance, m12 + pr.m12, m21 + pr.m21);
}

// sift.cc:118-143 for n1 <= 1024 * kCompactPer: cross check, ordered compaction and count in ONE workgroup
// (a launch costs more than the work: 8192 flags).  Larger sets take the three-kernel path below.
constexpr int kCompactPer = 16;
__device__ __forceinline__ void sift_keep_compact(const int* __restrict__ m12, const int* __restrict__ m21, int n1,
                                                  int cross_check, uint32_t* __restrict__ matches,
                                                  int* __restrict__ count) {
  __shared__ uint32_t s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (n1 + 1023) / 1024;            // <= kCompactPer consecutive rows per thread
  const int i0 = tid * per;
  uint32_t flags = 0, cnt = 0;
  // two rounds of independent loads (all m12 entries, then all m21 entries on clamped indices) instead of `per`
  // dependent pairs in a row: the single workgroup's time is the latency of this chain (17 -> 8 us for 8192 rows)
  int jj[kCompactPer], bb[kCompactPer];
#pragma unroll
  for (int k = 0; k < kCompactPer; ++k) jj[k] = (k < per && i0 + k < n1) ? m12[i0 + k] : -1;
#pragma unroll
  for (int k = 0; k < kCompactPer; ++k) bb[k] = (cross_check && jj[k] != -1) ? m21[jj[k]] : -1;
#pragma unroll
  for (int k = 0; k < kCompactPer; ++k) {
    bool keep = jj[k] != -1;
    if (keep && cross_check) keep = bb[k] != -1 && bb[k] == i0 + k;
    flags |= (keep ? 1u : 0u) << k;
    cnt += keep ? 1u : 0u;
  }
  // exclusive scan of cnt over the 1024 threads: DPP-free shuffle scan inside the wave, LDS across waves
  uint32_t inc = cnt;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t base = 0, total = 0;
  for (int w = 0; w < 16; ++w) {
    const uint32_t c = s_wave[w];
    if (w < wave) base += c;
    total += c;
  }
  uint32_t pos = base + inc - cnt;
#pragma unroll
  for (int k = 0; k < kCompactPer; ++k)
    if ((flags >> k) & 1u) {
      matches[2 * pos] = (uint32_t)(i0 + k);
      matches[2 * pos + 1] = (uint32_t)jj[k];
      ++pos;
    }
  if (tid == 0) *count = (int)total;
}

__global__ __launch_bounds__(1024) void k_sift_keep_compact(const int* __restrict__ m12, const int* __restrict__ m21,
                                                            int n1, int cross_check, uint32_t* __restrict__ matches,
                                                            int* __restrict__ count) {
  sift_keep_compact(m12, m21, n1, cross_check, matches, count);
}

// one workgroup per pair
__global__ __launch_bounds__(1024) void k_sift_keep_compact_batch(const SiftPairDev* __restrict__ pairs,
                                                                  const int* __restrict__ m12,
                                                                  const int* __restrict__ m21, int cross_check,
                                                                  uint32_t* __restrict__ matches,
                                                                  int* __restrict__ counts) {
  const SiftPairDev pr = pairs[blockIdx.x];
  sift_keep_compact(m12 + pr.m12, m21 + pr.m21, (int)pr.n1, cross_check, matches + 2 * pr.match, counts + blockIdx.x);
}

// dense packing of the per-pair lists (host entry): list p moves from matches_in + 2 * src_off[p] to
// matches_out + 2 * dense_off[p]
__global__ __launch_bounds__(256) void k_sift_pack_lists(const uint64_t* __restrict__ src_off,
                                                         const int* __restrict__ counts,
                                                         const uint64_t* __restrict__ dense_off,
                                                         const uint32_t* __restrict__ matches_in,
                                                         uint32_t* __restrict__ matches_out) {
  const int p = blockIdx.x;
  const uint2* __restrict__ src = reinterpret_cast<const uint2*>(matches_in) + src_off[p];
  uint2* __restrict__ dst = reinterpret_cast<uint2*>(matches_out) + dense_off[p];
  for (int i = threadIdx.x; i < counts[p]; i += blockDim.x) dst[i] = src[i];
}

// sift.cc:118-143: keep flags, in set-1 order
__global__ void k_sift_keep(const int* __restrict__ m12, const int* __restrict__ m21, int n1, int cross_check,
                            uint32_t* __restrict__ keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1) return;
  const int j = m12[i];
  bool k = j != -1;
  if (k && cross_check) k = (m21[j] != -1) && (m21[j] == i);
  keep[i] = k ? 1u : 0u;
}
__global__ void k_sift_compact(const int* __restrict__ m12, const uint32_t* __restrict__ keep,
                               const uint32_t* __restrict__ pos, int n1, uint32_t* __restrict__ matches,
                               int* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1) return;
  if (keep[i]) { matches[2 * pos[i]] = (uint32_t)i; matches[2 * pos[i] + 1] = (uint32_t)m12[i]; }
  if (i == n1 - 1) *count = (int)(pos[i] + keep[i]);
}

struct SiftScratch {
  DevBuf<uint8_t> d1, d2;
  DevBuf<uint8_t> xa;   // the prepared copy (k_sift_prep_*): re-centred bytes, images padded to 128 rows, + one stripe of slack
  DevBuf<int> cc;       // its per-row constants
  DevBuf<SiftImageDev> images;
  PinnedBuf<SiftImageDev> h_images;
  DevBuf<int> m12, m21, count;
  DevBuf<int4> part12, part21;
  DevBuf<uint32_t> keep, pos, matches;
  DevBuf<char> tmp;
  // batch entry
  DevBuf<uint8_t> arena;
  DevBuf<SiftPairDev> pairs;
  DevBuf<int> counts;
  DevBuf<uint64_t> dense_off;
  DevBuf<uint32_t> dense;
  // guided entries: the pair's records, the guide table (uploaded like the pair table, from h_guides), host locations
  DevBuf<float> grec, loc1, loc2, locs;
  DevBuf<SiftGuidePairDev> guides;
  PinnedBuf<SiftGuidePairDev> h_guides;
  // The scratch is per DEVICE and shared by every call on it.  Host side: g_sift_mu (recursive) is held for the whole
  // of a host entry point and while a *_device entry point enqueues.  Device side: calls on different streams are
  // ordered through ev_done (the next call's stream waits for the previous call's last kernel before any of its own
  // work touches part12 / m12 / pairs ...; calls on one stream are ordered anyway).  The pair table goes up with an
  // asynchronous copy on the caller's stream from h_pairs; ev_tab guards the pinned buffer against being rewritten
  // while that copy is still in flight.
  PinnedBuf<SiftPairDev> h_pairs;
  hipEvent_t ev_done = nullptr, ev_tab = nullptr;
  hipStream_t last_stream = nullptr;
  bool used = false, tab_pending = false;
  ~SiftScratch() {
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (ev_tab) (void)hipEventDestroy(ev_tab);
  }
};
static SiftScratch* g_sift[64] = {nullptr};
static std::recursive_mutex g_sift_mu;

// THE use of a device's shared scratch: body(scratch) enqueues on stream s with g_sift_mu held, behind the previous
// use's ev_done if that was on another stream.  ev_done is recorded on every way out of body -- an error return or an
// exception included, as body may have enqueued work that touches the scratch before it failed.  Uses nest (a host
// entry holds the scratch around the device entry it calls); device < 64 is the caller's check.
template <typename Body>
static pcd_status sift_use_scratch(int device, hipStream_t s, Body&& body) {
  std::lock_guard<std::recursive_mutex> g(g_sift_mu);
  PCD_HIP_TRY(hipSetDevice(device));
  if (!g_sift[device]) g_sift[device] = new SiftScratch();
  SiftScratch& sc = *g_sift[device];
  if (!sc.ev_done) {
    PCD_HIP_TRY(hipEventCreateWithFlags(&sc.ev_done, hipEventDisableTiming));
    PCD_HIP_TRY(hipEventCreateWithFlags(&sc.ev_tab, hipEventDisableTiming));
  }
  if (sc.used && sc.last_stream != s) PCD_HIP_TRY(hipStreamWaitEvent(s, sc.ev_done, 0));
  const pcd_status st = pcd::guard([&]() -> pcd_status { return body(sc); });
  PCD_HIP_TRY(hipEventRecord(sc.ev_done, s));
  sc.last_stream = s;
  sc.used = true;
  return st;
}

// the pinned staging of the pair / image / guide tables is free again (the previous upload has left it)
static pcd_status sift_tables_free(SiftScratch& sc) {
  if (sc.tab_pending) PCD_HIP_TRY(hipEventSynchronize(sc.ev_tab));
  return PCD_OK;
}
static pcd_status sift_tables_sent(SiftScratch& sc, hipStream_t s) {
  PCD_HIP_TRY(hipEventRecord(sc.ev_tab, s));
  sc.tab_pending = true;
  return PCD_OK;
}

static inline uint64_t sift_tiles(uint64_t n) { return (n + kSiftTile - 1) / kSiftTile; }

// one pair's guide table entry: its records start at float offset rec1 of the record buffer, side 2 behind side 1
// (H / F are read iff the mode names them)
static SiftGuidePairDev sift_guide_entry(const float* d_loc1, uint64_t n1, const float* d_loc2, uint64_t n2,
                                         uint64_t rec1, int mode, const float* H, const float* F) {
  SiftGuidePairDev g{};
  g.loc1 = d_loc1; g.loc2 = d_loc2; g.n1 = (uint32_t)n1; g.n2 = (uint32_t)n2;
  g.rec1 = rec1; g.rec2 = rec1 + sift_tiles(n1) * kSiftRecTile;
  g.mode = mode & (kSiftGuideH | kSiftGuideF);
  if (g.mode & kSiftGuideH) std::memcpy(g.H, H, sizeof(g.H));
  if (g.mode & kSiftGuideF) std::memcpy(g.F, F, sizeof(g.F));
  return g;
}

// one guided pair's table entry on the device (sc.guides[0]) for sift_device: its records at the start of sc.grec
static pcd_status sift_upload_guide(SiftScratch& sc, hipStream_t s, const float* d_loc1, int n1, const float* d_loc2,
                                    int n2, int mode, const float* H, const float* F) {
  PCD_TRY(sift_tables_free(sc));
  PCD_TRY(sc.h_guides.reserve(1)); PCD_TRY(sc.guides.reserve(1));
  sc.h_guides.p[0] = sift_guide_entry(d_loc1, n1, d_loc2, n2, 0, mode, H, F);
  PCD_HIP_TRY(hipMemcpyAsync(sc.guides.p, sc.h_guides.p, sizeof(SiftGuidePairDev), hipMemcpyHostToDevice, s));
  return sift_tables_sent(sc, s);
}

// One pair, both sets non-empty, on the device.  d_guide (guided): the pair's table entry on the device, laid out by
// sift_upload_guide; th / tf its thresholds.
static pcd_status sift_device(const uint8_t* d_d1, int n1, const uint8_t* d_d2, int n2, float max_ratio,
                              float max_distance, int cross_check, int* d_m12, int* d_m21, uint32_t* d_matches,
                              int* d_count, SiftScratch& sc, hipStream_t s, const SiftGuidePairDev* d_guide, float th,
                              float tf) {
  const int nb1 = (int)sift_tiles(n1), nb2 = (int)sift_tiles(n2);
  const int ns1 = (n1 + kSiftStripe - 1) / kSiftStripe, ns2 = (n2 + kSiftStripe - 1) / kSiftStripe;
  // stripe walks in both directions: enough (row stripe, chunk) workgroups to fill the chip twice over
  // pcd_sift_set_tuning (tests / fuzzing) can force the number of column chunks, e.g. 1 = every stripe walks all tiles
  const int nchunk_set = g_sift_nchunk.load(std::memory_order_relaxed);
  auto chunks = [&](int ncol_tiles) {
    const int want = nchunk_set > 0 ? nchunk_set : (512 + ns1 + ns2 - 1) / (ns1 + ns2);
    return std::max(1, std::min(want, ncol_tiles));
  };
  const int nchunk12 = chunks(nb2), nchunk21 = chunks(nb1);
  const int ct12 = (nb2 + nchunk12 - 1) / nchunk12, ct21 = (nb1 + nchunk21 - 1) / nchunk21;
  const int used12 = sift_chunks_used(nb2, nchunk12), used21 = sift_chunks_used(nb1, nchunk21);
  const dim3 grid(std::max(used12, used21), std::max(ns1, ns2), 2), block(64 * kSiftWaves);
  const uint32_t prow1 = 0, prow2 = (uint32_t)nb1 * kSiftTile;
  const size_t prows = (size_t)(nb1 + nb2) * kSiftTile + kSiftStripe;   // a stripe's row fragments are read unconditionally
  PCD_TRY(sc.xa.reserve(prows * 128)); PCD_TRY(sc.cc.reserve(prows));
  PCD_TRY(sc.part12.reserve((size_t)n1 * used12)); PCD_TRY(sc.part21.reserve((size_t)n2 * used21));
  PCD_TRY(sc.keep.reserve(n1)); PCD_TRY(sc.pos.reserve(n1));
  if (d_guide) PCD_TRY(sc.grec.reserve((size_t)(nb1 + nb2) * kSiftRecTile));
  {
    ScopedKernelTimer t("sift_prep", s);
    hipLaunchKernelGGL(k_sift_prep_pair, dim3(std::max(nb1, nb2), 2), dim3(256), 0, s, SiftImageDev{d_d1, (uint32_t)n1, prow1},
                       SiftImageDev{d_d2, (uint32_t)n2, prow2}, sc.xa.p, sc.cc.p);
  }
  if (d_guide) {
    ScopedKernelTimer t("sift_guide_prep", s);
    hipLaunchKernelGGL(k_sift_guide_prep, dim3(std::max(nb1, nb2), 2, 1), dim3(kSiftTile), 0, s, d_guide, sc.grec.p);
  }
  {
    ScopedKernelTimer t(d_guide ? "sift_guided_scores" : "sift_scores", s);
    if (d_guide)
      hipLaunchKernelGGL(k_sift_guided_stripe, grid, block, 0, s, sc.xa.p, sc.cc.p, prow1, n1, prow2, n2, sc.part12.p,
                         sc.part21.p, ct12, ct21, d_guide, sc.grec.p, th, tf);
    else
      hipLaunchKernelGGL(k_sift_scores_stripe, grid, block, 0, s, sc.xa.p, sc.cc.p, prow1, n1, prow2, n2, sc.part12.p,
                         sc.part21.p, ct12, ct21);
  }
  {
    ScopedKernelTimer t("sift_finalize", s);
    hipLaunchKernelGGL(k_sift_finalize, dim3(div_up(((uint64_t)n1 + n2) * 16, 256)), dim3(256), 0, s, sc.part12.p, n1,
                       used12, sc.part21.p, n2, used21, max_ratio, max_distance, d_m12, d_m21);
  }
  {
    ScopedKernelTimer t("sift_compact", s);
    if (n1 <= 1024 * kCompactPer) {
      hipLaunchKernelGGL(k_sift_keep_compact, dim3(1), dim3(1024), 0, s, d_m12, d_m21, n1, cross_check, d_matches,
                         d_count);
    } else {
      hipLaunchKernelGGL(k_sift_keep, dim3(div_up(n1, 256)), dim3(256), 0, s, d_m12, d_m21, n1, cross_check, sc.keep.p);
      PCD_TRY(exclusive_sum(sc.tmp, sc.keep.p, sc.pos.p, 0u, (size_t)n1, s));
      hipLaunchKernelGGL(k_sift_compact, dim3(div_up(n1, 256)), dim3(256), 0, s, d_m12, sc.keep.p, sc.pos.p, n1,
                         d_matches, d_count);
    }
  }
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

// ---- many pairs over one descriptor arena ---------------------------------------------------------------------------
// Sub-batches are cut so that the partial results of a sub-batch stay under kSiftBatchPartials int4 (2 GiB); each
// sub-batch is three launches (scores, finalize, cross check + compaction; guided: the records' launch in front), the
// arena's preparation one launch in front of all.  Nothing synchronises with the host.
constexpr size_t kSiftBatchPartials = (size_t)1 << 27;   // pcd_sift_set_tuning overrides it (tests: forces the cuts)

// what a batch call is given (guides == nullptr: unguided; d_locs = [rows][2] locations parallel to the arena)
struct SiftBatchArgs {
  const uint8_t* d_arena;
  const float* d_locs;
  const uint64_t* first_row;
  int n_images;
  const uint32_t* pair_ids;
  int n_pairs;
  const pcd_sift_guide* guides;
  float th, tf, max_ratio, max_distance;
  int cross_check;
  uint32_t* d_matches;
  const uint64_t* match_offset;
  int* d_counts;
  uint64_t rows(uint32_t image) const { return first_row[image + 1] - first_row[image]; }
};

// the pair list is consistent with the arena; *wide: some first set is too long for the one-workgroup compaction
static pcd_status sift_batch_validate(const SiftBatchArgs& a, bool* wide) {
  PCD_REQUIRE(a.first_row[a.n_images] < (1ull << 32), "arena larger than 2^32 descriptors");
  for (int i = 0; i < a.n_images; ++i) PCD_REQUIRE(a.first_row[i] <= a.first_row[i + 1], "first_row must ascend");
  *wide = false;
  for (int p = 0; p < a.n_pairs; ++p) {
    const uint32_t i1 = a.pair_ids[2 * p], i2 = a.pair_ids[2 * p + 1];
    PCD_REQUIRE(i1 < (uint32_t)a.n_images && i2 < (uint32_t)a.n_images, "pair names an image outside the arena");
    PCD_REQUIRE(a.rows(i1) < (1u << 30) && a.rows(i2) < (1u << 30), "image too large");
    *wide = *wide || a.rows(i1) > (uint64_t)1024 * kCompactPer;
  }
  return PCD_OK;
}

// batches with a wide set run pair by pair through sift_device (the three-kernel compaction)
static pcd_status sift_batch_pairwise(const SiftBatchArgs& a, SiftScratch& sc, hipStream_t s) {
  for (int p = 0; p < a.n_pairs; ++p) {
    const uint32_t i1 = a.pair_ids[2 * p], i2 = a.pair_ids[2 * p + 1];
    const int n1 = (int)a.rows(i1), n2 = (int)a.rows(i2);
    if (n1 == 0 || n2 == 0) { PCD_HIP_TRY(hipMemsetAsync(a.d_counts + p, 0, sizeof(int), s)); continue; }
    PCD_TRY(sc.m12.reserve(n1)); PCD_TRY(sc.m21.reserve(n2));
    const bool guided = a.guides && (a.guides[p].mode & (kSiftGuideH | kSiftGuideF));
    if (guided)
      PCD_TRY(sift_upload_guide(sc, s, a.d_locs + 2 * a.first_row[i1], n1, a.d_locs + 2 * a.first_row[i2], n2,
                                a.guides[p].mode, a.guides[p].H, a.guides[p].F));
    PCD_TRY(sift_device(a.d_arena + a.first_row[i1] * 128, n1, a.d_arena + a.first_row[i2] * 128, n2, a.max_ratio,
                        a.max_distance, a.cross_check, sc.m12.p, sc.m21.p, a.d_matches + 2 * a.match_offset[p],
                        a.d_counts + p, sc, s, guided ? sc.guides.p : nullptr, a.th, a.tf));
  }
  return PCD_OK;
}

// the prepared copy: every image padded to a multiple of 128 rows, one behind the other
struct SiftBatchLayout {
  std::vector<SiftImageDev> images;
  uint64_t prows = 0;       // rows of the copy
  uint32_t max_tiles = 0;   // of the largest image
};
static SiftBatchLayout sift_batch_layout(const SiftBatchArgs& a) {
  SiftBatchLayout l;
  l.images.resize((size_t)a.n_images);
  for (int i = 0; i < a.n_images; ++i) {
    const uint64_t n = a.rows(i);
    l.images[i] = SiftImageDev{a.d_arena + a.first_row[i] * 128, (uint32_t)n, (uint32_t)l.prows};
    l.max_tiles = std::max<uint32_t>(l.max_tiles, (uint32_t)sift_tiles(n));
    l.prows += sift_tiles(n) * kSiftTile;
  }
  return l;
}

// the sub-batches of a call: pairs [cut[k], cut[k + 1]) run in one launch set with nchunk[k] column chunks per walk
struct SiftBatchPlan {
  std::vector<SiftPairDev> pairs;         // for the whole call (uploaded once; sub-batches index into it)
  std::vector<SiftGuidePairDev> guides;   // guided: beside pairs; partials, best matches and records of a sub-batch from 0
  std::vector<int> cut, nchunk;
  size_t max12 = 0, max21 = 0, maxm12 = 0, maxm21 = 0, maxrec = 0;   // the largest sub-batch's scratch, in elements
};
// Pure host arithmetic (device pointers are only offset).  nchunk_set / budget: pcd_sift_set_tuning's values or the
// defaults; the budget counts 16-byte units: both partial arrays are int4.
static SiftBatchPlan sift_batch_plan(const SiftBatchArgs& a, const std::vector<SiftImageDev>& images, int nchunk_set,
                                     size_t budget) {
  SiftBatchPlan pl;
  pl.pairs.resize((size_t)a.n_pairs);
  pl.guides.resize(a.guides ? (size_t)a.n_pairs : 0);
  pl.cut.push_back(0);
  for (int p0 = 0; p0 < a.n_pairs;) {
    // how many column chunks per row stripe: enough workgroups to fill the chip twice when the batch is small
    // (decided on the first pair's size and the pairs left; any value gives the same results)
    const int nby0 = std::max<int>(1, (int)sift_tiles(a.rows(a.pair_ids[2 * p0])));
    const int nbx0 = std::max<int>(1, (int)sift_tiles(a.rows(a.pair_ids[2 * p0 + 1])));
    const long stripes0 = (nby0 * kSiftTile + kSiftStripe - 1) / kSiftStripe + (nbx0 * kSiftTile + kSiftStripe - 1) / kSiftStripe;   // stripes of both directions
    const long left = a.n_pairs - p0;
    const long want = nchunk_set > 0 ? nchunk_set : (512 + stripes0 * left - 1) / (stripes0 * left);
    const int nchunk = (int)std::max<long>(1, std::min<long>(want, std::max(nbx0, nby0)));
    size_t o12 = 0, o21 = 0, om12 = 0, om21 = 0, orec = 0;
    int p = p0;
    for (; p < a.n_pairs; ++p) {
      const uint32_t i1 = a.pair_ids[2 * p], i2 = a.pair_ids[2 * p + 1];
      uint64_t n1 = a.rows(i1), n2 = a.rows(i2);
      if (n1 == 0 || n2 == 0) n1 = n2 = 0;   // an empty image: no matches (sift_test.cc:311-318); every kernel skips the pair
      const size_t need12 = (size_t)nchunk * n1, need21 = (size_t)nchunk * n2;
      // (2 z-slices per pair in the scores launch: at most 32767 pairs)
      if (p > p0 && (o12 + need12 + o21 + need21 > budget || p - p0 >= 32767)) break;
      pl.pairs[p] = SiftPairDev{images[i1].prow, (uint32_t)n1, images[i2].prow, (uint32_t)n2, o12, o21, om12, om21, a.match_offset[p]};
      o12 += need12; o21 += need21; om12 += n1; om21 += n2;
      if (a.guides) {
        pl.guides[p] = sift_guide_entry(a.d_locs + 2 * a.first_row[i1], n1, a.d_locs + 2 * a.first_row[i2], n2, orec,
                                        a.guides[p].mode, a.guides[p].H, a.guides[p].F);
        orec = pl.guides[p].rec2 + sift_tiles(n2) * kSiftRecTile;
      }
    }
    pl.max12 = std::max(pl.max12, o12); pl.max21 = std::max(pl.max21, o21);
    pl.maxm12 = std::max(pl.maxm12, om12); pl.maxm21 = std::max(pl.maxm21, om21);
    pl.maxrec = std::max(pl.maxrec, orec);
    pl.cut.push_back(p);
    pl.nchunk.push_back(nchunk);
    p0 = p;
  }
  return pl;
}

// The tables go up ON THE CALLER'S STREAM (a null-stream copy is not ordered against a non-blocking stream: a second
// call could overwrite sc.pairs under the first call's kernels); pinned staging, guarded by ev_tab.
template <typename T>
static pcd_status sift_upload_table(DevBuf<T>& dev, PinnedBuf<T>& pinned, const std::vector<T>& tab, hipStream_t s) {
  PCD_TRY(pinned.reserve(tab.size())); PCD_TRY(dev.reserve(tab.size()));
  std::memcpy(pinned.p, tab.data(), sizeof(T) * tab.size());
  PCD_HIP_TRY(hipMemcpyAsync(dev.p, pinned.p, sizeof(T) * tab.size(), hipMemcpyHostToDevice, s));
  return PCD_OK;
}
static pcd_status sift_batch_upload(SiftScratch& sc, hipStream_t s, const SiftBatchLayout& l, const SiftBatchPlan& pl) {
  PCD_TRY(sift_tables_free(sc));
  PCD_TRY(sift_upload_table(sc.pairs, sc.h_pairs, pl.pairs, s));
  PCD_TRY(sift_upload_table(sc.images, sc.h_images, l.images, s));
  if (!pl.guides.empty()) PCD_TRY(sift_upload_table(sc.guides, sc.h_guides, pl.guides, s));
  return sift_tables_sent(sc, s);
}

// sub-batch k of the plan: (records,) scores, finalize, cross check + compaction
static void sift_batch_launch(const SiftBatchArgs& a, const SiftBatchPlan& pl, size_t k, SiftScratch& sc, hipStream_t s) {
  const int p0 = pl.cut[k], np = pl.cut[k + 1] - pl.cut[k], nchunk = pl.nchunk[k];
  uint32_t mx1 = 0, mx2 = 0, mxsum = 0;
  for (int p = p0; p < p0 + np; ++p) {
    const SiftPairDev& pr = pl.pairs[p];
    mx1 = std::max(mx1, pr.n1); mx2 = std::max(mx2, pr.n2); mxsum = std::max(mxsum, pr.n1 + pr.n2);
  }
  if (mx1 && mx2) {
    const uint32_t mx = std::max(mx1, mx2);
    const dim3 grid(nchunk, (mx + kSiftStripe - 1) / kSiftStripe, 2 * np), block(64 * kSiftWaves);
    if (a.guides) {
      ScopedKernelTimer t("sift_guide_prep", s);
      hipLaunchKernelGGL(k_sift_guide_prep, dim3((unsigned)sift_tiles(mx), 2, np), dim3(kSiftTile), 0, s, sc.guides.p + p0,
                         sc.grec.p);
    }
    {
      ScopedKernelTimer t(a.guides ? "sift_guided_scores" : "sift_scores", s);
      if (a.guides)
        hipLaunchKernelGGL(k_sift_guided_batch, grid, block, 0, s, sc.xa.p, sc.cc.p, sc.pairs.p + p0, sc.part12.p,
                           sc.part21.p, nchunk, sc.guides.p + p0, sc.grec.p, a.th, a.tf);
      else
        hipLaunchKernelGGL(k_sift_scores_batch, grid, block, 0, s, sc.xa.p, sc.cc.p, sc.pairs.p + p0, sc.part12.p,
                           sc.part21.p, nchunk);
    }
    ScopedKernelTimer t("sift_finalize", s);
    hipLaunchKernelGGL(k_sift_finalize_batch, dim3(div_up((uint64_t)mxsum * 16, 256), 1, np), dim3(256), 0, s,
                       sc.pairs.p + p0, sc.part12.p, sc.part21.p, nchunk, a.max_ratio, a.max_distance, sc.m12.p, sc.m21.p);
  }
  ScopedKernelTimer t("sift_compact", s);
  hipLaunchKernelGGL(k_sift_keep_compact_batch, dim3(np), dim3(1024), 0, s, sc.pairs.p + p0, sc.m12.p, sc.m21.p,
                     a.cross_check, a.d_matches, a.d_counts + p0);
}

static pcd_status sift_batch_device(const SiftBatchArgs& a, SiftScratch& sc, hipStream_t s) {
  bool wide = false;
  PCD_TRY(sift_batch_validate(a, &wide));
  if (wide) return sift_batch_pairwise(a, sc, s);
  const SiftBatchLayout l = sift_batch_layout(a);
  PCD_REQUIRE(l.prows + kSiftStripe < (1ull << 32), "arena larger than 2^32 descriptors");
  const uint64_t budget_set = g_sift_batch_partials.load(std::memory_order_relaxed);
  const SiftBatchPlan pl = sift_batch_plan(a, l.images, g_sift_nchunk.load(std::memory_order_relaxed),
                                           budget_set ? (size_t)budget_set : kSiftBatchPartials);
  // (+ one stripe: a stripe's row fragments are read unconditionally)
  PCD_TRY(sc.xa.reserve((l.prows + kSiftStripe) * 128)); PCD_TRY(sc.cc.reserve(l.prows + kSiftStripe));
  PCD_TRY(sc.part12.reserve(pl.max12)); PCD_TRY(sc.part21.reserve(pl.max21));
  PCD_TRY(sc.m12.reserve(pl.maxm12)); PCD_TRY(sc.m21.reserve(pl.maxm21));
  if (a.guides) PCD_TRY(sc.grec.reserve(pl.maxrec));
  PCD_TRY(sift_batch_upload(sc, s, l, pl));
  if (l.max_tiles) {
    ScopedKernelTimer t("sift_prep", s);
    hipLaunchKernelGGL(k_sift_prep_images, dim3(l.max_tiles, a.n_images), dim3(256), 0, s, sc.images.p, sc.xa.p, sc.cc.p);
  }
  for (size_t k = 0; k + 1 < pl.cut.size(); ++k) sift_batch_launch(a, pl, k, sc, s);
  PCD_HIP_TRY(hipGetLastError());
  return PCD_OK;
}

// ---- the entry points' bodies: one per family, the guided and the unguided exported function call the same one -----
// Argument checks in one order everywhere: sizes and the pointers every call needs, the device ordinal (before
// g_sift[device] is indexed), require_device, no capturing stream, the empty input's early return, then the pointers a
// non-empty input needs.

// pair on the device; guided iff H || F (then d_loc1 / d_loc2 are needed), otherwise the unguided result
static pcd_status sift_match_device(int device, const uint8_t* d_desc1, const float* d_loc1, int n1,
                                    const uint8_t* d_desc2, const float* d_loc2, int n2, const float* H, const float* F,
                                    float th, float tf, float max_ratio, float max_distance, int cross_check,
                                    int32_t* d_m12, int32_t* d_m21, uint32_t* d_matches, int32_t* d_num_matches,
                                    hipStream_t s) {
  return pcd::guard([&]() -> pcd_status {
  PCD_REQUIRE(n1 >= 0 && n2 >= 0 && d_num_matches, "sizes / count pointer");
  PCD_REQUIRE(device >= 0 && device < 64, "device ordinal");
  PCD_TRY(require_device(device));
  PCD_REFUSE_CAPTURE(s);
  if (n1 == 0 || n2 == 0) {   // MatchSiftFeaturesCPU with an empty set: no matches (sift_test.cc:311-318, :462-474)
    PCD_HIP_TRY(hipMemsetAsync(d_num_matches, 0, sizeof(int32_t), s));
    if (n1 && d_m12) PCD_HIP_TRY(hipMemsetAsync(d_m12, 0xFF, sizeof(int32_t) * n1, s));
    if (n2 && d_m21) PCD_HIP_TRY(hipMemsetAsync(d_m21, 0xFF, sizeof(int32_t) * n2, s));
    return PCD_OK;
  }
  const int mode = (H ? kSiftGuideH : 0) | (F ? kSiftGuideF : 0);
  PCD_REQUIRE(d_desc1 && d_desc2 && d_m12 && d_m21 && d_matches && (!mode || (d_loc1 && d_loc2)), "null pointer");
  return sift_use_scratch(device, s, [&](SiftScratch& sc) -> pcd_status {
    if (mode) PCD_TRY(sift_upload_guide(sc, s, d_loc1, n1, d_loc2, n2, mode, H, F));
    return sift_device(d_desc1, n1, d_desc2, n2, max_ratio, max_distance, cross_check, d_m12, d_m21, d_matches,
                       d_num_matches, sc, s, mode ? sc.guides.p : nullptr, th, tf);
  });
  });
}

// the end of a host pair call: the count comes down, is clipped to the caller's capacity, that many matches follow
static pcd_status sift_download_matches(const int32_t* d_count, const uint32_t* d_matches, int capacity, hipStream_t s,
                                        uint32_t* matches, int32_t* num_matches) {
  int cnt = 0;
  PCD_HIP_TRY(hipMemcpyAsync(&cnt, d_count, sizeof(int), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipStreamSynchronize(s));
  cnt = std::min(cnt, capacity);
  if (cnt) PCD_HIP_TRY(hipMemcpy(matches, d_matches, 2 * (size_t)cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
  *num_matches = cnt;
  return PCD_OK;
}

// pair from host memory (`matches` holds n1 entries)
static pcd_status sift_match_host(int device, const uint8_t* desc1, const float* loc1, int n1, const uint8_t* desc2,
                                  const float* loc2, int n2, const float* H, const float* F, float th, float tf,
                                  float max_ratio, float max_distance, int cross_check, uint32_t* matches,
                                  int32_t* num_matches) {
  return pcd::guard([&]() -> pcd_status {
  PCD_REQUIRE(num_matches && n1 >= 0 && n2 >= 0, "sizes / count pointer");
  *num_matches = 0;
  PCD_REQUIRE(device >= 0 && device < 64, "device ordinal");
  PCD_TRY(require_device(device));
  if (n1 == 0 || n2 == 0) return PCD_OK;
  const bool guided = H || F;
  PCD_REQUIRE(desc1 && desc2 && matches && (!guided || (loc1 && loc2)), "null pointer");
  hipStream_t s = nullptr;
  // the whole host call: it owns the scratch's d1 / d2 / m12 / matches until it has synchronised
  return sift_use_scratch(device, s, [&](SiftScratch& sc) -> pcd_status {
    PCD_TRY(sc.d1.reserve((size_t)n1 * 128)); PCD_TRY(sc.d2.reserve((size_t)n2 * 128));
    PCD_TRY(sc.m12.reserve(n1)); PCD_TRY(sc.m21.reserve(n2)); PCD_TRY(sc.matches.reserve(2 * (size_t)n1));
    PCD_TRY(sc.count.reserve(1));
    PCD_HIP_TRY(hipMemcpyAsync(sc.d1.p, desc1, (size_t)n1 * 128, hipMemcpyHostToDevice, s));
    PCD_HIP_TRY(hipMemcpyAsync(sc.d2.p, desc2, (size_t)n2 * 128, hipMemcpyHostToDevice, s));
    if (guided) {
      PCD_TRY(sc.loc1.reserve(2 * (size_t)n1)); PCD_TRY(sc.loc2.reserve(2 * (size_t)n2));
      PCD_HIP_TRY(hipMemcpyAsync(sc.loc1.p, loc1, 2 * sizeof(float) * (size_t)n1, hipMemcpyHostToDevice, s));
      PCD_HIP_TRY(hipMemcpyAsync(sc.loc2.p, loc2, 2 * sizeof(float) * (size_t)n2, hipMemcpyHostToDevice, s));
    }
    PCD_TRY(sift_match_device(device, sc.d1.p, sc.loc1.p, n1, sc.d2.p, sc.loc2.p, n2, H, F, th, tf, max_ratio,
                              max_distance, cross_check, sc.m12.p, sc.m21.p, sc.matches.p, sc.count.p, s));
    return sift_download_matches(sc.count.p, sc.matches.p, n1, s, matches, num_matches);
  });
  });
}

// batch on the device (guided: `guides` is needed, and d_locs beside a non-empty arena)
static pcd_status sift_match_batch_device(int device, bool guided, const SiftBatchArgs& a, hipStream_t s) {
  return pcd::guard([&]() -> pcd_status {
  PCD_REQUIRE(a.n_images >= 0 && a.n_pairs >= 0 && a.first_row, "sizes / first_row");
  PCD_REQUIRE(device >= 0 && device < 64, "device ordinal");
  PCD_TRY(require_device(device));
  PCD_REFUSE_CAPTURE(s);
  if (a.n_pairs == 0) return PCD_OK;
  PCD_REQUIRE(a.pair_ids && a.match_offset && a.d_counts && a.d_matches && (!guided || a.guides), "null pointer");
  PCD_REQUIRE(a.first_row[a.n_images] == 0 || (a.d_arena && (!guided || a.d_locs)), "null arena / locations");
  for (int p = 0; guided && p < a.n_pairs; ++p)
    PCD_REQUIRE(a.guides[p].mode >= PCD_SIFT_GUIDE_NONE && a.guides[p].mode <= PCD_SIFT_GUIDE_HF, "guide mode");
  return sift_use_scratch(device, s, [&](SiftScratch& sc) { return sift_batch_device(a, sc, s); });
  });
}

// batch from host memory (locs / guides: the guided one)
static pcd_status sift_match_batch_host(int device, const uint8_t* arena, const float* locs, const uint64_t* first_row,
                                        int n_images, const uint32_t* pairs, int n_pairs, const pcd_sift_guide* guides,
                                        float th, float tf, float max_ratio, float max_distance, int cross_check,
                                        uint32_t* matches, uint64_t matches_capacity, uint64_t* list_offset) {
  return pcd::guard([&]() -> pcd_status {
  PCD_REQUIRE(n_images >= 0 && n_pairs >= 0 && first_row && list_offset, "sizes / first_row / list_offset");
  list_offset[0] = 0;
  PCD_REQUIRE(device >= 0 && device < 64, "device ordinal");
  PCD_TRY(require_device(device));
  if (n_pairs == 0) return PCD_OK;
  PCD_REQUIRE(pairs, "null pair list");
  const uint64_t rows = first_row[n_images];
  PCD_REQUIRE(rows == 0 || (arena && (!guides || locs)), "null arena / locations");
  // the whole host call: arena / matches / counts / dense are the device's shared scratch
  return sift_use_scratch(device, nullptr, [&](SiftScratch& sc) -> pcd_status {
    hipStream_t s = nullptr;
    // worst-case list of pair p: one match per descriptor of its first image
    std::vector<uint64_t> off((size_t)n_pairs + 1, 0);
    for (int p = 0; p < n_pairs; ++p) {
      PCD_REQUIRE(pairs[2 * p] < (uint32_t)n_images && pairs[2 * p + 1] < (uint32_t)n_images, "pair names an image outside the arena");
      off[p + 1] = off[p] + (first_row[pairs[2 * p] + 1] - first_row[pairs[2 * p]]);
    }
    PCD_TRY(sc.arena.reserve(rows * 128)); PCD_TRY(sc.matches.reserve(2 * off[n_pairs] + 2));
    PCD_TRY(sc.counts.reserve(n_pairs)); PCD_TRY(sc.dense_off.reserve(2 * ((size_t)n_pairs + 1)));
    if (rows) PCD_HIP_TRY(hipMemcpy(sc.arena.p, arena, rows * 128, hipMemcpyHostToDevice));
    if (guides) {
      PCD_TRY(sc.locs.reserve(2 * rows));
      if (rows) PCD_HIP_TRY(hipMemcpy(sc.locs.p, locs, rows * 2 * sizeof(float), hipMemcpyHostToDevice));
    }
    PCD_TRY(sift_match_batch_device(device, guides != nullptr,
                                    SiftBatchArgs{sc.arena.p, sc.locs.p, first_row, n_images, pairs, n_pairs, guides, th, tf,
                                                  max_ratio, max_distance, cross_check, sc.matches.p, off.data(),
                                                  sc.counts.p},
                                    s));
    std::vector<int> cnt((size_t)n_pairs);
    PCD_HIP_TRY(hipMemcpy(cnt.data(), sc.counts.p, sizeof(int) * (size_t)n_pairs, hipMemcpyDeviceToHost));
    for (int p = 0; p < n_pairs; ++p) list_offset[p + 1] = list_offset[p] + (uint64_t)cnt[p];
    const uint64_t total = list_offset[n_pairs];
    if (total > matches_capacity) {
      set_error("pcd_sift_match_batch: %llu matches, capacity %llu", (unsigned long long)total, (unsigned long long)matches_capacity);
      return PCD_ERR_INVALID;
    }
    if (total == 0) return PCD_OK;
    PCD_REQUIRE(matches, "null match buffer");
    // pack the lists back to back on the device: one download of exactly the matches
    PCD_TRY(sc.dense.reserve(2 * total));
    const size_t np1 = (size_t)n_pairs + 1;
    PCD_HIP_TRY(hipMemcpy(sc.dense_off.p, list_offset, sizeof(uint64_t) * np1, hipMemcpyHostToDevice));
    PCD_HIP_TRY(hipMemcpy(sc.dense_off.p + np1, off.data(), sizeof(uint64_t) * np1, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sift_pack_lists, dim3(n_pairs), dim3(256), 0, s, sc.dense_off.p + np1, sc.counts.p,
                       sc.dense_off.p, sc.matches.p, sc.dense.p);
    PCD_HIP_TRY(hipGetLastError());
    PCD_HIP_TRY(hipMemcpy(matches, sc.dense.p, 2 * total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PCD_OK;
  });
  });
}
}  // namespace pcd

// ---- matcher handle: two descriptor slots resident on the device (SiftMatchGPU's usage pattern) ----
struct pcd_sift_matcher {
  int device = 0;
  int max_sift = 4096;
  int n[2] = {0, 0};
  pcd::DevBuf<uint8_t> d[2];
  pcd::DevBuf<float> loc[2];
  bool loc_ok[2] = {false, false};   // the slot's locations belong to its current descriptors
  pcd::DevBuf<int32_t> m12, m21, count;
  pcd::DevBuf<uint32_t> matches;
};

namespace pcd {
// GetSiftMatch / GetGuidedSiftMatch (guided iff H || F): at most max_match matches, in ascending index of set 0
static pcd_status sift_matcher_match(pcd_sift_matcher* m, int max_match, uint32_t* matches, const float* H,
                                     const float* F, float distmax, float ratiomax, float hdistmax, float fdistmax,
                                     int mutual_best_match, int32_t* num_matches) {
  PCD_REQUIRE(m && num_matches && max_match >= 0, "null pointer");
  *num_matches = 0;
  const int n1 = m->n[0], n2 = m->n[1];
  if (n1 == 0 || n2 == 0 || max_match == 0) return PCD_OK;
  if ((H || F) && (!m->loc_ok[0] || !m->loc_ok[1])) {
    set_error("pcd_sift_matcher_match_guided: a slot's descriptors were set after its locations (or none were set)");
    return PCD_ERR_INVALID;
  }
  PCD_REQUIRE(matches, "null match buffer");
  PCD_HIP_TRY(hipSetDevice(m->device));
  PCD_TRY(m->m12.reserve(n1)); PCD_TRY(m->m21.reserve(n2)); PCD_TRY(m->matches.reserve(2 * (size_t)n1));
  PCD_TRY(m->count.reserve(1));
  hipStream_t s = nullptr;
  PCD_TRY(sift_match_device(m->device, m->d[0].p, m->loc[0].p, n1, m->d[1].p, m->loc[1].p, n2, H, F, hdistmax, fdistmax,
                            ratiomax, distmax, mutual_best_match, m->m12.p, m->m21.p, m->matches.p, m->count.p, s));
  return sift_download_matches(m->count.p, m->matches.p, max_match, s, matches, num_matches);
}
}  // namespace pcd

using namespace pcd;

extern "C" {

/* tuning hook (tests, fuzzing; not part of the stable ABI): force the number of column chunks of a stripe walk and the
 * partial results per sub-batch of pcd_sift_match_batch, counted in int4 elements (16-byte units); 0 = the library's
 * choice */
pcd_status pcd_sift_set_tuning(int nchunk, uint64_t batch_partials_int4) {
  PCD_REQUIRE(nchunk >= 0, "nchunk");
  g_sift_nchunk.store(nchunk, std::memory_order_relaxed);
  g_sift_batch_partials.store(batch_partials_int4, std::memory_order_relaxed);
  return PCD_OK;
}

pcd_status pcd_sift_match_device(int device, const uint8_t* d_desc1, int n1, const uint8_t* d_desc2, int n2,
                                 float max_ratio, float max_distance, int cross_check, int32_t* d_m12,
                                 int32_t* d_m21, uint32_t* d_matches, int32_t* d_num_matches, void* stream) {
  return sift_match_device(device, d_desc1, nullptr, n1, d_desc2, nullptr, n2, nullptr, nullptr, 0.f, 0.f, max_ratio,
                           max_distance, cross_check, d_m12, d_m21, d_matches, d_num_matches, (hipStream_t)stream);
}

pcd_status pcd_sift_match(int device, const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float max_ratio,
                          float max_distance, int cross_check, uint32_t* matches, int32_t* num_matches) {
  return sift_match_host(device, desc1, nullptr, n1, desc2, nullptr, n2, nullptr, nullptr, 0.f, 0.f, max_ratio,
                         max_distance, cross_check, matches, num_matches);
}

pcd_status pcd_sift_match_batch_device(int device, const uint8_t* d_arena, const uint64_t* first_row, int n_images,
                                       const uint32_t* pairs, int n_pairs, float max_ratio, float max_distance,
                                       int cross_check, uint32_t* d_matches, const uint64_t* match_offset,
                                       int32_t* d_counts, void* stream) {
  return sift_match_batch_device(device, false,
                                 SiftBatchArgs{d_arena, nullptr, first_row, n_images, pairs, n_pairs, nullptr, 0.f, 0.f,
                                               max_ratio, max_distance, cross_check, d_matches, match_offset, d_counts},
                                 (hipStream_t)stream);
}

pcd_status pcd_sift_match_batch(int device, const uint8_t* arena, const uint64_t* first_row, int n_images,
                                const uint32_t* pairs, int n_pairs, float max_ratio, float max_distance, int cross_check,
                                uint32_t* matches, uint64_t matches_capacity, uint64_t* list_offset) {
  return sift_match_batch_host(device, arena, nullptr, first_row, n_images, pairs, n_pairs, nullptr, 0.f, 0.f, max_ratio,
                               max_distance, cross_check, matches, matches_capacity, list_offset);
}

// ---- guided matching (feature/sift.cc:1092-1162, lib/SiftGPU/SiftGPU.h:331-352); neither matrix: the unguided result
pcd_status pcd_sift_match_guided_device(int device, const uint8_t* d_desc1, const float* d_loc1, int n1,
                                        const uint8_t* d_desc2, const float* d_loc2, int n2, const float* H,
                                        const float* F, float h_max_residual, float f_max_residual, float max_ratio,
                                        float max_distance, int cross_check, int32_t* d_m12, int32_t* d_m21,
                                        uint32_t* d_matches, int32_t* d_num_matches, void* stream) {
  return sift_match_device(device, d_desc1, d_loc1, n1, d_desc2, d_loc2, n2, H, F, h_max_residual, f_max_residual,
                           max_ratio, max_distance, cross_check, d_m12, d_m21, d_matches, d_num_matches,
                           (hipStream_t)stream);
}

pcd_status pcd_sift_match_guided(int device, const uint8_t* desc1, const float* loc1, int n1, const uint8_t* desc2,
                                 const float* loc2, int n2, const float* H, const float* F, float h_max_residual,
                                 float f_max_residual, float max_ratio, float max_distance, int cross_check,
                                 uint32_t* matches, int32_t* num_matches) {
  return sift_match_host(device, desc1, loc1, n1, desc2, loc2, n2, H, F, h_max_residual, f_max_residual, max_ratio,
                         max_distance, cross_check, matches, num_matches);
}

pcd_status pcd_sift_match_guided_batch_device(int device, const uint8_t* d_arena, const float* d_locs,
                                              const uint64_t* first_row, int n_images, const uint32_t* pairs,
                                              int n_pairs, const pcd_sift_guide* guides, float h_max_residual,
                                              float f_max_residual, float max_ratio, float max_distance,
                                              int cross_check, uint32_t* d_matches, const uint64_t* match_offset,
                                              int32_t* d_counts, void* stream) {
  return sift_match_batch_device(device, true,
                                 SiftBatchArgs{d_arena, d_locs, first_row, n_images, pairs, n_pairs, guides,
                                               h_max_residual, f_max_residual, max_ratio, max_distance, cross_check,
                                               d_matches, match_offset, d_counts},
                                 (hipStream_t)stream);
}

pcd_status pcd_sift_match_guided_batch(int device, const uint8_t* arena, const float* locs, const uint64_t* first_row,
                                       int n_images, const uint32_t* pairs, int n_pairs, const pcd_sift_guide* guides,
                                       float h_max_residual, float f_max_residual, float max_ratio, float max_distance,
                                       int cross_check, uint32_t* matches, uint64_t matches_capacity,
                                       uint64_t* list_offset) {
  if (n_pairs > 0 && !guides) return (set_error("pcd_sift_match_guided_batch: null guides"), PCD_ERR_INVALID);
  return sift_match_batch_host(device, arena, locs, first_row, n_images, pairs, n_pairs, guides, h_max_residual,
                               f_max_residual, max_ratio, max_distance, cross_check, matches, matches_capacity,
                               list_offset);
}

pcd_status pcd_sift_matcher_create(int device, int max_sift, pcd_sift_matcher** out) {
  return pcd::guard([&]() -> pcd_status {
  PCD_REQUIRE(out && max_sift > 0, "null pointer / max_sift");
  PCD_REQUIRE(device >= 0 && device < 64, "device ordinal");
  PCD_TRY(require_device(device));
  pcd_sift_matcher* m = new pcd_sift_matcher();
  m->device = device;
  m->max_sift = max_sift;
  *out = m;
  return PCD_OK;
  });
}

void pcd_sift_matcher_destroy(pcd_sift_matcher* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;
}

pcd_status pcd_sift_matcher_set_max_sift(pcd_sift_matcher* m, int max_sift) {
  PCD_REQUIRE(m && max_sift > 0, "null pointer / max_sift");
  m->max_sift = max_sift;
  return PCD_OK;
}

// SiftMatchGPU::SetDescriptors(index, num, const unsigned char*): num is clipped to max_sift
pcd_status pcd_sift_matcher_set_descriptors(pcd_sift_matcher* m, int index, int num, const uint8_t* desc) {
  PCD_REQUIRE(m && (index == 0 || index == 1) && num >= 0, "index must be 0 or 1");
  PCD_REQUIRE(num == 0 || desc, "null descriptors");
  PCD_HIP_TRY(hipSetDevice(m->device));
  if (num > m->max_sift) num = m->max_sift;
  m->n[index] = num;
  m->loc_ok[index] = false;
  if (num) {
    PCD_TRY(m->d[index].reserve((size_t)num * 128));
    PCD_HIP_TRY(hipMemcpy(m->d[index].p, desc, (size_t)num * 128, hipMemcpyHostToDevice));
  }
  return PCD_OK;
}

// SiftMatchGPU::SetFeautreLocation(index, locations, gap): n[index] (x, y) pairs at a stride of 2 + gap floats
pcd_status pcd_sift_matcher_set_locations(pcd_sift_matcher* m, int index, const float* loc, int gap) {
  PCD_REQUIRE(m && (index == 0 || index == 1) && gap >= 0, "index must be 0 or 1, gap >= 0");
  const int n = m->n[index];
  PCD_REQUIRE(n == 0 || loc, "null locations");
  PCD_HIP_TRY(hipSetDevice(m->device));
  if (n) {
    std::vector<float> xy(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
      xy[2 * (size_t)i] = loc[(size_t)i * (2 + gap)];
      xy[2 * (size_t)i + 1] = loc[(size_t)i * (2 + gap) + 1];
    }
    PCD_TRY(m->loc[index].reserve(2 * (size_t)n));
    PCD_HIP_TRY(hipMemcpy(m->loc[index].p, xy.data(), xy.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  m->loc_ok[index] = true;
  return PCD_OK;
}

// SiftMatchGPU::GetSiftMatch: number of matches written (at most max_match, in ascending index of set 0)
pcd_status pcd_sift_matcher_match(pcd_sift_matcher* m, int max_match, uint32_t* matches, float distmax, float ratiomax,
                                  int mutual_best_match, int32_t* num_matches) {
  return sift_matcher_match(m, max_match, matches, nullptr, nullptr, distmax, ratiomax, 0.f, 0.f, mutual_best_match,
                            num_matches);
}

// SiftMatchGPU::GetGuidedSiftMatch (SiftGPU.h:343-352): hdistmax / fdistmax are the squared residual thresholds
pcd_status pcd_sift_matcher_match_guided(pcd_sift_matcher* m, int max_match, uint32_t* matches, const float* H,
                                         const float* F, float distmax, float ratiomax, float hdistmax, float fdistmax,
                                         int mutual_best_match, int32_t* num_matches) {
  return sift_matcher_match(m, max_match, matches, H, F, distmax, ratiomax, hdistmax, fdistmax, mutual_best_match,
                            num_matches);
}

}  // extern "C"

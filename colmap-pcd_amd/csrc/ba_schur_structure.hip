// ba_schur_structure.hip -- the co-visibility structure of the point elimination, built on the device:
// everything in SchurStructure (ba_schur_structure.h) from the handle's own image-major arrays and masks.  e is the
// image-major position of an observation; it is *eliminated* when its image has a slot and its point is not constant.
// The passes, all on the caller's stream:
//   k_st_slot_flag, exclusive_sum, k_st_slots   variable-pose images -> slots in ascending image index
//   k_st_positions                              per e: obs_pos, iota, its slot (-1: not eliminated), its sort key
//   sort_pairs                                  e stably by point (P for the rest): every point's list, ascending e
//   k_st_point_lists                            the slot of every list entry; the bounds of the lists
//   k_st_count, exclusive_sum x 2 (64-bit)      slots ascend along a list, so the partners of e in its own slot are a
//                                               run and those in later slots the suffix behind it: two binary searches
//                                               give the diagonal and pair entries of e; the scans their offsets
//   -- synchronisation 1: ns and the two 64-bit totals, which size the entry buffers (and decide the 32-bit guard)
//   k_st_expand<false>                          diagonal entries, written in place: ascending e is block order
//   k_st_expand<true>, sort_pairs               pair entries with the key (i << bits | j), stably to block order
//   k_st_head_flag, exclusive_sum               1 where the key changes -> the index of every pair block
//   -- synchronisation 2: npairs, which sizes pair_ij, blk_start and the row lists
//   k_st_diag_starts, k_st_blocks               blk_start; the sorted entries unpacked; pair_ij
//   sort_pairs, k_st_row_count, exclusive_sum, k_st_row_fill   the pairs stably by j -> the row lists of the product
// The expansion is balanced over the entries, not the observations: a workgroup takes kExpTile consecutive output
// entries, finds its first and last row with a search of the offsets, stages that segment of the offsets in LDS and lets
// every thread find the rows of its four consecutive entries there, so a track of any length costs what its entries
// cost and the stores are 128-bit and coalesced.  No atomics; nothing depends on the launch geometry; a repeated build
// gives the same bytes.
#include <chrono>

#include "ba_schur_structure.h"
#include "prim.h"

namespace pcd {

constexpr uint32_t kExpTile = 1024;     // output entries of a workgroup: 256 threads x 4 consecutive entries
constexpr uint32_t kExpWindow = 2048;   // offsets staged in LDS (16 KiB); a tile over more rows searches global memory
constexpr uint64_t kLayoutLimit = 0xFFFFFFF0ull;

// flag[i] = 1: image i gets a slot.  Thread I writes the closing 0 (the scan's last value is the count).
__global__ __launch_bounds__(256) void k_st_slot_flag(uint32_t I, const uint8_t* __restrict__ cpose,
                                                      uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > I) return;
  flag[i] = (i < I && !(cpose && cpose[i])) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_st_slots(uint32_t I, const uint32_t* __restrict__ flag,
                                                  const uint32_t* __restrict__ scan, int* __restrict__ img_slot,
                                                  int* __restrict__ slot_img) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= I) return;
  img_slot[i] = flag[i] ? (int)scan[i] : -1;
  if (flag[i]) slot_img[scan[i]] = (int)i;
}

__global__ __launch_bounds__(256) void k_st_positions(uint32_t O, uint32_t P, const uint32_t* __restrict__ img_obs,
                                                      const int* __restrict__ obs_image, const int* __restrict__ img_pt,
                                                      const uint8_t* __restrict__ cpt, const int* __restrict__ img_slot,
                                                      uint32_t* __restrict__ obs_pos, uint32_t* __restrict__ iota,
                                                      int* __restrict__ eslot, uint32_t* __restrict__ key) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= O) return;
  const uint32_t o = img_obs[e];
  const int p = img_pt[e];
  const int s = (cpt && cpt[p]) ? -1 : img_slot[obs_image[o]];
  obs_pos[o] = e; iota[e] = e; eslot[e] = s;
  key[e] = s >= 0 ? (uint32_t)p : P;
}

// first index in [lo, hi) whose value is >= v (kUpper: > v); hi if none
template <bool kUpper, typename T>
__device__ inline uint32_t st_bound(const T* __restrict__ a, uint32_t lo, uint32_t hi, T v, uint32_t stride = 1) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const T x = a[(size_t)mid * stride];
    if (kUpper ? x <= v : x < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_st_point_lists(uint32_t O, uint32_t P, const uint32_t* __restrict__ skey,
                                                        const uint32_t* __restrict__ pli, const int* __restrict__ eslot,
                                                        int* __restrict__ sslot, uint32_t* __restrict__ pst) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < O) sslot[k] = eslot[pli[k]];
  if (k <= P) pst[k] = st_bound<false>(skey, 0u, O, k);
}

// thread O writes the closing zeros
__global__ __launch_bounds__(256) void k_st_count(uint32_t O, const int* __restrict__ eslot, const int* __restrict__ img_pt,
                                                  const uint32_t* __restrict__ pst, const int* __restrict__ sslot,
                                                  uint32_t* __restrict__ dbeg, uint64_t* __restrict__ dcnt,
                                                  uint64_t* __restrict__ pcnt) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e > O) return;
  uint32_t b = 0, nd = 0, np = 0;
  const int s = e < O ? eslot[e] : -1;
  if (s >= 0) {
    const uint32_t lo = pst[img_pt[e]], hi = pst[img_pt[e] + 1];
    b = st_bound<false>(sslot, lo, hi, s);
    const uint32_t end = st_bound<true>(sslot, b, hi, s);
    nd = end - b; np = hi - end;
  }
  if (e < O) dbeg[e] = b;
  dcnt[e] = nd; pcnt[e] = np;
}

// the row r in [lo, hi) with off[r] <= t < off[r + 1], given off[lo] <= t < off[hi]
template <typename Ptr>
__device__ inline uint32_t st_row_of(Ptr off, uint32_t lo, uint32_t hi, uint64_t t) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename T>
__device__ inline void st_store4(T* __restrict__ p, const T (&v)[4]) {   // p is 4 * sizeof(T) aligned
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
    *reinterpret_cast<ulonglong2*>(p) = make_ulonglong2(v[0], v[1]);
    *reinterpret_cast<ulonglong2*>(p + 2) = make_ulonglong2(v[2], v[3]);
  }
}

// Output entry t of row e (off[e] <= t < off[e + 1]) is (e, pli[first(e) + t - off[e]]): first = dbeg for the diagonal
// entries, dbeg + dcnt (the suffix of later slots) for the pair entries.  kPair: key and packed entry for the sort,
// else ent_a / ent_b directly.  Grid: div_up(total, kExpTile).
template <bool kPair, typename K>
__global__ __launch_bounds__(256) void k_st_expand(uint32_t O, uint64_t total, const uint64_t* __restrict__ off,
                                                   const uint32_t* __restrict__ dbeg, const uint64_t* __restrict__ dcnt,
                                                   const int* __restrict__ eslot, const uint32_t* __restrict__ pli,
                                                   const int* __restrict__ sslot, unsigned jbits,
                                                   uint32_t* __restrict__ out_a, uint32_t* __restrict__ out_b,
                                                   K* __restrict__ out_key, uint64_t* __restrict__ out_val) {
  __shared__ uint64_t s_off[kExpWindow];
  __shared__ uint32_t s_row[2];
  const uint64_t t0 = (uint64_t)blockIdx.x * kExpTile;
  const uint64_t t1 = t0 + kExpTile < total ? t0 + kExpTile : total;
  if (threadIdx.x < 2) s_row[threadIdx.x] = st_row_of(off, 0u, O, threadIdx.x ? t1 - 1 : t0);
  __syncthreads();
  const uint32_t e0 = s_row[0], nrow = s_row[1] - e0 + 1;   // rows e0 .. e0 + nrow - 1; off[e0 + nrow] > t1 - 1 closes them
  const bool staged = nrow < kExpWindow;
  if (staged)
    for (uint32_t i = threadIdx.x; i <= nrow; i += 256) s_off[i] = off[e0 + i];
  __syncthreads();
  const uint64_t tb = t0 + 4u * threadIdx.x;
  if (tb >= t1) return;
  uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0}; K key[4] = {0, 0, 0, 0}; uint64_t val[4] = {0, 0, 0, 0};
  uint32_t r = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint64_t t = tb + c;
    if (t >= t1) break;
    uint64_t first;
    if (staged) { r = st_row_of(s_off, r, nrow, t); first = s_off[r]; }
    else { r = st_row_of(off + e0, r, nrow, t); first = off[e0 + r]; }
    const uint32_t e = e0 + r;
    const uint32_t k = dbeg[e] + (kPair ? (uint32_t)dcnt[e] : 0u) + (uint32_t)(t - first);
    a[c] = e; b[c] = pli[k];
    if (kPair) { key[c] = ((K)(uint32_t)eslot[e] << jbits) | (K)(uint32_t)sslot[k]; val[c] = ((uint64_t)e << 32) | b[c]; }
  }
  if (tb + 4 <= t1) {
    if (kPair) { st_store4(out_key + tb, key); st_store4(out_val + tb, val); }
    else { st_store4(out_a + tb, a); st_store4(out_b + tb, b); }
  } else {
    for (int c = 0; tb + c < t1; ++c) {
      if (kPair) { out_key[tb + c] = key[c]; out_val[tb + c] = val[c]; }
      else { out_a[tb + c] = a[c]; out_b[tb + c] = b[c]; }
    }
  }
}

// flag[t] = 1: sorted pair entry t opens a block.  Thread n writes the closing 0.
template <typename K>
__global__ __launch_bounds__(256) void k_st_head_flag(uint32_t n, const K* __restrict__ skey, uint32_t* __restrict__ flag) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t > n) return;
  flag[t] = (t < n && (t == 0 || skey[t] != skey[t - 1])) ? 1u : 0u;
}

// diagonal block s opens at the first diagonal entry of its image; thread ns: the first pair block (or the end)
__global__ __launch_bounds__(256) void k_st_diag_starts(uint32_t ns, uint32_t ndiag, const int* __restrict__ slot_img,
                                                        const uint32_t* __restrict__ img_obs_start,
                                                        const uint64_t* __restrict__ doff, uint32_t* __restrict__ blk_start) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s > ns) return;
  blk_start[s] = s < ns ? (uint32_t)doff[img_obs_start[slot_img[s]]] : ndiag;
}

// the sorted pair entries behind the diagonal ones; at a head: the block's bound, its slot pair, (j, q) for the row sort.
// Thread n closes blk_start.
template <typename K>
__global__ __launch_bounds__(256) void k_st_blocks(uint32_t n, uint32_t ns, uint32_t ndiag, unsigned jbits,
                                                   const K* __restrict__ skey, const uint64_t* __restrict__ sval,
                                                   const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                   uint32_t* __restrict__ ent_a, uint32_t* __restrict__ ent_b,
                                                   uint32_t* __restrict__ pair_ij, uint32_t* __restrict__ blk_start,
                                                   uint32_t* __restrict__ pj, uint32_t* __restrict__ pq) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t > n) return;
  if (t == n) { blk_start[ns + pos[n]] = ndiag + n; return; }
  const uint64_t v = sval[t];
  ent_a[ndiag + t] = (uint32_t)(v >> 32); ent_b[ndiag + t] = (uint32_t)v;
  if (!flag[t]) return;
  const uint32_t q = pos[t]; const K key = skey[t];
  const uint32_t i = (uint32_t)(key >> jbits), j = (uint32_t)(key & (((K)1 << jbits) - 1));
  pair_ij[2 * (size_t)q] = i; pair_ij[2 * (size_t)q + 1] = j;
  blk_start[ns + q] = ndiag + t;
  pj[q] = j; pq[q] = q;
}

// per slot s (thread ns: the closing values): the first pair with i >= s, the first of the j-sorted pairs with j >= s,
// and the length of row s: the (k, s) blocks, the diagonal, the (s, j) blocks
__global__ __launch_bounds__(256) void k_st_row_count(uint32_t ns, uint32_t npairs, const uint32_t* __restrict__ pair_ij,
                                                      const uint32_t* __restrict__ pj_sorted, uint32_t* __restrict__ ilo,
                                                      uint32_t* __restrict__ jlo, uint32_t* __restrict__ rcnt) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s > ns) return;
  const uint32_t i0 = st_bound<false>(pair_ij, 0u, npairs, s, 2), j0 = st_bound<false>(pj_sorted, 0u, npairs, s);
  ilo[s] = i0; jlo[s] = j0;
  if (s == ns) { rcnt[s] = 0; return; }
  const uint32_t i1 = st_bound<false>(pair_ij, i0, npairs, s + 1, 2), j1 = st_bound<false>(pj_sorted, j0, npairs, s + 1);
  rcnt[s] = (j1 - j0) + 1u + (i1 - i0);
}

__global__ __launch_bounds__(256) void k_st_row_fill(uint32_t ns, uint32_t npairs, const uint32_t* __restrict__ pair_ij,
                                                     const uint32_t* __restrict__ pj_sorted,
                                                     const uint32_t* __restrict__ pq_sorted, const uint32_t* __restrict__ ilo,
                                                     const uint32_t* __restrict__ jlo, const uint32_t* __restrict__ row_start,
                                                     uint32_t* __restrict__ row_blk, uint32_t* __restrict__ row_col) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < npairs) {
    // the t-th of the j-sorted pairs: block (k, s), transposed, in row s
    const uint32_t s = pj_sorted[t], q = pq_sorted[t];
    uint32_t r = row_start[s] + (t - jlo[s]);
    row_blk[r] = ns + q; row_col[r] = (pair_ij[2 * (size_t)q] << 1) | 1u;
    // pair t = (i, j) in row i, behind the transposed blocks and the diagonal
    const uint32_t i = pair_ij[2 * (size_t)t];
    r = row_start[i] + (jlo[i + 1] - jlo[i]) + 1u + (t - ilo[i]);
    row_blk[r] = ns + t; row_col[r] = pair_ij[2 * (size_t)t + 1] << 1;
  }
  if (t < ns) {
    const uint32_t r = row_start[t] + (jlo[t + 1] - jlo[t]);
    row_blk[r] = t; row_col[r] = t << 1;
  }
}

// smallest number of bits that holds every value <= v
static unsigned bits_for(uint64_t v) {
  unsigned bits = 0;
  while (bits < 64 && (v >> bits)) ++bits;
  return bits;
}

static dim3 grid_of(uint64_t n) { return dim3(std::max(1u, div_up(n, 256))); }

// the pair entries: expansion, sort to block order, block heads.  Leaves the pair count in h_count[3] behind the second
// synchronisation and the sorted keys / entries in pkey_out / pval_out.
template <typename K>
static pcd_status st_pair_entries(SchurStructure& T, uint32_t O, uint32_t npe, unsigned jbits, hipStream_t s, int* syncs) {
  SchurBuildScratch& W = T.tmp;
  PCD_TRY(W.pkey_in.reserve(((size_t)npe + 1) * sizeof(K))); PCD_TRY(W.pkey_out.reserve(((size_t)npe + 1) * sizeof(K)));
  PCD_TRY(W.pval_in.reserve((size_t)npe + 1)); PCD_TRY(W.pval_out.reserve((size_t)npe + 1));
  K* key_in = reinterpret_cast<K*>(W.pkey_in.p); K* key_out = reinterpret_cast<K*>(W.pkey_out.p);
  hipLaunchKernelGGL((k_st_expand<true, K>), dim3(div_up(npe, kExpTile)), dim3(256), 0, s, O, (uint64_t)npe, W.poff.p, W.dbeg.p,
                     W.dcnt.p, W.eslot.p, W.pli.p, W.sslot.p, jbits, (uint32_t*)nullptr, (uint32_t*)nullptr, key_in, W.pval_in.p);
  PCD_TRY(sort_pairs(W.prim, key_in, key_out, W.pval_in.p, W.pval_out.p, (size_t)npe, 0u, 2 * jbits, s));
  // the inputs of the sort are dead: their storage takes the head flags and the scan
  uint32_t* flag = reinterpret_cast<uint32_t*>(W.pkey_in.p); uint32_t* pos = reinterpret_cast<uint32_t*>(W.pval_in.p);
  hipLaunchKernelGGL(k_st_head_flag<K>, grid_of((uint64_t)npe + 1), dim3(256), 0, s, npe, key_out, flag);
  PCD_TRY(exclusive_sum(W.prim, flag, pos, 0u, (size_t)npe + 1, s));
  PCD_HIP_TRY(hipGetLastError());
  W.h_count.p[3] = 0;
  PCD_HIP_TRY(hipMemcpyAsync(&W.h_count.p[3], pos + npe, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipStreamSynchronize(s)); ++*syncs;
  return PCD_OK;
}

template <typename K>
static void st_pair_blocks(SchurStructure& T, uint32_t npe, uint32_t ndiag, unsigned jbits, hipStream_t s) {
  SchurBuildScratch& W = T.tmp;
  hipLaunchKernelGGL(k_st_blocks<K>, grid_of((uint64_t)npe + 1), dim3(256), 0, s, npe, (uint32_t)T.ns, ndiag, jbits,
                     reinterpret_cast<const K*>(W.pkey_out.p), W.pval_out.p, reinterpret_cast<const uint32_t*>(W.pkey_in.p),
                     reinterpret_cast<const uint32_t*>(W.pval_in.p), T.ent_a.p, T.ent_b.p, T.pair_ij.p, T.blk_start.p, W.pj.p,
                     W.pq.p);
}

pcd_status schur_structure_build(const pcd_ba* b, SchurStructure& T, hipStream_t s, int* num_syncs) {
  SchurBuildScratch& W = T.tmp;
  const uint32_t O = (uint32_t)b->O, P = (uint32_t)b->P, I = (uint32_t)b->I;
  const auto t0 = std::chrono::steady_clock::now();
  int syncs = 0;
  T.built = false;
  ScopedKernelTimer timer("ba_schur_build", s);
  // ---- slots, positions, the point lists, the entry counts of every observation
  PCD_TRY(W.flag.reserve((size_t)I + 1)); PCD_TRY(W.scan.reserve((size_t)I + 1));
  PCD_TRY(T.img_slot.reserve(at_least_1(I))); PCD_TRY(T.slot_img.reserve(at_least_1(I)));
  PCD_TRY(T.obs_pos.reserve(at_least_1(O))); PCD_TRY(T.iota.reserve(at_least_1(O)));
  PCD_TRY(W.eslot.reserve(at_least_1(O))); PCD_TRY(W.key.reserve(at_least_1(O))); PCD_TRY(W.skey.reserve(at_least_1(O)));
  PCD_TRY(W.pli.reserve(at_least_1(O))); PCD_TRY(W.sslot.reserve(at_least_1(O))); PCD_TRY(W.pst.reserve((size_t)P + 2));
  PCD_TRY(W.dbeg.reserve(at_least_1(O)));
  for (DevBuf<uint64_t>* d : {&W.dcnt, &W.pcnt, &W.doff, &W.poff}) PCD_TRY(d->reserve((size_t)O + 1));
  PCD_TRY(W.h_count.reserve(4));
  hipLaunchKernelGGL(k_st_slot_flag, grid_of((uint64_t)I + 1), dim3(256), 0, s, I, b->const_poses(), W.flag.p);
  PCD_TRY(exclusive_sum(W.prim, W.flag.p, W.scan.p, 0u, (size_t)I + 1, s));
  if (I) hipLaunchKernelGGL(k_st_slots, grid_of(I), dim3(256), 0, s, I, W.flag.p, W.scan.p, T.img_slot.p, T.slot_img.p);
  if (O) {
    hipLaunchKernelGGL(k_st_positions, grid_of(O), dim3(256), 0, s, O, P, b->img_obs.p, b->obs_image.p, b->img_pt.p,
                       b->const_points(), T.img_slot.p, T.obs_pos.p, T.iota.p, W.eslot.p, W.key.p);
    PCD_TRY(sort_pairs(W.prim, W.key.p, W.skey.p, T.iota.p, W.pli.p, (size_t)O, 0u, bits_for(P), s));
  }
  hipLaunchKernelGGL(k_st_point_lists, grid_of(std::max<uint64_t>(O, (uint64_t)P + 1)), dim3(256), 0, s, O, P, W.skey.p,
                     W.pli.p, W.eslot.p, W.sslot.p, W.pst.p);
  hipLaunchKernelGGL(k_st_count, grid_of((uint64_t)O + 1), dim3(256), 0, s, O, W.eslot.p, b->img_pt.p, W.pst.p, W.sslot.p,
                     W.dbeg.p, W.dcnt.p, W.pcnt.p);
  PCD_TRY(exclusive_sum(W.prim, W.dcnt.p, W.doff.p, (uint64_t)0, (size_t)O + 1, s));
  PCD_TRY(exclusive_sum(W.prim, W.pcnt.p, W.poff.p, (uint64_t)0, (size_t)O + 1, s));
  PCD_HIP_TRY(hipGetLastError());
  // ---- synchronisation 1: the counts that size the entry buffers
  W.h_count.p[0] = 0;
  PCD_HIP_TRY(hipMemcpyAsync(&W.h_count.p[0], W.scan.p + I, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipMemcpyAsync(&W.h_count.p[1], W.doff.p + O, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipMemcpyAsync(&W.h_count.p[2], W.poff.p + O, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PCD_HIP_TRY(hipStreamSynchronize(s)); ++syncs;
  const uint32_t ns = (uint32_t)W.h_count.p[0];
  const uint64_t ndiag = W.h_count.p[1], npe = W.h_count.p[2], nent = ndiag + npe;
  if (nent >= kLayoutLimit) {   // from the counts alone: no entry buffer exists yet
    set_error("point elimination: %zu block entries exceed the 32-bit layout", (size_t)nent);
    return PCD_ERR_UNSUPPORTED;
  }
  T.ns = (int)ns;
  // ---- the entries: the diagonal ones in place, the pair ones through the sort
  PCD_TRY(T.ent_a.reserve(at_least_1(nent))); PCD_TRY(T.ent_b.reserve(at_least_1(nent)));
  if (ndiag)
    hipLaunchKernelGGL((k_st_expand<false, uint32_t>), dim3(div_up(ndiag, kExpTile)), dim3(256), 0, s, O, ndiag, W.doff.p,
                       W.dbeg.p, W.dcnt.p, W.eslot.p, W.pli.p, W.sslot.p, 0u, T.ent_a.p, T.ent_b.p, (uint32_t*)nullptr,
                       (uint64_t*)nullptr);
  const unsigned jbits = ns > 1 ? bits_for(ns - 1) : 0;   // a slot is below 2^jbits; the key (i << jbits | j) has 2 jbits
  const bool wide = 2 * jbits > 32;
  uint64_t npairs = 0;
  if (npe) {
    PCD_TRY(wide ? st_pair_entries<uint64_t>(T, O, (uint32_t)npe, jbits, s, &syncs)
                 : st_pair_entries<uint32_t>(T, O, (uint32_t)npe, jbits, s, &syncs));
    npairs = W.h_count.p[3];   // ---- synchronisation 2 is behind us
  }
  const uint64_t nblk = ns + npairs, nrow = ns + 2 * npairs;
  if (nblk + 1 >= kLayoutLimit || nrow >= kLayoutLimit) {
    set_error("point elimination: %zu block entries exceed the 32-bit layout", (size_t)nent);
    return PCD_ERR_UNSUPPORTED;
  }
  PCD_TRY(T.blk_start.reserve(nblk + 1)); PCD_TRY(T.pair_ij.reserve(at_least_1(2 * npairs)));
  PCD_TRY(T.row_start.reserve((size_t)ns + 1)); PCD_TRY(T.row_blk.reserve(at_least_1(nrow))); PCD_TRY(T.row_col.reserve(at_least_1(nrow)));
  for (DevBuf<uint32_t>* d : {&W.pj, &W.pq, &W.pj_sorted, &W.pq_sorted}) PCD_TRY(d->reserve(at_least_1(npairs)));
  for (DevBuf<uint32_t>* d : {&W.ilo, &W.jlo, &W.rcnt}) PCD_TRY(d->reserve((size_t)ns + 1));
  hipLaunchKernelGGL(k_st_diag_starts, grid_of((uint64_t)ns + 1), dim3(256), 0, s, ns, (uint32_t)ndiag, T.slot_img.p,
                     b->img_obs_start.p, W.doff.p, T.blk_start.p);
  if (npe) {
    if (wide) st_pair_blocks<uint64_t>(T, (uint32_t)npe, (uint32_t)ndiag, jbits, s);
    else st_pair_blocks<uint32_t>(T, (uint32_t)npe, (uint32_t)ndiag, jbits, s);
  }
  // ---- the row lists of the product
  if (npairs) PCD_TRY(sort_pairs(W.prim, W.pj.p, W.pj_sorted.p, W.pq.p, W.pq_sorted.p, (size_t)npairs, 0u, jbits, s));
  hipLaunchKernelGGL(k_st_row_count, grid_of((uint64_t)ns + 1), dim3(256), 0, s, ns, (uint32_t)npairs, T.pair_ij.p,
                     W.pj_sorted.p, W.ilo.p, W.jlo.p, W.rcnt.p);
  PCD_TRY(exclusive_sum(W.prim, W.rcnt.p, T.row_start.p, 0u, (size_t)ns + 1, s));
  if (nblk)
    hipLaunchKernelGGL(k_st_row_fill, grid_of(std::max<uint64_t>(ns, npairs)), dim3(256), 0, s, ns, (uint32_t)npairs,
                       T.pair_ij.p, W.pj_sorted.p, W.pq_sorted.p, W.ilo.p, W.jlo.p, T.row_start.p, T.row_blk.p, T.row_col.p);
  PCD_HIP_TRY(hipGetLastError());
  T.npairs = npairs; T.nent = nent; T.built = true;
  T.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (num_syncs) *num_syncs = syncs;
  return PCD_OK;
}

}  // namespace pcd

// brick_clip_kernel.h -- the first stage of the NN grid path (included by nn.hip behind brick_kernel.h).
//
// Comparing every query of a brick with every point of the brick's 6x6x6-cell region (what this kernel does with the
// clip switched off, pcd_nn_set_search(1)) costs 1 293 point-query pairs per query on workload M, 278 M staged points
// for a 10 M-point cloud.  Most of them cannot matter: a query that sits on a sampled surface has its neighbour a few
// centimetres away, the region reaches 0.49 m.  This kernel uses the machinery of brick_kernel.h (one wavefront per work
// item of <= 8 queries of one brick, wave-uniform queries, LDS-DMA tiles, FLANN's float arithmetic + v_min_f64 on the
// packed key, one transposed reduction per item) and clips the region INSIDE the item, wave-uniformly:
//
//   stage A   the brick's own 2x2x2 cells (one contiguous range of the centre quad row) are staged and compared,
//             64 points per step; one reduction gives every query its tentative distance d_k (or the bound it came
//             with: gate-bounded search, refining another shard's result).  A brick without a point of its own
//             takes the first <= 128 records of a neighbouring brick's span of the region instead (issue_a);
//   clip      a point that can still beat query k lies in the ball of radius sqrt(d_k) around it.  Lane k turns its
//             ball's bounding box into a mask of (quad row, x cell) pairs of the region -- 9 rows x 6 cells = 54 bits;
//             the masks of the item's queries are OR-ed (three DPP steps) and become wave-uniform scalars;
//   stage B   of every quad row only the hull of its masked x cells is staged (the row of stage A without the records
//             stage A compared); rows the balls do not touch are dropped.  The ranges come from ONE table per item -- lane
//             7 row + k holds cell_start at x boundary k of quad row `row` (63 loads in one instruction, prefetched
//             an item ahead) -- so clipping costs no dependent memory access: v_readlane with a scalar lane index.
//
// A query is final when best < (distance to the region's boundary)^2 (proven_bound_f below, nn.hip header); the others
// go to the exact fallback with their tentative key as starting bound.  Work items are software-pipelined: the item
// record of item k+2 and the query / boundary-table loads of item k+1 are issued before item k is processed.
//
// Exactness.  Every point that is not compared lies (a) outside the region -- the region bound of nn.hip's header
// decides whether the query is final -- or (b) inside the region but outside the box of every query's ball:
// then its float distance to query k exceeds d_k >= the final distance (strictly; an equal distance lies inside the
// closed ball).  For (b): FLANN's sum is monotone in every term, so fl_dist(q, p) <= d implies fl((qx - px)^2) <= d,
// i.e. |qx - px| <= sqrt(d) (1 + 2^-23); the radius is widened by 1e-5 relative, the box by 2e-7 relative outwards, and
// cells are compared through the very expression the build bins points with (grid.h cell_coord: monotone in the
// coordinate), so a point's cell lies between the cells of the box's corners.
// The argument asks of d_k only that it is an upper bound of query k's final distance.  The records stage A compares
// for an empty brick are real cloud points of the region like the brick's own, their keys enter the minimum in the
// same arithmetic, so d_k is such a bound whichever span they come from; stage B still covers every record of the
// masked hulls that stage A did not compare (the split of stage A's row below).
#pragma once

namespace pcd {

constexpr int kClipNk = 7;      // x boundaries of a region row: cells 2 bx - 2 .. 2 bx + 4
constexpr int kClipRows = 9;    // quad rows of the region: (by - 1 .. by + 1) x (bz - 1 .. bz + 1)
constexpr int kATile = 128;     // points stage A stages at most (2 DMA instructions); the rest of its range joins stage B
constexpr int kClipRanges = 10; // 8 rows + the left and right parts of the row stage A took its records from
// The work schedule inside a block class (k_nn_brick_clip below): the first kSchedStaticPct % of a wavefront's strided
// rounds are static, the rest of the class's items is handed out in chunks of kSchedChunk from a cursor.
#ifndef PCD_SCHED_STATIC_PCT
#define PCD_SCHED_STATIC_PCT 50
#endif
#ifndef PCD_SCHED_CHUNK
#define PCD_SCHED_CHUNK 2
#endif
constexpr uint32_t kSchedStaticPct = PCD_SCHED_STATIC_PCT, kSchedChunk = PCD_SCHED_CHUNK;
static_assert(kSchedStaticPct < 100 && kSchedChunk >= 1 && (kSchedChunk & (kSchedChunk - 1)) == 0, "a share below 1, a power of two");
#ifdef PCD_ABLATE   // timing-only ablations (tools/nn_ablate.py; results are wrong): brick_kernel.h
constexpr int kAblateClipMath = 0x10000, kAblateBound = 0x20000, kAblateStageA = 0x40000, kAblateSelect = 0x80000;
#else
constexpr int kAblateClipMath = 0, kAblateBound = 0, kAblateStageA = 0, kAblateSelect = 0;
#endif

// one staged point against ONE query (the odd query of a group when a step holds one point per lane)
__device__ __forceinline__ void compare_q1p1(const f32x4 p, const float qx, const float qy, const float qz, double& best) {
  asm("v_mov_b32 v120, %[pw]\n\t"
      "v_sub_f32 v122, %[qx], %[px]\n\tv_sub_f32 v123, %[qy], %[py]\n\tv_sub_f32 v124, %[qz], %[pz]\n\t"
      "v_mul_f32 v122, v122, v122\n\tv_mul_f32 v123, v123, v123\n\tv_mul_f32 v124, v124, v124\n\t"
      "v_add_f32 v122, v122, v123\n\tv_add_f32 v121, v122, v124\n\t"
      "v_min_f64 %[b], %[b], v[120:121]\n\t"
      : [b] "+v"(best)
      : [px] "v"(p.x), [py] "v"(p.y), [pz] "v"(p.z), [pw] "v"(p.w), [qx] "v"(qx), [qy] "v"(qy), [qz] "v"(qz)
      : "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
}

// NP (1 or 2) staged points per lane against the first NQ queries of the group
template <int NQ, int NP>
__device__ __forceinline__ void compare_step(const f32x4 (&p)[2], const float (&qx)[8], const float (&qy)[8],
                                             const float (&qz)[8], double (&best)[8]) {
  static_assert(NQ >= 1 && NQ <= 8 && (NP == 1 || NP == 2), "1..8 queries, 1 or 2 points");
  constexpr int E = NQ & ~1;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    if (E >= 4) compare_point4(p[k], qx, qy, qz, best);
    if (E == 8) compare_point4(p[k], qx + 4, qy + 4, qz + 4, best + 4);
    if (E == 2 || E == 6) compare_point2(p[k], qx + (E - 2), qy + (E - 2), qz + (E - 2), best + (E - 2));
  }
  if (NQ & 1) {
    if (NP == 2) compare_query1(p[0], p[1], qx[NQ - 1], qy[NQ - 1], qz[NQ - 1], best[NQ - 1]);
    else compare_q1p1(p[0], qx[NQ - 1], qy[NQ - 1], qz[NQ - 1], best[NQ - 1]);
  }
}

// The region bound of nn.hip's header: squared safe radius around q inside the cells [c0, c1), in float and rounded to
// the safe side; faces on the grid boundary do not bound anything (no points beyond them).  < 0: nothing is proven.
// Exactness.  Let m be the real distance from q to the nearest bounding face.  A point binned outside the range can lie
// at most grid.slack inside it because of float rounding in the binning (grid.slack = 9.6e-7 max(extent, |coord|) >= 4
// roundings of 2^-24), so its real distance to q is >= m - slack and its float distance >= (m - slack)^2 (1 - 2.4e-7).
// The face positions and the differences computed here carry at most 2 ulp of max(|face|, |q|) = 2.4e-7 max |coord| of
// rounding, which a second grid.slack covers: margin - 2 slack <= m - slack.  The square is shrunk by 1e-5: the 2.4e-7
// above and the roundings of the two multiplications stay far below it.  So best < bound implies that no point outside
// the range is as near as best.
__device__ __forceinline__ float proven_bound_f(const GridParams& g, float qx, float qy, float qz, const int c0[3],
                                                const int c1[3]) {
  const float q[3] = {qx, qy, qz};
  float margin = 3e38f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (c0[d] > 0) margin = fminf(margin, q[d] - (g.origin[d] + (float)c0[d] * g.h));
    if (c1[d] < g.dims[d]) margin = fminf(margin, (g.origin[d] + (float)c1[d] * g.h) - q[d]);
  }
  if (margin >= 3e38f) return 3e38f;   // the range covers the whole grid
  margin -= 2.0f * g.slack;
  if (!(margin > 0.0f)) return -1.0f;
  return margin * margin * (1.0f - 1e-5f);
}

// lanes 7 r + 2 j of the boundary table whose two-cell span (row r, x cells 2 j, 2 j + 1) is a neighbouring brick of
// class cls: 1 shares a face with the item's brick, 2 an edge, 3 a corner
constexpr uint64_t span_lanes(int cls) {
  uint64_t m = 0;
  for (int r = 0; r < kClipRows; ++r)
    for (int j = 0; j < 3; ++j)
      if ((j != 1) + (r % 3 != 1) + (r / 3 != 1) == cls) m |= 1ull << (kClipNk * r + 2 * j);
  return m;
}

struct ClipMeta {    // per-item loads issued one item ahead
  float4 q;          // lane < cnt: query (x, y, z, bits(query id))
  uint64_t prior;    // lane < cnt: the key the query came with
  uint32_t bnd;      // lane 7 row + k: cell_start at x boundary k of region row `row` (0 for rows outside the grid)
};

// lpos: the lane's place in the boundary table, k | ry << 8 | rz << 16 (rz == 3: no such row)
__device__ __forceinline__ ClipMeta clip_load_meta(const GridParams& g, const uint4 it, const float4* __restrict__ qsorted,
                                                   const uint64_t* __restrict__ ksorted,
                                                   const uint32_t* __restrict__ cell_start, uint32_t lpos) {
  const int lane = threadIdx.x & 63;
  const int lk = (int)(lpos & 0xFFu), lry = (int)((lpos >> 8) & 0xFFu), lrz = (int)(lpos >> 16);
  ClipMeta m;
  // Every lane issues every load (indices clamped, results masked afterwards): a load under a
  // divergent `if` may be branched around, and then hipcc can no longer count the loads in flight and
  // falls back to s_waitcnt vmcnt(0) at the first use -- which would serialise the prefetch.
  const int cnt = item_count(it);   // >= 1
  m.q = qsorted[it.x + (lane < cnt ? lane : cnt - 1)];
  m.prior = ksorted[it.x + (lane < cnt ? lane : cnt - 1)];
  const int bx = (int)it.y, by = (int)it.z, bz = (int)(it.w & 0x0FFFFFFFu);
  const int yq = by - 1 + lry, zq = bz - 1 + lrz;
  const bool ok = lrz < 3 && yq >= 0 && yq < g.qdims[0] && zq >= 0 && zq < g.qdims[1];
  const int x = min(max(2 * bx - 2 + lk, 0), g.dims[0]);
  const uint32_t v = cell_start[quad_row_base(g, ok ? yq : 0, ok ? zq : 0) + 4u * (uint64_t)x];
  m.bnd = ok ? v : 0u;
  return m;
}

__global__ __launch_bounds__(256, 4) void k_nn_brick_clip(GridParams g, const float4* __restrict__ sorted,
                                                          const uint32_t* __restrict__ cell_start,
                                                          const float4* __restrict__ qsorted,
                                                          const uint64_t* __restrict__ ksorted,
                                                          const uint4* __restrict__ items, NnCounters* __restrict__ ctr,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ fb_list,
                                                          uint32_t* __restrict__ fb_count, int flags,
                                                          unsigned long long* __restrict__ wave_rec) {
  constexpr int G = 8;
  constexpr int NK = kClipNk, NC = kClipNk - 1;   // x boundaries / cells of a region row
  const int collect_stats = flags & 1;
  const bool no_clip = (flags & 2) != 0;   // A/B switch: stage the whole region in stage B (results identical)
  __shared__ __attribute__((aligned(16))) float4 s_tile[4][2][kTile];
  __shared__ __attribute__((aligned(16))) float4 s_a[4][kATile];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform for the compiler too: LDS tile addresses and M0 values stay in SGPRs
  // statistics passes with bit 4: the wavefront's record {start, end, items} (wall_clock64 ticks) for
  // tools/brick_tail_probe.py; a scalar address, so that the loop below does not carry it in VGPRs
  unsigned long long* const rec = wave_rec + 3u * (blockIdx.x * 4u + (uint32_t)wave);
  if ((flags & 4) && lane == 0) rec[0] = wall_clock64();
  const uint32_t nitems = ctr->nitems;
  const uint32_t nwaves = gridDim.x * 4;
  unsigned long long st_staged = 0, st_pairs = 0, st_groups = 0;
  uint32_t fb_base = 0, fb_left = 0;
  // the lane's place in the boundary table
  uint32_t lpos;
  {
    const int lrow = (lane * 9363) >> 16, lk = lane - 7 * lrow;   // lane / 7 for lane < 64
    const int lrz = (lrow * 21846) >> 16, lry = lrow - 3 * lrz;   // lrow / 3 (lane 63: row 9 = (0, 3), not a row)
    lpos = (uint32_t)lk | ((uint32_t)lry << 8) | ((uint32_t)lrz << 16);
    asm volatile("" : "+v"(lpos));   // one register; not three hoisted ones
  }
  // entry e of the table of item metadata m (e wave-uniform)
#define PCD_BND(m, e) PCD_RL((m).bnd, (e))

  // XCD-aware work split: blocks b, b+8, b+16, ... share an XCD (and its 4 MiB L2), so each of the 8
  // block classes walks its own contiguous eighth of the item list (items are in brick order, x fastest):
  // bricks that are neighbours in space -- and share most of their staged rows -- meet in one L2.
  // (speed only: any mapping gives the same results.)
  //
  // Inside a class [c0, item_end) the S wavefronts of the class take items in two phases.  Static: wavefront w takes
  // c0 + w, c0 + w + S, ... for R_s = floor(kSchedStaticPct % of ceil(per / S)) rounds, per = the items of a full class
  // (the last class may hold up to 7 fewer, and then fewer static items or no dynamic ones).  Dynamic: the rest,
  // [stat_end, item_end) with stat_end = min(c0 + R_s S, item_end), goes out in chunks of kSchedChunk consecutive
  // items; a wavefront that runs out takes chunk number atomicAdd(cursor of the class, 1).  The items cost between 1
  // and ~12 tiles x 1..8 queries: with the static schedule alone the kernel waits for the wavefront that drew the
  // dearest ~57 items.  flags & 8: static only (stat_end = item_end; the A/B reference).
  // The cursors count from 0 in NnCounters, cleared with the block (nn.hip take_counters); they run past the last
  // chunk by at most one grab per wavefront.
  // The loop below is pipelined two items deep (record of item k + 2, metadata of item k + 1), so a wavefront knows
  // its next two indices i1, i2; a grab is issued at the top of the iteration BEFORE the one that needs its result
  // (`pend`, consumed after that iteration's s_waitcnt vmcnt(0)): its latency hides under an item, and it is older
  // than every DMA the counted waits of the tile loop count.
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  uint32_t i0, item_end, stride, stat_end;
  unsigned int* cursor;
  {
    uint32_t c0, full;   // full: items of a full class
    if ((gridDim.x & 7u) == 0) {
      const uint32_t cls = blockIdx.x & 7u, per = (nitems + 7u) / 8u;
      stride = (gridDim.x >> 3) * 4;
      c0 = min(nitems, cls * per);
      i0 = c0 + (blockIdx.x >> 3) * 4 + wave;
      item_end = min(nitems, (cls + 1) * per);
      cursor = &ctr->sched_cursor[kSchedCursorWords * cls];
      full = per;
    } else {
      stride = nwaves;
      c0 = 0;
      i0 = blockIdx.x * 4 + wave;
      item_end = nitems;
      cursor = &ctr->sched_cursor[0];
      full = nitems;
    }
    const uint32_t rounds = (full + stride - 1) / stride;
    stat_end = (flags & 8) ? item_end : min(c0 + (rounds * kSchedStaticPct / 100u) * stride, item_end);
  }
  // one returning atomic from one lane (the other lanes hold 0); the value is read with PCD_UNI once it has landed
  // The address is the cursor + an offset of 0 in a VGPR the compiler cannot see through: for an address it knows to
  // be wave-uniform it rewrites the atomic into "one lane adds the number of active lanes, every lane adds its rank",
  // which needs the result on the spot -- an s_waitcnt vmcnt(0) right behind the atomic, its whole latency exposed in
  // every item.  (An offset, not the pointer: a laundered pointer loses its address space and becomes a FLAT atomic,
  // which counts in lgkmcnt as well and would be waited for by the LDS reads.)
  auto grab = [&]() -> uint32_t {
    uint32_t v = 0, off = 0;
    asm volatile("" : "+v"(off));
    if (lane == 0) v = atomicAdd(cursor + off, 1u);
    return v;
  };
  auto chunk_first = [&](uint32_t v) -> uint32_t { return stat_end + kSchedChunk * PCD_UNI(v); };
  // does the item after item i of this wavefront come out of a new chunk?  (i >= item_end: there is no item i)
  auto wants_chunk = [&](uint32_t i) -> bool {
    if (i >= item_end) return false;
    if (i < stat_end) return i + stride >= stat_end && stat_end < item_end;
    return ((i - stat_end) & (kSchedChunk - 1)) == kSchedChunk - 1;
  };
  // the item after item i; `chunk`: first item of the chunk grabbed for it, where wants_chunk(i).  >= item_end: none
  auto successor = [&](uint32_t i, uint32_t chunk) -> uint32_t {
    if (i >= item_end) return kNone;
    if (i < stat_end) return i + stride < stat_end ? i + stride : stat_end < item_end ? chunk : kNone;
    return ((i - stat_end) & (kSchedChunk - 1)) != kSchedChunk - 1 ? i + 1 : chunk;
  };
  if (i0 >= stat_end) i0 = stat_end < item_end ? chunk_first(grab()) : kNone;   // (no static round: few items)
  if (i0 >= item_end) {
    if ((flags & 4) && lane == 0) { rec[1] = wall_clock64(); rec[2] = 0; }
    return;
  }
  uint32_t i1 = successor(i0, wants_chunk(i0) ? chunk_first(grab()) : kNone);
  uint32_t pend = 0;
  if (wants_chunk(i1)) pend = grab();
  const char* __restrict__ src_bytes = reinterpret_cast<const char*>(sorted);
  float4* const bufA = s_a[wave];
#define PCD_RL(v, r) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (int)(r)))
  // stage A of an item: the brick's own cells = x boundaries 2 .. 4 of the centre row (row 4); always exactly two
  // DMA instructions (lanes past the range re-read its last record; an empty range reads the record at its start,
  // which exists -- `sorted` ends with spare records -- and is not compared).
  // An EMPTY brick (48 % of workload M's items: the queries sit off the surfaces, only the halo is occupied) would
  // leave every d_k at its incoming value and stage the whole region.  It takes a substitute range from the boundary
  // table alone: the 26 other two-cell spans (row r, x boundaries 2 j .. 2 j + 2) are the neighbouring bricks; lane
  // 7 r + 2 j forms its span's size from the table entry two lanes up (two wave shifts), one ballot gives the spans
  // that hold a point, constant lane masks sort them into face, edge and corner neighbours, and the lowest class
  // with a point is searched for its fullest span with one minimum over the lanes, ties to the lowest table entry
  // (tools/brick_clip_sim.py prices the rules).  The range is wave-uniform -- its first record, and its length and
  // first table entry in one word -- and is carried to the item's own iteration: the stage-B split follows it.
  struct ARange { uint32_t s, ne; };   // first record; records staged (<= kATile) | first table entry (7 row + k) << 8
  auto issue_a = [&](const ClipMeta& m) -> ARange {
    uint32_t sA = PCD_BND(m, 4 * NK + 2), eA = PCD_BND(m, 4 * NK + 4);
    uint32_t e = 4 * NK + 2;
    if (sA == eA) {   // wave-uniform
      // wave_shl:1 twice: lane l reads lane l + 2 (lanes 62 / 63 keep their own value: not a span's first lane)
      uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp((int)m.bnd, (int)m.bnd, 0x130, 0xf, 0xf, false);
      up = (uint32_t)__builtin_amdgcn_update_dpp((int)up, (int)up, 0x130, 0xf, 0xf, false);
      const uint32_t size = up - m.bnd;
      const uint64_t occ = __builtin_amdgcn_ballot_w64(size != 0u);   // (the own span is empty; other lanes are masked away)
      const uint64_t fc = occ & span_lanes(1), ed = occ & span_lanes(2), co = occ & span_lanes(3);
      const uint64_t pick = fc ? fc : ed ? ed : co;
      if (pick & (pick - 1)) {   // several spans of the class: the fullest
        uint32_t key = ((0xFFFFFFu - min(size, 0xFFFFFFu)) << 6) | (uint32_t)lane;
        asm("v_cndmask_b32_e64 %0, -1, %1, %2" : "=v"(key) : "v"(key), "s"(pick));
        e = wave_min_u32(key) & 63u;
      } else if (pick) {   // (a brick with an empty halo never becomes an item; a table of zeros would keep the own span)
        e = (uint32_t)__builtin_ctzll(pick);
      }
      sA = PCD_RL(m.bnd, e); eA = PCD_RL(m.bnd, e + 2u);   // e = 7 row + 2 j: both entries lie in the row
    }
    const uint32_t nA = min(eA - sA, (uint32_t)kATile);
    const uint32_t last = nA ? nA - 1u : 0u;
    const uint32_t i0 = sA + min((uint32_t)lane, last), i1 = sA + min((uint32_t)lane + 64u, last);
    lds_dma16(reinterpret_cast<const float4*>(src_bytes + ((uint64_t)i0 << 4)), bufA);
    lds_dma16(reinterpret_cast<const float4*>(src_bytes + ((uint64_t)i1 << 4)), bufA + 64);
    return ARange{sA, nA | (e << 8)};
  };

  uint4 it0 = items[PCD_UNI(i0)];   // through uniform (scalar) indices: brick_kernel.h PCD_UNI
  ClipMeta m0 = clip_load_meta(g, it0, qsorted, ksorted, cell_start, lpos);
  uint4 it1 = items[PCD_UNI(min(i1, item_end - 1))];
  ARange a0 = issue_a(m0);

  while (i0 < item_end) {
    // stage A of this item (issued while the previous item was compared) has landed, and so has the chunk grabbed
    // during the previous item; nothing else is in flight
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const uint32_t i2 = successor(i1, chunk_first(pend));
    if (wants_chunk(i2)) pend = grab();   // for the item after i2: needed at the top of the next iteration
    // ---- prefetch: metadata of the next item, item record of the one after (clamped to the last item) ----
    const ClipMeta m1 = clip_load_meta(g, it1, qsorted, ksorted, cell_start, lpos);
    const uint4 it2 = items[PCD_UNI(min(i2, item_end - 1))];

    const uint32_t cnt = (uint32_t)item_count(it0);
    // The item's queries as wave-uniform values in VGPRs (an SGPR operand halves the VALU rate: brick_kernel.h PCD_CMP_PAIR).  Through
    // LDS: every lane writes its record (lanes >= cnt hold a copy of the last query) into the first tile buffer -- free
    // between two items' tiles -- and all lanes read the first 8 records back, 12 bytes each, same address for the whole
    // wavefront (a broadcast).  One ds_write_b128 + 8 ds_read_b96 on the LDS port instead of 24 v_readlane + 24 v_mov
    // on the VALU and a branch per query slot.
    float qx[G], qy[G], qz[G];
    {
      typedef float f32x3 __attribute__((ext_vector_type(3)));
      const uint32_t qb = lds_addr(s_tile[wave][0]);
      const f32x4 qrec = {m0.q.x, m0.q.y, m0.q.z, m0.q.w};
      f32x3 qv[G];
      asm volatile("ds_write_b128 %9, %8\n\ts_waitcnt lgkmcnt(0)\n\t"
                   "ds_read_b96 %0, %10\n\tds_read_b96 %1, %10 offset:16\n\tds_read_b96 %2, %10 offset:32\n\t"
                   "ds_read_b96 %3, %10 offset:48\n\tds_read_b96 %4, %10 offset:64\n\tds_read_b96 %5, %10 offset:80\n\t"
                   "ds_read_b96 %6, %10 offset:96\n\tds_read_b96 %7, %10 offset:112\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(qv[0]), "=&v"(qv[1]), "=&v"(qv[2]), "=&v"(qv[3]), "=&v"(qv[4]), "=&v"(qv[5]), "=&v"(qv[6]), "=&v"(qv[7])
                   : "v"(qrec), "v"(qb + (uint32_t)lane * 16u), "v"(qb)
                   : "memory");
#pragma unroll
      for (int k = 0; k < G; ++k) { qx[k] = qv[k].x; qy[k] = qv[k].y; qz[k] = qv[k].z; }
    }
    const int bx = (int)it0.y, by = (int)it0.z, bz = (int)(it0.w & 0x0FFFFFFFu);
    double best[G];
#pragma unroll
    for (int k = 0; k < G; ++k) best[k] = __builtin_bit_cast(double, kKeyInit);

    // ---- stage A: the brick's own cells, or the neighbouring span issue_a chose for an empty brick ---------------
    const uint32_t sA = a0.s, nA = a0.ne & 0xFFu;
    if (nA > 0 && !(flags & kAblateStageA)) {
      f32x4 pa[2];
      const uint32_t rd = lds_addr(bufA) + lane * 16;
      asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(pa[0]), "=&v"(pa[1]) : "v"(rd) : "memory");
      if (flags & kAblateCompare) {
        asm volatile("" ::"v"(pa[0]), "v"(pa[1]));
      } else if (nA > 64) {
        switch (cnt) {   // wave-uniform
          case 1: compare_step<1, 2>(pa, qx, qy, qz, best); break;
          case 2: compare_step<2, 2>(pa, qx, qy, qz, best); break;
          case 3: compare_step<3, 2>(pa, qx, qy, qz, best); break;
          case 4: compare_step<4, 2>(pa, qx, qy, qz, best); break;
          case 5: compare_step<5, 2>(pa, qx, qy, qz, best); break;
          case 6: compare_step<6, 2>(pa, qx, qy, qz, best); break;
          case 7: compare_step<7, 2>(pa, qx, qy, qz, best); break;
          default: compare_step<8, 2>(pa, qx, qy, qz, best); break;
        }
      } else {
        switch (cnt) {
          case 1: compare_step<1, 1>(pa, qx, qy, qz, best); break;
          case 2: compare_step<2, 1>(pa, qx, qy, qz, best); break;
          case 3: compare_step<3, 1>(pa, qx, qy, qz, best); break;
          case 4: compare_step<4, 1>(pa, qx, qy, qz, best); break;
          case 5: compare_step<5, 1>(pa, qx, qy, qz, best); break;
          case 6: compare_step<6, 1>(pa, qx, qy, qz, best); break;
          case 7: compare_step<7, 1>(pa, qx, qy, qz, best); break;
          default: compare_step<8, 1>(pa, qx, qy, qz, best); break;
        }
      }
    }
    // lane k < cnt: the tentative key of query k (value v of the reduction sits in the lanes with bits (5,4,3) = v)
    const int holder = ((lane & 4) ? 32 : 0) | ((lane & 2) ? 16 : 0) | ((lane & 1) ? 8 : 0);
    uint64_t mine;
    {
      const uint64_t red = __builtin_bit_cast(uint64_t, (flags & kAblateReduce) ? best[0] : wave_min8_key(best));
      mine = ((uint64_t)__shfl((uint32_t)(red >> 32), holder) << 32) | __shfl((uint32_t)red, holder);
      mine = min_u64(mine, m0.prior);
    }
    // ---- clip: mask of the (row, x cell) pairs the balls of the item's queries touch --------------------------
    uint32_t w0 = 0, w1 = 0, w2 = 0;   // z slab 0 / 1 / 2: bit 6 ry + k
    if (flags & kAblateClipMath) {
      w0 = w1 = w2 = lane < (int)cnt ? 0x3FFFFu : 0u;
    } else if (lane < (int)cnt) {
      // radius: sqrt(d) widened by 1e-5 (v_sqrt_f32's 1 ulp, the roundings of FLANN's sum) + the rounding of q -+ r
      // (half an ulp of |q| + r: 2.4e-7 |q| covers it four times over).  Cells in float: t = (p - origin) / h as the
      // build computes it (grid.h cell_coord_raw); floor(t) - first cell of the region clamped to the region is what the
      // clamped integer cell coordinate gives or wider (only the clamp to the grid is missing, and cells outside the
      // grid are empty ranges of the boundary table); quad rows: floor(floor(t) / 2) = floor(t / 2), exact in float.
      const float d = __uint_as_float((uint32_t)(mine >> 32));
      const float r = __builtin_amdgcn_sqrtf(d) * 1.00001f + ((fabsf(m0.q.x) + fabsf(m0.q.y)) + fabsf(m0.q.z)) * 2.4e-7f + 1e-18f;
      const float tx0 = floorf((m0.q.x - r - g.origin[0]) * g.inv_h), tx1 = floorf((m0.q.x + r - g.origin[0]) * g.inv_h);
      const float ty0 = floorf((m0.q.y - r - g.origin[1]) * g.inv_h * 0.5f), ty1 = floorf((m0.q.y + r - g.origin[1]) * g.inv_h * 0.5f);
      const float tz0 = floorf((m0.q.z - r - g.origin[2]) * g.inv_h * 0.5f), tz1 = floorf((m0.q.z + r - g.origin[2]) * g.inv_h * 0.5f);
      const float fx = (float)(2 * bx - 2), fy = (float)(by - 1), fz = (float)(bz - 1);
      const uint32_t kx0 = (uint32_t)__builtin_amdgcn_fmed3f(tx0 - fx, 0.f, (float)(NC - 1)), kx1 = (uint32_t)__builtin_amdgcn_fmed3f(tx1 - fx, 0.f, (float)(NC - 1));
      const uint32_t ry0 = (uint32_t)__builtin_amdgcn_fmed3f(ty0 - fy, 0.f, 2.f), ry1 = (uint32_t)__builtin_amdgcn_fmed3f(ty1 - fy, 0.f, 2.f);
      const uint32_t rz0 = (uint32_t)__builtin_amdgcn_fmed3f(tz0 - fz, 0.f, 2.f), rz1 = (uint32_t)__builtin_amdgcn_fmed3f(tz1 - fz, 0.f, 2.f);
      const uint32_t xm = (2u << kx1) - (1u << kx0);                     // bits kx0 .. kx1
      const uint32_t ym = (2u << ry1) - (1u << ry0), zm = (2u << rz1) - (1u << rz0);
      const uint32_t pat = xm * ((ym * 0x421u) & 0x1041u);               // the x mask in the 6-bit fields of the rows ry0 .. ry1
      w0 = (zm & 1u) ? pat : 0u; w1 = (zm & 2u) ? pat : 0u; w2 = (zm & 4u) ? pat : 0u;
      if (no_clip) w0 = w1 = w2 = 0x3FFFFu;
    }
    // OR over lanes 0..7 (row_shr 1, 2, 4; lanes without a source contribute 0): lane 7 holds the item's mask
#define PCD_OR_SHR(v, ctrl) v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xf, 0xf, true)
    PCD_OR_SHR(w0, 0x111); PCD_OR_SHR(w1, 0x111); PCD_OR_SHR(w2, 0x111);
    PCD_OR_SHR(w0, 0x112); PCD_OR_SHR(w1, 0x112); PCD_OR_SHR(w2, 0x112);
    PCD_OR_SHR(w0, 0x114); PCD_OR_SHR(w1, 0x114); PCD_OR_SHR(w2, 0x114);
#undef PCD_OR_SHR
    const uint32_t M[3] = {PCD_RL(w0, 7), PCD_RL(w1, 7), PCD_RL(w2, 7)};
    // ---- stage B ranges (all wave-uniform scalars): start and length of the 10 ranges -------------------------
    // The concatenation of the ranges is addressed in GROUPS of 4 consecutive slots: every range is
    // padded to a multiple of 4 slots (the <= 3 padding slots read the records that follow the range in memory:
    // real cloud points of the neighbouring cells, harmless extra candidates; the `sorted` buffer ends with 4
    // spare records), so the 4 slots of a group are 4 consecutive records.  Lane l of tile t takes group
    // t * 64 + l: ONE source address per lane per tile, and the tile's 4 DMA instructions are that address +
    // 0 / 16 / 32 / 48 bytes (instruction k fills LDS slot k * 64 + l -- a permutation of the tile, and the
    // compare does not care about the order).  The range of a group is found with one compare + select per
    // range start (the starts are wave-uniform): no per-window tables, no v_readlane inside the tile loop,
    // any number of range starts inside a tile.  Round 1-2a computed an address per 64-slot DMA window (three
    // v_readlane + ~10 VALU each, plus a generic path for windows with two starts); timing-only ablations put
    // that address generation at 0.34 ms of the kernel's 0.84.
    // The row stage A took its records from (row 4, or the substitute's) goes without them: [s, min(e, sA)) stays the
    // row's range -- the lanes of that row clamp their table entries to sA, so the row is read like every other --
    // and [max(s, sA + nA), e) is range 9 (the hull need not contain a substitute's span; it does contain the
    // brick's own cells, the queries lie in them).
    const uint32_t rowA = ((a0.ne >> 8) * 9363u) >> 16;   // table entry / 7
    const uint32_t bndL = (uint32_t)lane - 7u * rowA < 7u ? min(m0.bnd, sA) : m0.bnd;
    uint32_t rs[kClipRanges], rl[kClipRanges];
#pragma unroll
    for (int r = 0; r < kClipRows; ++r) {
      const uint32_t xm = (M[r / 3] >> (6 * (r % 3))) & 63u;
      const int k0 = xm ? __builtin_ctz(xm) : 0, k1 = xm ? 32 - __builtin_clz(xm) : 0;   // cells k0 .. k1 - 1
      const uint32_t s = PCD_RL(bndL, r * NK + k0), e = PCD_RL(bndL, r * NK + k1);   // (no masked cell: s == e)
      rs[r] = s; rl[r] = e - s;
    }
    {
      const uint64_t m54 = (uint64_t)M[0] | ((uint64_t)M[1] << 18) | ((uint64_t)M[2] << 36);
      const uint32_t xm = (uint32_t)(m54 >> (6u * rowA)) & 63u;
      const uint32_t k0 = xm ? (uint32_t)__builtin_ctz(xm) : 0u, k1 = xm ? 32u - (uint32_t)__builtin_clz(xm) : 0u;
      const uint32_t e = PCD_BND(m0, rowA * NK + k1);
      rs[9] = max(PCD_BND(m0, rowA * NK + k0), sA + nA);
      rl[9] = e > rs[9] ? e - rs[9] : 0u;
    }
    uint32_t ro[kClipRanges + 1];   // start of range i in the concatenation padded to groups of 4 slots
    ro[0] = 0;
#pragma unroll
    for (int i = 0; i < kClipRanges; ++i) ro[i + 1] = ro[i] + ((rl[i] + 3u) & ~3u);
    const uint32_t T = (flags & kAblateTiles) ? 0u : ro[kClipRanges];
    const int ntiles = (int)((T + kTile - 1) / kTile);

    ARange a1;   // the next item's stage-A range: chosen once, where its DMAs are issued
    if (T > 0) {
      uint32_t dv[kClipRanges];   // source - start deltas in VGPRs (v_cndmask cannot read an SGPR next to VCC)
#pragma unroll
      for (int i = 0; i < kClipRanges; ++i) asm volatile("v_mov_b32 %0, %1" : "=v"(dv[i]) : "s"(rs[i] - ro[i]));
      // issue the 4 DMAs of tile t (always exactly 4 instructions: groups past T re-read the last group, which
      // cannot change a minimum -- the compare needs no tail mask)
      auto issue_tile = [&](int t) {
        float4* buf = s_tile[wave][t & 1];
        const uint32_t s4 = min((uint32_t)t * kTile + 4u * (uint32_t)lane, T - 4u);
        uint32_t dl = dv[0];   // empty ranges share their start with the next one: the last one wins
        if (!(flags & kAblateSelect)) {
#define PCD_SEL(o, d) asm("v_cmp_le_u32_e32 vcc, %2, %1\n\tv_cndmask_b32_e32 %0, %0, %3, vcc" : "+v"(dl) : "v"(s4), "s"(o), "v"(d) : "vcc")
        PCD_SEL(ro[1], dv[1]); PCD_SEL(ro[2], dv[2]); PCD_SEL(ro[3], dv[3]); PCD_SEL(ro[4], dv[4]); PCD_SEL(ro[5], dv[5]);
        PCD_SEL(ro[6], dv[6]); PCD_SEL(ro[7], dv[7]); PCD_SEL(ro[8], dv[8]); PCD_SEL(ro[9], dv[9]);
#undef PCD_SEL
        }
        // uniform base + byte offset (64-bit: a cloud may exceed 2^28 points = 4 GiB of records)
        const float4* gp = reinterpret_cast<const float4*>(src_bytes + ((uint64_t)(s4 + dl) << 4));
        if (flags & kAblateNoDma) { asm volatile("" ::"v"(gp)); return; }
        // the instruction offset is added to the LDS address as well as to the source address
        // (LDS address = M0 base + instruction offset + lane * 16): take it off the base again
        lds_dma16_off<0>(gp, buf);
        lds_dma16_off<16>(gp, buf + 64 - 1);
        lds_dma16_off<32>(gp, buf + 128 - 2);
        lds_dma16_off<48>(gp, buf + 192 - 3);
      };
      issue_tile(0);
      a1 = issue_a(m1);   // stage A of the NEXT item: lands under this item's tiles
      // One tile loop per group size (cnt is wave-uniform): the dispatch on the number of queries happens once per item,
      // not once per tile -- the compare-and-branch chain in front of every tile's compare block was 7 % of the kernel
      // (0.488 -> 0.453 ms), more than any memory instruction of the loop.
      auto run_tiles = [&](auto nq_tag) {
        constexpr int NQ = decltype(nq_tag)::value;
        for (int t = 0; t < ntiles; ++t) {
          // in flight, oldest first: tile 0 (4), stage A of the next item (2), tile 1 (4), ...
          if (t + 1 < ntiles) {
            issue_tile(t + 1);
            if (t == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          } else {
            if (t == 0) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
          __builtin_amdgcn_wave_barrier();
          // The tile is read with inline-asm ds_read_b128: for an ordinary LDS load hipcc would insert
          // s_waitcnt vmcnt(0) (it cannot tell the two buffers apart) and drain tile t+1's DMAs.
          f32x4 p[4];
          const uint32_t rd = lds_addr(s_tile[wave][t & 1]) + lane * 16;
          if (flags & kAblateNoLdsRead) {
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = f32x4{(float)lane, (float)t, (float)k, 0.f};
          } else
          asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\t"
                       "ds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072\n\t"
                       "s_waitcnt lgkmcnt(0)"
                       : "=&v"(p[0]), "=&v"(p[1]), "=&v"(p[2]), "=&v"(p[3])
                       : "v"(rd)
                       : "memory");
          if (flags & kAblateCompare) {
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("" ::"v"(p[k]));
          } else {
            compare_tile<NQ>(p, qx, qy, qz, best);
          }
        }
      };
      switch (cnt) {   // wave-uniform
        case 1: run_tiles(std::integral_constant<int, 1>{}); break;
        case 2: run_tiles(std::integral_constant<int, 2>{}); break;
        case 3: run_tiles(std::integral_constant<int, 3>{}); break;
        case 4: run_tiles(std::integral_constant<int, 4>{}); break;
        case 5: run_tiles(std::integral_constant<int, 5>{}); break;
        case 6: run_tiles(std::integral_constant<int, 6>{}); break;
        case 7: run_tiles(std::integral_constant<int, 7>{}); break;
        default: run_tiles(std::integral_constant<int, 8>{}); break;
      }
      // the second reduction: stage A's result and the key the query came with are in `mine` already
      const uint64_t red = __builtin_bit_cast(uint64_t, (flags & kAblateReduce) ? best[0] : wave_min8_key(best));
      mine = min_u64(mine, ((uint64_t)__shfl((uint32_t)(red >> 32), holder) << 32) | __shfl((uint32_t)red, holder));
    } else {
      a1 = issue_a(m1);
    }
    // ---- epilogue: final, or on to the exact fallback with the tentative key as starting bound ----------------
    bool unproven = false;
    if (lane < (int)cnt) {
      const uint32_t my_qi = __float_as_uint(m0.q.w);
      const int c0[3] = {max(2 * bx - 2, 0), max(2 * by - 2, 0), max(2 * bz - 2, 0)};
      const int c1[3] = {min(2 * bx + 4, g.dims[0]), min(2 * by + 4, g.dims[1]), min(2 * bz + 4, g.dims[2])};
      const float bound = (flags & kAblateBound) ? 3e38f : proven_bound_f(g, m0.q.x, m0.q.y, m0.q.z, c0, c1);
      unproven = !(__uint_as_float((uint32_t)(mine >> 32)) < bound) && !(flags & kAblateFallback);
      keys[my_qi] = unproven ? mine : finalized_key(mine);   // final, or the starting bound of the exact fallback
    }
    const unsigned long long um = __ballot(unproven);
    if (um) {
      // the wavefront appends to the fallback list inside chunks of kFbChunk slots it reserves with ONE returning
      // atomic each (an atomic per item exposed its latency on every fourth item); the slots of a chunk it does not
      // use get 0xFFFFFFFF when the chunk is left (here and at the end of the kernel): the list needs no memset;
      // k_fb_compact squeezes the sentinels out
      const uint32_t k = (uint32_t)__popcll(um);
      if (k > fb_left) {
        if (lane < (int)fb_left) fb_list[fb_base + lane] = 0xFFFFFFFFu;
        uint32_t nb = 0;
        if (lane == 0) nb = atomicAdd(fb_count, (uint32_t)kFbChunk);
        fb_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)nb);
        fb_left = kFbChunk;
      }
      if (unproven) fb_list[fb_base + __builtin_amdgcn_mbcnt_hi((uint32_t)(um >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)um, 0u))] = __float_as_uint(m0.q.w);
      fb_base += k;
      fb_left -= k;
    }
    if (collect_stats) {
      const uint32_t slots = (nA > 64 ? 128u : nA ? 64u : 0u) + (uint32_t)ntiles * kTile;
      st_staged += nA + T; st_pairs += (unsigned long long)slots * cnt; st_groups += 1;
    }
    it0 = it1; it1 = it2; m0 = m1; a0 = a1;
    i0 = i1; i1 = i2;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last (redundant) stage-A prefetch must not outlive the wavefront's LDS
  if (lane < (int)fb_left) fb_list[fb_base + lane] = 0xFFFFFFFFu;   // rest of the last chunk
  if (collect_stats && lane == 0) {
    atomicAdd(&ctr->staged_points, st_staged);
    atomicAdd(&ctr->pair_evals, st_pairs);
    atomicAdd(&ctr->brick_groups, st_groups);
    if (flags & 4) { rec[1] = wall_clock64(); rec[2] = st_groups; }
  }
#undef PCD_BND
#undef PCD_RL
}

}  // namespace pcd

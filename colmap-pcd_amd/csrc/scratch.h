// scratch.h -- grow-only per-cloud device scratch shared by nn.hip and assoc.hip
#pragma once
#include <cstddef>

#include "cloud.h"

namespace pcd {

// k_nn_brick_clip's cursors (brick_clip_kernel.h): one per block class = per XCD, each on a 128-byte line of its own --
// eight cursors on one line had the eight L2s pass that line around with every grab.  The array and the struct are
// aligned to the line, so that in both blocks no cursor shares its line with nitems / fb_count, which every XCD touches
#ifndef PCD_SCHED_CURSOR_WORDS
#define PCD_SCHED_CURSOR_WORDS 32
#endif
constexpr int kSchedCursorWords = PCD_SCHED_CURSOR_WORDS;

struct alignas(128) NnCounters {
  unsigned long long brick_groups, staged_points, fallback_queries, fallback_points, pair_evals;
  unsigned int nitems, fb_count;
  unsigned int pad[2];   // pad[0] = length of the squeezed fallback list
  unsigned int n_in_grid;     // brick-sorted positions 0 .. n_in_grid-1 are the finite queries inside the grid
  unsigned int pad2[3];
  unsigned int fb_max_steps, fb_max_leaves;   // statistics passes: longest walk of k_nn_fallback (steps, leaf scans)
  unsigned long long fb_steps, fb_leaves;
  alignas(128) unsigned int sched_cursor[8 * kSchedCursorWords];   // [kSchedCursorWords * class]: chunks handed out of the class's dynamic range
};

static_assert(sizeof(NnCounters) % 128 == 0 && offsetof(NnCounters, sched_cursor) % 128 == 0, "cursors on line boundaries in both blocks");

struct QueryScratch {
  DevBuf<float4> qf4;          // (float)query, w = 1 valid / 0 not finite
  DevBuf<uint64_t> keys;       // host-API result keys
  DevBuf<uint32_t> bk_keys, bk_vals;   // radix-sort bookkeeping: (brick id, query id) pairs, unsorted | sorted halves
  DevBuf<uint32_t> bk_item;            // radix-sort bookkeeping: work items per tile of 1024 sorted positions
  // counting-sort bookkeeping (nn.hip): bk_slot = one bit per brick whose halo region holds a cloud point, built once
  // (valid while bk_nslots is the cloud's number of bricks); per batch bk_keys = every query's sort key (brick id, or
  // fallback / skip), bk_vals = the Q {fine key, query id} pairs of the scatter
  DevBuf<uint32_t> bk_slot, bk_chist;   // bk_chist: coarse bucket totals | bucket starts | items per bucket
  DevBuf<uint32_t> bk_hmat;             // coarse histogram per range of queries: [ranges <= 256][buckets <= 4096], <= 4 MB
  uint32_t bk_nslots = 0;
  DevBuf<float4> qsorted;      // brick-sorted query records {x,y,z,bits(query id)}
  DevBuf<uint64_t> ksorted;    // their incoming keys, same order
  DevBuf<uint4> items;         // {first query, brick x, brick y, brick z | count << 28}
  DevBuf<uint32_t> fb_list, fb_dense;   // fallback list as the brick kernel fills it (chunked) / squeezed
  DevBuf<float4> fb_seed;      // k_nn_fallback's seed table, built on first use (nn.hip fb_seed_table)
  bool fb_seed_ok = false;
  DevBuf<NnCounters> counters;   // two blocks, used alternately by the grid-path calls (nn.hip counters_for)
  int ctr_cur = 0;               // the block of the last call
  bool ctr_next_clean = false;   // the other block is zero (or will be when the stream gets there)
  // statistics passes that ask for it (pcd_nn_set_tuning bit 4): {start, end, items} of every wavefront of the last
  // k_nn_brick_clip launch, wall_clock64 ticks; reserved in such a pass only
  DevBuf<unsigned long long> wave_rec;
  uint32_t wave_rec_n = 0;
  // the same for k_nn_fallback (bit 16): {start, end, walk steps} of every wavefront of its last launch
  DevBuf<unsigned long long> fb_rec;
  uint32_t fb_rec_n = 0;
  DevBuf<char> tmp;
  DevBuf<double> d_q;          // staging of host queries
  DevBuf<uint32_t> d_idx; DevBuf<float> d_sq; DevBuf<uint8_t> d_found;
  // host-API association staging
  DevBuf<double> a_mr, a_xyz, a_abcd, a_dist, a_angle, a_d2p;
  DevBuf<uint8_t> a_type;
  DevBuf<uint64_t> a_keys;
  // staged host path (pcd_assoc_staging / pcd_associate_staged): pinned inputs / results, compaction scratch
  PinnedBuf<double> h_q, h_mr;
  PinnedBuf<pcd_assoc_hit> h_hits;
  PinnedBuf<uint32_t> h_count;
  // staged host path: copies in / compute / copies out on their own streams, chunk by chunk (assoc.hip)
  static constexpr int kStageChunks = 4;
  hipStream_t st_in = nullptr, st_comp = nullptr, st_out = nullptr, st_cnt = nullptr;
  hipEvent_t ev_in[kStageChunks] = {}, ev_comp[kStageChunks] = {}, ev_cnt[kStageChunks] = {};
  ~QueryScratch() {
    for (int k = 0; k < kStageChunks; ++k) {
      if (ev_in[k]) (void)hipEventDestroy(ev_in[k]);
      if (ev_comp[k]) (void)hipEventDestroy(ev_comp[k]);
      if (ev_cnt[k]) (void)hipEventDestroy(ev_cnt[k]);
    }
    if (st_in) (void)hipStreamDestroy(st_in);
    if (st_comp) (void)hipStreamDestroy(st_comp);
    if (st_out) (void)hipStreamDestroy(st_out);
    if (st_cnt) (void)hipStreamDestroy(st_cnt);
  }
  DevBuf<pcd_assoc_hit> d_hits;
  DevBuf<uint32_t> hit_pos, hit_count;
  // normal estimation (normals.hip): 64-query passes per leaf and their exclusive scan, the (leaf, pass) work items,
  // the per-block partial sums followed by their totals, and the staging of the host API's outputs
  DevBuf<uint32_t> nr_pass, nr_off;
  DevBuf<uint2> nr_items;
  DevBuf<unsigned long long> nr_part;
  DevBuf<char> nr_tmp;
  DevBuf<uint32_t> nr_count;
  DevBuf<double> nr_curv;
};

inline QueryScratch* scratch_of(pcd_cloud* c) {
  if (!c->scratch) c->scratch = new QueryScratch();
  return c->scratch;
}

// nn.hip: the search of pcd_nn_query_device; the same bounded by the gate (d_max_range: 1 or Q entries, NULL: fixed_range)
pcd_status nn_query_device_internal(pcd_cloud* c, const double* d_q, uint64_t Q, int algo, uint64_t* d_keys,
                                    hipStream_t s);
pcd_status nn_query_bounded_internal(pcd_cloud* c, const double* d_q, uint64_t Q, const double* d_max_range,
                                     uint64_t mr_count, double fixed_range, uint64_t* d_keys, hipStream_t s);

}  // namespace pcd

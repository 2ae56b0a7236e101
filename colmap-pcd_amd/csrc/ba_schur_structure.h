// ba_schur_structure.h -- the co-visibility structure of the point elimination: what ba_schur_structure.hip builds on
// the device and ba_solve.hip's kernels read.  Internal.
#pragma once
#include "ba_handle.h"

namespace pcd {

// Scratch of the build (ba_schur_structure.hip), kept in the handle so that a rebuild after an edit allocates nothing
// the first build has not.  e = image-major position of an observation; k = position in the sorted point lists.
struct SchurBuildScratch {
  DevBuf<uint32_t> flag, scan;          // [I+1] variable pose? and its exclusive scan (the last value: ns)
  DevBuf<int> eslot;                    // [O] slot of e, -1: takes no part in the elimination
  DevBuf<uint32_t> key, skey, pli;      // [O] point of e (P: not eliminated); sorted; the e of k (iota is the unsorted value)
  DevBuf<int> sslot;                    // [O] slot of pli[k]
  DevBuf<uint32_t> pst;                 // [P+1] first k of a point's list; pst[P]: the eliminated observations
  DevBuf<uint32_t> dbeg;                // [O] first k of the partners of e in its own slot
  DevBuf<uint64_t> dcnt, pcnt, doff, poff;   // [O+1] diagonal / pair entries of e (the last 0) and their exclusive scans
  DevBuf<char> pkey_in, pkey_out;       // [npe] keys of the pair entries, (i << bits | j): 4 or 8 bytes each
  DevBuf<uint64_t> pval_in, pval_out;   // [npe+1] the entries, a << 32 | b.  After the sort pkey_in / pval_in hold the
                                        // block-head flags and their scan.
  DevBuf<uint32_t> pj, pq, pj_sorted, pq_sorted;   // [npairs] j and index of every pair; stably by j
  DevBuf<uint32_t> ilo, jlo, rcnt;      // [ns+1] first pair with i >= s; first of the j-sorted with j >= s; row lengths
  DevBuf<char> prim;                    // rocPRIM temporary storage
  PinnedBuf<uint64_t> h_count;          // ns, diagonal entries, pair entries; npairs
  uint64_t bytes() const {
    return dev_bytes(flag, scan, eslot, key, skey, pli, sslot, pst, dbeg, dcnt, pcnt, doff, poff, pkey_in, pkey_out, pval_in,
                     pval_out, pj, pq, pj_sorted, pq_sorted, ilo, jlo, rcnt, prim);
  }
};

// Blocks: the ns diagonal blocks, then the pair blocks in ascending (i, j).  Entries (a, b) of a block: a ascending
// (image-major position in image i), then b ascending (image j).  A diagonal block holds (a, a) and the pairs of a point
// observed more than once in the image.  Only variable-pose observations of non-constant points take part.  Every sum
// downstream runs in the order of these lists.
struct SchurStructure {   // built on the device by the first Schur call (schur_structure_build), then read only
  bool built = false; int ns = 0; uint64_t npairs = 0, nent = 0; double build_ms = 0.0;
  uint32_t nblk() const { return (uint32_t)(ns + npairs); }   // the ns diagonal blocks, then the pair blocks
  DevBuf<int> img_slot, slot_img;
  DevBuf<uint32_t> blk_start, ent_a, ent_b, pair_ij, iota, obs_pos;
  // rows of S for y = S x, ascending partner slot: [ns+1]; block (< ns: diagonal, else ns + pair); partner << 1 | transposed
  DevBuf<uint32_t> row_start, row_blk, row_col;
  SchurBuildScratch tmp;
  uint64_t bytes() const {
    return dev_bytes(img_slot, slot_img, blk_start, ent_a, ent_b, pair_ij, iota, obs_pos, row_start, row_blk, row_col) +
           tmp.bytes();
  }
};

// Builds T from the handle's device arrays on stream s (the device is set, the stream does not capture).  On failure T
// stays not built and the handle usable.  *num_syncs (may be null): the stream synchronisations made.
pcd_status schur_structure_build(const pcd_ba* b, SchurStructure& T, hipStream_t s, int* num_syncs);

}  // namespace pcd

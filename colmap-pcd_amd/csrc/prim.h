// prim.h -- the rocPRIM device primitives the library uses, with each operation's arguments written once.
// rocPRIM wants two calls per operation: one with a null storage pointer that only reports the bytes of temporary
// storage, then the real one.  The *_at forms take the storage explicitly (nullptr: report `bytes`, touch nothing --
// voxel.hip sizes its arena with them); the forms with a DevBuf query, grow the buffer (grow-only, so one kept in a
// scratch stops allocating) and run.  Iterator, size and config types pass through unchanged: the kernels instantiated
// are those of the plain calls.
#pragma once
#include <cstring>  // rocprim's texture_cache_iterator.hpp needs memset declared first

#include <rocprim/rocprim.hpp>

#include "common.h"

namespace pcd {

// out[i] = init + in[0] + ... + in[i-1]
template <class In, class Out, class T>
inline hipError_t exclusive_sum_at(void* storage, size_t& bytes, In in, Out out, T init, size_t n, hipStream_t s) {
  return rocprim::exclusive_scan(storage, bytes, in, out, init, n, rocprim::plus<T>(), s);
}
// out[i] = in[0] + ... + in[i]  (this form only: the one caller is voxel.hip's arena path)
template <class In, class Out>
inline hipError_t inclusive_sum_at(void* storage, size_t& bytes, In in, Out out, size_t n, hipStream_t s) {
  using T = typename std::iterator_traits<In>::value_type;
  return rocprim::inclusive_scan(storage, bytes, in, out, n, rocprim::plus<T>(), s);
}
// stable sort of (key, value) pairs by the key bits [begin_bit, end_bit)
template <class Config = rocprim::default_config, class K, class V, class Size>
inline hipError_t sort_pairs_at(void* storage, size_t& bytes, K* keys_in, K* keys_out, V* vals_in, V* vals_out, Size n,
                                unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  return rocprim::radix_sort_pairs<Config>(storage, bytes, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, s);
}

// key bits of a sort whose keys are at most max_value (end_bit of sort_pairs): the smallest b with 2^b > max_value, 1 .. 32
inline unsigned key_bits(uint64_t max_value) {
  unsigned bits = 1;
  while (bits < 32 && (1ull << bits) <= max_value) ++bits;
  return bits;
}
// The largest temporary storage over exclusive sums of uint32_t of the given lengths and sorts of (uint32_t, uint32_t)
// pairs of the given shapes (n == 0: a sort that is not run, not asked about): what a scratch reserves ahead of its first
// launch so that no call has to grow the buffer.  No monotonicity in n is assumed.
struct SortShape { size_t n; unsigned end_bit; };
inline pcd_status prim_storage_u32(std::initializer_list<size_t> scans, std::initializer_list<SortShape> sorts, size_t& need) {
  uint32_t* const u = nullptr;   // a size query reads no pointer
  need = 0;
  size_t bytes = 0;
  for (size_t n : scans) {
    PCD_HIP_TRY(exclusive_sum_at(nullptr, bytes, u, u, 0u, n, nullptr));
    need = std::max(need, bytes);
  }
  for (const SortShape& k : sorts) {
    if (!k.n) continue;
    PCD_HIP_TRY(sort_pairs_at(nullptr, bytes, u, u, u, u, k.n, 0u, k.end_bit, nullptr));
    need = std::max(need, bytes);
  }
  return PCD_OK;
}

// size query, tmp.reserve, run: `op(storage, bytes)` is one of the forms above with its arguments bound
template <class Op>
inline pcd_status prim_run(DevBuf<char>& tmp, Op&& op) {
  size_t bytes = 0;
  PCD_HIP_TRY(op(nullptr, bytes));
  PCD_TRY(tmp.reserve(bytes));
  PCD_HIP_TRY(op(tmp.p, bytes));
  return PCD_OK;
}
template <class In, class Out, class T>
inline pcd_status exclusive_sum(DevBuf<char>& tmp, In in, Out out, T init, size_t n, hipStream_t s) {
  return prim_run(tmp, [&](void* st, size_t& b) { return exclusive_sum_at(st, b, in, out, init, n, s); });
}
template <class Config = rocprim::default_config, class K, class V, class Size>
inline pcd_status sort_pairs(DevBuf<char>& tmp, K* keys_in, K* keys_out, V* vals_in, V* vals_out, Size n,
                             unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  return prim_run(tmp, [&](void* st, size_t& b) {
    return sort_pairs_at<Config>(st, b, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, s);
  });
}

}  // namespace pcd

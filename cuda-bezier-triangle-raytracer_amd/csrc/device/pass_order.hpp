// pass_order.hpp -- the near-first order of a batch of collected leaves (trace.hip trace_segment), kept up while
// the batch is collected.  Plain C++: the host compiles it too (tests/cpp/pass_order_test.cpp).
//
// The order is the stable ascending order of the entries' keys: entry e's place is
//   place(e) = #{j : key(j) < key(e)} + #{j < e : key(j) == key(e)}.
// Entries arrive one at a time (e = 0, 1, ...), and the order of those seen so far is one 64-bit word: nibble p
// names the entry at place p (at most 16 entries).  When entry e arrives with key k it goes behind every earlier
// entry with key <= k (an equal key came earlier and stays in front: ties keep their collection order), so its
// place is their number,
//   front = #{j < e : key(j) <= k},
// and the entries at and behind that place -- exactly those with key > k -- move one place back.  No entry is
// ever moved: whoever runs the batch reads the word.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BZR_ORDER_FN __host__ __device__ __forceinline__
#else
#define BZR_ORDER_FN inline
#endif

namespace bzr_dev {

constexpr uint32_t kOrderEntries = 16;  // nibbles of the order word

// Entry `e` (< 16; e entries are in `order`) arrives and takes place `front` (<= e).
BZR_ORDER_FN uint64_t order_insert(uint64_t order, uint32_t e, uint32_t front) {
  const uint64_t below = (uint64_t(1) << (4u * front)) - 1u;  // the places in front of it (4 * front <= 60)
  return (order & below) | (uint64_t(e) << (4u * front)) | ((order & ~below) << 4);
}
// The entry at place p.
BZR_ORDER_FN uint32_t order_at(uint64_t order, uint32_t p) { return uint32_t(order >> (4u * p)) & 15u; }

}  // namespace bzr_dev

// index_home.h — the arithmetic the four open-addressing tables of an open stream share: the digest
// index over the book (book_index.h), the load per requestor (requestor_index.h), the tick's quota
// table (stream_quota.h) and the usage per requestor (stream_usage.h; DESIGN 3.3.11, 3.3.13, 3.3.14,
// 3.3.20). Plain C++, no HIP, no context: the home slot
// of a key is book_index_mix(key) & (slots - 1), and each table has the smallest power of two of slots
// that keeps its load at or below 1/2, never fewer than 1024 (index_slots). Written once for the kernels and
// the host calls, and for a host program that pins a restatement against it (tests/native/hash_home_test.cc),
// as admit_clip.h, lease_filter.h and fair_level.h are. The probe that starts at the home slot: slot_probe.h.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YDC_HOME_HD __host__ __device__ __forceinline__
#else
#define YDC_HOME_HD inline
#endif

namespace ydc {

constexpr uint32_t kIndexMinSlots = 1024;

// splitmix64's finaliser.
YDC_HOME_HD uint64_t book_index_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// Slots for n entries: the smallest power of two >= 2 n (load <= 1/2), at least kIndexMinSlots, at most 2^31.
inline uint32_t index_slots(uint64_t n) {
  uint32_t s = kIndexMinSlots;
  while (s < 2 * n && s < (1u << 31)) s <<= 1;
  return s;
}

// The tables' own names for it: a book of n entries (n <= 2^30), n entries of L and W together, a stream with
// max_tasks new requests per tick, n distinct requestors of the usage table.
inline uint32_t book_index_slots(uint32_t n) { return index_slots(n); }
inline uint32_t requestor_index_slots(uint64_t n) { return index_slots(n); }
inline uint32_t quota_slots(uint32_t max_tasks) { return index_slots(max_tasks); }
inline uint32_t usage_slots(uint64_t n) { return index_slots(n); }

}  // namespace ydc

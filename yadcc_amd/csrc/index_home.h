// index_home.h — the arithmetic the four open-addressing tables of an open stream share: the digest
// index over the book (book_index.h), the load per requestor (requestor_index.h), the tick's quota
// table (stream_quota.h) and the usage per requestor (stream_usage.h; DESIGN 3.3.11, 3.3.13, 3.3.14,
// 3.3.20). Plain C++, no HIP, no context: the home slot
// of a key is book_index_mix(key) & (slots - 1), and each table has the smallest power of two of slots
// that keeps its load at or below 1/2, never fewer than 1024. Written once for the kernels and the host
// calls, and for a host program that pins a restatement against it (tests/native/hash_home_test.cc), as
// admit_clip.h, lease_filter.h and fair_level.h are.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YDC_HOME_HD __host__ __device__ __forceinline__
#else
#define YDC_HOME_HD inline
#endif

namespace ydc {

constexpr uint32_t kBookIndexMinSlots = 1024;
constexpr uint32_t kRequestorMinSlots = 1024;
constexpr uint32_t kQuotaMinSlots = 1024;
constexpr uint32_t kUsageMinSlots = 1024;

// splitmix64's finaliser.
YDC_HOME_HD uint64_t book_index_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// Slots for a book of n entries.
inline uint32_t book_index_slots(uint32_t n) {
  uint32_t s = kBookIndexMinSlots;
  while (s < 2ull * n) s <<= 1;  // (n <= 2^30: at most 2^31)
  return s;
}

// Slots for n entries of L and W together.
inline uint32_t requestor_index_slots(uint64_t n) {
  uint32_t s = kRequestorMinSlots;
  while (s < 2 * n && s < (1u << 31)) s <<= 1;
  return s;
}

// Slots of the table of a stream with max_tasks new requests per tick (load <= 1/2).
inline uint32_t quota_slots(uint32_t max_tasks) {
  uint32_t s = kQuotaMinSlots;
  while (s < 2 * (uint64_t)max_tasks && s < (1u << 31)) s <<= 1;
  return s;
}

// Slots of the usage table (stream_usage.h) for n distinct requestors (load <= 1/2).
inline uint32_t usage_slots(uint64_t n) {
  uint32_t s = kUsageMinSlots;
  while (s < 2 * n && s < (1u << 31)) s <<= 1;
  return s;
}

}  // namespace ydc

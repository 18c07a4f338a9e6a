// usage_quanta.h — the interval arithmetic of the usage accounting (ydc_stream_usage_begin,
// ydc_usage_quanta). Plain C++, no HIP, no context: written once for the host's tick
// (which hands the device one word per tick) and for a host program that pins it against the rule
// written with 128-bit intermediates (tests/native/usage_quanta_test.cc), as admit_clip.h and
// fair_level.h are.
//
//   dq = floor(now / quantum) - floor(last / quantum)     as a uint64 modulo 2^64, quantum > 0.
//
// The division rounds toward minus infinity (clocks may be negative), so the sum of dq over a chain of
// ticks telescopes: floor(now_n / q) - floor(now_0 / q), whatever the ticks in between were. Valid for
// every pair of int64 clocks: each floor fits an int64 (|x / q| <= |x|), and the difference is taken in
// unsigned arithmetic, where it wraps instead of overflowing.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YDC_USAGE_HD __host__ __device__
#else
#define YDC_USAGE_HD
#endif

namespace ydc {

// floor(x / q) for q > 0.
YDC_USAGE_HD inline int64_t usage_floor_div(int64_t x, int64_t q) {
  const int64_t d = x / q;  // (toward zero; q > 0, so no INT64_MIN / -1)
  return (x % q < 0) ? d - 1 : d;
}

// quantum <= 0: 0 (the callers refuse it before they get here).
YDC_USAGE_HD inline uint64_t usage_quanta(int64_t last, int64_t now, int64_t quantum) {
  if (quantum <= 0) return 0;
  return (uint64_t)usage_floor_div(now, quantum) - (uint64_t)usage_floor_div(last, quantum);
}

}  // namespace ydc

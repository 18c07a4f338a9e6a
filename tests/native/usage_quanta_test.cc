// The interval arithmetic of usage_quanta.h against its rule written with 128-bit intermediates: the edges
// (INT64_MIN / INT64_MAX on either side, quantum 1 and INT64_MAX, negative clocks that are exact
// multiples) and a seeded sweep of 10^5 triples. ASan + UBSan, no GPU
// (tests/test_stream_usage_binding.py builds and runs it).
#include "usage_quanta.h"

#include <cstdint>
#include <cstdio>
#include <random>

typedef __int128 i128;

static int g_failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                 \
    }                                                               \
  } while (0)

// floor(x / q), q > 0, by the definition: the largest d with d q <= x.
static i128 floor128(i128 x, i128 q) {
  i128 d = x / q;
  while (d * q > x) --d;
  while ((d + 1) * q <= x) ++d;
  return d;
}

static uint64_t by_the_rule(int64_t last, int64_t now, int64_t q) {
  const i128 d = floor128(now, q) - floor128(last, q);
  return (uint64_t)(unsigned __int128)d;  // modulo 2^64
}

static void compare(int64_t last, int64_t now, int64_t q) {
  const uint64_t got = ydc::usage_quanta(last, now, q), want = by_the_rule(last, now, q);
  if (got != want) {
    std::printf("FAILED last %lld now %lld quantum %lld: got %llu want %llu\n", (long long)last, (long long)now, (long long)q,
                (unsigned long long)got, (unsigned long long)want);
    ++g_failures;
  }
}

int main() {
  const int64_t lo = INT64_MIN, hi = INT64_MAX;
  const int64_t edges[] = {lo, lo + 1, lo + 2, -1000000007, -1001, -1000, -999, -7, -2, -1, 0, 1, 2, 6, 7, 8, 999, 1000, 1001,
                           1000000007, hi - 2, hi - 1, hi};
  const int64_t quanta[] = {1, 2, 3, 7, 1000, 1000000007, (int64_t)1 << 32, ((int64_t)1 << 62) + 1, hi - 1, hi};
  for (int64_t q : quanta)
    for (int64_t a : edges)
      for (int64_t b : edges) compare(a, b, q);
  // Negative dividends that are exact multiples, and their neighbours.
  for (int64_t q : {1ll, 7ll, 1000ll, 4294967296ll})
    for (int64_t k = -5; k <= 5; ++k)
      for (int64_t d = -1; d <= 1; ++d) {
        compare(k * q + d, 0, q);
        compare(0, k * q + d, q);
        compare(-3 * q, k * q + d, q);
      }
  // Hand values.
  CHECK(ydc::usage_quanta(-1, 0, 10) == 1);
  CHECK(ydc::usage_quanta(0, 9, 10) == 0);
  CHECK(ydc::usage_quanta(9, 10, 10) == 1);
  CHECK(ydc::usage_quanta(-10, -1, 10) == 0);
  CHECK(ydc::usage_quanta(-11, -10, 10) == 1);
  CHECK(ydc::usage_quanta(5, 5, 1) == 0);
  CHECK(ydc::usage_quanta(lo, hi, 1) == ~0ull);
  CHECK(ydc::usage_quanta(hi, lo, 1) == 1ull);  // (modulo 2^64)
  CHECK(ydc::usage_quanta(lo, hi, hi) == 3ull);  // floor(lo / hi) == -2
  CHECK(ydc::usage_quanta(3, 4, 0) == 0 && ydc::usage_quanta(3, 4, -5) == 0);
  // The sum over a chain of ticks telescopes.
  std::mt19937_64 rng(20261021);
  for (int round = 0; round < 200; ++round) {
    const int64_t q = (int64_t)(rng() % 1000) + 1;
    int64_t t = (int64_t)(rng() % 2000000) - 1000000;
    const int64_t t0 = t;
    uint64_t sum = 0;
    for (int i = 0; i < 50; ++i) {
      const int64_t next = t + (int64_t)(rng() % (3 * (uint64_t)q));
      sum += ydc::usage_quanta(t, next, q);
      t = next;
    }
    CHECK(sum == ydc::usage_quanta(t0, t, q));
  }
  // A seeded sweep: 10^5 triples, clocks over the whole range, quanta of every magnitude.
  for (int i = 0; i < 100000; ++i) {
    const int64_t a = (int64_t)rng(), b = (int64_t)rng();
    const unsigned shift = (unsigned)(rng() % 63);
    int64_t q = (int64_t)((rng() >> 1) >> shift);
    if (q <= 0) q = 1;
    compare(a, b, q);
    compare(a >> shift, b >> shift, q);
  }
  if (g_failures) {
    std::printf("%d failures\n", g_failures);
    return 1;
  }
  std::printf("USAGE-QUANTA-OK\n");
  return 0;
}

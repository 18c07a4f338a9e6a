// The fair-share arithmetic of fair_level.h against the literal progressive fill of its header with
// 128-bit sums: hand-written edges (n = 0, values at 2^32 - 2, a saturating pool) and a seeded sweep.
// ASan + UBSan, no GPU (`make fairlevel`; tests/test_stream_fair_binding.py builds and runs it).
#include "fair_level.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef unsigned __int128 u128;
using ydc::kFairPoolMax;
using ydc::kFairUnlimited;

static int g_failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                            \
    }                                                          \
  } while (0)

static u128 min128(u128 a, u128 b) { return a < b ? a : b; }
static u128 max128(u128 a, u128 b) { return a > b ? a : b; }

struct Case {
  std::vector<uint32_t> h, a, cap;  // cap == kFairUnlimited: fair
  uint64_t others, pool;
};

static u128 f_at(const Case& c, u128 level) {
  u128 s = c.others;
  for (size_t i = 0; i < c.h.size(); ++i) {
    const u128 lv = c.cap[i] == kFairUnlimited ? level : (u128)c.cap[i];
    s += max128(c.h[i], min128((u128)c.h[i] + c.a[i], lv));
  }
  return s;
}

// The written rule. step: the fill raises the level by `step` while it can and then by one (the
// literal fill where the numbers are small; with large ones the coarse steps only save time, every
// comparison is the rule's own).
static uint32_t by_the_rule(const Case& c) {
  const u128 P = min128(c.pool, kFairPoolMax);
  u128 D = 0;
  bool any = false;
  for (size_t i = 0; i < c.h.size(); ++i)
    if (c.cap[i] == kFairUnlimited) {
      any = true;
      D = max128(D, (u128)c.h[i] + c.a[i]);
    }
  if (!any || f_at(c, D) <= P) return kFairUnlimited;
  if (f_at(c, 0) > P) return 0;
  u128 lv = 0;
  for (u128 step = (u128)1 << 40; step >= 1; step >>= 1)
    while (lv + step < D && f_at(c, lv + step) <= P) lv += step;
  CHECK(lv < D && f_at(c, lv) <= P && f_at(c, lv + 1) > P);
  return (uint32_t)lv;
}

static uint32_t by_the_header(const Case& c, bool null_caps = false) {
  return ydc::fair_level(c.h.data(), c.a.data(), null_caps ? nullptr : c.cap.data(), (uint32_t)c.h.size(), c.others,
                         c.pool);
}

int main() {
  const uint32_t U = kFairUnlimited, BIG = 0xFFFFFFFEu;
  // n = 0, and nobody fair
  CHECK(ydc::fair_level(nullptr, nullptr, nullptr, 0, 0, 0) == U);
  CHECK(ydc::fair_level(nullptr, nullptr, nullptr, 0, ~0ull, 5) == U);
  CHECK(by_the_header(Case{{1, 0}, {5, 9}, {3, 0}, 7, 0}) == U);
  // the hand vector: O = 2, P = 20, askers (0, 10), (3, 10), (8, 4): f(0 .. 6) = 13 14 15 16 18 20 22
  const Case hand{{0, 3, 8}, {10, 10, 4}, {U, U, U}, 2, 20};
  const unsigned want_f[7] = {13, 14, 15, 16, 18, 20, 22};
  for (unsigned lv = 0; lv < 7; ++lv) CHECK(f_at(hand, lv) == want_f[lv]);
  CHECK(by_the_header(hand) == 5 && by_the_rule(hand) == 5 && by_the_header(hand, true) == 5);
  // f(D) == P and P + 1; f(0) == P and P + 1
  Case c = hand;
  c.pool = 37;
  CHECK(by_the_header(c) == U);
  c.pool = 36;
  CHECK(by_the_header(c) == 12);
  c.pool = 13;
  CHECK(by_the_header(c) == 0);
  c.pool = 12;
  CHECK(by_the_header(c) == 0);
  // values at 2^32 - 2 and a saturating pool
  CHECK(by_the_header(Case{{BIG, 0}, {BIG, 5}, {U, U}, 0, 1ull << 40}) == 0);
  CHECK(by_the_header(Case{{0}, {BIG}, {U}, 0, ~0ull}) == U);
  CHECK(by_the_header(Case{{0}, {U}, {U}, 0, ~0ull}) == BIG);
  CHECK(by_the_header(Case{{BIG, BIG, BIG}, {BIG, BIG, BIG}, {U, BIG, U}, ~0ull, ~0ull}) == 0);
  CHECK(ydc::fair_pool(1ull << 40, 100) == kFairPoolMax && ydc::fair_pool(199, 50) == 99 && ydc::fair_pool(3, 150) == 4);
  CHECK(ydc::fair_pool(~0ull, 1) == kFairPoolMax && ydc::fair_pool(~0ull, 0xFFFFFFFFu) == kFairPoolMax);
  CHECK(ydc::fair_pool(0xFFFFFFFEull * 100, 1) == kFairPoolMax && ydc::fair_pool(0xFFFFFFFDull * 100 + 99, 1) == 0xFFFFFFFDull);
  CHECK(ydc::fair_top(8, 0, 4, 0) == 4 && ydc::fair_top(2, 1, 4, 1) == 2 && ydc::fair_top(8, 8, 4, 0) == 0 &&
        ydc::fair_top(8, 0, 0, 0) == 0 && ydc::fair_top(8, 0, 4, 2) == 0);
  CHECK(ydc::fair_cap(5, 0, U) == 5 && ydc::fair_cap(2, 3, U) == 3 && ydc::fair_cap(U, 3, 40) == 40 && ydc::fair_cap(9, 0, 4) == 4);
  // the sweep: small numbers (the literal fill), then numbers around 2^32 - 2
  std::mt19937_64 rng(20240917);
  unsigned seen[3] = {0, 0, 0};
  for (int it = 0; it < 60000; ++it) {
    const bool large = it % 4 == 3;
    const uint32_t n = (uint32_t)(rng() % 7);
    Case k;
    auto val = [&](uint32_t small) -> uint32_t {
      if (!large) return (uint32_t)(rng() % small);
      switch (rng() % 4) {
        case 0: return BIG - (uint32_t)(rng() % 3);
        case 1: return (uint32_t)(rng() % 5);
        default: return (uint32_t)rng() & 0xFFFFFFFEu;
      }
    };
    for (uint32_t i = 0; i < n; ++i) {
      k.h.push_back(val(30));
      k.a.push_back(val(30));
      k.cap.push_back(rng() % 4 == 0 ? val(40) : U);
    }
    k.others = large ? (rng() % 3 ? rng() % (1ull << 33) : rng()) : rng() % 40;
    k.pool = large ? (rng() % 3 ? rng() % (1ull << 34) : rng()) : rng() % 160;
    const uint32_t got = by_the_header(k), want = by_the_rule(k);
    if (got != want) std::printf("case %d: header %u rule %u\n", it, got, want);
    CHECK(got == want);
    ++seen[got == U ? 0 : got == 0 ? 1 : 2];
  }
  CHECK(seen[0] > 1000 && seen[1] > 1000 && seen[2] > 1000);
  if (g_failures) {
    std::printf("%d checks FAILED\n", g_failures);
    return 1;
  }
  std::printf("FAIR-LEVEL-OK (levels: %u unlimited, %u zero, %u between)\n", seen[0], seen[1], seen[2]);
  return 0;
}

// The arithmetic of a sharded batch (yadcc_amd/csrc/shard_plan.h) against the rules written out
// below from their descriptions, with 128-bit intermediates, under ASan + UBSan. Includes nothing
// but that header. Named edges first (empty and tiny batches, N / 8 crossing 8192, saturation at
// N = 2^32 - 1 with the widest margin, tuned margins of 0 and 2^31, registries around both
// sort_items thresholds, pass hints around the clamp, the ring of 64 counters across its wrap,
// slices with zeros), then a seeded sweep of 10^5 random inputs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "shard_plan.h"

typedef unsigned __int128 u128;

static int g_failures = 0;
#define EXPECT(cond, ...)                                       \
  do {                                                          \
    if (!(cond)) {                                              \
      ++g_failures;                                             \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fprintf(stderr, "\n");                               \
    }                                                           \
  } while (0)

static const uint32_t kThreads = 256;  // threads of a sort block (kernels.h: kSortThreads)

// The rule of the window: margin = the tuned one, or scale * max(N / 8, 8192); the window holds
// N + 2 margins + an eighth of the registry's slots + 65536, and never more than the registry has;
// the margin handed to the kernel saturates at 2^31 - 1; 2 keys per thread up to 300000 slots, 4 up
// to 700000, 8 beyond; tiles of threads * keys slots, rounded up, at least one.
static void check_window(uint32_t N, uint32_t scale, int64_t tuned, uint32_t full) {
  const ydc::ShardWindow w = ydc::shard_window(N, scale, tuned, full, kThreads);
  u128 margin;
  if (tuned >= 0) {
    margin = (u128)(uint64_t)tuned;
  } else {
    u128 eighth = N / 8;
    margin = (u128)scale * (eighth > 8192 ? eighth : (u128)8192);
  }
  u128 window = (u128)N + margin + margin + (u128)(full / 8) + 65536;
  const u128 bound = window < (u128)full ? window : (u128)full;
  const u128 sat = margin < (u128)0x7FFFFFFFu ? margin : (u128)0x7FFFFFFFu;
  const uint32_t items = bound <= 300000 ? 2 : bound <= 700000 ? 4 : 8;
  u128 tiles = (bound + (u128)kThreads * items - 1) / ((u128)kThreads * items);
  if (tiles < 1) tiles = 1;
  EXPECT((u128)w.win_margin == sat, "win_margin %u (N %u scale %u tuned %lld full %u)", w.win_margin, N, scale,
         (long long)tuned, full);
  EXPECT((u128)w.slot_bound == bound, "slot_bound %u (N %u scale %u tuned %lld full %u)", w.slot_bound, N, scale,
         (long long)tuned, full);
  EXPECT(w.sort_items == items, "sort_items %u, want %u (slot_bound %u)", w.sort_items, items, w.slot_bound);
  EXPECT((u128)w.n_tiles == tiles, "n_tiles %u (slot_bound %u)", w.n_tiles, w.slot_bound);
  EXPECT(w.win_margin <= 0x7FFFFFFFu && w.slot_bound <= full && w.n_tiles >= 1, "ranges");
}

// The rule of the pass groups: the first is the hint, at least 2 and at most 12; later ones are 3.
static void check_group(uint32_t launched, uint32_t hint) {
  uint32_t want = 3;
  if (launched == 0) want = hint < 2 ? 2 : hint > 12 ? 12 : hint;
  const uint32_t got = ydc::shard_pass_group(launched, hint);
  EXPECT(got == want, "pass group %u, want %u (launched %u, hint %u)", got, want, launched, hint);
}

// The rule of `rounds`: pass r's count is at ring[r mod 64]; of the group's passes, the first
// whose count is 0, counted from 1. (The caller asks only when the group's last pass has 0.)
static void check_rounds(const std::vector<uint32_t>& ring, uint32_t first, uint32_t count) {
  uint32_t want = first + count;
  for (uint64_t r = first; r < (uint64_t)first + count; ++r)
    if (ring[(size_t)(r % 64)] == 0) {
      want = (uint32_t)(r + 1);
      break;
    }
  const uint32_t got = ydc::shard_rounds(ring.data(), first, count);
  EXPECT(got == want, "rounds %u, want %u (first %u, count %u)", got, want, first, count);
}

// The rule of the slices: the largest size but at least 1, the sum, the sum of the ranks before.
static void check_slices(const std::vector<uint32_t>& sizes, uint32_t rank) {
  u128 total = 0, off = 0, max_n = 1;
  for (size_t r = 0; r < sizes.size(); ++r) {
    if (sizes[r] > max_n) max_n = sizes[r];
    if (r < rank) off += sizes[r];
    total += sizes[r];
  }
  const ydc::ShardSlices s = ydc::shard_slices(sizes.data(), (uint32_t)sizes.size(), rank);
  EXPECT((u128)s.max_n == max_n && (u128)s.total == total && (u128)s.my_off == off,
         "slices (%u, %u, %u) for rank %u of %zu", s.max_n, s.total, s.my_off, rank, sizes.size());
}

// The rule of the predicate, clause by clause.
static void check_windowed(const ydc::WindowedInputs& w) {
  bool want = true;
  if (w.n_ranks <= 1) want = false;
  if (!w.shard_sort) want = false;
  if (!w.exact_keys) want = false;
  if (w.n_parts != 1) want = false;
  if (w.use_generic) want = false;
  if (w.n_classes < 2) want = false;
  if (w.any_shared) want = false;
  if (w.binsort && w.group_binsort) want = false;
  EXPECT(ydc::shard_windowed(w) == want, "windowed, want %d", (int)want);
}

static ydc::WindowedInputs windowed_from_bits(uint32_t bits, uint32_t ranks, uint32_t parts, uint32_t classes) {
  ydc::WindowedInputs w;
  w.n_ranks = ranks;
  w.n_parts = parts;
  w.n_classes = classes;
  w.shard_sort = bits & 1;
  w.exact_keys = bits & 2;
  w.use_generic = bits & 4;
  w.any_shared = bits & 8;
  w.binsort = bits & 16;
  w.group_binsort = bits & 32;
  return w;
}

int main() {
  // The window: named edges.
  const uint32_t Ns[] = {0u, 1u, 65535u, 65536u, 65537u, 0xFFFFFFFFu};
  const uint32_t fulls[] = {0u,      1u,      1000u,   65536u,  299999u,  300000u,    300001u,
                            699999u, 700000u, 700001u, 5000000u, 0x7FFFFFFFu, 0xFFFFFFFFu};
  const int64_t tuned[] = {-1, 0, 1, 8192, (int64_t)1 << 31, ((int64_t)1 << 31) + 1};
  for (uint32_t N : Ns)
    for (uint32_t full : fulls)
      for (int64_t t : tuned)
        for (uint32_t scale : {1u, 2u, 64u}) check_window(N, scale, t, full);
  {
    // Saturation, no wrap: 64 * (2^32 - 1) / 8 is far beyond 2^31.
    const ydc::ShardWindow w = ydc::shard_window(0xFFFFFFFFu, 64, -1, 0xFFFFFFFFu, kThreads);
    EXPECT(w.win_margin == 0x7FFFFFFFu && w.slot_bound == 0xFFFFFFFFu && w.sort_items == 8, "saturation");
    // N / 8 crosses 8192 between 65535 and 65536: the margin stays 8192 up to there.
    EXPECT(ydc::shard_window(65535, 1, -1, 0xFFFFFFFFu, kThreads).win_margin == 8192, "margin below the crossing");
    EXPECT(ydc::shard_window(65536, 1, -1, 0xFFFFFFFFu, kThreads).win_margin == 8192, "margin at the crossing");
    EXPECT(ydc::shard_window(65544, 1, -1, 0xFFFFFFFFu, kThreads).win_margin == 8193, "margin above the crossing");
    // A registry smaller than the window: the min picks the registry.
    EXPECT(ydc::shard_window(100000, 1, -1, 1000, kThreads).slot_bound == 1000, "the registry bounds the window");
    EXPECT(ydc::shard_window(0, 1, 0, 0, kThreads).n_tiles == 1, "at least one tile");
    // Windows around the thresholds with a tuned margin of 0: N + full / 8 + 65536.
    EXPECT(ydc::shard_window(300000 - 65536 - 125000, 1, 0, 1000000, kThreads).sort_items == 2, "at 300000");
    EXPECT(ydc::shard_window(300001 - 65536 - 125000, 1, 0, 1000000, kThreads).sort_items == 4, "above 300000");
    EXPECT(ydc::shard_window(700000 - 65536 - 125000, 1, 0, 1000000, kThreads).sort_items == 4, "at 700000");
    EXPECT(ydc::shard_window(700001 - 65536 - 125000, 1, 0, 1000000, kThreads).sort_items == 8, "above 700000");
  }
  for (uint32_t s : {1u, 2u, 16u, 32u, 64u})
    EXPECT(ydc::shard_margin_after_miss(s) == (s >= 32 ? 64u : 2 * s), "margin scale after a miss of %u", s);

  // Pass groups.
  for (uint32_t hint : {0u, 1u, 2u, 3u, 11u, 12u, 13u, 0xFFFFFFFFu})
    for (uint32_t launched : {0u, 2u, 12u, 255u, 200001u}) check_group(launched, hint);

  // Rounds: the first zero at the group's first, middle and last pass; across the wrap of the ring.
  for (uint32_t first : {0u, 3u, 61u, 62u, 63u, 64u, 126u, 200000u})
    for (uint32_t count : {2u, 3u, 12u})
      for (uint32_t zero_at = 0; zero_at < count; ++zero_at) {
        std::vector<uint32_t> ring(64, 7u);  // stale counts of earlier passes everywhere else
        for (uint32_t k = zero_at; k < count; ++k) ring[(first + k) & 63] = k == zero_at || k == count - 1 ? 0u : 5u;
        check_rounds(ring, first, count);
        EXPECT(ydc::shard_rounds(ring.data(), first, count) == first + zero_at + 1, "first zero at %u of %u from %u",
               zero_at, count, first);
      }

  // Slices: zeros at the front, in the middle, at the end; all zero.
  const std::vector<std::vector<uint32_t>> slices = {
      {0, 0, 5, 9}, {4, 0, 0, 9}, {4, 9, 0, 0}, {0, 0, 0}, {0}, {7}, {0, 3, 0, 3, 0}, {1000000000u, 2000000000u, 5u}};
  for (const auto& sz : slices)
    for (uint32_t rank = 0; rank < sz.size(); ++rank) check_slices(sz, rank);
  {
    const uint32_t none[3] = {0, 0, 0};
    const ydc::ShardSlices s = ydc::shard_slices(none, 3, 2);
    EXPECT(s.max_n == 1 && s.total == 0 && s.my_off == 0, "an empty batch still sends one word");
  }

  // The predicate: every combination of the switches, ranks 0 .. 3, parts 0 .. 2, classes 0 .. 3.
  for (uint32_t bits = 0; bits < 64; ++bits)
    for (uint32_t ranks = 0; ranks < 4; ++ranks)
      for (uint32_t parts = 0; parts < 3; ++parts)
        for (uint32_t classes = 0; classes < 4; ++classes) check_windowed(windowed_from_bits(bits, ranks, parts, classes));

  // The sweep.
  std::mt19937_64 rng(20240607);
  auto any32 = [&]() -> uint32_t {
    switch (rng() % 4) {
      case 0: return (uint32_t)(rng() % 100);
      case 1: return (uint32_t)(rng() % 2000000);
      case 2: return (uint32_t)(0xFFFFFFFFu - rng() % 100);
      default: return (uint32_t)rng();
    }
  };
  for (int it = 0; it < 100000; ++it) {
    const uint32_t scale = 1u << (rng() % 7);
    int64_t t = -1;
    if (rng() % 3 == 0) t = (int64_t)(rng() % 5 == 0 ? rng() >> 24 : rng() % 3000000);  // below 2^40
    check_window(any32(), scale, t, any32());
    check_group(rng() % 2 ? 0 : any32(), any32());
    std::vector<uint32_t> ring(64);
    for (auto& v : ring) v = rng() % 3 ? (uint32_t)(rng() % 4) : 0u;
    const uint32_t first = rng() % 4 ? (uint32_t)(rng() % 200) : any32() % 0xFFFFFF00u;
    const uint32_t count = 1 + (uint32_t)(rng() % 12);
    ring[(first + count - 1) & 63] = 0;  // what the caller guarantees
    check_rounds(ring, first, count);
    std::vector<uint32_t> sizes(1 + rng() % 16);
    for (auto& v : sizes) v = rng() % 3 ? (uint32_t)(rng() % 100000000u) : 0u;  // 16 slices of < 10^8 sum below 2^32
    check_slices(sizes, (uint32_t)(rng() % sizes.size()));
    check_windowed(windowed_from_bits((uint32_t)(rng() % 64), (uint32_t)(rng() % 9), (uint32_t)(rng() % 3),
                                      (uint32_t)(rng() % 300)));
  }

  if (g_failures) {
    std::fprintf(stderr, "%d failures\n", g_failures);
    return 1;
  }
  std::printf("SHARD-PLAN-OK\n");
  return 0;
}

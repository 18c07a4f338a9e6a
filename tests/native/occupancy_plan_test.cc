// The occupancy rule of a batch (yadcc_amd/csrc/occupancy_plan.h) row by row, as a program of its
// own: built with the host sanitizers (`make occupancyplan`; tests/test_occupancy_plan.py), no GPU,
// no HIP. The width of a k_bin_sort workgroup: narrow for a batch that may have a neighbour on the
// other lane, wide on a device of its own; a forced width wins; a width no build has is the rule's.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "occupancy_plan.h"

using namespace ydc;

static int g_failed = 0;

static void expect(bool ok, const char* what, uint32_t tuned, bool beside, uint32_t got) {
  if (!ok) {
    ++g_failed;
    std::printf("FAILED: %s (tuned %u, beside %d: %u)\n", what, tuned, (int)beside, got);
  }
}

int main() {
  struct Row {
    uint32_t tuned;
    bool beside;
    uint32_t want;
  };
  static const Row kRows[] = {
      {0, false, 1024},    {0, true, 512},        // the rule
      {512, false, 512},   {512, true, 512},      // forced narrow
      {1024, false, 1024}, {1024, true, 1024},    // forced wide
      {1, false, 1024},    {1, true, 512},        // widths no build has: the rule
      {64, false, 1024},   {64, true, 512},
      {256, false, 1024},  {256, true, 512},
      {511, false, 1024},  {513, true, 512},
      {768, false, 1024},  {768, true, 512},
      {1023, false, 1024}, {1025, true, 512},
      {2048, false, 1024}, {2048, true, 512},
      {0xFFFFFFFFu, false, 1024}, {0xFFFFFFFFu, true, 512},
  };
  for (const Row& r : kRows) {
    const uint32_t got = bin_sort_threads(r.tuned, r.beside);
    expect(got == r.want, "the table's width", r.tuned, r.beside, got);
    expect(got == kBinThreadsNarrow || got == kBinThreadsWide, "a width bin_sort.h builds", r.tuned, r.beside, got);
  }
  // Every value around the two builds' widths, both ways.
  for (uint32_t t = 500; t <= 1030; ++t) {
    for (bool beside : {false, true}) {
      const uint32_t got = bin_sort_threads(t, beside);
      const uint32_t want = t == 512 || t == 1024 ? t : (beside ? 512u : 1024u);
      expect(got == want, "only 512 and 1024 force a width", t, beside, got);
    }
  }
  static_assert(bin_sort_threads(0, true) == 512 && bin_sort_threads(0, false) == 1024, "constexpr");
  static_assert(kBinThreadsNarrow == 512 && kBinThreadsWide == 1024, "the two builds of bin_sort.h");

  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("OCCUPANCY-PLAN-OK\n");
  return 0;
}

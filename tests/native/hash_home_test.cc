// The arithmetic the digest index, the requestor index, the quota table and the usage table share
// (index_home.h), printed for tests/test_hash_index_model.py and tests/test_usage_table_model.py, which
// compare it with the restatement of tests/hash_index_cases.py.
// Includes only index_home.h; built with ASan + UBSan and run as a program of its own.
//
// stdin, one request per line:  k <key, hex>  ->  <book_index_mix(key), hex>
//                               s <n, decimal> ->  <book_index_slots(n)> <requestor_index_slots(n)> <quota_slots(n)>
//                               u <n, decimal> ->  <usage_slots(n)>          (n up to 2^32)
// "HASH-HOME-OK <lines answered>" ends the output; a line it cannot read ends the program with status 2.
#include <cinttypes>
#include <cstdio>

#include "index_home.h"

// The four tables' slot counts are one function. The digest index once had a loop of its own, without the
// 2^31 ceiling; over its documented range, n <= 2^30, that loop and the shared one agree.
static bool book_slots_agree() {
  for (uint32_t k = 0; k <= 30; ++k)
    for (int64_t d = -2; d <= 2; ++d) {
      const int64_t n = (int64_t(1) << k) + d;
      if (n < 0 || n > (int64_t(1) << 30)) continue;
      uint32_t s = 1024;
      while (s < 2ull * (uint64_t)n) s <<= 1;
      if (ydc::book_index_slots((uint32_t)n) != s || ydc::index_slots((uint64_t)n) != s) return false;
    }
  return ydc::kIndexMinSlots == 1024 && ydc::index_slots(0) == 1024 && ydc::index_slots(1ull << 32) == (1u << 31);
}

int main() {
  if (!book_slots_agree()) {
    std::fprintf(stderr, "book_index_slots differs from its former loop\n");
    return 3;
  }
  char line[128];
  unsigned long long answered = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    uint64_t v = 0;
    if (std::sscanf(line, "k %" SCNx64, &v) == 1) {
      std::printf("%016" PRIx64 "\n", ydc::book_index_mix(v));
    } else if (std::sscanf(line, "s %" SCNu64, &v) == 1 && v <= (1ull << 30)) {
      std::printf("%u %u %u\n", (unsigned)ydc::book_index_slots((uint32_t)v), (unsigned)ydc::requestor_index_slots(v),
                  (unsigned)ydc::quota_slots((uint32_t)v));
    } else if (std::sscanf(line, "u %" SCNu64, &v) == 1 && v <= (1ull << 32)) {
      std::printf("%u\n", (unsigned)ydc::usage_slots(v));
    } else {
      std::fprintf(stderr, "cannot read: %s", line);
      return 2;
    }
    ++answered;
  }
  std::printf("HASH-HOME-OK %llu\n", answered);
  return 0;
}

// The admission arithmetic of admit_clip.h against the rule of its header written out row by row
// with 128-bit sums, on hand-written edges and a seeded sweep that includes wants and loads near
// 2^32 - 1. ASan + UBSan, no GPU (tests/test_stream_requestor_model.py builds and runs it).
#include "admit_clip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using ydc::AdmitLoad;
typedef unsigned __int128 u128;

static int g_failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                            \
    }                                                          \
  } while (0)

static u128 min128(u128 a, u128 b) { return a < b ? a : b; }

// The written rule: O(n^2), nothing carried from row to row.
static void by_the_rule(const std::vector<uint32_t>& ip, const std::vector<uint32_t>& imm, const uint32_t* pre,
                        const std::vector<AdmitLoad>& load, uint32_t cap, std::vector<uint32_t>* out_imm,
                        std::vector<uint32_t>* out_pre) {
  const size_t n = ip.size();
  out_imm->assign(n, 0);
  out_pre->assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    u128 before = 0;
    for (size_t j = 0; j < i; ++j)
      if (ip[j] == ip[i]) before += (u128)imm[j] + (pre ? pre[j] : 0u);
    const u128 held = (u128)load[i].leases + load[i].waiting_rows;
    const u128 room = (u128)cap - min128(cap, held);
    const u128 want = (u128)imm[i] + (pre ? pre[i] : 0u);
    const u128 a = min128(before + want, room) - min128(before, room);
    (*out_imm)[i] = (uint32_t)min128(imm[i], a);
    (*out_pre)[i] = (uint32_t)(a - (*out_imm)[i]);
  }
}

static void compare(const std::vector<uint32_t>& ip, const std::vector<uint32_t>& imm, const std::vector<uint32_t>& pre,
                    bool with_pre, const std::vector<AdmitLoad>& load, uint32_t cap) {
  const uint32_t n = (uint32_t)ip.size();
  std::vector<uint32_t> want_imm, want_pre, got_imm(n, 0xABCDu), got_pre(n, 0xABCDu);
  by_the_rule(ip, imm, with_pre ? pre.data() : nullptr, load, cap, &want_imm, &want_pre);
  const bool ok = ydc::admit_clip(ip.data(), imm.data(), with_pre ? pre.data() : nullptr, n, load.data(), cap,
                                  got_imm.data(), with_pre ? got_pre.data() : nullptr);
  CHECK(ok);
  for (uint32_t i = 0; i < n; ++i) {
    CHECK(got_imm[i] == want_imm[i]);
    if (with_pre) CHECK(got_pre[i] == want_pre[i]);
    else CHECK(want_pre[i] == 0 && got_pre[i] == 0xABCDu);  // (a NULL column is not written)
  }
}

static AdmitLoad held(uint32_t ip, uint32_t leases, uint32_t rows) { return AdmitLoad{ip, leases, 0, 0, 0, rows}; }

int main() {
  const uint32_t M = 0xFFFFFFFFu;
  // The cap reached in the middle of a row; prefetch clipped first; outstanding > cap.
  compare({5, 5, 5}, {4, 4, 4}, {0, 0, 0}, true, {held(5, 3, 1), held(5, 3, 1), held(5, 3, 1)}, 10);
  compare({5, 5}, {3, 1}, {4, 0}, true, {held(5, 5, 0), held(5, 5, 0)}, 10);
  compare({5, 5}, {1, 2}, {1, 0}, true, {held(5, 8, 9), held(5, 8, 9)}, 10);
  // Near 2^32 - 1: wants whose sum passes 2^32 and 2^33, loads whose sum does, the largest cap.
  compare({1, 1, 1}, {M, M, M}, {M, M, M}, true, {held(1, 0, 0), held(1, 0, 0), held(1, 0, 0)}, M);
  compare({1, 1}, {M - 1, 7}, {M, M}, true, {held(1, 1, 0), held(1, 1, 0)}, M);
  compare({1, 2}, {M, M}, {0, 1}, true, {held(1, M - 1, M - 1), held(2, M - 1, 0)}, M);
  compare({1}, {M}, {}, false, {held(1, M - 1, 0)}, M);
  compare({1}, {3}, {3}, true, {held(1, M - 1, M - 1)}, 0);
  compare({}, {}, {}, true, {}, 5);
  {  // An unknown load refuses, and writes nothing.
    std::vector<uint32_t> ip{1, 2}, imm{1, 1}, out{7, 7};
    std::vector<AdmitLoad> load{held(1, 0, 0), held(2, ydc::kAdmitUnknown, 0)};
    CHECK(!ydc::admit_clip(ip.data(), imm.data(), nullptr, 2, load.data(), 5, out.data(), nullptr));
    CHECK(out[0] == 7 && out[1] == 7);
  }
  std::mt19937_64 rng(12345);
  auto pick = [&](int kind) -> uint32_t {
    switch (kind % 4) {
      case 0: return (uint32_t)(rng() % 8);
      case 1: return M - (uint32_t)(rng() % 4);
      case 2: return (uint32_t)(rng() % 2) ? 0u : (uint32_t)rng();
      default: return (uint32_t)rng();
    }
  };
  for (int c = 0; c < 20000; ++c) {
    const size_t n = 1 + rng() % 12;
    const int kind = (int)(rng() % 16);
    std::vector<uint32_t> ip(n), imm(n), pre(n);
    std::vector<AdmitLoad> load(n);
    // (leases == 2^32 - 1 means "unknown": the largest known count is one below)
    const uint32_t l[3] = {std::min(pick(kind), M - 1), std::min(pick(kind >> 2), M - 1), std::min(pick(kind), M - 1)}, r[3] = {pick(kind >> 2), pick(kind), pick(kind >> 2)};
    for (size_t i = 0; i < n; ++i) {
      const uint32_t who = (uint32_t)(rng() % 3);
      ip[i] = who == 2 ? M : who;  // (0xFFFFFFFF is a requestor like any other)
      imm[i] = pick(kind >> 1);
      pre[i] = pick(kind >> 3);
      load[i] = held(ip[i], l[who], r[who]);
    }
    compare(ip, imm, pre, (c & 3) != 0, load, pick(kind >> 1));
  }
  if (g_failures) {
    std::printf("%d checks failed\n", g_failures);
    return 1;
  }
  std::printf("ADMIT-CLIP-OK\n");
  return 0;
}

// fair_level.h — the arithmetic of the fair-share level (ydc_stream_quota_fair, ydc_fair_level; DESIGN
// 3.3.17). Plain C++, no HIP, no context: written once for the host call (ydc_fair_level) and for the
// tick's own launch on the device (stream_fair.h, k_fair_level), as admit_clip.h and lease_filter.h are.
//
//   top(s)   = 0 if the servant is short of memory, max_tasks == 0 or load >= nproc, else
//              min(max_tasks, nproc): servant_slot_count of dispatch_core.h at running == 0.
//   P        = cap_now * percent / 100 with cap_now = sum of top(s), floored, saturated at 2^32 - 2.
//   term     = max(h, min(h + a, level)): what a requestor that holds h and asks for a more may hold
//              under `level`. An override is the same term at its own cap, whatever the level.
//   f(level) = others + sum of the fair askers' terms + sum of the overrides' fixed terms.
//   level    = YDC_QUOTA_UNLIMITED if there is no fair asker or f(D) <= P, D = max (h + a) over the
//              fair askers; 0 if f(0) > P; else the largest integer in [0, D) with f(level) <= P.
//
// f is non-decreasing, so the level is found by bisection. A level below D has f(level) >= level (the
// asker with the largest h + a alone contributes min(D, level)), so it is at most P < 2^32 - 1: the
// search runs over [0, min(D, P + 1)) and takes at most 32 rounds. Sums are 64 bit and saturate (a term
// is below 2^33, so a saturated sum stays saturated and is above every P).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YDC_FAIR_HD __host__ __device__
#else
#define YDC_FAIR_HD
#endif

namespace ydc {

constexpr uint32_t kFairOff = 0, kFairRegistry = 1, kFairFixed = 2;  // YDC_FAIR_OFF / _REGISTRY / _FIXED
constexpr uint32_t kFairUnlimited = 0xFFFFFFFFu;                     // YDC_QUOTA_UNLIMITED
constexpr uint64_t kFairPoolMax = 0xFFFFFFFEull;                     // a pool saturates here
constexpr uint32_t kFairLowMemory = 2u;                              // YDC_SERVANT_LOW_MEMORY

YDC_FAIR_HD inline uint32_t fair_top(uint32_t nproc, uint32_t load, uint32_t max_tasks, uint32_t flags) {
  if ((flags & kFairLowMemory) || max_tasks == 0 || load >= nproc) return 0;
  return max_tasks < nproc ? max_tasks : nproc;
}

// cap_now * percent / 100, floored, saturated. (cap_now / 100 above the bound: percent >= 1 saturates it.)
YDC_FAIR_HD inline uint64_t fair_pool(uint64_t cap_now, uint32_t percent) {
  const uint64_t q = cap_now / 100, r = cap_now % 100;
  if (percent && q > kFairPoolMax) return kFairPoolMax;
  const uint64_t p = q * percent + r * percent / 100;  // (q <= 2^32: no wrap)
  return p < kFairPoolMax ? p : kFairPoolMax;
}

YDC_FAIR_HD inline uint64_t fair_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? ~0ull : s;
}

YDC_FAIR_HD inline uint64_t fair_term(uint32_t h, uint32_t a, uint64_t level) {
  const uint64_t want = (uint64_t)h + a;
  const uint64_t upto = want < level ? want : level;
  return upto > h ? upto : h;
}

// The cap of a requestor without an override.
YDC_FAIR_HD inline uint32_t fair_cap(uint32_t level, uint32_t floor_cap, uint32_t default_cap) {
  const uint32_t at = level > floor_cap ? level : floor_cap;
  return at < default_cap ? at : default_cap;
}

// base: others + the overrides' fixed terms; D: the largest h + a of a fair asker; sum_at(level): the
// sum of the fair askers' terms (every caller of a group that computes it together gets the same
// value, so every one of them takes the same branches).
template <class SumAt>
YDC_FAIR_HD inline uint32_t fair_bisect(bool any_fair, uint64_t base, uint64_t D, uint64_t pool, SumAt sum_at) {
  if (!any_fair) return kFairUnlimited;
  const uint64_t P = pool < kFairPoolMax ? pool : kFairPoolMax;
  if (fair_add(base, sum_at(D)) <= P) return kFairUnlimited;
  if (fair_add(base, sum_at(0)) > P) return 0;
  uint64_t lo = 0, hi = D < P + 1 ? D : P + 1;  // f(lo) <= P < f(hi)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (fair_add(base, sum_at(mid)) <= P) lo = mid;
    else hi = mid;
  }
  return (uint32_t)lo;
}

// ydc_fair_level. fixed_cap == NULL: everybody is fair.
inline uint32_t fair_level(const uint32_t* held, const uint32_t* asked, const uint32_t* fixed_cap, uint32_t n,
                           uint64_t others, uint64_t pool) {
  uint64_t base = others, D = 0;
  bool any_fair = false;
  for (uint32_t i = 0; i < n; ++i) {
    if (fixed_cap && fixed_cap[i] != kFairUnlimited) {
      base = fair_add(base, fair_term(held[i], asked[i], fixed_cap[i]));
      continue;
    }
    const uint64_t want = (uint64_t)held[i] + asked[i];
    D = want > D ? want : D;
    any_fair = true;
  }
  return fair_bisect(any_fair, base, D, pool, [&](uint64_t level) {
    uint64_t s = 0;
    for (uint32_t i = 0; i < n; ++i)
      if (!fixed_cap || fixed_cap[i] == kFairUnlimited) s = fair_add(s, fair_term(held[i], asked[i], level));
    return s;
  });
}

}  // namespace ydc

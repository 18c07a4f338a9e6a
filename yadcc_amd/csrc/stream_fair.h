// stream_fair.h — a fair-share level per tick, computed on the device from demand
// (ydc_stream_quota_fair / _fair_result), for an open stream that has the quota on
// (ydc_stream_quota_begin): a waiting-and-leased or rpc stream with inspection on.
//
// The tick evaluates everything at the quota's clip point. That point lies:
//   - behind steps 1 - 6,
//   - behind the servants' expiry,
//   - behind k_apply_tick (this tick's heartbeats are in the registry columns),
//   - behind withdrawal's and departure's marks,
//   - behind k_quota_loads,
//   - in front of k_quota_clip.
//
// The pool P has two modes.
//   - Registry mode.
//       cap_now = sum over s of top(s) over the registry's rows.
//       top(s) = 0 if the low-memory flag is set, max_tasks == 0 or load >= nproc.
//       Otherwise top(s) = min(max_tasks, nproc).
//       This is servant_slot_count of dispatch_core.h at running == 0, so it does not depend on
//       running_tasks.
//       P = cap_now * percent / 100, with 64-bit arithmetic, floored and saturated at 2^32 - 2.
//   - Fixed mode. P is the caller's number.
//
// Consumption and demand.
//   - T = live leases that are not parked (servant < kParkedZombie), attributed or not, zombies
//     included, plus the rows of W's entries with deadline > now.
//   - Askers are the distinct requestor_ips of the tick's new requests.
//   - For an asker r: h_r = the quota's held(r), unchanged, as k_quota_loads leaves it. a_r = the sum of
//     its new requests' wants (n_immediate + n_prefetch, or 1 outside rpc mode).
//   - O = T - sum over the askers of h_r. This is everything held by requestors that ask nothing in this
//     tick, or by nobody.
//   - It is taken as given. The tick revokes nothing.
//   - A requestor with an override is outside the fair share. It contributes the fixed term
//     max(h_r, min(h_r + a_r, cap_r)) and keeps its override as its cap.
//
// The level.
//   - f(level) = O + sum over the fair askers of max(h_r, min(h_r + a_r, level)) + sum over the
//     overrides of fixed_r. It is non-decreasing in the level.
//   - D = max over the fair askers of (h_r + a_r).
//   - If there is no fair asker, or f(D) <= P: level = YDC_QUOTA_UNLIMITED. All demand fits.
//   - Else if f(0) > P: level = 0.
//   - Else the level is the largest integer in [0, D) with f(level) <= P.
//   - Sums are 64 bit.
//   - The remainder P - f(level), less than one row per asker above the level, stays free in that tick.
//
// The cap.
//   - For a requestor without an override: min(default_cap, max(level, floor_cap)).
//   - For a requestor with an override: its override.
//   - The clip is then exactly the existing rule (admit_clip.h), unchanged.
//
// Defining property. The tick and all later ticks, the labels and ydc_stream_quota_result included, are
// exactly those of a stream with the static quota whose default_cap was set to that value for this tick.
//
// Invariant. With floor_cap == 0, after the clip: O + sum over the askers of (h_r + admitted_r) <=
// max(P, T).
// (Where askers have overrides, what those are admitted stands on top of T: they are outside the fair
// share and keep their own caps, so the bound is max(P, T + sum over the overrides of admitted_r).)
//
// Three launches of its own, none while the mode is off; no kernel of stream_quota.h is edited:
//
//   k_fair_sums    between k_quota_loads and k_quota_clip, block ranges over four things: the registry's
//                  rows (top(s), 64-bit sums, one atomic per workgroup), L's slots in k_lease_sweep's
//                  shape (four per thread, 16-byte loads of state and servant: the live unparked leases),
//                  W's positions (the live rows), and the tick's new requests, whose wants go into
//                  ask[slot] of the quota's table through QuotaTick::slot, equal slots combined inside
//                  the wave before the atomic (wave_combine of stream_tile.h).
//   k_fair_level   one workgroup. It walks the table's slots once: held, ask and, by one binary search
//                  per asker, the override. An override's fixed term goes into the base; a fair asker's
//                  (h, a) pair goes to the end of a list in HBM (a counter in LDS hands out the places),
//                  so that the rounds cost what the askers are, not what the table is. Up to
//                  kFairRegAskers fair askers every thread then keeps its kFairPerThread pairs of the list
//                  in registers; above that every round reads the list again, from L2. Then fair_level.h's
//                  bisection, at most 32 rounds, each a workgroup reduction of 64-bit partial sums. It
//                  writes a two-word header of its own — the effective default, and the overrides' number
//                  copied from the settings' header — which k_quota_clip is launched with as
//                  QuotaCaps::hdr (the override arrays are the settings' own, which are never
//                  overwritten), and the result block in HBM. ask[] is cleared during the walk and the
//                  three sums at the end, for the next tick.
//   k_fair_done    behind the batch, gated like k_quota_label and k_depart_done: the result block to
//                  page-locked memory, once, with plain stores.
//
// Nobody waits for anybody inside a launch: what one launch leaves, the next one reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fair_level.h"
#include "stream_quota.h"

namespace ydc {

constexpr uint32_t kFairThreads = 256;
constexpr uint32_t kFairPerThread = 16;                             // pairs a thread keeps in registers
constexpr uint32_t kFairRegAskers = kFairThreads * kFairPerThread;  // fair askers of a tick up to which it does (4096)

// HBM: the settings (ydc_stream_quota_fair), read by k_fair_level: a change of numbers needs no new capture.
struct FairSet {
  uint32_t mode, pool, floor_cap, pad;
};

// HBM: what k_fair_sums adds up; zero between ticks (k_fair_level clears it).
struct FairSums {
  unsigned long long cap_now, leases, w_rows;
};

// ydc_fair_result. In HBM, and page-locked for the host.
struct FairResult {
  uint32_t level, cap_default_effective, n_askers, n_override_askers;
  unsigned long long pool, held_total, held_others, asked_rows, capacity_now;
  uint32_t tick_no, mode;
};
static_assert(sizeof(FairResult) == 64, "ydc_fair_result is 64 bytes");

struct FairTick {
  uint32_t* ask;  // [slots] beside the quota's table: the wants of the tick's new requests per requestor
  uint2* pair;    // [slots] the tick's list of (h, a) of the fair askers, in no order
  FairSums* sums;
  uint32_t* hdr;  // [2] the clip's header of this tick
  FairResult* res;
  const FairSet* set;
};

// The registry's columns as the tick's heartbeats left them.
struct FairRegistry {
  const uint32_t *nproc, *load, *max_tasks, *flags;
  uint32_t n;
};

// Sum over the workgroup's 256 threads (every thread gets it). lds: 4 words of the workgroup's.
__device__ __forceinline__ unsigned long long fair_block_sum(unsigned long long v, unsigned long long* lds) {
  v = wave_sum_u64(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned long long r = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();  // (the words are free again)
  return r;
}

__device__ __forceinline__ unsigned long long fair_block_max(unsigned long long v, unsigned long long* lds) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = lds[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) r = lds[k] > r ? lds[k] : r;
  __syncthreads();
  return r;
}

// r_blocks workgroups over the registry's rows, l_blocks over L's slots (four per thread), w_blocks over
// W's positions, then ceil(MT / 256) over the tick's new requests. w_imm == NULL (no rpc stream): an
// entry of W is one row; in_imm == NULL likewise for a new request.
__global__ __launch_bounds__(256) void k_fair_sums(FairRegistry reg, uint32_t r_blocks, LeaseCols L, uint32_t l_blocks,
                                                   const int64_t* w_deadline, const uint32_t* w_imm,
                                                   const uint32_t* w_pre, const WaitState* ws, uint32_t MW,
                                                   uint32_t w_blocks, const LeaseHdr* hdr, const uint32_t* in_imm,
                                                   const uint32_t* in_pre, const uint32_t* in_n, uint32_t MT,
                                                   QuotaTick t, QuotaTable tb, FairTick f) {
  __shared__ unsigned long long lds[4];
  uint32_t b = blockIdx.x;
  if (b < r_blocks) {
    const uint32_t s = b * blockDim.x + threadIdx.x;
    unsigned long long top = 0;
    if (s < reg.n) top = fair_top(reg.nproc[s], reg.load[s], reg.max_tasks[s], reg.flags[s]);
    top = fair_block_sum(top, lds);
    if (threadIdx.x == 0 && top) atomicAdd(&f.sums->cap_now, top);
    return;
  }
  b -= r_blocks;
  if (b < l_blocks) {
    const uint32_t i0 = (b * blockDim.x + threadIdx.x) * 4;
    unsigned long long n = 0;
    if (i0 <= L.mask) {  // (the servant column's guard: both loads are issued together)
      const uint4 st = lease_states4(L, i0);
      const uint4 sv = *reinterpret_cast<const uint4*>(L.servant + i0);
      // (a zombie still holds its slot; a parked lease — its servant expired in this tick — is gone once the tick ends)
      n = ((st.x & kLeaseLive) && sv.x < kParkedZombie) + ((st.y & kLeaseLive) && sv.y < kParkedZombie) +
          ((st.z & kLeaseLive) && sv.z < kParkedZombie) + ((st.w & kLeaseLive) && sv.w < kParkedZombie);
    }
    n = fair_block_sum(n, lds);
    if (threadIdx.x == 0 && n) atomicAdd(&f.sums->leases, n);
    return;
  }
  b -= l_blocks;
  if (b < w_blocks) {
    const uint32_t j = b * blockDim.x + threadIdx.x;
    // (an entry that expires or was withdrawn in this tick — deadline INT64_MIN — no longer counts)
    const bool live = j < min(ws->count, MW) && w_deadline[j] > hdr->now;
    unsigned long long rows = !live ? 0u : w_imm ? (unsigned long long)w_imm[j] + w_pre[j] : 1u;
    rows = fair_block_sum(rows, lds);
    if (threadIdx.x == 0 && rows) atomicAdd(&f.sums->w_rows, rows);
    return;
  }
  b -= w_blocks;
  const uint32_t k = b * blockDim.x + threadIdx.x;
  const uint32_t slot = k < min(*in_n, MT) ? t.slot[k] : kNone;
  const uint32_t want = slot == kNone ? 0u : in_imm ? in_imm[k] + in_pre[k] : 1u;
  // Equal slots combined inside the wave first (wave_combine: every lane of the wave gets here): one
  // requestor sending most of a tick is the normal case.
  bool active = slot != kNone && slot <= tb.mask && want != 0;
  active = wave_combine(active, slot, [&](uint32_t s0, bool mine, unsigned long long, bool leads, uint32_t) {
    const uint32_t sum = wave_sum_u32(mine ? want : 0u);
    if (leads) atomicAdd(&f.ask[s0], sum);
  });
  if (active) atomicAdd(&f.ask[slot], want);
}

// The bisection over the compacted list of the fair askers. REG: at most kFairRegAskers of them, every
// thread keeps its pairs in registers; otherwise every round reads the list again (from L2).
template <bool REG>
__device__ __forceinline__ uint32_t fair_level_find(const FairTick& f, uint32_t n_fair, uint64_t base, uint64_t D,
                                                    uint64_t P, unsigned long long* lds) {
  uint32_t h[REG ? kFairPerThread : 1], a[REG ? kFairPerThread : 1];
  if (REG) {
#pragma unroll
    for (uint32_t k = 0; k < kFairPerThread; ++k) {
      const uint32_t i = k * kFairThreads + threadIdx.x;
      const uint2 p = i < n_fair ? f.pair[i] : make_uint2(0u, 0u);  // (the pair (0, 0) has the term 0)
      h[k] = p.x;
      a[k] = p.y;
    }
  }
  // (every thread calls sum_at with the same level and gets the same sum: the branches are uniform)
  return fair_bisect(n_fair != 0, base, D, P, [&](uint64_t lv) {
    unsigned long long s = 0;
    if (REG) {
#pragma unroll
      for (uint32_t k = 0; k < kFairPerThread; ++k) s += fair_term(h[k], a[k], lv);
    } else {
      for (uint32_t i = threadIdx.x; i < n_fair; i += kFairThreads) {
        const uint2 p = f.pair[i];
        s += fair_term(p.x, p.y, lv);
      }
    }
    return (uint64_t)fair_block_sum(s, lds);
  });
}

// One workgroup of kFairThreads threads.
__global__ __launch_bounds__(256) void k_fair_level(QuotaTable tb, QuotaCaps caps, FairTick f, const LeaseHdr* hdr) {
  __shared__ unsigned long long lds[4];
  __shared__ uint32_t s_fair;
  if (threadIdx.x == 0) s_fair = 0;
  __syncthreads();
  const uint32_t slots = tb.mask + 1;
  const FairSet set = *f.set;
  const uint32_t n_over = min(caps.hdr[1], caps.max);
  unsigned long long fixed = 0, held = 0, asked = 0, D = 0, n_ask = 0, n_fix = 0;
  // The walk: thread t owns slots t, t + 256, ... An override's term goes into the base, a fair asker's pair to
  // the end of the list (its order does not matter: the sums are integers). ask[] is cleared on the way: only a
  // slot that a requestor of this tick claimed has anything in it, and this thread is its one reader.
  for (uint32_t i = threadIdx.x; i < slots; i += kFairThreads) {
    const unsigned long long w = tb.word[i];
    if (w == 0) continue;
    const uint32_t ip = (uint32_t)w, hi = tb.held[i], ai = f.ask[i];
    f.ask[i] = 0;
    held += hi;
    asked += ai;
    ++n_ask;
    uint32_t lo = 0, up = n_over;
    while (lo < up) {
      const uint32_t mid = (lo + up) >> 1;
      if (caps.ip[mid] < ip) lo = mid + 1; else up = mid;
    }
    if (lo < n_over && caps.ip[lo] == ip) {
      fixed += fair_term(hi, ai, caps.cap[lo]);
      ++n_fix;
      continue;
    }
    const unsigned long long want = (unsigned long long)hi + ai;
    D = want > D ? want : D;
    const uint32_t at = atomicAdd(&s_fair, 1u);  // (LDS; at < slots: a slot is listed once)
    f.pair[at] = make_uint2(hi, ai);
  }
  fixed = fair_block_sum(fixed, lds);  // (its barriers: the list is complete, and the workgroup sees it)
  held = fair_block_sum(held, lds);
  asked = fair_block_sum(asked, lds);
  n_ask = fair_block_sum(n_ask, lds);
  n_fix = fair_block_sum(n_fix, lds);
  D = fair_block_max(D, lds);
  const uint32_t n_fair = s_fair;
  const FairSums sums = *f.sums;
  const unsigned long long T = sums.leases + sums.w_rows;
  const unsigned long long others = T - (held < T ? held : T);  // (held <= T: an attributed lease is a lease)
  const unsigned long long P = set.mode == kFairRegistry ? fair_pool(sums.cap_now, set.pool)
                                                         : (set.pool < kFairPoolMax ? set.pool : kFairPoolMax);
  const uint64_t base = fair_add(others, fixed);
  const uint32_t level = n_fair <= kFairRegAskers ? fair_level_find<true>(f, n_fair, base, D, P, lds)  // (workgroup-uniform)
                                                  : fair_level_find<false>(f, n_fair, base, D, P, lds);
  __syncthreads();  // (without a fair asker the bisection has no barrier: everybody has read the sums)
  if (threadIdx.x == 0) {
    const uint32_t eff = fair_cap(level, set.floor_cap, caps.hdr[0]);
    f.hdr[0] = eff;
    f.hdr[1] = caps.hdr[1];
    *f.res = FairResult{level, eff, (uint32_t)n_ask, (uint32_t)n_fix, P, T, others, asked, sums.cap_now, hdr->tick_no,
                        set.mode};
    *f.sums = FairSums{0, 0, 0};
  }
}

// One wave. prm == NULL: ungated.
__global__ __launch_bounds__(64) void k_fair_done(const FairResult* res, FairResult* done, const DeviceParams* prm,
                                                  uint32_t check_slot) {
  if (prm && !batch_is_final(prm, check_slot)) return;
  if (threadIdx.x == 0) *done = *res;
}

}  // namespace ydc

// stream_tile.h — what the streaming modes' ticket-ordered tile passes share (wait_queue.h,
// lease_table.h, wait_lease.h, rpc_stream.h): a pass of ceil(n / 1024) workgroups of 256 threads,
// thread i of a workgroup owning four consecutive positions, the workgroups ordered by a ticket
// (not by blockIdx: a workgroup that looks back only ever waits for workgroups that have started)
// and chained by a decoupled look-back. Beside them the wave's helpers of the passes over L and W:
// the wave sum and the combine of equal keys inside a wave (wave_combine).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace ydc {

// Sum over the wave of a value per lane (every lane gets it).
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(v), 63);
}

constexpr uint32_t kRequestorRounds = 4;  // distinct keys a wave combines before its lanes go alone

// Equal keys combined inside the wave before a global atomic (one requestor that owns most of a table is
// the normal case, and a plain pass would put an atomic per entry on one address). Round by round the
// first active lane broadcasts its key, the lanes that hold it are balloted, and
//   each(key0, mine, same, leads, round)
// is called by all lanes together: key0 the round's key, `mine` whether this lane holds it, `same` the
// ballot of those lanes, `leads` true in the one lane that adds for them. The functor may use wave
// operations (it takes its sums over `mine`), and only the leading lane may write. After
// kRequestorRounds distinct keys the loop ends — a wave of 64 distinct keys would otherwise loop 64
// times to save nothing — and the lanes still active are returned: those add for themselves.
// EVERY LANE OF THE WAVE MUST GET HERE (wave-uniform control flow around the call), active or not.
template <class Each>
__device__ __forceinline__ bool wave_combine(bool active, uint32_t key, Each&& each) {
  const uint32_t lane = lane_id();
  unsigned long long todo = __ballot(active);
  for (uint32_t round = 0; todo && round < kRequestorRounds; ++round) {  // (wave-uniform)
    const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
    const uint32_t key0 = (uint32_t)__shfl((int)key, (int)lead, 64);
    const bool mine = active && key == key0;
    const unsigned long long same = __ballot(mine);
    each(key0, mine, same, lane == lead, round);
    active = active && !mine;
    todo &= ~same;
  }
  return active;
}

// A look-back word: flag (2 bits; 0: not published yet) | payload (62 bits). A payload is two
// counts, hi (31 bits) | lo (31 bits); a pass with one count leaves hi 0. Every count of every
// mode, and every sum of them over a pass, is below 2^31, so payloads add as plain integers.
constexpr unsigned long long kLbAggregate = 1ull << 62, kLbInclusive = 2ull << 62;
constexpr unsigned long long kLbValue = (1ull << 62) - 1;

__device__ __forceinline__ unsigned long long lb_pack(uint32_t lo, uint32_t hi = 0) {
  return (unsigned long long)lo | ((unsigned long long)hi << 31);
}
__device__ __forceinline__ uint32_t lb_lo(unsigned long long v) { return (uint32_t)(v & 0x7FFFFFFFu); }
__device__ __forceinline__ uint32_t lb_hi(unsigned long long v) { return (uint32_t)(v >> 31); }

template <int W>
struct LbWords {
  unsigned long long w[W];
};

// The decoupled look-back, called by wave 0 of the workgroup that drew ticket `bid`. A tile has W
// words, lookback[W * bid + k]; each k is a chain of its own. agg: the tile's own payloads.
// Publishes them as aggregates, sums the predecessors' words 64 tiles at a time (all W chains in
// the same loop, each ending independently at the first inclusive word it meets, so no ordering
// between a tile's W stores is needed), publishes the inclusive prefixes and returns the
// predecessors' sums, per word, to every lane. The words are zero when the pass begins.
// Every publication is a release store by lane 0: what lane 0 wrote before the call is visible to
// whoever reads this tile's word with the acquire load below. A value that the pass's last
// workgroup changes at the end (next_id) must be read before the ticket is drawn: the last
// workgroup gets there only after every other one has published, hence drawn its ticket.
template <int W>
__device__ __forceinline__ LbWords<W> tile_lookback(unsigned long long* lookback, uint32_t bid, uint32_t lane,
                                                    const LbWords<W>& agg) {
  unsigned long long* const mine = lookback + (size_t)W * bid;
  LbWords<W> pre;
#pragma unroll
  for (int k = 0; k < W; ++k) pre.w[k] = 0;
  if (bid == 0) {
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < W; ++k)
        __hip_atomic_store(&mine[k], kLbInclusive | agg.w[k], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    return pre;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < W; ++k)
      __hip_atomic_store(&mine[k], kLbAggregate | agg.w[k], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  bool done[W];
#pragma unroll
  for (int k = 0; k < W; ++k) done[k] = false;
  for (int look = (int)bid - 1;; look -= 64) {
    const int q = look - (int)lane;
    unsigned long long st[W];
#pragma unroll
    for (int k = 0; k < W; ++k) st[k] = kLbInclusive;  // (before block 0: an empty inclusive prefix)
    while (true) {
      bool empty = false;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        if (q >= 0) st[k] = __hip_atomic_load(&lookback[(size_t)W * q + k], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        empty |= (st[k] >> 62) == 0;
      }
      if (__ballot(empty) == 0) break;
      __builtin_amdgcn_s_sleep(1);
    }
    bool all = true;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (!done[k]) {
        const unsigned long long incl = __ballot((st[k] >> 62) == 2);
        const uint32_t upto = incl ? (uint32_t)__builtin_ctzll(incl) : 63u;
        const unsigned long long v = lane <= upto ? (st[k] & kLbValue) : 0ull;
        pre.w[k] += lb_pack(wave_sum_u32(lb_lo(v)), wave_sum_u32(lb_hi(v)));
        done[k] = incl != 0;
      }
      all &= done[k];
    }
    if (all) break;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < W; ++k)
      __hip_atomic_store(&mine[k], kLbInclusive | (pre.w[k] + agg.w[k]), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  return pre;
}

// The five columns every waiting entry has (WaitCols, RpcEntryCols), position j of `from` to ps of `to`.
template <class To, class From>
__device__ __forceinline__ void copy_entry(const To& to, uint32_t ps, const From& from, uint32_t j) {
  to.env[ps] = from.env[j];
  to.minv[ps] = from.minv[j];
  to.ip[ps] = from.ip[j];
  to.deadline[ps] = from.deadline[j];
  to.tag[ps] = from.tag[j];
}

// A thread's four answers and ids (positions j0 .. j0 + 3 of [0, n)) to page-locked memory; the
// caller's answers begin at position `base`. Once, 16 / 32 bytes per thread, where the four are
// four whole, aligned answers (base a multiple of 4, mostly).
__device__ __forceinline__ void store_answers(uint32_t* out, unsigned long long* out_id, uint32_t j0, uint32_t base,
                                              uint32_t n, const uint32_t (&r)[4], const unsigned long long (&ids)[4]) {
  if (j0 >= base && ((j0 - base) & 3) == 0 && j0 + 3 < n) {
    const uint32_t k = j0 - base;
    *reinterpret_cast<uint4*>(out + k) = make_uint4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<ulonglong2*>(out_id + k) = make_ulonglong2(ids[0], ids[1]);
    *reinterpret_cast<ulonglong2*>(out_id + k + 2) = make_ulonglong2(ids[2], ids[3]);
  } else {
    for (int i = 0; i < 4; ++i) {
      const uint32_t j = j0 + i;
      if (j < base || j >= n) continue;
      out[j - base] = r[i];
      out_id[j - base] = ids[i];
    }
  }
}

}  // namespace ydc

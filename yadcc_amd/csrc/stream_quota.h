// stream_quota.h — a cap of outstanding grants per requestor, enforced inside the tick
// (ydc_stream_quota_begin / _set / _result), for a waiting-and-leased or rpc stream
// with inspection on.
//
// The rule is admit_clip.h's, the loads are those of L and W at the moment the batch is built: after
// the tick's frees, reports, expiry and withdrawals, before W and the new requests are gathered. A
// clipped request is a request that asked for less; a refused one (nothing admitted) is a request
// that was never sent. So the feature touches neither the scan / gather in front of the batch nor
// the commit pass / settling behind it. Four small launches of its own stand around them, and a
// stream that never switched the capability on launches none of them:
//
//   k_quota_claim   thread per new request: its requestor's slot in a table keyed by the tick's new
//                   requestor_ips (open addressing, one 64-bit CAS per claim: requestor_index.h's
//                   word and requestor_claim). Whoever claims or finds a slot zeroes its two sums; the tick's counters,
//                   the clip pass's ticket and chain words are reset.
//   k_quota_loads   one launch over L's slots (k_requestor_leases' shape: four slots per thread) and
//                   W's positions: a live, attributed lease that is not parked adds 1, an entry of W
//                   with deadline > now adds its rows. Both only LOOK UP: a requestor that asks for
//                   nothing in this tick is a miss and is skipped. Equal keys are combined inside the
//                   wave before the global atomic (one requestor owning most of L is the normal case).
//   k_quota_clip    pre_i in arrival order, then the rule. Tiles of 256 requests, one per thread, in
//                   ticket order and chained STRICTLY: a tile starts its table updates when the tile
//                   in front has finished its own. Inside a wave the lanes of one requestor are found
//                   by a ballot / readlane loop (no atomics in it), which gives every lane its group's
//                   first lane, the wants in front of it and the group's sum; then the first lanes add
//                   their sums to the table, all in one atomic instruction, and the old value they get
//                   back is pre at the group's start. The four waves of a tile take turns (barriers).
//                   The admitted counts go to HBM: in rpc mode the two arrays k_rpc_scan reads as the
//                   new requests' n_immediate / n_prefetch (rows == 0 is padding there, so a refused
//                   RPC takes no rows and is never tried; k_rpc_settle copies the admitted counts into
//                   W); otherwise a copy of the env column in which a refused request carries the
//                   padding digest (k_wait_gather: it consumes nothing and cannot wait).
//   (gather / scan, front, passes, k_finalize, commit pass / grant + settle)
//   k_quota_label   first, ungated: the table's words cleared for the next tick. Then, gated like the
//                   commit pass: YDC_IDX_OVER_QUOTA into the page-locked answer / status of the
//                   requests that were admitted nothing, the admitted counts and the result block.
//                   It decides by the counts in HBM, never by the answer: a genuinely unknown digest
//                   stays EnvironmentNotFound. Plain stores only.
//
// The only wait is lane 0 of a tile's first wave for the release store of ANOTHER workgroup that has
// drawn its ticket already; nobody spins on a store of a thread of its own wave (slot_probe.h).
//
// 32 bits are enough for every sum: an accepted tick has rows(new) <= max_rows <= 2^30, so pre + want
// < 2^31, and |L| + rows(W) <= max_leases + max_rows < 2^31, so held < 2^31. With cap ==
// YDC_QUOTA_UNLIMITED room is then >= 2^31 > pre + want: nothing is ever clipped, without a special case.
//
// YDC_IDX_OVER_QUOTA is written behind the commit pass, into page-locked memory only: no kernel ever
// compares it with kIdxWaiting ("is a grant").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "admit_clip.h"
#include "index_home.h"
#include "kernels.h"
#include "lease_table.h"
#include "requestor_index.h"
#include "servant_alive.h"
#include "stream_inspect.h"
#include "stream_tile.h"
#include "wait_queue.h"

namespace ydc {

constexpr uint32_t kIdxOverQuota = 0xFFFFFFFBu;   // YDC_IDX_OVER_QUOTA
constexpr uint32_t kQuotaUnlimited = 0xFFFFFFFFu;  // YDC_QUOTA_UNLIMITED
constexpr uint32_t kQuotaTile = 256;               // requests per workgroup of the clip pass

// (quota_slots: index_home.h)

// HBM: the table keyed by the tick's new requestors. word: requestor_index.h's.
struct QuotaTable {
  unsigned long long* word;  // [mask + 1]: 0, or kRequestorOccupied | requestor_ip
  uint32_t* held;            // leases + rows of W's live entries
  uint32_t* asked;           // wants of the new requests the clip pass has been through
  uint32_t mask;
};

// HBM: the settings (ydc_stream_quota_set). hdr[0]: the default cap, hdr[1]: the overrides' number.
struct QuotaCaps {
  const uint32_t* ip;  // ascending, no duplicates
  const uint32_t* cap;
  const uint32_t* hdr;
  uint32_t max;
};

// HBM: per new request [max_tasks], and the tick's bookkeeping.
struct QuotaTick {
  uint32_t* slot;     // the requestor's slot (kNone behind the tick's requests)
  uint32_t* adm_imm;  // admitted n_immediate (outside rpc mode: 0 / 1)
  uint32_t* adm_pre;  // admitted n_prefetch (rpc mode only)
  uint32_t* env;      // outside rpc mode: the env column with the refused requests as padding
  uint32_t* count;    // [0] rows clipped, [1] requests refused, [2] the clip pass's ticket
  uint32_t* chain;    // [tiles] 1: the tile has finished its table updates
};

// Page-locked: what the host reads after the tick.
struct QuotaDone {
  uint32_t n, rows_clipped, n_refused, tick_no;
};

// The cap of `ip`: its override, or the default.
__device__ __forceinline__ uint32_t quota_cap(const QuotaCaps& q, uint32_t ip) {
  const uint32_t n = min(q.hdr[1], q.max);
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (q.ip[mid] < ip) lo = mid + 1; else hi = mid;
  }
  return lo < n && q.ip[lo] == ip ? q.cap[lo] : q.hdr[0];
}

// Thread per position of max(MT, tiles). in_ip / in_n: the arena's, as the step sees it.
__global__ __launch_bounds__(256) void k_quota_claim(const uint32_t* in_ip, const uint32_t* in_n, uint32_t MT,
                                                     uint32_t tiles, QuotaTable tb, QuotaTick t) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) t.count[0] = t.count[1] = t.count[2] = 0;
  if (k < tiles) t.chain[k] = 0;
  if (k >= MT) return;
  uint32_t h = kNone;
  if (k < min(*in_n, MT)) {
    h = requestor_claim(tb.word, tb.mask, in_ip[k]);
    if (h != kNone) tb.held[h] = tb.asked[h] = 0;  // (everybody who shares the slot stores the same)
  }
  t.slot[k] = h;
}

// `n` for key `ip` per active lane, looked up (a miss is skipped), equal keys combined inside the wave
// first. Every lane of the wave must get here (wave_combine).
__device__ __forceinline__ void quota_add(const QuotaTable& tb, bool active, uint32_t ip, uint32_t n) {
  active = wave_combine(active, ip, [&](uint32_t ip0, bool mine, unsigned long long, bool leads, uint32_t) {
    const uint32_t sum = wave_sum_u32(mine ? n : 0u);
    if (leads) {
      const uint32_t h = requestor_lookup(tb.word, tb.mask, ip0);
      if (h != kNone && sum) atomicAdd(&tb.held[h], sum);
    }
  });
  if (active) {
    const uint32_t h = requestor_lookup(tb.word, tb.mask, ip);
    if (h != kNone && n) atomicAdd(&tb.held[h], n);
  }
}

// l_blocks workgroups over L's slots (four per thread), then ceil(MW / 256) over W's positions.
// w_imm == NULL (no rpc stream): an entry of W is one row.
__global__ __launch_bounds__(256) void k_quota_loads(LeaseCols L, const uint4* rec, uint32_t l_blocks,
                                                     const uint32_t* w_ip, const int64_t* w_deadline,
                                                     const uint32_t* w_imm, const uint32_t* w_pre, const WaitState* ws,
                                                     uint32_t MW, const LeaseHdr* hdr, QuotaTable tb) {
  if (blockIdx.x < l_blocks) {
    const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const uint4 sv = lease_states4(L, i0);
    const uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bool counts = (st4[k] & kLeaseLive) != 0;  // (a zombie still holds its slot)
      uint32_t ip = 0;
      if (counts) {
        const uint4 r = rec[i0 + k];
        ip = r.w;
        // A lease granted while inspection was off belongs to nobody; a parked one (its servant
        // expired in this tick, servant_alive.h) is gone once the tick ends.
        counts = inspect_started(r) != kInspectNoTime && L.servant[i0 + k] < kParkedZombie;
      }
      quota_add(tb, counts, ip, 1u);
    }
    return;
  }
  const uint32_t j = (blockIdx.x - l_blocks) * blockDim.x + threadIdx.x;
  // (an entry that expires or was withdrawn in this tick — deadline INT64_MIN — no longer counts)
  const bool live = j < min(ws->count, MW) && w_deadline[j] > hdr->now;
  const uint32_t ip = live ? w_ip[j] : 0u;
  const uint32_t rows = !live ? 0u : w_imm ? w_imm[j] + w_pre[j] : 1u;
  quota_add(tb, live, ip, rows);
}

// ceil(MT / kQuotaTile) workgroups of 256 threads, thread i of the workgroup with ticket b owning
// request 256 b + i. in_*: the arena's columns (in_imm == NULL outside rpc mode: one row each).
__global__ __launch_bounds__(256) void k_quota_clip(const uint32_t* in_ip, const uint32_t* in_env,
                                                    const uint32_t* in_imm, const uint32_t* in_pre,
                                                    const uint32_t* in_n, uint32_t MT, QuotaTable tb, QuotaCaps caps,
                                                    QuotaTick t) {
  __shared__ uint32_t s_bid;
  if (threadIdx.x == 0) s_bid = atomicAdd(&t.count[2], 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t k = bid * kQuotaTile + threadIdx.x;
  const uint32_t n = min(*in_n, MT);
  const uint32_t slot = k < n ? t.slot[k] : kNone;
  const bool active = slot != kNone;
  uint32_t imm = 0, pre = 0, ip = 0;
  if (k < n) {
    imm = in_imm ? in_imm[k] : 1u;
    pre = in_imm ? in_pre[k] : 0u;
    ip = in_ip[k];
  }
  const uint32_t want = imm + pre;
  // The wave's groups of equal requestors: lead (the group's first lane), ex (the group's wants in
  // front of this lane), tot (the group's sum). ALU only; at most one round per distinct requestor.
  // (Not wave_combine: every lane needs its group's prefix, so the rounds go on until no group is left.)
  uint32_t lead = lane, ex = 0, tot = want;
  for (unsigned long long todo = __ballot(active); todo;) {  // (wave-uniform)
    const uint32_t l0 = (uint32_t)__builtin_ctzll(todo);
    const uint32_t s0 = (uint32_t)__shfl((int)slot, (int)l0, 64);
    const bool mine = active && slot == s0;
    const unsigned long long same = __ballot(mine);
    const uint32_t inc = wave_inclusive_scan(mine ? want : 0u);
    const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    if (mine) {
      lead = l0;
      ex = inc - want;
      tot = sum;
    }
    todo &= ~same;
  }
  uint32_t old = 0;
  const uint32_t k0 = bid * kQuotaTile;
  if (k0 < n) {  // (workgroup-uniform; a tile behind the tick's requests has nothing to add and nobody waits for it)
    // The chain: the tile in front has finished its table updates (it drew its ticket before this one).
    if (bid && threadIdx.x == 0)
      while (__hip_atomic_load(&t.chain[bid - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0)
        __builtin_amdgcn_s_sleep(1);
    __syncthreads();
    const uint32_t waves = (min(n - k0, kQuotaTile) + 63) / 64;
    for (uint32_t w = 0; w < waves; ++w) {  // the tile's waves that have requests, in order
      // (acquire: the wave goes on only when the add has been performed and its old value is here)
      if (wave == w && active && lane == lead)
        old = __hip_atomic_fetch_add(&tb.asked[slot], tot, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      __threadfence();
      __hip_atomic_store(&t.chain[bid], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  old = (uint32_t)__shfl((int)old, (int)lead, 64);
  uint32_t a = want;  // (a request without a slot — never: the table has 2 max_tasks slots — is let through)
  if (active) {
    const uint32_t room = admit_room_of<uint32_t>(quota_cap(caps, ip), tb.held[slot]);
    a = admit_rows<uint32_t>(old + ex, want, room);
  }
  const uint32_t a_imm = admit_split(imm, a);
  const uint32_t clipped = wave_sum_u32(want - a), refused = wave_sum_u32(want && !a ? 1u : 0u);
  if (lane == 0 && clipped) {
    atomicAdd(&t.count[0], clipped);
    if (refused) atomicAdd(&t.count[1], refused);
  }
  if (k >= MT) return;
  t.adm_imm[k] = a_imm;
  if (in_imm) t.adm_pre[k] = a - a_imm;
  else t.env[k] = want && !a ? kPadEnv : in_env[k];
}

// Thread per position of max(MT, slots). status: the page-locked answer (rpc: status) of the new
// requests. prm == NULL: ungated.
__global__ __launch_bounds__(256) void k_quota_label(QuotaTable tb, QuotaTick t, const uint32_t* in_n, uint32_t MT,
                                                     const LeaseHdr* hdr, uint32_t* status, uint32_t* out_imm,
                                                     uint32_t* out_pre, QuotaDone* done, const DeviceParams* prm,
                                                     uint32_t check_slot) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= tb.mask) tb.word[i] = 0;  // (the clip is done with the table; a second run finds it clear)
  if (prm && !batch_is_final(prm, check_slot)) return;  // (every workgroup alike)
  const uint32_t n = min(*in_n, MT);
  if (i == 0) *done = QuotaDone{n, t.count[0], t.count[1], hdr->tick_no};
  if (i >= n) return;
  const uint32_t a_imm = t.adm_imm[i], a_pre = out_pre ? t.adm_pre[i] : 0u;
  out_imm[i] = a_imm;
  if (out_pre) out_pre[i] = a_pre;
  if (a_imm + a_pre == 0) status[i] = kIdxOverQuota;
}

}  // namespace ydc

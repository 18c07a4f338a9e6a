// lease_table.h — the device-resident lease table of a streaming context
// (ydc_stream_begin_leased / ydc_stream_tick_leased).
//
// The reference remembers every grant in tasks_ (task_dispatcher.cc:127-135): a task id from
// next_task_id, the servant, expires_at, the zombie flag. KeepTaskAlive (:142-167), FreeTask
// (:169-188), the task loop of OnExpirationTimer (:522-535), NotifyServantRunningTasks with
// UnsafeSweepZombiesOf (:225-275, :453-476) and UnsafeSweepOrphans (:478-496) work on that table.
// A leased streaming context keeps it in HBM and applies a tick's renewals, frees, expiry and
// servant reports with four launches in front of the batch and one behind it, so the captured
// step needs no per-tick host arguments (counts, clock and tick number are read from the arena):
//
//   k_lease_renew    a renewal looks its id up; a live, non-zombie lease is renewed. Several
//                    renewals of one id: the last in array order wins (they bid with their
//                    position; k_lease_free's first workgroups store the winner's expiry).
//   k_lease_free     a free claims its lease with one CAS on the key (a duplicate id loses), gives
//                    the slot back (running_tasks - 1) and erases the lease.
//   k_lease_report   a reporting servant stamps its row with the tick number; a reported id that
//                    is a lease of that very servant stamps the lease; out_report_unknown.
//   k_lease_sweep    one pass over the table: overdue -> zombie; zombie whose servant reported
//                    this tick without listing it -> freed.
//   (k_apply_tick, front, passes, k_finalize place the tick's requests as in a plain tick)
//   k_lease_grant    the commit pass of wait_lease.h in its form without a queue: out_task_id[i]
//                    = next_id + rank among the granted, the lease inserted; the last workgroup
//                    bumps next_id and |L| and stores the tick's outcome block to page-locked memory.
// Outside the tick: k_lease_remap (ydc_remove_servants) and k_lease_rehash (ydc_stream_reserve: the
// table filed again into a larger one).
//
// running_tasks: the decrements of frees and sweeps are atomicSub on the column k_apply_tick's
// releases decrement too (the same instruction, the same column; the kernels run one after another
// on one stream). Heartbeats keep running_tasks and everything else only decrements it, so the
// order of these launches and k_apply_tick among themselves does not change the result.
//
// The table is open addressing over cap = 2^k >= 2 * max_leases slots (load <= 1/2), linear
// probing from the home slot (id * 2^64 / phi) >> (64 - k): multiplicative hashing spreads the
// reference's dense id sequence evenly, and it keeps doing so when a block of long-lived leases
// stays behind while the ids wrap around the table many times. (The home slot id & (cap - 1) is
// collision-free for any cap consecutive ids, but a block of B long-lived consecutive ids then
// displaces every later id that lands in it by up to B slots: measured, a tick at |L| = 10^6 took
// 169 ms that way.) The largest displacement ever used is kept on the device and bounds every
// probe; an erased slot is simply empty again (a lookup never stops at an empty slot, it stops at
// the bound), so there are no tombstones. Keys are compared in full (64 bit).
// Hot columns are SoA: key u64 | expires_at i64 | servant u32 | state u32 (live, zombie, stamp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "stream_tile.h"

namespace ydc {

constexpr unsigned long long kLeaseEmpty = ~0ull;
constexpr uint32_t kLeaseLive = 1u << 31, kLeaseZombie = 1u << 30;
// Tick number of the last report that listed the lease (mod 2^30; a tick number is never 0 there).
constexpr uint32_t kLeaseStamp = kLeaseZombie - 1;
constexpr uint32_t kLeaseTile = 1024;  // positions per workgroup of k_lease_sweep and the commit pass (256 x 4)

struct LeaseCols {
  unsigned long long* key;  // task id, kLeaseEmpty: free slot
  int64_t* expires;
  uint32_t* servant;
  uint32_t* state;    // 0: free slot; kLeaseLive | kLeaseZombie? | stamp
  uint32_t* ren_win;  // a tick's renewals bid here (position + 1); 0 between ticks
  uint32_t mask;      // cap - 1
  uint32_t shift;     // 64 - log2(cap)
};

__device__ __forceinline__ uint32_t lease_home(const LeaseCols& L, unsigned long long id) {
  return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> L.shift);
}

// Device memory of the table's bookkeeping.
struct LeaseState {
  unsigned long long next_id;
  uint32_t n_leases;  // |L|
  uint32_t max_disp;  // largest displacement from the home slot any insert has used
  uint32_t ticket;    // workgroups of the commit pass started
  uint32_t expired, swept, freed, renew_refused;  // of the tick in flight (lease_close_tick clears them)
  uint32_t pad;
};

// The tick's scalars, in the arena beside the columns.
struct LeaseHdr {
  int64_t now;
  uint32_t n_renew, n_free, n_rep, n_ids;
  uint32_t tick_no;  // 1, 2, ... (never 0)
  uint32_t pad;
};

// Page-locked: what the host reads after the tick (lease_close_tick).
struct LeaseOutcome {
  unsigned long long next_id;
  uint32_t n_leases, expired, swept, freed, renew_refused;
  uint32_t tick_no;
};

// The lease columns of a tick as the host staged them (page-locked arena, or its device copy).
struct LeaseIn {
  const LeaseHdr* hdr;
  const unsigned long long* ren_id;
  const int64_t* ren_exp;
  const unsigned long long* free_id;
  const uint32_t *rep_srv, *rep_off;
  const unsigned long long* rep_id;
  const int64_t* lease_exp;  // per request
};

// Slot of lease `id`, or kNone. An id the table has not handed out yet needs no probe.
__device__ __forceinline__ uint32_t lease_find(const LeaseCols& L, const LeaseState* st, unsigned long long id) {
  if (id >= st->next_id) return kNone;
  const uint32_t md = st->max_disp, h = lease_home(L, id);
  for (uint32_t d = 0; d <= md; ++d) {
    const uint32_t slot = (h + d) & L.mask;
    if (L.key[slot] == id) return slot;
  }
  return kNone;
}

// THE insert: lease `id` filed in the first free slot from its home on, which one CAS on the key takes;
// the winner then stores the columns and raises max_disp, in that order. A new grant's state word is
// kLeaseLive; a rehash, a restore and a delta store the word they carry. Returns the slot (whoever keeps
// columns beside the table stores them there afterwards). kNone never happens: the host checks before
// the launch that |L| plus everything it can add is <= max_leases <= cap / 2.
__device__ __forceinline__ uint32_t lease_file(const LeaseCols& L, LeaseState* st, unsigned long long id,
                                               int64_t expires, uint32_t servant, uint32_t state) {
  const uint32_t h = lease_home(L, id);
  for (uint32_t d = 0; d <= L.mask; ++d) {
    const uint32_t slot = (h + d) & L.mask;
    if (L.key[slot] != kLeaseEmpty || atomicCAS(&L.key[slot], kLeaseEmpty, id) != kLeaseEmpty) continue;
    L.expires[slot] = expires;
    L.servant[slot] = servant;
    L.state[slot] = state;
    if (d) atomicMax(&st->max_disp, d);
    return slot;
  }
  return kNone;
}

// The state words of slots i0 .. i0 + 3, one 16-byte load, for the passes in which thread i owns four
// consecutive slots (i0 = 4 i; cap is a multiple of 4). Zeros, which no live slot has, beyond the table.
__device__ __forceinline__ uint4 lease_states4(const LeaseCols& L, uint32_t i0) {
  if (i0 > L.mask) return make_uint4(0, 0, 0, 0);
  return *reinterpret_cast<const uint4*>(L.state + i0);
}

// The last workgroup of the last kernel of a leased tick: |L|, the outcome block, the tick's
// counters cleared. Returns the new next_id, which the caller stores to LeaseState.
__device__ __forceinline__ unsigned long long lease_close_tick(LeaseState* st, const LeaseHdr* hdr, LeaseOutcome* lout,
                                                               uint32_t granted, unsigned long long next_id_before) {
  const uint32_t n = st->n_leases - st->freed - st->swept + granted;
  const unsigned long long next = next_id_before + granted;
  lout->next_id = next;
  lout->n_leases = n;
  lout->expired = st->expired;
  lout->swept = st->swept;
  lout->freed = st->freed;
  lout->renew_refused = st->renew_refused;
  lout->tick_no = hdr->tick_no;
  st->n_leases = n;
  st->expired = st->swept = st->freed = st->renew_refused = 0;
  return next;
}

// One atomicAdd per wave for a per-lane 0/1.
__device__ __forceinline__ void wave_count(uint32_t* counter, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m && lane_id() == (uint32_t)__builtin_ctzll(m)) atomicAdd(counter, (uint32_t)__popcll(m));
}

// Thread per renewal (and per look-back word of the kernels behind the batch, which this first
// launch clears).
__global__ __launch_bounds__(256) void k_lease_renew(LeaseCols L, LeaseState* st, LeaseIn in, uint32_t max_renew,
                                                     uint32_t* ren_slot, uint8_t* out_renewed,
                                                     unsigned long long* lookback, uint32_t n_lookback) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) st->ticket = 0;
  if (j < n_lookback) lookback[j] = 0;
  const bool mine = j < max_renew && j < in.hdr->n_renew;
  bool ok = false;
  if (mine) {
    const uint32_t slot = lease_find(L, st, in.ren_id[j]);
    ok = slot != kNone && !(L.state[slot] & kLeaseZombie);
    ren_slot[j] = ok ? slot : kNone;
    if (ok) atomicMax(&L.ren_win[slot], j + 1);
    out_renewed[j] = ok ? 1 : 0;
  }
  wave_count(&st->renew_refused, mine && !ok);
}

// Workgroups [0, ren_blocks): the winning renewal of every lease stores its expiry. The others:
// thread per free.
__global__ __launch_bounds__(256) void k_lease_free(LeaseCols L, LeaseState* st, LeaseIn in, uint32_t max_renew,
                                                    uint32_t ren_blocks, const uint32_t* ren_slot,
                                                    uint32_t max_free, uint32_t n_servants, uint32_t* running) {
  if (blockIdx.x < ren_blocks) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= max_renew || j >= in.hdr->n_renew) return;
    const uint32_t slot = ren_slot[j];
    if (slot != kNone && L.ren_win[slot] == j + 1) {
      L.expires[slot] = in.ren_exp[j];
      L.ren_win[slot] = 0;
    }
    return;
  }
  const uint32_t j = (blockIdx.x - ren_blocks) * blockDim.x + threadIdx.x;
  bool won = false;
  if (j < max_free && j < in.hdr->n_free) {
    const unsigned long long id = in.free_id[j];
    const uint32_t slot = lease_find(L, st, id);
    won = slot != kNone && atomicCAS(&L.key[slot], id, kLeaseEmpty) == id;
    if (won) {
      const uint32_t s = L.servant[slot];
      L.state[slot] = 0;
      if (s < n_servants) atomicSub(&running[s], 1u);
    }
  }
  wave_count(&st->freed, won);
}

// Workgroups [0, rep_blocks): thread per reporting servant. The others: thread per reported id.
__global__ __launch_bounds__(256) void k_lease_report(LeaseCols L, const LeaseState* st, LeaseIn in,
                                                      uint32_t max_rep, uint32_t rep_blocks, uint32_t max_ids,
                                                      uint32_t n_servants, uint32_t* rep_tick,
                                                      uint8_t* out_unknown) {
  const uint32_t n_rep = min(in.hdr->n_rep, max_rep);
  if (blockIdx.x < rep_blocks) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rep && in.rep_srv[r] < n_servants) rep_tick[in.rep_srv[r]] = in.hdr->tick_no;
    return;
  }
  const uint32_t k = (blockIdx.x - rep_blocks) * blockDim.x + threadIdx.x;
  if (k >= max_ids || k >= in.hdr->n_ids || n_rep == 0) return;
  // The report k belongs to: the last r with rep_off[r] <= k.
  uint32_t lo = 0, hi = n_rep;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (in.rep_off[mid] <= k) lo = mid; else hi = mid;
  }
  const uint32_t s = in.rep_srv[lo];
  const uint32_t slot = lease_find(L, st, in.rep_id[k]);
  bool live = false;
  if (slot != kNone && L.servant[slot] == s) {
    const uint32_t sv = L.state[slot];
    // (every thread that stamps this lease in this launch stores the same word)
    L.state[slot] = (sv & ~kLeaseStamp) | (in.hdr->tick_no & kLeaseStamp);
    // Expiry (step 5) precedes the reports: an overdue lease is a zombie by now.
    live = !(sv & kLeaseZombie) && !(L.expires[slot] < in.hdr->now);
  }
  out_unknown[k] = live ? 0 : 1;
}

// ceil(cap / kLeaseTile) workgroups; thread i owns four consecutive slots.
__global__ __launch_bounds__(256) void k_lease_sweep(LeaseCols L, LeaseState* st, const LeaseHdr* hdr,
                                                     uint32_t n_servants, const uint32_t* rep_tick,
                                                     uint32_t* running) {
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  uint32_t n_exp = 0, n_swept = 0;
  const uint4 sv = lease_states4(L, i0);
  if ((sv.x | sv.y | sv.z | sv.w) & kLeaseLive) {
    const int64_t now = hdr->now;
    const uint32_t tick = hdr->tick_no, stamp = tick & kLeaseStamp;
    const uint4 srv = *reinterpret_cast<const uint4*>(L.servant + i0);
    const longlong2 e01 = *reinterpret_cast<const longlong2*>(L.expires + i0);
    const longlong2 e23 = *reinterpret_cast<const longlong2*>(L.expires + i0 + 2);
    uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
    const uint32_t s4[4] = {srv.x, srv.y, srv.z, srv.w};
    const int64_t e4[4] = {e01.x, e01.y, e23.x, e23.y};
    bool changed = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t v = st4[k];
      if (!(v & kLeaseLive)) continue;
      if (!(v & kLeaseZombie) && e4[k] < now) {
        v |= kLeaseZombie;
        ++n_exp;
      }
      if ((v & kLeaseZombie) && (v & kLeaseStamp) != stamp && s4[k] < n_servants && rep_tick[s4[k]] == tick) {
        L.key[i0 + k] = kLeaseEmpty;
        atomicSub(&running[s4[k]], 1u);
        v = 0;
        ++n_swept;
      }
      changed |= v != st4[k];
      st4[k] = v;
    }
    if (changed) *reinterpret_cast<uint4*>(L.state + i0) = make_uint4(st4[0], st4[1], st4[2], st4[3]);
  }
  // One atomic per workgroup and counter.
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t we = wave_sum_u32(n_exp), ws = wave_sum_u32(n_swept);
  if ((threadIdx.x & 63) == 0) {
    if (we) atomicAdd(&s_cnt[0], we);
    if (ws) atomicAdd(&s_cnt[1], ws);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(&st->expired, s_cnt[0]);
  if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(&st->swept, s_cnt[1]);
}

// ydc_remove_servants with a leased stream open (UnsafeSweepOrphans, task_dispatcher.cc:478-496):
// leases of removed rows vanish, the others follow the order-preserving compaction of the
// registry. removed[]: ascending. Thread per slot.
__global__ __launch_bounds__(256) void k_lease_remap(LeaseCols L, LeaseState* st, const uint32_t* removed,
                                                     uint32_t n_removed) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  bool gone = false;
  if (slot <= L.mask && (L.state[slot] & kLeaseLive)) {
    const uint32_t s = L.servant[slot];
    const uint32_t before = lower_bound_u32(removed, n_removed, s);
    gone = before < n_removed && removed[before] == s;
    if (gone) {
      L.key[slot] = kLeaseEmpty;
      L.state[slot] = 0;
    } else {
      L.servant[slot] = s - before;
    }
  }
  const unsigned long long m = __ballot(gone);
  if (m && lane_id() == (uint32_t)__builtin_ctzll(m)) atomicSub(&st->n_leases, (uint32_t)__popcll(m));
}

// ydc_stream_reserve: every lease of the table `o` filed into the larger, empty table `n` by
// lease_file (multiplicative home, linear probing, one CAS on the key), its state word
// stored as it is: live, zombie and the report stamp. One pass shaped like k_lease_sweep:
// ceil(old cap / kLeaseTile) workgroups, thread i owns four consecutive slots of `o`. n's
// bookkeeping starts cleared: n_leases counts what was filed (the host compares it with |L|),
// max_disp is that of the new table alone (the bound is tightened again), next_id is o's.
// No order is kept and none is needed: a slot's place depends on its key and on which of the
// probing inserts came first, and every reader finds a key by probing up to max_disp.
__global__ __launch_bounds__(256) void k_lease_rehash(LeaseCols o, const LeaseState* ost, LeaseCols n,
                                                      LeaseState* nst) {
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  uint32_t moved = 0;
  if (i0 <= o.mask) {  // (cap is a multiple of 4)
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(o.key + i0);
    const ulonglong2 k23 = *reinterpret_cast<const ulonglong2*>(o.key + i0 + 2);
    const unsigned long long k4[4] = {k01.x, k01.y, k23.x, k23.y};
    if ((k4[0] & k4[1] & k4[2] & k4[3]) != kLeaseEmpty) {
      const uint4 sv = lease_states4(o, i0);
      const uint4 srv = *reinterpret_cast<const uint4*>(o.servant + i0);
      const longlong2 e01 = *reinterpret_cast<const longlong2*>(o.expires + i0);
      const longlong2 e23 = *reinterpret_cast<const longlong2*>(o.expires + i0 + 2);
      const uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
      const uint32_t s4[4] = {srv.x, srv.y, srv.z, srv.w};
      const int64_t e4[4] = {e01.x, e01.y, e23.x, e23.y};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k4[k] != kLeaseEmpty && lease_file(n, nst, k4[k], e4[k], s4[k], st4[k]) != kNone) ++moved;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) nst->next_id = ost->next_id;
  // One atomic per workgroup.
  __shared__ uint32_t s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const uint32_t wm = wave_sum_u32(moved);
  if ((threadIdx.x & 63) == 0 && wm) atomicAdd(&s_cnt, wm);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(&nst->n_leases, s_cnt);
}

}  // namespace ydc

// servant_alive.h — the servants' expiry column of a leased streaming context
// (ydc_stream_alive_begin / ydc_stream_alive_stage / ydc_stream_alive_removed / ydc_stream_alive_get).
//
// The reference keeps an expires_at per servant (KeepServantAlive, task_dispatcher.cc:190-220) and
// OnExpirationTimer (:498-536) erases the servants with expires_at < now, drops their book entries,
// erases their leases as orphans (no zombie stage) and only then makes overdue leases zombies. With
// aliveness on, step 5 of a leased tick is that whole call. The column E (int64 per servant) lives in
// HBM beside the registry's columns and is sized by the registry.
//
//   k_alive_beat     in every tick, in front of the lease kernels: heartbeat i files
//                    E[upd_idx[i]] = upd_expires_at[i]. The only addition to an ordinary tick.
//   k_alive_due      only when the host's lower bound of min(E) is below the tick's clock: the due
//                    rows to a list, the exact minimum of the others to a device word.
// The captured step never changes the registry's structure. A tick in which a servant really
// expires takes the eager route of a structural heartbeat, in front of the step:
//   k_alive_compact  E follows the registry's order-preserving compaction (k_compact_rows' rule).
//   k_alive_remap    k_lease_remap, but a lease of a removed row is PARKED instead of erased: its
//                    servant becomes kParkedLive, or kParkedZombie if it was a zombie already. The
//                    tick's steps 2 and 3 still have to find it (a renewal of a lease that is
//                    orphaned in the same tick answers 1, a free of it counts).
//   k_alive_orphans  behind the step: every parked lease erased and counted.
//
// The design rests on four guards of the existing lease kernels (lease_table.h), none of which is
// edited. With s = the parked lease's servant word, which is >= n_servants for every registry:
//   k_lease_renew    finds a lease by its key alone and refuses only the zombie bit: a parked live
//                    lease is renewed (1), a parked zombie is refused (0), as in the reference, where
//                    KeepTaskAlive runs before the timer.
//   k_lease_free     erases the lease it claims and gives the slot back only `if (s < n_servants)`:
//                    a parked lease is freed and counted, no running_tasks is touched.
//   k_lease_report   stamps and permits only `L.servant[slot] == s` for the reporting servant s. The
//                    host rewrites the report of a removed row to servant 0xFFFFFFFF, which is
//                    neither parked value, so such a report matches no lease at all (every id
//                    unknown, nothing stamped; `rep_srv < n_servants` keeps rep_tick untouched), and
//                    no survivor's report matches a parked lease. This is why the parked values are
//                    0xFFFFFFFE / 0xFFFFFFFD and not 0xFFFFFFFF: a parked lease listed in its removed
//                    servant's own report would otherwise be answered "known".
//   k_lease_sweep    frees a zombie only when `s4[k] < n_servants`: a parked lease is never swept.
//                    It does mark an overdue parked-live lease a zombie and counts it in `expired`;
//                    k_alive_orphans counts exactly those (parked as live, zombie bit set now) and
//                    the host takes them off again: an orphan is never counted as expired.
// k_book_commit files only ids that k_lease_report answered 0, so it files nothing for a removed
// row's report; the removed rows' old entries went with k_book_remap in front of the step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"

namespace ydc {

constexpr uint32_t kParkedLive = 0xFFFFFFFEu, kParkedZombie = 0xFFFFFFFDu;
constexpr uint32_t kRemovedRow = 0xFFFFFFFFu;  // what a release or a report of a removed row is rewritten to
constexpr int64_t kAliveNever = INT64_MAX;

// Device memory: what k_alive_due and k_alive_orphans hand to the host (one small copy each).
struct AliveState {
  long long min_expires;  // of the rows that are not due
  uint32_t n_due;
  uint32_t n_orphans;  // parked leases k_alive_orphans erased
  uint32_t n_late;     // ... of which parked as live and marked zombie by this tick's sweep
  uint32_t pad;
};

// Thread per heartbeat. Padding (0xFFFFFFFF) and rows the registry does not have are no-ops.
__global__ __launch_bounds__(256) void k_alive_beat(const uint32_t* idx, const int64_t* upd_expires,
                                                    uint32_t n_upd, uint32_t n_servants, int64_t* expires) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_upd) return;
  const uint32_t s = idx[i];
  if (s < n_servants) expires[s] = upd_expires[i];
}

// Minimum over the 64 lanes (every lane gets it); off the hot path.
__device__ __forceinline__ long long wave_min_i64(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const long long o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

// Thread per servant. st: cleared by the host to {kAliveNever, 0, ...}. list: page-locked, n_servants
// entries, filled in no particular order (the host sorts the few there are).
__global__ __launch_bounds__(256) void k_alive_due(const int64_t* expires, uint32_t n_servants, int64_t now,
                                                   AliveState* st, uint32_t* list) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const bool mine = s < n_servants;
  const int64_t e = mine ? expires[s] : kAliveNever;
  const bool due = mine && e < now;
  // One atomicAdd per wave (wave_count's pattern, with the base handed to the wave's lanes).
  const unsigned long long m = __ballot(due);
  if (m) {
    const uint32_t lane = lane_id(), leader = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&st->n_due, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader, 64);
    if (due) {
      const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (at < n_servants) list[at] = s;  // (always: at most n_servants rows are due)
    }
  }
  const long long mn = wave_min_i64(due ? kAliveNever : (long long)e);
  if (lane_id() == 0 && mn != kAliveNever) atomicMin(&st->min_expires, mn);
}

// The expiry column through the registry's compaction. removed[]: ascending. Thread per old row.
__global__ __launch_bounds__(256) void k_alive_compact(const int64_t* in, int64_t* out, const uint32_t* removed,
                                                       uint32_t n_removed, uint32_t n) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t before = lower_bound_u32(removed, n_removed, s);
  if (before < n_removed && removed[before] == s) return;
  out[s - before] = in[s];
}

// k_lease_remap with the leases of removed rows parked. removed[]: ascending. Thread per slot.
// |L| is not changed here: a parked lease still counts until k_alive_orphans or a free erases it.
__global__ __launch_bounds__(256) void k_alive_remap(LeaseCols L, const uint32_t* removed, uint32_t n_removed) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot > L.mask) return;
  const uint32_t sv = L.state[slot];
  if (!(sv & kLeaseLive)) return;
  const uint32_t s = L.servant[slot];
  const uint32_t before = lower_bound_u32(removed, n_removed, s);
  if (before < n_removed && removed[before] == s) L.servant[slot] = (sv & kLeaseZombie) ? kParkedZombie : kParkedLive;
  else L.servant[slot] = s - before;
}

// Behind the step, shaped like k_lease_sweep: ceil(cap / kLeaseTile) workgroups, thread i owns four
// consecutive slots. Every parked lease is erased; |L| on the device follows.
__global__ __launch_bounds__(256) void k_alive_orphans(LeaseCols L, LeaseState* ls, AliveState* st) {
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  uint32_t n_orph = 0, n_late = 0;
  const uint4 sv = lease_states4(L, i0);
  if ((sv.x | sv.y | sv.z | sv.w) & kLeaseLive) {
    const uint4 srv = *reinterpret_cast<const uint4*>(L.servant + i0);
    uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
    const uint32_t s4[4] = {srv.x, srv.y, srv.z, srv.w};
    bool changed = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(st4[k] & kLeaseLive) || (s4[k] != kParkedLive && s4[k] != kParkedZombie)) continue;
      n_late += (s4[k] == kParkedLive && (st4[k] & kLeaseZombie)) ? 1u : 0u;
      ++n_orph;
      L.key[i0 + k] = kLeaseEmpty;
      st4[k] = 0;
      changed = true;
    }
    if (changed) *reinterpret_cast<uint4*>(L.state + i0) = make_uint4(st4[0], st4[1], st4[2], st4[3]);
  }
  // One atomic per workgroup and counter.
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t wo = wave_sum_u32(n_orph), wl = wave_sum_u32(n_late);
  if ((threadIdx.x & 63) == 0) {
    if (wo) atomicAdd(&s_cnt[0], wo);
    if (wl) atomicAdd(&s_cnt[1], wl);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[0]) {
    atomicAdd(&st->n_orphans, s_cnt[0]);
    atomicSub(&ls->n_leases, s_cnt[0]);
  }
  if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(&st->n_late, s_cnt[1]);
}

}  // namespace ydc

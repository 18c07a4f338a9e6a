// wait_lease.h — a streaming context with the waiting queue W and the lease table L at once
// (ydc_stream_begin_waiting_leased / ydc_stream_tick_waiting_leased).
//
// The reference's grant call waits AND records a lease (task_dispatcher.cc:93-140): a request that
// was queued in an earlier tick is granted in this one, takes next_task_id++ at that moment and its
// lease runs from the grant: expires_at = now of the granting tick + expires_in. So W carries a
// sixth column, the lease DURATION (k_wait_gather copies it beside deadline and tag), and the
// kernel behind the batch reads the tick's clock.
//
// That kernel, k_wait_lease_commit, is the one stable pass over the max_waiting + max_tasks placed
// positions that does what k_wait_compact and k_lease_grant do in their modes:
//   - a position is a survivor (stays in / joins W), resolved (a waiting entry's answer) or an
//     answered new request; independently of that it is granted or not;
//   - three counts (survivors, resolved, granted) are scanned through ONE ticket-ordered chain;
//   - the new W (six columns), the resolved list (tag, answer, task id), the new requests' answers
//     and ids (page-locked), the leases of all grants (queue region first, then the new requests:
//     one id sequence in batch order, as sequential WaitForStartingNewTask calls would take them);
//   - the last workgroup stores |W|, |L|, next_id and both outcome blocks.
//
// Look-back layout: TWO words per tile, each a complete look-back word of its own with its own
// 2-bit flag: word 2b = flag | resolved (31 bits) | survivors (31 bits), exactly wait_queue.h's;
// word 2b + 1 = flag | granted (32 bits), exactly lease_table.h's. The two chains are walked by
// the same loop (both words of 64 predecessors per step) but end independently, each at the first
// inclusive word it meets, so no ordering between a tile's two stores is needed and no count is
// narrower than in the existing modes: any max_waiting + max_tasks that ydc_stream_begin_waiting
// accepts (< 2^31) is representable, nothing is truncated, nothing more is refused at begin.
// k_lease_renew, the step's first launch, clears the 2 * tiles words and resets LeaseState::ticket,
// the one ticket this kernel draws from (k_wait_gather clears nothing in this mode).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"
#include "wait_queue.h"

namespace ydc {

// The lease durations beside WaitCols: W's column, the batch's, and the page-locked resolved ids.
struct WaitLeaseCols {
  int64_t* w_for;   // W: lease duration per entry
  int64_t* t_for;   // the tick's batch (k_wait_gather fills it)
  unsigned long long* res_id;  // page-locked: task id beside res_tag / res_idx
};

// ceil(N / kWaitTile) workgroups of 256 threads; thread i of a workgroup owns four consecutive
// positions. prm == NULL: ungated (the host has just placed the batch itself).
__global__ __launch_bounds__(256) void k_wait_lease_commit(
    WaitCols t, WaitLeaseCols lf, const uint32_t* placed, const LeaseHdr* hdr, uint32_t MW, uint32_t N, WaitCols w,
    WaitState* ws, LeaseCols L, LeaseState* st, unsigned long long* lookback, uint32_t* out_new,
    unsigned long long* out_task_id, uint64_t* res_tag, uint32_t* res_idx, WaitOutcome* wout, LeaseOutcome* lout,
    const DeviceParams* prm, uint32_t check_slot) {
  if (prm) {
    const bool final = (check_slot == kNone || prm->n_changed[check_slot] == 0) && !prm->window_miss &&
                       !prm->overflow;
    if (!final) return;  // (every workgroup alike: W, L and next_id stay as they are)
  }
  __shared__ uint32_t s_bid, s_pre_surv, s_pre_res, s_pre_gr;
  __shared__ unsigned long long s_next;
  __shared__ uint32_t lds[17];
  if (threadIdx.x == 0) {
    // next_id is read before this workgroup publishes anything; the last workgroup changes it only
    // after every other one has published.
    s_next = __hip_atomic_load(&st->next_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_bid = atomicAdd(&st->ticket, 1u);
  }
  __syncthreads();
  const uint32_t bid = s_bid;
  const uint32_t snap = ws->snap;
  const int64_t now = hdr->now;
  const uint32_t j0 = bid * kWaitTile + threadIdx.x * 4;
  // Per position: kind 1 survivor, 2 resolved (val: the waiting entry's answer), 0 neither;
  // r < kIdxWaiting: a grant (an expired entry and an unused slot were placed as kPadEnv).
  uint32_t kind[4], r[4];
  uint32_t n_surv = 0, n_res = 0, n_gr = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    kind[i] = 0;
    r[i] = kIdxEnvNotFound;
    if (j >= N) continue;
    const uint32_t p = placed[j];
    if (j < MW) {
      if (j < snap) {
        if (t.deadline[j] <= now) {
          kind[i] = 2;
          r[i] = kIdxTimeout;
        } else {
          kind[i] = p == kIdxTimeout ? 1u : 2u;
          r[i] = p;
        }
      }
    } else {
      const bool queue = p == kIdxTimeout && t.deadline[j] > now;
      kind[i] = queue ? 1u : 0u;
      r[i] = queue ? kIdxWaiting : p;
    }
    n_surv += kind[i] == 1;
    n_res += kind[i] == 2;
    n_gr += r[i] < kIdxWaiting;
  }
  // Workgroup-local prefixes: survivors and resolved in one word (each <= 1024), the grants apart.
  uint32_t tot, tot_gr;
  const uint32_t ex = block_exclusive_scan(n_surv | (n_res << 16), lds, &tot);
  const uint32_t ex_gr = block_exclusive_scan(n_gr, lds, &tot_gr);
  if (threadIdx.x < 64) {
    // Decoupled look-back by wave 0 over both words of the predecessors, 64 tiles at a time; each
    // chain stops at its own first inclusive word.
    const uint32_t lane = threadIdx.x;
    const unsigned long long agg = (unsigned long long)(tot & 0xFFFFu) | ((unsigned long long)(tot >> 16) << 31);
    unsigned long long* const mine = lookback + 2 * (size_t)bid;
    uint32_t pre_s = 0, pre_r = 0, pre_g = 0;
    if (bid == 0) {
      if (lane == 0) {
        __hip_atomic_store(&mine[0], kLbInclusive | agg, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&mine[1], kLbInclusive | tot_gr, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      if (lane == 0) {
        __hip_atomic_store(&mine[0], kLbAggregate | agg, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&mine[1], kLbAggregate | tot_gr, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
      int look = (int)bid - 1;
      bool done_a = false, done_b = false;
      while (true) {
        const int q = look - (int)lane;
        unsigned long long a = kLbInclusive, b = kLbInclusive;  // (before block 0: empty inclusive prefixes)
        while (true) {
          if (q >= 0) {
            a = __hip_atomic_load(&lookback[2 * (size_t)q], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            b = __hip_atomic_load(&lookback[2 * (size_t)q + 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (__ballot((a >> 62) == 0 || (b >> 62) == 0) == 0) break;
          __builtin_amdgcn_s_sleep(1);
        }
        if (!done_a) {
          const unsigned long long incl = __ballot((a >> 62) == 2);
          const uint32_t upto = incl ? (uint32_t)__builtin_ctzll(incl) : 63u;
          const unsigned long long v = lane <= upto ? (a & kLbValue) : 0ull;
          pre_s += wave_sum_u32((uint32_t)(v & 0x7FFFFFFFu));
          pre_r += wave_sum_u32((uint32_t)(v >> 31));
          done_a = incl != 0;
        }
        if (!done_b) {
          const unsigned long long incl = __ballot((b >> 62) == 2);
          const uint32_t upto = incl ? (uint32_t)__builtin_ctzll(incl) : 63u;
          pre_g += wave_sum_u32(lane <= upto ? (uint32_t)(b & 0xFFFFFFFFull) : 0u);
          done_b = incl != 0;
        }
        if (done_a && done_b) break;
        look -= 64;
      }
      if (lane == 0) {
        const unsigned long long inc = ((unsigned long long)(pre_s + (tot & 0xFFFFu))) |
                                       ((unsigned long long)(pre_r + (tot >> 16)) << 31);
        __hip_atomic_store(&mine[0], kLbInclusive | inc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&mine[1], kLbInclusive | (unsigned long long)(pre_g + tot_gr), __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (lane == 0) {
      s_pre_surv = pre_s;
      s_pre_res = pre_r;
      s_pre_gr = pre_g;
      if (bid == gridDim.x - 1) {  // the last workgroup: the totals
        const uint32_t n_waiting = pre_s + (tot & 0xFFFFu), n_resolved = pre_r + (tot >> 16);
        const uint32_t granted = pre_g + tot_gr;
        ws->count = n_waiting;
        wout->n_waiting = n_waiting;
        wout->n_resolved = n_resolved;
        const uint32_t n = st->n_leases - st->freed - st->swept + granted;
        const unsigned long long next = s_next + granted;
        lout->next_id = next;
        lout->n_leases = n;
        lout->expired = st->expired;
        lout->swept = st->swept;
        lout->freed = st->freed;
        lout->renew_refused = st->renew_refused;
        lout->tick_no = hdr->tick_no;
        st->n_leases = n;
        st->expired = st->swept = st->freed = st->renew_refused = 0;
        __hip_atomic_store(&st->next_id, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  uint32_t ps = s_pre_surv + (ex & 0xFFFFu), pr = s_pre_res + (ex >> 16);
  unsigned long long id = s_next + s_pre_gr + ex_gr;
  unsigned long long ids[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    ids[i] = kLeaseEmpty;
    if (r[i] < kIdxWaiting) {
      ids[i] = id++;
      const uint32_t h = lease_home(L, ids[i]);
      // (always ends: |L| + |W| + n <= max_leases <= cap / 2 is checked before the tick)
      for (uint32_t d = 0; d <= L.mask; ++d) {
        const uint32_t slot = (h + d) & L.mask;
        if (L.key[slot] != kLeaseEmpty || atomicCAS(&L.key[slot], kLeaseEmpty, ids[i]) != kLeaseEmpty) continue;
        L.expires[slot] = now + lf.t_for[j];  // the lease runs from the grant
        L.servant[slot] = r[i];
        L.state[slot] = kLeaseLive;
        if (d) atomicMax(&st->max_disp, d);
        break;
      }
    }
    if (kind[i] == 1) {
      if (ps < MW) {  // (always: |W| + n <= max_waiting is checked before the tick)
        w.env[ps] = t.env[j];
        w.minv[ps] = t.minv[j];
        w.ip[ps] = t.ip[j];
        w.deadline[ps] = t.deadline[j];
        w.tag[ps] = t.tag[j];
        lf.w_for[ps] = lf.t_for[j];
      }
      ++ps;
    } else if (kind[i] == 2) {
      if (pr < MW) {
        res_tag[pr] = t.tag[j];
        res_idx[pr] = r[i];
        lf.res_id[pr] = ids[i];
      }
      ++pr;
    }
  }
  // The new requests' answers and ids go to page-locked memory once, 16 / 32 bytes per thread
  // where the thread's four positions are four whole answers (max_waiting a multiple of 4).
  if (j0 >= MW && ((j0 - MW) & 3) == 0 && j0 + 3 < N) {
    const uint32_t k = j0 - MW;
    *reinterpret_cast<uint4*>(out_new + k) = make_uint4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<ulonglong2*>(out_task_id + k) = make_ulonglong2(ids[0], ids[1]);
    *reinterpret_cast<ulonglong2*>(out_task_id + k + 2) = make_ulonglong2(ids[2], ids[3]);
  } else {
    for (int i = 0; i < 4; ++i) {
      const uint32_t j = j0 + i;
      if (j < MW || j >= N) continue;
      out_new[j - MW] = r[i];
      out_task_id[j - MW] = ids[i];
    }
  }
}

}  // namespace ydc

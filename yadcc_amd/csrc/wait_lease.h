// wait_lease.h — the commit pass behind a streaming tick's placed batch, in the three modes that
// have one: k_wait_compact (a queue W: ydc_stream_begin_waiting), k_lease_grant (a lease table L:
// ydc_stream_begin_leased), k_wait_lease_commit (both: ydc_stream_begin_waiting_leased).
//
// With both, the reference's grant call waits AND records a lease (task_dispatcher.cc:93-140): a
// request that was queued in an earlier tick is granted in this one, takes next_task_id++ at that
// moment and its lease runs from the grant: expires_at = now of the granting tick + expires_in. So
// W carries a sixth column, the lease DURATION (k_wait_gather copies it beside deadline and tag),
// and the pass reads the tick's clock; without a queue a request brings its absolute expiry.
//
// The pass is one stable, ticket-ordered tile pass (stream_tile.h) over the placed positions
// [max_waiting region | max_tasks region]:
//   - a position is a survivor (stays in / joins W), resolved (a waiting entry's answer) or an
//     answered new request; independently of that it is granted or not;
//   - the counts (survivors, resolved | granted) are scanned through one look-back: one word per
//     tile for either pair, TWO words per tile (2b: survivors, resolved; 2b + 1: granted) with
//     both, so no count is narrower with both than in a mode of its own;
//   - the new W, the resolved list (tag, answer, task id), the new requests' answers and ids
//     (page-locked), the leases of all grants (queue region first, then the new requests: one id
//     sequence in batch order, as sequential WaitForStartingNewTask calls would take them);
//   - the last workgroup stores |W|, |L|, next_id and the outcome blocks.
//
// It is gated like k_finalize: a batch that has not become final (the captured passes were not
// enough, a bin of the bin sort overflowed) leaves W, L and next_id as they were, and the host
// places the batch again and runs the pass ungated (prm == NULL) behind it.
// The look-back words are cleared and the ticket is reset by the step's first launch: k_lease_renew
// with leases (LeaseState::ticket), k_wait_gather without (WaitState::ticket).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"
#include "stream_inspect.h"
#include "stream_tile.h"
#include "wait_queue.h"

namespace ydc {

// The lease durations beside WaitCols: W's column, the batch's, and the page-locked resolved ids.
struct WaitLeaseCols {
  int64_t* w_for;   // W: lease duration per entry
  int64_t* t_for;   // the tick's batch (k_wait_gather fills it)
  unsigned long long* res_id;  // page-locked: task id beside res_tag / res_idx
};

// ceil(N / 1024) workgroups of 256 threads; thread i of a workgroup owns four consecutive
// positions. What a mode does not have is NULL / 0: !kWait: t, lf, MW, w, ws, res_*, wout;
// !kLease: lf, hdr, lease_exp, L, st, out_task_id, lout. now_p: the clock without leases (with
// them: hdr->now). lease_exp: the requests' absolute expiries without a queue (with one: lf).
// kInspect (stream_inspect.h; needs kLease): the inserting thread also files the grant's detail
// record and counts it for its servant; ins: empty without.
template <bool kWait, bool kLease, bool kInspect = false>
__device__ __forceinline__ void commit_pass(WaitCols t, WaitLeaseCols lf, const uint32_t* placed, const int64_t* now_p,
                                            const int64_t* lease_exp, const LeaseHdr* hdr, uint32_t MW, uint32_t N,
                                            WaitCols w, WaitState* ws, LeaseCols L, LeaseState* st,
                                            unsigned long long* lookback, uint32_t* out_new,
                                            unsigned long long* out_task_id, uint64_t* res_tag, uint32_t* res_idx,
                                            WaitOutcome* wout, LeaseOutcome* lout, const DeviceParams* prm,
                                            uint32_t check_slot, const InspectIn& ins = InspectIn{}) {
  if (prm && !batch_is_final(prm, check_slot)) return;  // (every workgroup alike)
  __shared__ uint32_t s_bid, s_pre_surv, s_pre_res, s_pre_gr;
  __shared__ unsigned long long s_next;
  __shared__ uint32_t lds[17];
  if (threadIdx.x == 0) {
    if constexpr (kLease) {
      // (next_id before the ticket: stream_tile.h)
      s_next = __hip_atomic_load(&st->next_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_bid = atomicAdd(&st->ticket, 1u);
    } else {
      s_bid = atomicAdd(&ws->ticket, 1u);
    }
  }
  __syncthreads();
  const uint32_t bid = s_bid;
  uint32_t mw = 0, snap = 0;  // the queue region
  int64_t now = 0;
  if constexpr (kWait) {
    mw = MW;
    snap = ws->snap;
    if constexpr (kLease) now = hdr->now;
    else now = *now_p;
  }
  const uint32_t j0 = bid * kWaitTile + threadIdx.x * 4;
  // Per position: kind 1 survivor, 2 resolved (r: the waiting entry's answer), 0 neither;
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
    if (j < mw) {
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
      // (without a queue a Timeout is final whatever the request's deadline)
      const bool queue = kWait && p == kIdxTimeout && t.deadline[j] > now;
      kind[i] = queue ? 1u : 0u;
      r[i] = queue ? kIdxWaiting : p;
    }
    n_surv += kind[i] == 1;
    n_res += kind[i] == 2;
    n_gr += r[i] < kIdxWaiting;
  }
  // Workgroup-local prefixes: survivors and resolved in one word (each <= 1024), the grants apart.
  uint32_t tot = 0, tot_gr = 0, ex = 0, ex_gr = 0;
  if constexpr (kWait) ex = block_exclusive_scan(n_surv | (n_res << 16), lds, &tot);
  if constexpr (kLease) ex_gr = block_exclusive_scan(n_gr, lds, &tot_gr);
  if (threadIdx.x < 64) {
    constexpr int kWords = kWait && kLease ? 2 : 1;
    LbWords<kWords> agg;
    if constexpr (kLease) agg.w[kWords - 1] = lb_pack(tot_gr);
    if constexpr (kWait) agg.w[0] = lb_pack(tot & 0xFFFFu, tot >> 16);
    const LbWords<kWords> pre = tile_lookback<kWords>(lookback, bid, threadIdx.x, agg);
    if (threadIdx.x == 0) {
      const bool last = bid == gridDim.x - 1;  // the last workgroup: the totals
      if constexpr (kWait) {
        const uint32_t pre_s = lb_lo(pre.w[0]), pre_r = lb_hi(pre.w[0]);
        s_pre_surv = pre_s;
        s_pre_res = pre_r;
        if (last) {
          const uint32_t n_waiting = pre_s + (tot & 0xFFFFu), n_resolved = pre_r + (tot >> 16);
          ws->count = n_waiting;
          wout->n_waiting = n_waiting;
          wout->n_resolved = n_resolved;
        }
      }
      if constexpr (kLease) {
        const uint32_t pre_g = lb_lo(pre.w[kWords - 1]);
        s_pre_gr = pre_g;
        if (last) {
          const unsigned long long next = lease_close_tick(st, hdr, lout, pre_g + tot_gr, s_next);
          __hip_atomic_store(&st->next_id, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
  __syncthreads();
  uint32_t ps = 0, pr = 0;
  if constexpr (kWait) {
    ps = s_pre_surv + (ex & 0xFFFFu);
    pr = s_pre_res + (ex >> 16);
  }
  unsigned long long id = 0;
  if constexpr (kLease) id = s_next + s_pre_gr + ex_gr;
  unsigned long long ids[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    ids[i] = kLeaseEmpty;
    if constexpr (kLease) {
      if (r[i] < kIdxWaiting) {
        ids[i] = id++;
        int64_t expires;
        if constexpr (kWait) expires = now + lf.t_for[j];  // the lease runs from the grant
        else expires = lease_exp[j];
        if constexpr (kInspect) {
          // (started_at: the clock at the grant, task_dispatcher.cc:133; no prefetch in these modes)
          lease_insert_inspected(L, st, ins, ids[i], expires, r[i], hdr->now, j, false);
        } else {
          lease_file(L, st, ids[i], expires, r[i], kLeaseLive);
        }
      }
    }
    if constexpr (kWait) {
      if (kind[i] == 1) {
        if (ps < mw) {  // (always: |W| + n <= max_waiting is checked before the tick)
          copy_entry(w, ps, t, j);
          if constexpr (kLease) lf.w_for[ps] = lf.t_for[j];
        }
        ++ps;
      } else if (kind[i] == 2) {
        if (pr < mw) {
          res_tag[pr] = t.tag[j];
          res_idx[pr] = r[i];
          if constexpr (kLease) lf.res_id[pr] = ids[i];
        }
        ++pr;
      }
    }
  }
  // The new requests' answers (and ids) to page-locked memory.
  if constexpr (kLease) {
    store_answers(out_new, out_task_id, j0, mw, N, r, ids);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t j = j0 + i;
      if (j >= mw && j < N) out_new[j - mw] = r[i];
    }
  }
}

// prm == NULL: ungated (the host has just placed the batch itself).
__global__ __launch_bounds__(256) void k_wait_compact(WaitCols t, const uint32_t* placed, const int64_t* now_p,
                                                      uint32_t MW, uint32_t N, WaitCols w, WaitState* ws,
                                                      unsigned long long* lookback, uint32_t* out_new,
                                                      uint64_t* res_tag, uint32_t* res_idx,
                                                      WaitOutcome* outcome, const DeviceParams* prm,
                                                      uint32_t check_slot) {
  commit_pass<true, false>(t, /*lf=*/WaitLeaseCols{}, placed, now_p, /*lease_exp=*/nullptr, /*hdr=*/nullptr, MW, N, w, ws,
                           /*L=*/LeaseCols{}, /*st=*/nullptr, lookback, out_new, /*out_task_id=*/nullptr, res_tag,
                           res_idx, outcome, /*lout=*/nullptr, prm, check_slot);
}

__global__ __launch_bounds__(256) void k_lease_grant(const uint32_t* placed, uint32_t N, const int64_t* lease_exp,
                                                     const LeaseHdr* hdr, LeaseCols L, LeaseState* st,
                                                     unsigned long long* lookback, uint32_t* out_idx,
                                                     unsigned long long* out_task_id, LeaseOutcome* outcome,
                                                     const DeviceParams* prm, uint32_t check_slot) {
  commit_pass<false, true>(/*t=*/WaitCols{}, /*lf=*/WaitLeaseCols{}, placed, /*now_p=*/nullptr, lease_exp, hdr,
                           /*MW=*/0, N, /*w=*/WaitCols{}, /*ws=*/nullptr, L, st, lookback, out_idx, out_task_id,
                           /*res_tag=*/nullptr, /*res_idx=*/nullptr, /*wout=*/nullptr, outcome, prm, check_slot);
}

__global__ __launch_bounds__(256) void k_wait_lease_commit(
    WaitCols t, WaitLeaseCols lf, const uint32_t* placed, const LeaseHdr* hdr, uint32_t MW, uint32_t N, WaitCols w,
    WaitState* ws, LeaseCols L, LeaseState* st, unsigned long long* lookback, uint32_t* out_new,
    unsigned long long* out_task_id, uint64_t* res_tag, uint32_t* res_idx, WaitOutcome* wout, LeaseOutcome* lout,
    const DeviceParams* prm, uint32_t check_slot) {
  commit_pass<true, true>(t, lf, placed, /*now_p=*/nullptr, /*lease_exp=*/nullptr, hdr, MW, N, w, ws, L, st, lookback, out_new, out_task_id,
                          res_tag, res_idx, wout, lout, prm, check_slot);
}

// The two leased forms with inspection on (stream_inspect.h): the same pass, the detail record and
// the servant's count at the insert.
__global__ __launch_bounds__(256) void k_lease_grant_inspect(const uint32_t* placed, uint32_t N,
                                                             const int64_t* lease_exp, const LeaseHdr* hdr, LeaseCols L,
                                                             LeaseState* st, unsigned long long* lookback,
                                                             uint32_t* out_idx, unsigned long long* out_task_id,
                                                             LeaseOutcome* outcome, const DeviceParams* prm,
                                                             uint32_t check_slot, InspectIn ins) {
  commit_pass<false, true, true>(/*t=*/WaitCols{}, /*lf=*/WaitLeaseCols{}, placed, /*now_p=*/nullptr, lease_exp, hdr,
                                 /*MW=*/0, N, /*w=*/WaitCols{}, /*ws=*/nullptr, L, st, lookback, out_idx, out_task_id,
                                 /*res_tag=*/nullptr, /*res_idx=*/nullptr, /*wout=*/nullptr, outcome, prm, check_slot,
                                 ins);
}

__global__ __launch_bounds__(256) void k_wait_lease_commit_inspect(
    WaitCols t, WaitLeaseCols lf, const uint32_t* placed, const LeaseHdr* hdr, uint32_t MW, uint32_t N, WaitCols w,
    WaitState* ws, LeaseCols L, LeaseState* st, unsigned long long* lookback, uint32_t* out_new,
    unsigned long long* out_task_id, uint64_t* res_tag, uint32_t* res_idx, WaitOutcome* wout, LeaseOutcome* lout,
    const DeviceParams* prm, uint32_t check_slot, InspectIn ins) {
  commit_pass<true, true, true>(t, lf, placed, /*now_p=*/nullptr, /*lease_exp=*/nullptr, hdr, MW, N, w, ws, L, st,
                                lookback, out_new, out_task_id, res_tag, res_idx, wout, lout, prm, check_slot, ins);
}

}  // namespace ydc

// wait_queue.h — the device-resident queue of waiting requests of a streaming context
// (ydc_stream_begin_waiting / ydc_stream_tick_waiting).
//
// The reference's grant call waits: TaskDispatcher::WaitForStartingNewTask sleeps on its
// condition variable until a servant frees a slot or the deadline passes, trying again on every
// wake-up (task_dispatcher.cc:93-118). In waiting mode a streaming tick keeps the requests that
// found no free servant in a queue W in HBM, in arrival order, and tries them again at the start
// of every later tick, ahead of that tick's new requests. Two launches around the unchanged batch
// pipeline do the bookkeeping, so the captured step needs no per-tick host arguments:
//
//   k_wait_gather   builds the tick's request columns [max_waiting region | max_tasks region]:
//                   entry j of W at position j (an expired entry or an unused slot becomes a
//                   request for a digest nobody has: it consumes nothing), the tick's new requests
//                   behind; deadlines and tags travel beside them. W is only read.
//   (front, passes, k_finalize place the max_waiting + max_tasks requests as one batch)
//   k_wait_compact  one stable pass over the placed batch: W's Timeouts whose deadline has not
//                   passed and the new requests' Timeouts with a deadline still ahead are the new
//                   W (order kept); W's grants, EnvironmentNotFounds and expiries are the resolved
//                   list (queue order); the new requests' answers go to the caller, a queued one as
//                   YDC_IDX_WAITING. Workgroups are ordered by a ticket and chained by a decoupled
//                   look-back over (survivors, resolved) counts; the last one writes |W|.
//
// k_wait_compact is gated like k_finalize: a batch that has not become final (the captured
// passes were not enough, a bin of the bin sort overflowed) leaves W as it was, and the host
// places the batch again and runs the compaction behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace ydc {

constexpr uint32_t kIdxWaiting = 0xFFFFFFFDu;  // YDC_IDX_WAITING
constexpr uint32_t kPadEnv = 0xFFFFFFFFu;      // a digest nobody has: EnvironmentNotFound, consumes nothing
constexpr uint32_t kWaitTile = 1024;           // positions per k_wait_compact workgroup (256 threads x 4)

// Columns of W, or of one tick's batch (max_waiting + max_tasks entries).
struct WaitCols {
  uint32_t* env;
  uint32_t* minv;
  uint32_t* ip;
  int64_t* deadline;
  uint64_t* tag;
};

// The tick's new requests as the host staged them (page-locked arena, or its device copy).
struct WaitNew {
  const uint32_t* env;
  const uint32_t* minv;
  const uint32_t* ip;
  const int64_t* deadline;
  const uint64_t* tag;
  const int64_t* now;
};

// Device memory of the queue's bookkeeping.
struct WaitState {
  uint32_t count;   // |W|
  uint32_t snap;    // |W| as k_wait_gather found it (k_wait_compact reads this one)
  uint32_t ticket;  // k_wait_compact workgroups started
  uint32_t pad;
};

// Page-locked: what the host reads after the tick (stored by the last k_wait_compact workgroup).
struct WaitOutcome {
  uint32_t n_waiting;
  uint32_t n_resolved;
  uint32_t reserved[2];
};

// Look-back words of k_wait_compact: flag (2 bits) | resolved (31 bits) | survivors (31 bits).
constexpr unsigned long long kLbAggregate = 1ull << 62, kLbInclusive = 2ull << 62;
constexpr unsigned long long kLbValue = (1ull << 62) - 1;

// A further int64 column that travels with the entries where the context has one (wait_lease.h:
// the lease durations); all NULL otherwise.
struct WaitExtra {
  const int64_t* w;   // W's column
  int64_t* t;         // the batch's
  const int64_t* nw;  // the new requests'
};

// Thread per batch position j in [0, max_waiting + max_tasks).
__global__ __launch_bounds__(256) void k_wait_gather(WaitCols w, WaitCols t, WaitNew nw, uint32_t MW,
                                                     uint32_t N, WaitState* ws,
                                                     unsigned long long* lookback, uint32_t n_lookback,
                                                     WaitExtra x) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t cnt = ws->count;
  if (j == 0) {
    ws->snap = cnt;
    ws->ticket = 0;
  }
  if (j < n_lookback) lookback[j] = 0;
  if (j >= N) return;
  if (j < MW) {
    uint32_t e = kPadEnv, mv = 0, ip = 0;
    if (j < cnt) {
      const int64_t dl = w.deadline[j];
      t.deadline[j] = dl;
      t.tag[j] = w.tag[j];
      if (x.t) x.t[j] = x.w[j];
      if (dl > *nw.now) {  // (deadline <= now: expired, resolved as Timeout without being tried)
        e = w.env[j];
        mv = w.minv[j];
        ip = w.ip[j];
      }
    }
    t.env[j] = e;
    t.minv[j] = mv;
    t.ip[j] = ip;
  } else {
    const uint32_t k = j - MW;
    t.env[j] = nw.env[k];
    t.minv[j] = nw.minv[k];
    t.ip[j] = nw.ip[k];
    t.deadline[j] = nw.deadline[k];
    t.tag[j] = nw.tag[k];
    if (x.t) x.t[j] = x.nw[k];
  }
}

// Sum over the wave of a value per lane (every lane gets it).
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(v), 63);
}

// ceil(N / kWaitTile) workgroups of 256 threads; thread i of a workgroup owns four consecutive
// positions. prm == NULL: ungated (the host has just placed the batch itself).
__global__ __launch_bounds__(256) void k_wait_compact(WaitCols t, const uint32_t* placed, const int64_t* now_p,
                                                      uint32_t MW, uint32_t N, WaitCols w, WaitState* ws,
                                                      unsigned long long* lookback, uint32_t* out_new,
                                                      uint64_t* res_tag, uint32_t* res_idx,
                                                      WaitOutcome* outcome, const DeviceParams* prm,
                                                      uint32_t check_slot) {
  if (prm) {
    const bool final = (check_slot == kNone || prm->n_changed[check_slot] == 0) && !prm->window_miss &&
                       !prm->overflow;
    if (!final) return;  // (every workgroup alike: W stays as it is)
  }
  __shared__ uint32_t s_bid;
  __shared__ uint32_t lds[17];
  __shared__ uint32_t s_pre_surv, s_pre_res;
  if (threadIdx.x == 0) s_bid = atomicAdd(&ws->ticket, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const uint32_t snap = ws->snap;
  const int64_t now = *now_p;
  const uint32_t j0 = bid * kWaitTile + threadIdx.x * 4;
  // Per position: 1 survivor (stays in / joins W), 2 resolved (a waiting entry's answer), 0 neither.
  uint32_t kind[4], val[4];
  uint32_t n_surv = 0, n_res = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    kind[i] = 0;
    val[i] = 0;
    if (j >= N) continue;
    const uint32_t r = placed[j];
    if (j < MW) {
      if (j < snap) {
        if (t.deadline[j] <= now) {
          kind[i] = 2;
          val[i] = kIdxTimeout;
        } else if (r == kIdxTimeout) {
          kind[i] = 1;
        } else {
          kind[i] = 2;
          val[i] = r;
        }
      }
    } else {
      const bool queue = r == kIdxTimeout && t.deadline[j] > now;
      kind[i] = queue ? 1u : 0u;
      out_new[j - MW] = queue ? kIdxWaiting : r;
    }
    n_surv += kind[i] == 1;
    n_res += kind[i] == 2;
  }
  // Workgroup-local prefix of both counts at once (each < 2^16 per workgroup).
  uint32_t tot;
  const uint32_t ex = block_exclusive_scan(n_surv | (n_res << 16), lds, &tot);
  if (threadIdx.x < 64) {
    // Decoupled look-back by wave 0: publish the aggregate, sum the predecessors' words 64 at a
    // time until one carries an inclusive prefix, publish the inclusive prefix.
    const uint32_t lane = threadIdx.x;
    const unsigned long long agg = (unsigned long long)(tot & 0xFFFFu) | ((unsigned long long)(tot >> 16) << 31);
    uint32_t pre_s = 0, pre_r = 0;
    if (bid == 0) {
      if (lane == 0) __hip_atomic_store(&lookback[0], kLbInclusive | agg, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (lane == 0) __hip_atomic_store(&lookback[bid], kLbAggregate | agg, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      int look = (int)bid - 1;
      while (true) {
        const int q = look - (int)lane;
        unsigned long long st = kLbInclusive;  // (before block 0: an empty inclusive prefix)
        while (true) {
          if (q >= 0) st = __hip_atomic_load(&lookback[q], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          if (__ballot((st >> 62) == 0) == 0) break;
          __builtin_amdgcn_s_sleep(1);
        }
        const unsigned long long incl = __ballot((st >> 62) == 2);
        const uint32_t upto = incl ? (uint32_t)__builtin_ctzll(incl) : 63u;
        const unsigned long long v = lane <= upto ? (st & kLbValue) : 0ull;
        pre_s += wave_sum_u32((uint32_t)(v & 0x7FFFFFFFu));
        pre_r += wave_sum_u32((uint32_t)(v >> 31));
        if (incl) break;
        look -= 64;
      }
      if (lane == 0) {
        const unsigned long long inc = ((unsigned long long)(pre_s + (tot & 0xFFFFu))) |
                                       ((unsigned long long)(pre_r + (tot >> 16)) << 31);
        __hip_atomic_store(&lookback[bid], kLbInclusive | inc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (lane == 0) {
      s_pre_surv = pre_s;
      s_pre_res = pre_r;
      if (bid == gridDim.x - 1) {  // the last workgroup: the totals
        const uint32_t n_waiting = pre_s + (tot & 0xFFFFu), n_resolved = pre_r + (tot >> 16);
        ws->count = n_waiting;
        outcome->n_waiting = n_waiting;
        outcome->n_resolved = n_resolved;
      }
    }
  }
  __syncthreads();
  uint32_t ps = s_pre_surv + (ex & 0xFFFFu), pr = s_pre_res + (ex >> 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    if (kind[i] == 1) {
      if (ps < MW) {  // (always: |W| + n <= max_waiting is checked before the tick)
        w.env[ps] = t.env[j];
        w.minv[ps] = t.minv[j];
        w.ip[ps] = t.ip[j];
        w.deadline[ps] = t.deadline[j];
        w.tag[ps] = t.tag[j];
      }
      ++ps;
    } else if (kind[i] == 2) {
      if (pr < MW) {
        res_tag[pr] = t.tag[j];
        res_idx[pr] = val[i];
      }
      ++pr;
    }
  }
}

}  // namespace ydc

// rpc_stream.h — one request row per WaitForStartingTask RPC (ydc_stream_begin_rpc /
// ydc_stream_tick_rpc), on top of the waiting queue W and the lease table L of wait_lease.h.
//
// The unit a scheduler receives is one RPC (scheduler_service_impl.cc:209-271): one personality
// asking for n_immediate + n_prefetch grants. Only the first grant may wait until the deadline,
// the others are tried at the moment the first is granted, the loops stop at the first failure,
// and an RPC that ends without a grant is NO_QUOTA (EnvironmentNotFound fails it only inside the
// immediate loop). A request row carries the two counts, one entry of W stands for one blocked
// RPC, and the device expands the entries into batch rows:
//
//   k_rpc_scan     positions [max_waiting slots of W | max_requests new requests]: the entry's
//                  eight columns are copied beside the position (W is only read), rows = n_immediate
//                  + n_prefetch (0: unused slot, expired entry, padding) is scanned with a
//                  decoupled look-back and row_start[] goes to HBM.
//   k_rpc_expand   thread per batch row: the owner by binary search in row_start (as
//                  k_lease_report in report_off), the three batch columns and lease_for; rows from
//                  the tick's total up to max_rows are a digest nobody has.
//   (front, passes, k_finalize place the max_rows rows as one batch)
//   k_rpc_grant    thread per row, gated like k_finalize: stable scan of "granted", id = next_id +
//                  rank, the lease (lease_file of lease_table.h), the exclusive
//                  rank per row to HBM, servants and ids to page-locked memory: W's region packed by
//                  rank (it leads the batch, so an entry's first grant is the rank of its first
//                  row), the new requests' rows at row - rows(W).
//   k_rpc_settle   thread per position: g = rank difference over the entry's rows; granted-g /
//                  env-not-available / no-quota / waiting; stable scan of (survivors, resolved);
//                  the new W, the resolved list, the new requests' status and count. The last
//                  workgroup stores |W|, rows(W), |L|, next_id and the outcome blocks.
//
// Whether a row is a prefetch (rank within its RPC >= n_immediate) is stored only with inspection on
// (stream_inspect.h): the reference logs is_prefetch (task_dispatcher.cc:464,531) and DumpInternals
// prints it as prefetched_task (:598).
//
// Look-back (stream_tile.h): one word per tile, three arrays (scan, settle, grant). k_lease_renew,
// the step's first launch, clears them; k_rpc_expand, which runs when the scan is complete and
// before the other two start, resets the three tickets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"
#include "stream_inspect.h"
#include "stream_tile.h"
#include "wait_queue.h"

namespace ydc {

constexpr uint32_t kRpcTile = 1024;  // positions / rows per workgroup of scan, grant, settle (256 x 4)

// Eight columns per RPC: W (max_waiting entries: WaitCols' five, the lease durations of
// wait_lease.h and this mode's two counts) or the tick's positions (max_waiting + max_requests).
struct RpcEntryCols {
  uint32_t *env, *minv, *ip;
  int64_t* deadline;
  uint64_t* tag;
  int64_t* lease_for;
  uint32_t *n_imm, *n_pre;
};

// The tick's new requests as the host staged them (page-locked arena, or its device copy).
struct RpcNew {
  const uint32_t *env, *minv, *ip;
  const int64_t* deadline;
  const uint64_t* tag;
  const int64_t* lease_for;
  const uint32_t *n_imm, *n_pre;  // (0, 0 behind the tick's requests)
};

// The expanded batch (max_rows rows) and what is kept about it in HBM.
struct RpcBatch {
  uint32_t *env, *minv, *ip;
  int64_t* lease_for;
  const uint32_t* placed;  // k_finalize's answers
  uint32_t* rank;          // [max_rows + 1] grants in front of a row
  uint32_t* row_start;     // [positions + 1] first row of a position
};

struct RpcState {
  uint32_t t_scan, t_grant, t_settle;  // workgroups started (tickets)
  uint32_t w_rows;                     // rows of the survivors (k_rpc_settle adds them up)
};

// Page-locked: what the host reads after the tick.
struct RpcOutcome {
  uint32_t n_waiting, n_resolved, n_waiting_rows;
  uint32_t n_rows;        // rows of the tick's batch (padding excluded)
  uint32_t n_res_grants;  // grants of W's entries (the packed lists' length)
  uint32_t granted;
  uint32_t reserved[2];
};

// Page-locked results (device addresses).
struct RpcOut {
  uint32_t* new_srv;               // [max_rows] expanded layout, first new row at 0
  unsigned long long* new_id;      // [max_rows]
  uint32_t *status, *n_granted;    // [max_requests]
  uint64_t* res_tag;               // [max_waiting]
  uint32_t *res_status, *res_n, *res_first;
  uint32_t* res_srv;               // [max_rows] W's grants packed by rank
  unsigned long long* res_id;      // [max_rows]
  RpcOutcome* outcome;
};

// k_rpc_scan's own look-back, the form it was timed with (tile_lookback<1> of stream_tile.h is the
// same protocol; under it the compiler schedules the scan's column copies differently, and that was
// measured 1.5 us slower). Wave 0 of the workgroup with ticket `bid`: publishes the workgroup's two totals (each < 2^31,
// sums too) and returns the sums over the workgroups in front (every lane gets them).
__device__ __forceinline__ void rpc_lookback(unsigned long long* lookback, uint32_t bid, uint32_t lane,
                                             uint32_t tot_lo, uint32_t tot_hi, uint32_t* pre_lo, uint32_t* pre_hi) {
  const unsigned long long agg = (unsigned long long)tot_lo | ((unsigned long long)tot_hi << 31);
  uint32_t lo = 0, hi = 0;
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
      lo += wave_sum_u32((uint32_t)(v & 0x7FFFFFFFu));
      hi += wave_sum_u32((uint32_t)(v >> 31));
      if (incl) break;
      look -= 64;
    }
    if (lane == 0) {
      const unsigned long long inc = (unsigned long long)(lo + tot_lo) | ((unsigned long long)(hi + tot_hi) << 31);
      __hip_atomic_store(&lookback[bid], kLbInclusive | inc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  *pre_lo = lo;
  *pre_hi = hi;
}

// ceil(P / kRpcTile) workgroups of 256 threads over the P = MW + max_requests positions; thread i
// of a workgroup owns four consecutive positions.
__global__ __launch_bounds__(256) void k_rpc_scan(RpcEntryCols w, RpcNew nw, RpcEntryCols p, const LeaseHdr* hdr,
                                                  uint32_t MW, uint32_t P, WaitState* ws, RpcState* rs,
                                                  unsigned long long* lookback, uint32_t* row_start) {
  __shared__ uint32_t s_bid, s_pre;
  __shared__ uint32_t lds[17];
  if (threadIdx.x == 0) s_bid = atomicAdd(&rs->t_scan, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const uint32_t cnt = ws->count;  // (k_rpc_settle's last workgroup changes it, launches later)
  const int64_t now = hdr->now;
  if (bid == 0 && threadIdx.x == 0) ws->snap = cnt;
  const uint32_t j0 = bid * kRpcTile + threadIdx.x * 4;
  uint32_t rows[4], sum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    rows[i] = 0;
    if (j >= P) continue;
    uint32_t a = 0, b = 0;
    int64_t dl = 0;
    if (j < MW) {
      if (j < cnt) {
        dl = w.deadline[j];
        a = w.n_imm[j];
        b = w.n_pre[j];
        p.env[j] = w.env[j];
        p.minv[j] = w.minv[j];
        p.ip[j] = w.ip[j];
        p.tag[j] = w.tag[j];
        p.lease_for[j] = w.lease_for[j];
        // (deadline <= now: expired, resolved as no-quota without being tried)
        rows[i] = dl > now ? a + b : 0u;
      }
    } else {
      const uint32_t k = j - MW;
      dl = nw.deadline[k];
      a = nw.n_imm[k];
      b = nw.n_pre[k];
      p.env[j] = nw.env[k];
      p.minv[j] = nw.minv[k];
      p.ip[j] = nw.ip[k];
      p.tag[j] = nw.tag[k];
      p.lease_for[j] = nw.lease_for[k];
      rows[i] = a + b;
    }
    p.deadline[j] = dl;
    p.n_imm[j] = a;
    p.n_pre[j] = b;
    sum += rows[i];
  }
  uint32_t tot;
  const uint32_t ex = block_exclusive_scan(sum, lds, &tot);
  if (threadIdx.x < 64) {
    uint32_t pre, unused;
    rpc_lookback(lookback, bid, threadIdx.x, tot, 0u, &pre, &unused);
    if (threadIdx.x == 0) {
      s_pre = pre;
      if (bid == gridDim.x - 1) row_start[P] = pre + tot;  // the last workgroup: the tick's rows
    }
  }
  __syncthreads();
  uint32_t at = s_pre + ex;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (j0 + i < P) row_start[j0 + i] = at;
    at += rows[i];
  }
}

// Thread per batch row j in [0, NR).
__global__ __launch_bounds__(256) void k_rpc_expand(RpcEntryCols p, uint32_t P, uint32_t NR, RpcBatch b,
                                                    RpcState* rs) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) {  // (the scan is complete, grant and settle have not begun)
    rs->t_scan = rs->t_grant = rs->t_settle = 0;
    rs->w_rows = 0;
  }
  if (j >= NR) return;
  uint32_t e = kPadEnv, mv = 0, ip = 0;
  int64_t lf = 0;
  if (j < b.row_start[P]) {
    // The position row j belongs to: the last q with row_start[q] <= j (positions without rows in
    // front of it share its row_start and lie before it).
    uint32_t lo = 0, hi = P;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (b.row_start[mid] <= j) lo = mid; else hi = mid;
    }
    e = p.env[lo];
    mv = p.minv[lo];
    ip = p.ip[lo];
    lf = p.lease_for[lo];
  }
  b.env[j] = e;
  b.minv[j] = mv;
  b.ip[j] = ip;
  b.lease_for[j] = lf;
}

// ceil(NR / kRpcTile) workgroups of 256 threads over the rows of the placed batch; thread i of a
// workgroup owns four consecutive rows. prm == NULL: ungated (the host has just placed the batch
// itself). k_rpc_grant_inspect below is this kernel's twin: a change here belongs there as well.
__global__ __launch_bounds__(256) void k_rpc_grant(RpcBatch b, uint32_t NR, uint32_t MW, const LeaseHdr* hdr,
                                                   LeaseCols L, LeaseState* st, RpcState* rs,
                                                   unsigned long long* lookback, RpcOut o,
                                                   const DeviceParams* prm, uint32_t check_slot) {
  if (prm && !batch_is_final(prm, check_slot)) return;  // (every workgroup alike: L stays as it is)
  __shared__ uint32_t s_bid, s_pre;
  __shared__ uint32_t lds[17];
  if (threadIdx.x == 0) s_bid = atomicAdd(&rs->t_grant, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const unsigned long long next = st->next_id;  // (k_rpc_settle's last workgroup changes it, a launch later)
  const int64_t now = hdr->now;
  const uint32_t w_rows = b.row_start[MW];  // W's region leads the batch
  const uint32_t j0 = bid * kRpcTile + threadIdx.x * 4;
  uint32_t r[4];
  uint32_t n_gr = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r[i] = j0 + i < NR ? b.placed[j0 + i] : kIdxEnvNotFound;
    n_gr += r[i] < kIdxWaiting;
  }
  uint32_t tot;
  const uint32_t ex = block_exclusive_scan(n_gr, lds, &tot);
  if (threadIdx.x < 64) {
    const uint32_t pre = lb_lo(tile_lookback<1>(lookback, bid, threadIdx.x, {{lb_pack(tot)}}).w[0]);
    if (threadIdx.x == 0) {
      s_pre = pre;
      if (bid == gridDim.x - 1) b.rank[NR] = pre + tot;  // the last workgroup: the tick's grants
    }
  }
  __syncthreads();
  uint32_t rk = s_pre + ex;
  unsigned long long ids[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    ids[i] = kLeaseEmpty;
    if (j < NR) b.rank[j] = rk;
    if (r[i] >= kIdxWaiting) continue;
    ids[i] = next + rk;
    lease_file(L, st, ids[i], now + b.lease_for[j], r[i], kLeaseLive);  // the lease runs from the grant
    if (j < w_rows) {  // a waiting RPC's grant: packed by rank (rk <= j < NR)
      o.res_srv[rk] = r[i];
      o.res_id[rk] = ids[i];
    }
    ++rk;
  }
  // The new requests' rows to page-locked memory (vector stores where rows(W) is a multiple of 4).
  store_answers(o.new_srv, o.new_id, j0, w_rows, NR, r, ids);
}

// k_rpc_grant with inspection on (stream_inspect.h): the inserting thread also files the grant's
// detail record (started_at = the granting tick's now; the row is a prefetch iff its rank inside its
// RPC is >= n_immediate) and counts it for its servant. A kernel of its own, not a shared pass with a
// compile-time flag as in wait_lease.h: moving k_rpc_grant's body into a function both kernels call
// changed k_rpc_grant's register allocation (its assembly was compared), and a stream without
// inspection launches the code it launched before.
__global__ __launch_bounds__(256) void k_rpc_grant_inspect(RpcBatch b, uint32_t NR, uint32_t MW, const LeaseHdr* hdr,
                                                           LeaseCols L, LeaseState* st, RpcState* rs,
                                                           unsigned long long* lookback, RpcOut o,
                                                           const DeviceParams* prm, uint32_t check_slot,
                                                           InspectIn ins) {
  if (prm && !batch_is_final(prm, check_slot)) return;  // (every workgroup alike: L stays as it is)
  __shared__ uint32_t s_bid, s_pre;
  __shared__ uint32_t lds[17];
  if (threadIdx.x == 0) s_bid = atomicAdd(&rs->t_grant, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const unsigned long long next = st->next_id;  // (k_rpc_settle's last workgroup changes it, a launch later)
  const int64_t now = hdr->now;
  const uint32_t w_rows = b.row_start[MW];  // W's region leads the batch
  const uint32_t j0 = bid * kRpcTile + threadIdx.x * 4;
  uint32_t r[4];
  uint32_t n_gr = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r[i] = j0 + i < NR ? b.placed[j0 + i] : kIdxEnvNotFound;
    n_gr += r[i] < kIdxWaiting;
  }
  uint32_t tot;
  const uint32_t ex = block_exclusive_scan(n_gr, lds, &tot);
  if (threadIdx.x < 64) {
    const uint32_t pre = lb_lo(tile_lookback<1>(lookback, bid, threadIdx.x, {{lb_pack(tot)}}).w[0]);
    if (threadIdx.x == 0) {
      s_pre = pre;
      if (bid == gridDim.x - 1) b.rank[NR] = pre + tot;  // the last workgroup: the tick's grants
    }
  }
  __syncthreads();
  uint32_t rk = s_pre + ex;
  unsigned long long ids[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    ids[i] = kLeaseEmpty;
    if (j < NR) b.rank[j] = rk;
    if (r[i] >= kIdxWaiting) continue;
    ids[i] = next + rk;
    // The position row j belongs to (k_rpc_expand's search), and with it the row's rank in its RPC.
    uint32_t lo = 0, hi = ins.P;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (b.row_start[mid] <= j) lo = mid; else hi = mid;
    }
    lease_insert_inspected(L, st, ins, ids[i], now + b.lease_for[j], r[i], now, j,
                           j - b.row_start[lo] >= ins.n_imm[lo]);  // the lease runs from the grant
    if (j < w_rows) {  // a waiting RPC's grant: packed by rank (rk <= j < NR)
      o.res_srv[rk] = r[i];
      o.res_id[rk] = ids[i];
    }
    ++rk;
  }
  // The new requests' rows to page-locked memory (vector stores where rows(W) is a multiple of 4).
  store_answers(o.new_srv, o.new_id, j0, w_rows, NR, r, ids);
}

// ceil(P / kRpcTile) workgroups of 256 threads over the positions; thread i of a workgroup owns
// four consecutive positions. prm as k_rpc_grant (which has run: rank[] is complete).
__global__ __launch_bounds__(256) void k_rpc_settle(RpcEntryCols p, RpcBatch b, uint32_t MW, uint32_t P, uint32_t NR,
                                                    const LeaseHdr* hdr, RpcEntryCols w, WaitState* ws,
                                                    RpcState* rs, LeaseState* st, unsigned long long* lookback,
                                                    RpcOut o, LeaseOutcome* lout, const DeviceParams* prm,
                                                    uint32_t check_slot) {
  if (prm && !batch_is_final(prm, check_slot)) return;  // (every workgroup alike: W, L and next_id stay as they are)
  __shared__ uint32_t s_bid, s_pre_surv, s_pre_res;
  __shared__ uint32_t lds[17];
  if (threadIdx.x == 0) s_bid = atomicAdd(&rs->t_settle, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const uint32_t snap = ws->snap;
  const int64_t now = hdr->now;
  const uint32_t j0 = bid * kRpcTile + threadIdx.x * 4;
  // Per position: kind 1 survivor (stays in / joins W), 2 resolved (a waiting RPC's answer), 0 neither.
  uint32_t kind[4], status[4], g[4], first[4];
  uint32_t n_surv = 0, n_res = 0, surv_rows = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    kind[i] = 0;
    status[i] = kIdxEnvNotFound;
    g[i] = first[i] = 0;
    if (j >= P) continue;
    const uint32_t r0 = b.row_start[j], r1 = b.row_start[j + 1];
    first[i] = b.rank[r0];
    g[i] = b.rank[r1] - first[i];
    const bool tried = r1 > r0;
    if (j < MW && j >= snap) continue;  // an unused slot of W
    if (g[i]) {
      status[i] = 0;
    } else if (tried && b.placed[r0] == kIdxEnvNotFound) {
      // (EnvironmentNotFound fails the RPC only inside the immediate loop; the prefetch loop just
      // breaks and the RPC ends as NO_QUOTA)
      status[i] = p.n_imm[j] ? kIdxEnvNotFound : kIdxTimeout;
    } else if (tried && p.deadline[j] > now) {
      status[i] = kIdxWaiting;
    } else if (tried || j < MW) {
      status[i] = kIdxTimeout;  // (untried: an entry of W whose deadline has passed)
    }
    if (tried || j < MW) kind[i] = status[i] == kIdxWaiting ? 1u : j < MW ? 2u : 0u;
    if (j >= MW) {
      o.status[j - MW] = status[i];
      o.n_granted[j - MW] = g[i];
    }
    n_surv += kind[i] == 1;
    n_res += kind[i] == 2;
    if (kind[i] == 1) surv_rows += r1 - r0;
  }
  uint32_t tot, tot_rows;
  const uint32_t ex = block_exclusive_scan(n_surv | (n_res << 16), lds, &tot);
  (void)block_exclusive_scan(surv_rows, lds, &tot_rows);
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    // (before the workgroup's word is published: the last workgroup reads the sum behind it)
    if (lane == 0 && tot_rows) atomicAdd(&rs->w_rows, tot_rows);
    const LbWords<1> pre = tile_lookback<1>(lookback, bid, lane, {{lb_pack(tot & 0xFFFFu, tot >> 16)}});
    const uint32_t pre_s = lb_lo(pre.w[0]), pre_r = lb_hi(pre.w[0]);
    if (lane == 0) {
      s_pre_surv = pre_s;
      s_pre_res = pre_r;
      if (bid == gridDim.x - 1) {  // the last workgroup: the totals
        const uint32_t n_waiting = pre_s + (tot & 0xFFFFu), n_resolved = pre_r + (tot >> 16);
        const uint32_t granted = b.rank[NR];
        const uint32_t w_rows = __hip_atomic_load(&rs->w_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ws->count = n_waiting;
        o.outcome->n_waiting = n_waiting;
        o.outcome->n_resolved = n_resolved;
        o.outcome->n_waiting_rows = w_rows;
        o.outcome->n_rows = b.row_start[P];
        o.outcome->n_res_grants = b.rank[b.row_start[MW]];
        o.outcome->granted = granted;
        st->next_id = lease_close_tick(st, hdr, lout, granted, st->next_id);
      }
    }
  }
  __syncthreads();
  uint32_t ps = s_pre_surv + (ex & 0xFFFFu), pr = s_pre_res + (ex >> 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = j0 + i;
    if (kind[i] == 1) {
      if (ps < MW) {  // (always: |W| + n_req <= max_waiting is checked before the tick)
        copy_entry(w, ps, p, j);
        w.lease_for[ps] = p.lease_for[j];
        w.n_imm[ps] = p.n_imm[j];
        w.n_pre[ps] = p.n_pre[j];
      }
      ++ps;
    } else if (kind[i] == 2) {
      if (pr < MW) {
        o.res_tag[pr] = p.tag[j];
        o.res_status[pr] = status[i];
        o.res_n[pr] = g[i];
        o.res_first[pr] = first[i];
      }
      ++pr;
    }
  }
}

}  // namespace ydc

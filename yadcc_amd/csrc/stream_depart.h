// stream_depart.h — a departed requestor's leases and waiting calls leave inside the tick
// (ydc_stream_depart_begin / _stage / _result), in the three modes that keep leases, with inspection on.
//
// A departure is nothing the tick does not know already: the leases go as FreeTask frees them
// (task_dispatcher.cc:169-188), the waiting calls as calls whose max_wait ended (:93-118). What is new is
// the pass that picks them by requestor: every lease has its requestor in its inspection record
// (stream_inspect.h), every entry of W in its ip column. Small launches of its own stand around the
// unchanged tick kernels, and a stream that never switched the capability on launches none of them:
//
//   k_depart_load    the staged requestors (sorted, duplicates removed by the host — the kernels search
//                    the list, and the host keeps each staged requestor's place in it for the result
//                    call, as k_withdraw_load says for tags) and their number from the tick's arena into
//                    HBM, and four zeroed counts per requestor beside them: leases | zombies | waiting |
//                    waiting_rows. The arena of the captured step is page-locked host memory; a search
//                    in it would cross the bus at every probe.
//   (k_lease_renew, k_lease_free: the caller's own renewals and frees come first; a lease the caller
//    freed is the caller's)
//   k_depart_leases  k_lease_sweep's shape over L: ceil(cap / 1024) workgroups of 256 threads, four
//                    consecutive slots per thread, their states one 16-byte load. EVERY THREAD RETURNS
//                    BEFORE IT TOUCHES L WHEN THE LIST IS EMPTY: the idle price is the launch, not a pass
//                    over the table. A live slot's record is read (an erased slot keeps a stale one, so
//                    the live bit decides); a record without a time (granted while inspection was off)
//                    belongs to nobody; the requestor is searched in the list. A hit is freed exactly as
//                    k_lease_free frees a won lease: key = kLeaseEmpty, state = 0, running_tasks - 1 under
//                    s < n_servants (a lease parked by aliveness touches no row), one more in
//                    LeaseState::freed, so lease_close_tick's arithmetic holds unchanged. The list is
//                    copied to LDS while it has at most kDepartLds = 2048 requestors (8 KB: several
//                    workgroups per CU keep their room, and ten probes of a search stay on chip); a
//                    longer list is searched in HBM / L2. One requestor that holds most of L is the usual
//                    departure, so equal hits are combined before the global atomic: a thread's four
//                    slots first, then inside the wave (wave_combine of stream_tile.h), then the four waves'
//                    first rounds through LDS, so the hot requestor's count takes one atomic per
//                    workgroup, as `freed` does. (Combined inside the wave only, the pass over 10^6
//                    leases of one requestor took 755 us, all of it the 32 768 atomics on one address;
//                    k_lease_sweep reads the same table in 11 us.)
//   (k_lease_report: a departed lease is unknown to a report of the same tick; k_lease_sweep)
//   k_depart_mark    streams with W, behind k_withdraw_mark and in front of the quota's load pass and
//                    the gather. Thread per position j < |W|: the entry's requestor searched in the list;
//                    on a hit whose deadline is not INT64_MIN yet (withdrawal's mark of this tick, which
//                    counts and labels the entry itself) the deadline becomes INT64_MIN and the entry and
//                    its rows are counted. A natural deadline is never INT64_MIN in W.
//   (gather / scan … commit pass / settling: the entry resolves as Timeout at its queue position)
//   k_depart_done    gated like the commit pass and k_withdraw_label: the counts stored once, with plain
//                    stores, to the page-locked result block. A launch of its own and not folded into
//                    k_depart_mark or k_depart_leases: those run in front of the batch, where no gate
//                    exists yet, and a leased stream has no k_depart_mark at all; folding it into
//                    k_withdraw_label or k_quota_label would edit an existing kernel.
//
// Every index is bounded by the table's cap, max_waiting or max_depart as the launch was sized; the
// list's length read from HBM is clipped to max_depart wherever it is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"
#include "requestor_index.h"
#include "stream_inspect.h"
#include "wait_queue.h"

namespace ydc {

constexpr uint32_t kDepartLds = 2048;  // requestors of the list a workgroup of k_depart_leases keeps in LDS

// HBM: the tick's list, [max_depart] each, and how many of them the tick staged.
struct DepartList {
  uint32_t* ip;  // ascending, no duplicates
  uint4* count;  // per requestor: leases | zombies | waiting | waiting_rows
  uint32_t* n;
};

// Page-locked: what the host reads after the tick. n: the list's length as k_depart_done saw it.
struct DepartDone {
  uint32_t n;
  uint32_t tick_no;
  uint32_t reserved[2];
};

// Position of `key` in ip[0, n) (ascending, unique), or n (withdraw_find's search).
template <typename P>
__device__ __forceinline__ uint32_t depart_find(P ip, uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ip[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo < n && ip[lo] == key ? lo : n;
}

// One entry per active lane for the list's place `at`: a | b into the pair of counts at `col`, equal
// places combined inside the wave first. Every lane of the wave must get here (wave_combine).
// first != NULL: the first round's sums are left there (place | a | b) for the workgroup to combine,
// instead of being added.
__device__ __forceinline__ void depart_add(uint4* count, bool active, uint32_t at, uint32_t col, uint32_t a,
                                           uint32_t b, uint32_t* first = nullptr) {
  active = wave_combine(active, at, [&](uint32_t at0, bool mine, unsigned long long, bool leads, uint32_t round) {
    const uint32_t sa = wave_sum_if_any(mine ? a : 0u), sb = wave_sum_if_any(mine ? b : 0u);
    if (leads) {
      if (first && round == 0) {
        first[0] = at0, first[1] = sa, first[2] = sb;
      } else {
        uint32_t* const p = reinterpret_cast<uint32_t*>(count + at0) + col;
        if (sa) atomicAdd(p, sa);
        if (sb) atomicAdd(p + 1, sb);
      }
    }
  });
  if (active) {
    uint32_t* const p = reinterpret_cast<uint32_t*>(count + at) + col;
    if (a) atomicAdd(p, a);
    if (b) atomicAdd(p + 1, b);
  }
}

// Thread per slot i of the list, i in [0, MX). in_ip / in_n: the arena's, as the step sees it.
__global__ __launch_bounds__(256) void k_depart_load(const uint32_t* in_ip, const uint32_t* in_n, uint32_t MX,
                                                     DepartList l) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = min(*in_n, MX);
  if (i == 0) *l.n = n;
  if (i >= n) return;
  l.ip[i] = in_ip[i];
  l.count[i] = make_uint4(0, 0, 0, 0);
}

// ceil(cap / kLeaseTile) workgroups; thread i owns four consecutive slots. rec: the inspection records,
// parallel to L's slots.
__global__ __launch_bounds__(256) void k_depart_leases(LeaseCols L, LeaseState* st, const uint4* rec, DepartList l,
                                                       uint32_t MX, uint32_t n_servants, uint32_t* running) {
  __shared__ uint32_t s_ip[kDepartLds];
  __shared__ uint32_t s_freed;
  __shared__ uint32_t s_first[4][3];  // per wave: its first round's place | leases | zombies
  const uint32_t n = min(*l.n, MX);
  if (n == 0) return;  // (every thread of every workgroup alike; L is not touched)
  const bool in_lds = n <= kDepartLds;
  if (in_lds)
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) s_ip[i] = l.ip[i];
  if (threadIdx.x == 0) s_freed = 0;
  if (threadIdx.x < 4) s_first[threadIdx.x][0] = kNone;
  __syncthreads();
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint4 sv = lease_states4(L, i0);
  uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
  uint32_t n_freed = 0;
  if (__ballot(((st4[0] | st4[1] | st4[2] | st4[3]) & kLeaseLive) != 0)) {  // (wave-uniform)
    uint32_t at4[4], a4[4], z4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t at = n;
      if (st4[k] & kLeaseLive) {
        const uint4 r = rec[i0 + k];
        if (inspect_started(r) != kInspectNoTime)
          at = in_lds ? depart_find((const uint32_t*)s_ip, n, r.w) : depart_find((const uint32_t*)l.ip, n, r.w);
      }
      const bool hit = at != n;
      if (hit) {
        const uint32_t s = L.servant[i0 + k];
        L.key[i0 + k] = kLeaseEmpty;
        if (s < n_servants) atomicSub(&running[s], 1u);
        ++n_freed;
      }
      at4[k] = at, a4[k] = hit ? 1u : 0u, z4[k] = hit && (st4[k] & kLeaseZombie) ? 1u : 0u;
      if (hit) st4[k] = 0;
    }
    if (n_freed) *reinterpret_cast<uint4*>(L.state + i0) = make_uint4(st4[0], st4[1], st4[2], st4[3]);
    // The thread's equal places into the first of them, and its first entry to the front: entry 0 then
    // carries what the wave's first round and the workgroup combine.
#pragma unroll
    for (int k = 1; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < k; ++j)
        if (a4[k] && a4[j] && at4[j] == at4[k]) {
          a4[j] += a4[k], z4[j] += z4[k];
          a4[k] = 0, at4[k] = n;
        }
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (!a4[0] && a4[k]) {
        at4[0] = at4[k], a4[0] = a4[k], z4[0] = z4[k];
        a4[k] = 0, at4[k] = n;
      }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      depart_add(l.count, a4[k] != 0, at4[k], 0, a4[k], z4[k], k == 0 ? s_first[threadIdx.x >> 6] : nullptr);
  }
  // One atomic per workgroup.
  const uint32_t wf = wave_sum_if_any(n_freed);
  if ((threadIdx.x & 63) == 0 && wf) atomicAdd(&s_freed, wf);
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (s_freed) atomicAdd(&st->freed, s_freed);
  for (uint32_t w = 0; w < 4; ++w) {  // (the waves' first rounds: equal places once)
    const uint32_t at = s_first[w][0];
    if (at == kNone) continue;
    uint32_t a = s_first[w][1], b = s_first[w][2];
    for (uint32_t v = w + 1; v < 4; ++v)
      if (s_first[v][0] == at) {
        a += s_first[v][1], b += s_first[v][2];
        s_first[v][0] = kNone;
      }
    uint32_t* const p = reinterpret_cast<uint32_t*>(l.count + min(at, MX - 1));
    if (a) atomicAdd(p, a);
    if (b) atomicAdd(p + 1, b);
  }
}

// Thread per position j of W, j in [0, MW). W is as the previous tick left it (ws->count entries) and
// as k_withdraw_mark has marked it. w_imm == NULL (no rpc stream): an entry is one row.
__global__ __launch_bounds__(256) void k_depart_mark(DepartList l, uint32_t MX, const uint32_t* w_ip,
                                                     int64_t* w_deadline, const uint32_t* w_imm, const uint32_t* w_pre,
                                                     const WaitState* ws, uint32_t MW) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = min(*l.n, MX);
  if (n == 0) return;  // (every thread alike)
  uint32_t at = n;
  if (j < min(ws->count, MW) && w_deadline[j] != INT64_MIN) at = depart_find((const uint32_t*)l.ip, n, w_ip[j]);
  const bool hit = at != n;
  uint32_t rows = 0;
  if (hit) {
    w_deadline[j] = INT64_MIN;
    rows = w_imm ? w_imm[j] + w_pre[j] : 1u;
  }
  depart_add(l.count, hit, at, 2, 1u, rows);
}

// Thread per slot i of the list, i in [0, MX). prm == NULL: ungated.
__global__ __launch_bounds__(256) void k_depart_done(DepartList l, uint32_t MX, const LeaseHdr* hdr, uint4* out_count,
                                                     DepartDone* done, const DeviceParams* prm, uint32_t check_slot) {
  if (prm && !batch_is_final(prm, check_slot)) return;  // (every workgroup alike)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = min(*l.n, MX);
  if (i == 0) {
    done->n = n;
    done->tick_no = hdr->tick_no;
  }
  if (i < n) out_count[i] = l.count[i];
}

}  // namespace ydc

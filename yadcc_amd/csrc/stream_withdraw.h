// stream_withdraw.h — waiting requests taken out of W by tag, inside the tick
// (ydc_stream_withdraw_begin / _stage / _result), in the three modes that have a queue.
//
// A withdrawn entry is an entry whose deadline ends in this tick: the reference's call whose max_wait
// ran out (task_dispatcher.cc:93-118). So the feature touches neither the gather / scan in front of
// the batch nor the commit pass / settling behind it. Three small launches of its own stand around
// them, and a stream that never switched the capability on launches none of them:
//
//   k_withdraw_load   the staged tags (sorted, duplicates removed by the host) and their number from
//                     the tick's arena into HBM, and a zeroed count per tag beside them. The arena of
//                     the captured step is page-locked host memory; a search in it would cross the bus
//                     at every probe.
//   k_withdraw_mark   thread per position j < |W|: binary search of W.tag[j] in the list (the idiom of
//                     k_rpc_expand and k_lease_report). On a hit W.deadline[j] = INT64_MIN and the
//                     tag's count grows by one. Only an entry the thread actually changes is counted,
//                     so a second run finds nothing to do. A natural deadline is never INT64_MIN in W:
//                     an entry is only queued with deadline > now.
//   (gather / scan: the entry is expired — a request for a digest nobody has, it consumes nothing;
//    front, passes, k_finalize; commit pass / settling: it resolves as Timeout at its queue position)
//   k_withdraw_label  gated like the commit pass. Thread per resolved entry: binary search of its tag
//                     in the list; a hit's answer (rpc: its status) becomes YDC_IDX_WITHDRAWN. Every
//                     entry of W with a staged tag was marked and new requests never enter the
//                     resolved list, so a hit is a withdrawn entry. The same launch stores the counts
//                     to the page-locked result block: once, with plain stores (the adding was done
//                     in HBM).
//
// YDC_IDX_WITHDRAWN is written behind the commit pass, into page-locked memory only: no kernel ever
// compares it with kIdxWaiting ("is a grant").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "wait_queue.h"

namespace ydc {

constexpr uint32_t kIdxWithdrawn = 0xFFFFFFFCu;  // YDC_IDX_WITHDRAWN

// HBM: the tick's list, [max_withdraw] each, and how many of them the tick staged.
struct WithdrawList {
  unsigned long long* tag;  // ascending, no duplicates
  uint32_t* count;          // entries of W marked per tag
  uint32_t* n;
};

// Page-locked: what the host reads after the tick. n: the list's length as the label pass saw it.
struct WithdrawDone {
  uint32_t n;
  uint32_t reserved[3];
};

// Position of `key` in tag[0, n) (ascending, unique), or n.
__device__ __forceinline__ uint32_t withdraw_find(const unsigned long long* tag, uint32_t n, unsigned long long key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tag[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo < n && tag[lo] == key ? lo : n;
}

// Thread per slot i of the list, i in [0, MX). in_tag / in_n: the arena's, as the step sees it.
__global__ __launch_bounds__(256) void k_withdraw_load(const uint64_t* in_tag, const uint32_t* in_n, uint32_t MX,
                                                       WithdrawList l) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = min(*in_n, MX);
  if (i == 0) *l.n = n;
  if (i >= n) return;
  l.tag[i] = in_tag[i];
  l.count[i] = 0;
}

// Thread per position j of W, j in [0, MW). W is as the previous tick left it: ws->count entries.
__global__ __launch_bounds__(256) void k_withdraw_mark(WithdrawList l, uint32_t MX, const uint64_t* w_tag,
                                                       int64_t* w_deadline, const WaitState* ws, uint32_t MW) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = min(*l.n, MX);
  if (n == 0 || j >= min(ws->count, MW)) return;
  const uint32_t at = withdraw_find(l.tag, n, w_tag[j]);
  if (at == n || w_deadline[j] == INT64_MIN) return;
  w_deadline[j] = INT64_MIN;
  atomicAdd(&l.count[at], 1u);
}

// Thread per position of max(MW, MX): resolved entry i of the tick's list (n_resolved: the outcome
// block's, stored by the commit pass's last workgroup) and slot i of the counts. prm == NULL: ungated.
__global__ __launch_bounds__(256) void k_withdraw_label(WithdrawList l, uint32_t MX, const uint64_t* res_tag,
                                                        uint32_t* res_idx, const uint32_t* n_resolved, uint32_t MW,
                                                        uint32_t* out_count, WithdrawDone* done,
                                                        const DeviceParams* prm, uint32_t check_slot) {
  if (prm && !batch_is_final(prm, check_slot)) return;  // (every workgroup alike)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = min(*l.n, MX);
  if (i == 0) done->n = n;
  if (n == 0) return;
  if (i < n) out_count[i] = l.count[i];
  if (i >= min(*n_resolved, MW)) return;
  if (withdraw_find(l.tag, n, res_tag[i]) != n) res_idx[i] = kIdxWithdrawn;
}

}  // namespace ydc

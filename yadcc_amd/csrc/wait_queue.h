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
//   k_wait_compact  the commit pass of wait_lease.h in its form without leases: W's Timeouts whose
//                   deadline has not passed and the new requests' Timeouts with a deadline still
//                   ahead are the new W (order kept); W's grants, EnvironmentNotFounds and expiries
//                   are the resolved list (queue order); the new requests' answers go to the
//                   caller, a queued one as YDC_IDX_WAITING.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "stream_tile.h"

namespace ydc {

constexpr uint32_t kIdxWaiting = 0xFFFFFFFDu;  // YDC_IDX_WAITING
constexpr uint32_t kPadEnv = 0xFFFFFFFFu;      // a digest nobody has: EnvironmentNotFound, consumes nothing
constexpr uint32_t kWaitTile = 1024;           // positions per workgroup of the commit pass (256 threads x 4)

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
  uint32_t snap;    // |W| as k_wait_gather found it (the commit pass reads this one)
  uint32_t ticket;  // workgroups of the commit pass started (without leases)
  uint32_t pad;
};

// Page-locked: what the host reads after the tick (stored by the commit pass's last workgroup).
struct WaitOutcome {
  uint32_t n_waiting;
  uint32_t n_resolved;
  uint32_t reserved[2];
};

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

}  // namespace ydc

// stream_inspect_delta.h — the device side of ydc_stream_delta_inspect / ydc_stream_delta_apply_inspected
// (DESIGN 3.3.19): inspection's detail records (stream_inspect.h) follow a standby through delta snapshots.
//
// A record never changes after the granting thread stored it, and an erased lease's record dies with its
// slot, so a delta's sidecar needs the records of the delta's inserted leases only:
//
//   k_inspect_gather            the primary: thread per inserted id (the delta's list, ascending). lease_find in
//                               the live table, one 16-byte load of the slot's record and its prefetch byte, the
//                               four columns written at the id's position: the output is in id order without a
//                               sort. Misses are counted, one atomicAdd per wave.
//   k_lease_delta_apply_inspect the standby: k_lease_delta_apply_new's twin (stream_delta.h; why a twin: a
//                               stream without inspection launches what it launched). The thread whose
//                               lease_file took a slot then stores, into the same slot, the record and the
//                               prefetch byte, as lease_insert_inspected does: a stale record a reused slot
//                               held is overwritten by that store. No second probe, and no atomicAdd into
//                               ever_assigned: that column is carried whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lease_table.h"
#include "stream_inspect.h"
#include "stream_snapshot.h"

namespace ydc {

// The records of a sidecar on the device, column by column (n entries each).
struct InspectRecords {
  int64_t* started_at;
  uint32_t* env;
  uint32_t* ip;
  uint8_t* prefetch;
};

// ceil(max(n, 1) / 256) workgroups, thread per id. Read-only on the table. *n_missing: cleared by the host.
__global__ __launch_bounds__(256) void k_inspect_gather(LeaseCols L, const LeaseState* st, const uint4* rec,
                                                        const uint8_t* pre, const unsigned long long* id, uint32_t n,
                                                        InspectRecords out, uint32_t* n_missing) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool miss = false;
  if (i < n) {
    uint32_t slot = lease_find(L, st, id[i]);
    if (slot != kNone && !(L.state[slot] & kLeaseLive)) slot = kNone;
    miss = slot == kNone;
    if (!miss) {
      const uint4 r = rec[slot];
      out.started_at[i] = inspect_started(r);
      out.env[i] = r.z;
      out.ip[i] = r.w;
      out.prefetch[i] = pre[slot];
    }
  }
  wave_count(n_missing, miss);
}

// ceil(max(n_ins, 1) / 256) workgroups, thread per insert, behind k_lease_delta_apply_old. The host has
// checked |L| <= max_leases <= cap / 2 (every probe ends) and that no inserted id is in the table.
__global__ __launch_bounds__(256) void k_lease_delta_apply_inspect(LeaseCols L, LeaseState* st, LeasePacked ins,
                                                                   InspectRecords in, uint32_t n_ins,
                                                                   unsigned long long next_id, uint32_t n_leases,
                                                                   uint4* rec, uint8_t* pre) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_ins && i < ins.cap) {
    const uint32_t slot = lease_file(L, st, ins.id[i], ins.expires[i], ins.servant[i], ins.state[i]);
    if (slot != kNone) {
      rec[slot] = inspect_rec(in.started_at[i], in.env[i], in.ip[i]);
      pre[slot] = in.prefetch[i];
    }
  }
  if (i == 0) {
    st->next_id = next_id;
    st->n_leases = n_leases;
  }
}

}  // namespace ydc

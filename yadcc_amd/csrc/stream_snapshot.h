// stream_snapshot.h — the device side of ydc_stream_snapshot / ydc_stream_restore.
//
// Of everything an open stream keeps in HBM only the lease table has a geometry: W, B, E and the
// registry columns are compact arrays, copied [0, n) as they lie. The table is packed on the way
// out and filed again on the way in:
//
//   k_lease_pack   one pass over the slots, shaped like k_lease_sweep; the live slots are appended
//                  to four packed columns, one atomicAdd per wave (k_alive_due's pattern). An
//                  append, not a compaction: slot order means nothing across table sizes, the host
//                  sorts the |L| records by id. |L| records cross the bus, not 2^k slots.
//   k_lease_load   thread per packed record into the freshly reset table of the restoring stream,
//                  by lease_file (lease_table.h) with the state word stored as given (as
//                  k_lease_rehash, fed from packed columns instead of another table's slots).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"

namespace ydc {

// The packed form of L on the device (cap records each).
struct LeasePacked {
  unsigned long long* id;
  int64_t* expires;
  uint32_t* servant;
  uint32_t* state;
  uint32_t cap;
};

// ceil(cap / kLeaseTile) workgroups; thread i owns four consecutive slots. *n_packed: cleared by the
// host; counts every live slot, also those beyond out.cap (which are not written).
__global__ __launch_bounds__(256) void k_lease_pack(LeaseCols L, LeasePacked out, uint32_t* n_packed) {
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  uint32_t st4[4] = {0, 0, 0, 0}, s4[4] = {0, 0, 0, 0};
  unsigned long long k4[4] = {0, 0, 0, 0};
  int64_t e4[4] = {0, 0, 0, 0};
  const uint4 sv = lease_states4(L, i0);
  if ((sv.x | sv.y | sv.z | sv.w) & kLeaseLive) {
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(L.key + i0);
    const ulonglong2 k23 = *reinterpret_cast<const ulonglong2*>(L.key + i0 + 2);
    const uint4 srv = *reinterpret_cast<const uint4*>(L.servant + i0);
    const longlong2 e01 = *reinterpret_cast<const longlong2*>(L.expires + i0);
    const longlong2 e23 = *reinterpret_cast<const longlong2*>(L.expires + i0 + 2);
    st4[0] = sv.x, st4[1] = sv.y, st4[2] = sv.z, st4[3] = sv.w;
    s4[0] = srv.x, s4[1] = srv.y, s4[2] = srv.z, s4[3] = srv.w;
    k4[0] = k01.x, k4[1] = k01.y, k4[2] = k23.x, k4[3] = k23.y;
    e4[0] = e01.x, e4[1] = e01.y, e4[2] = e23.x, e4[3] = e23.y;
  }
  // One atomicAdd per wave: the wave's records in (k, lane) order behind the base it drew.
  unsigned long long m4[4];
  uint32_t total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m4[k] = __ballot((st4[k] & kLeaseLive) != 0);
    total += (uint32_t)__popcll(m4[k]);
  }
  if (!total) return;  // (wave-uniform)
  const uint32_t lane = lane_id();
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(n_packed, total);
  base = (uint32_t)__shfl((int)base, 0, 64);
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (st4[k] & kLeaseLive) {
      const uint32_t at = base + (uint32_t)__popcll(m4[k] & below);
      if (at < out.cap) {
        out.id[at] = k4[k];
        out.expires[at] = e4[k];
        out.servant[at] = s4[k];
        out.state[at] = st4[k];
      }
    }
    base += (uint32_t)__popcll(m4[k]);
  }
}

// ceil(max(count, 1) / 256) workgroups, thread per record of `in` (count <= in.cap records, distinct
// ids) into the empty table n, whose bookkeeping starts cleared: n_leases counts what was filed (the
// host compares it with count), max_disp is that of this table, next_id is stored as given.
__global__ __launch_bounds__(256) void k_lease_load(LeaseCols n, LeaseState* nst, LeasePacked in, uint32_t count,
                                                    unsigned long long next_id) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t filed = 0;
  if (i < count && i < in.cap)
    filed = lease_file(n, nst, in.id[i], in.expires[i], in.servant[i], in.state[i]) != kNone ? 1u : 0u;
  if (i == 0) nst->next_id = next_id;
  // One atomic per workgroup.
  __shared__ uint32_t s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const uint32_t wf = wave_sum_u32(filed);
  if ((threadIdx.x & 63) == 0 && wf) atomicAdd(&s_cnt, wf);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(&nst->n_leases, s_cnt);
}

}  // namespace ydc

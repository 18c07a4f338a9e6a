// stream_inspect.h — what DumpInternals prints beyond the lease table and the registry's columns,
// kept on the device by a leased, waiting-and-leased or rpc stream (ydc_stream_inspect_begin /
// _load / _servants / _tasks).
//
// The reference's dump (task_dispatcher.cc:538-614) shows per task requestor_ip, compiler_digest,
// started_at and prefetched_task (:133, :594-598), per servant discovered_at, ever_assigned_tasks
// (:124, :208) and capacity_available (GetCapacityAvailable, :283-313), and five totals (:604-612).
// With inspection on:
//
//   detail records     columns parallel to the lease table's SLOTS: one 16-byte record (started_at |
//                      env_id | requestor_ip) and one byte (prefetch) per slot. The thread that
//                      inserts a lease stores them into the slot it took; an erased lease leaves a
//                      stale record behind that the slot's next insert overwrites, so free, sweep,
//                      orphan and k_lease_remap need nothing.
//   servant columns    discovered_at (int64) and ever_assigned (u64) per servant, sized by the
//                      registry like E (servant_alive.h); the inserting thread adds 1 to its servant.
//
// The write rides in the three granting passes: commit_pass<…, kInspect> of wait_lease.h behind a
// compile-time flag (k_lease_grant_inspect, k_wait_lease_commit_inspect), and k_rpc_grant_inspect of
// rpc_stream.h, k_rpc_grant's twin (why a twin: there). A stream without inspection launches the
// kernels it launched before.
//
//   k_inspect_fill      ydc_stream_inspect_begin: every slot's record = the sentinels (a lease
//                       granted while inspection was off has no details).
//   k_inspect_rehash    k_lease_rehash that moves a slot's record with its lease (ydc_stream_reserve,
//                       ydc_stream_book_begin with inspection on).
//   k_inspect_find      ydc_stream_inspect_load, first half: the slot of every given id, the misses
//   k_inspect_file      counted; second half, only when none missed: the records stored.
//   k_inspect_pack      k_lease_pack with the record beside the lease (ydc_stream_inspect_tasks).
//   k_inspect_servants  capacity_available per servant in closed form and the totals' three sums.
//   k_inspect_compact   the two servant columns through the registry's compaction (k_alive_compact).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch_core.h"
#include "kernels.h"
#include "lease_table.h"

namespace ydc {

constexpr uint32_t kInspectNoId = 0xFFFFFFFFu;
constexpr int64_t kInspectNoTime = INT64_MIN;

// What a granting pass needs to file a grant's details. env / ip: the batch's columns, indexed as
// the pass indexes its positions. n_imm / row_start / P: rpc mode only (the row's rank in its RPC).
struct InspectIn {
  uint4* rec;                 // per slot: started_at (lo, hi) | env_id | requestor_ip
  uint8_t* prefetch;          // per slot
  unsigned long long* ever;   // per servant
  uint32_t n_ever;            // rows of `ever`
  const uint32_t *env, *ip;
  const uint32_t* n_imm;      // per position
  uint32_t P;
};

__device__ __forceinline__ uint4 inspect_rec(int64_t started_at, uint32_t env, uint32_t ip) {
  return make_uint4((uint32_t)(unsigned long long)started_at, (uint32_t)((unsigned long long)started_at >> 32), env, ip);
}

__device__ __forceinline__ int64_t inspect_started(const uint4& r) {
  return (int64_t)((unsigned long long)r.x | ((unsigned long long)r.y << 32));
}

// The insert of a granting pass with inspection on: the lease (lease_file of lease_table.h), its record
// into the slot it took, its servant's count.
__device__ __forceinline__ void lease_insert_inspected(const LeaseCols& L, LeaseState* st, const InspectIn& ins,
                                                       unsigned long long id, int64_t expires, uint32_t servant,
                                                       int64_t now, uint32_t j, bool prefetch) {
  const uint32_t slot = lease_file(L, st, id, expires, servant, kLeaseLive);
  if (slot != kNone) {
    ins.rec[slot] = inspect_rec(now, ins.env[j], ins.ip[j]);
    ins.prefetch[slot] = prefetch ? 1 : 0;
  }
  if (servant < ins.n_ever) atomicAdd(&ins.ever[servant], 1ull);
}

// Thread per slot.
__global__ __launch_bounds__(256) void k_inspect_fill(uint4* rec, uint8_t* prefetch, uint32_t slots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slots) return;
  rec[i] = inspect_rec(kInspectNoTime, kInspectNoId, kInspectNoId);
  prefetch[i] = 0;
}

// k_lease_rehash (lease_table.h) with the record, which goes into the slot lease_file took: thread per
// slot of `o`. Off the hot path, so one slot per thread and scalar loads.
__global__ __launch_bounds__(256) void k_inspect_rehash(LeaseCols o, const LeaseState* ost, const uint4* orec,
                                                        const uint8_t* opre, LeaseCols n, LeaseState* nst, uint4* nrec,
                                                        uint8_t* npre) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool moved = false;
  if (i <= o.mask) {
    const unsigned long long id = o.key[i];
    if (id != kLeaseEmpty) {
      const uint32_t slot = lease_file(n, nst, id, o.expires[i], o.servant[i], o.state[i]);
      moved = slot != kNone;
      if (moved) {
        nrec[slot] = orec[i];
        npre[slot] = opre[i];
      }
    }
  }
  if (i == 0) nst->next_id = ost->next_id;
  wave_count(&nst->n_leases, moved);
}

// Thread per given id: its slot (kNone: no such lease, counted in *n_missing).
__global__ __launch_bounds__(256) void k_inspect_find(LeaseCols L, const LeaseState* st, const unsigned long long* id,
                                                      uint32_t n, uint32_t* slot_of, uint32_t* n_missing) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool miss = false;
  if (i < n) {
    uint32_t slot = lease_find(L, st, id[i]);
    if (slot != kNone && !(L.state[slot] & kLeaseLive)) slot = kNone;
    slot_of[i] = slot;
    miss = slot == kNone;
  }
  wave_count(n_missing, miss);
}

// Thread per given record into the slot k_inspect_find found for it.
__global__ __launch_bounds__(256) void k_inspect_file(const uint32_t* slot_of, uint32_t n, uint32_t slots,
                                                      const int64_t* started_at, const uint32_t* env,
                                                      const uint32_t* ip, const uint8_t* prefetch, uint4* rec,
                                                      uint8_t* pre) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = slot_of[i];
  if (slot >= slots) return;
  rec[slot] = inspect_rec(started_at ? started_at[i] : kInspectNoTime, env ? env[i] : kInspectNoId,
                          ip ? ip[i] : kInspectNoId);
  pre[slot] = prefetch && prefetch[i] ? 1 : 0;
}

// The packed form of L with its details (cap records each).
struct InspectPacked {
  unsigned long long* id;
  int64_t* expires;
  uint4* rec;
  uint32_t* servant;
  uint32_t* state;
  uint8_t* prefetch;
  uint32_t cap;
};

// k_lease_pack's shape (stream_snapshot.h): ceil(cap / kLeaseTile) workgroups, thread i owns four
// consecutive slots, one atomicAdd per wave for the base. *n_packed: cleared by the host; counts
// every live slot, also those beyond out.cap (which are not written).
__global__ __launch_bounds__(256) void k_inspect_pack(LeaseCols L, const uint4* rec, const uint8_t* pre,
                                                      InspectPacked out, uint32_t* n_packed) {
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint4 sv = lease_states4(L, i0);
  const uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
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
      const uint32_t at = base + (uint32_t)__popcll(m4[k] & below), slot = i0 + k;
      if (at < out.cap) {
        out.id[at] = L.key[slot];
        out.expires[at] = L.expires[slot];
        out.rec[at] = rec[slot];
        out.servant[at] = L.servant[slot];
        out.state[at] = st4[k];
        out.prefetch[at] = pre[slot];
      }
    }
    base += (uint32_t)__popcll(m4[k]);
  }
}

// Sum over the 64 lanes (every lane gets it), modulo 2^64.
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
  return v;
}

// The three sums DumpInternals accumulates (:583-586), modulo 2^64; cleared by the host.
struct InspectSums {
  unsigned long long running, capacity, unavailable;
};

// GetCapacityAvailable (:283-313) from the registry's columns. NOT servant_slot_count of
// dispatch_core.h, which counts the slots that are still free.
__device__ __forceinline__ uint32_t capacity_available(uint32_t nproc, uint32_t load, uint32_t max_tasks,
                                                       uint32_t running, uint32_t flags) {
  if (flags & kFlagLowMemory) return running;
  const long long foreign = max((long long)load - (long long)running, 0ll);
  const long long avail = max((long long)nproc - foreign, 0ll);
  return (uint32_t)min((long long)max_tasks, avail);
}

// Thread per servant, coalesced column loads; a wave reduction of the sums and one atomic per
// workgroup and sum. The sums are integer: their value does not depend on the order.
__global__ __launch_bounds__(256) void k_inspect_servants(const uint32_t* nproc, const uint32_t* load,
                                                          const uint32_t* max_tasks, const uint32_t* running,
                                                          const uint32_t* flags, uint32_t n, uint32_t* out_avail,
                                                          InspectSums* sums) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long run = 0, cap = 0, unav = 0;
  if (s < n) {
    const uint32_t mt = max_tasks[s], r = running[s];
    const uint32_t av = capacity_available(nproc[s], load[s], mt, r, flags[s]);
    out_avail[s] = av;
    run = r;
    cap = mt;
    unav = (unsigned long long)mt - (unsigned long long)av;  // (wraps where a low-memory servant runs more than max_tasks, as :585-586 does)
  }
  __shared__ unsigned long long s_sum[3];
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  __syncthreads();
  run = wave_sum_u64(run);
  cap = wave_sum_u64(cap);
  unav = wave_sum_u64(unav);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s_sum[0], run);
    atomicAdd(&s_sum[1], cap);
    atomicAdd(&s_sum[2], unav);
  }
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&sums->running, s_sum[0]);
  if (threadIdx.x == 1) atomicAdd(&sums->capacity, s_sum[1]);
  if (threadIdx.x == 2) atomicAdd(&sums->unavailable, s_sum[2]);
}

// The two servant columns through the registry's compaction (k_alive_compact's rule). removed[]:
// ascending. Thread per old row.
__global__ __launch_bounds__(256) void k_inspect_compact(const int64_t* disc_in, const unsigned long long* ever_in,
                                                         int64_t* disc_out, unsigned long long* ever_out,
                                                         const uint32_t* removed, uint32_t n_removed, uint32_t n) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t before = lower_bound_u32(removed, n_removed, s);
  if (before < n_removed && removed[before] == s) return;
  disc_out[s - before] = disc_in[s];
  ever_out[s - before] = ever_in[s];
}

}  // namespace ydc

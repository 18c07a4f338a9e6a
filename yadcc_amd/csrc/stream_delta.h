// stream_delta.h — the device side of ydc_stream_delta_base / ydc_stream_delta / ydc_stream_delta_apply
// (DESIGN 3.3.18).
//
// The primary keeps a base image of L: the packed columns k_lease_pack leaves (arbitrary order) and
// next_id. A delta is found in two passes over memory the device already owns:
//
//   k_lease_delta_scan   one pass over the slots, shaped like k_lease_pack: every live slot is appended
//                        to the NEW image, and those whose id the base had not handed out yet
//                        (id >= base next_id) to the insert list as well.
//   k_lease_delta_diff   thread per record of the OLD image: lease_find in the live table. Absent: the
//                        id goes to the erase list. Present with another expiry or state word: to the
//                        update list. Present on another servant: the error flag (never expected).
//   k_book_delta_same    B's columns against the base's copy, reduced to one flag.
//
// The standby checks a delta against its table before it writes anything, then applies it:
//
//   k_lease_delta_check  read-only: how many of the erased and updated ids, and how many of the
//                        inserted ones, the table holds. The host compares with the lists' lengths.
//   k_lease_delta_apply_old   thread per erase (k_lease_free's CAS on the key, state 0; running_tasks is
//                        carried as a column, not counted) and per update (expiry and state stored).
//   k_lease_delta_apply_new   thread per insert, by lease_file (lease_table.h) with the state word stored
//                        as given (as k_lease_load); thread 0 stores next_id and |L|.
// Appends are one ballot and one atomicAdd per wave and list (k_alive_due's pattern).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"
#include "running_book.h"
#include "stream_snapshot.h"

namespace ydc {

// The counters of one delta or one check, cleared by the host before the launches.
struct DeltaCounts {
  uint32_t n_img, n_ins, n_era, n_upd;  // records appended (also those beyond a list's cap, which are not written)
  uint32_t servant_changed;             // k_lease_delta_diff: a lease sits on another servant than in the base
  uint32_t book_differs;                // k_book_delta_same
  uint32_t found_old, found_new;        // k_lease_delta_check
};

// The update list (cap records each).
struct LeaseUpdates {
  unsigned long long* id;
  int64_t* expires;
  uint32_t* state;
  uint32_t cap;
};

// The wave's flagged lanes draw consecutive places behind *counter: the place of this lane (valid where flag).
__device__ __forceinline__ uint32_t wave_append(uint32_t* counter, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (!m) return 0;  // (wave-uniform)
  const uint32_t lane = lane_id();
  uint32_t base = 0;
  if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, __builtin_ctzll(m), 64);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// ceil(cap / kLeaseTile) workgroups; thread i owns four consecutive slots.
__global__ __launch_bounds__(256) void k_lease_delta_scan(LeaseCols L, LeasePacked img, LeasePacked ins,
                                                          unsigned long long base_next_id, DeltaCounts* cnt) {
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
  // One atomicAdd per wave and list: the wave's records in (k, lane) order behind the base it drew.
  unsigned long long m4[4], n4[4];
  uint32_t total = 0, total_new = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool live = (st4[k] & kLeaseLive) != 0;
    m4[k] = __ballot(live);
    n4[k] = __ballot(live && k4[k] >= base_next_id);
    total += (uint32_t)__popcll(m4[k]);
    total_new += (uint32_t)__popcll(n4[k]);
  }
  if (!total) return;  // (wave-uniform)
  const uint32_t lane = lane_id();
  uint32_t base = 0, base_new = 0;
  if (lane == 0) {
    base = atomicAdd(&cnt->n_img, total);
    if (total_new) base_new = atomicAdd(&cnt->n_ins, total_new);
  }
  base = (uint32_t)__shfl((int)base, 0, 64);
  base_new = (uint32_t)__shfl((int)base_new, 0, 64);
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (st4[k] & kLeaseLive) {
      const uint32_t at = base + (uint32_t)__popcll(m4[k] & below);
      if (at < img.cap) {
        img.id[at] = k4[k];
        img.expires[at] = e4[k];
        img.servant[at] = s4[k];
        img.state[at] = st4[k];
      }
      if (k4[k] >= base_next_id) {
        const uint32_t to = base_new + (uint32_t)__popcll(n4[k] & below);
        if (to < ins.cap) {
          ins.id[to] = k4[k];
          ins.expires[to] = e4[k];
          ins.servant[to] = s4[k];
          ins.state[to] = st4[k];
        }
      }
    }
    base += (uint32_t)__popcll(m4[k]);
    base_new += (uint32_t)__popcll(n4[k]);
  }
}

// ceil(max(n_old, 1) / 256) workgroups, thread per record of the old image.
__global__ __launch_bounds__(256) void k_lease_delta_diff(LeaseCols L, const LeaseState* st, LeasePacked old,
                                                          uint32_t n_old, unsigned long long* era_id, uint32_t era_cap,
                                                          LeaseUpdates upd, DeltaCounts* cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool gone = false, changed = false, moved = false;
  unsigned long long id = 0;
  int64_t exp = 0;
  uint32_t state = 0;
  if (i < n_old && i < old.cap) {
    id = old.id[i];
    const uint32_t slot = lease_find(L, st, id);
    if (slot == kNone) {
      gone = true;
    } else {
      exp = L.expires[slot];
      state = L.state[slot];
      changed = exp != old.expires[i] || state != old.state[i];
      moved = L.servant[slot] != old.servant[i];
    }
  }
  const uint32_t e = wave_append(&cnt->n_era, gone);
  if (gone && e < era_cap) era_id[e] = id;
  const uint32_t u = wave_append(&cnt->n_upd, changed);
  if (changed && u < upd.cap) {
    upd.id[u] = id;
    upd.expires[u] = exp;
    upd.state[u] = state;
  }
  wave_count(&cnt->servant_changed, moved);
}

// ceil(max(n, 1) / 256) workgroups, thread per entry of B (n entries in both).
__global__ __launch_bounds__(256) void k_book_delta_same(BookCols cur, BookCols base, uint32_t n, DeltaCounts* cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool differs = false;
  if (i < n)
    differs = cur.grant[i] != base.grant[i] || cur.stid[i] != base.stid[i] || cur.dkey[i] != base.dkey[i] ||
              cur.servant[i] != base.servant[i];
  wave_count(&cnt->book_differs, differs);
}

// ceil(max(n_era + n_upd + n_ins, 1) / 256) workgroups, thread per id of the three lists. Read-only.
__global__ __launch_bounds__(256) void k_lease_delta_check(LeaseCols L, const LeaseState* st,
                                                           const unsigned long long* era_id, uint32_t n_era,
                                                           const unsigned long long* upd_id, uint32_t n_upd,
                                                           const unsigned long long* ins_id, uint32_t n_ins,
                                                           DeltaCounts* cnt) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  bool old_found = false, new_found = false;
  if (t < n_era) old_found = lease_find(L, st, era_id[t]) != kNone;
  else if (t - n_era < n_upd) old_found = lease_find(L, st, upd_id[t - n_era]) != kNone;
  else if (t - n_era - n_upd < n_ins) new_found = lease_find(L, st, ins_id[t - n_era - n_upd]) != kNone;
  wave_count(&cnt->found_old, old_found);
  wave_count(&cnt->found_new, new_found);
}

// ceil(max(n_era + n_upd, 1) / 256) workgroups, thread per erase and per update (the check has found every id).
__global__ __launch_bounds__(256) void k_lease_delta_apply_old(LeaseCols L, const LeaseState* st,
                                                               const unsigned long long* era_id, uint32_t n_era,
                                                               LeaseUpdates upd, uint32_t n_upd) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_era) {
    const unsigned long long id = era_id[t];
    const uint32_t slot = lease_find(L, st, id);
    if (slot != kNone && atomicCAS(&L.key[slot], id, kLeaseEmpty) == id) L.state[slot] = 0;
  } else if (t - n_era < n_upd) {
    const uint32_t j = t - n_era;
    const uint32_t slot = lease_find(L, st, upd.id[j]);
    if (slot != kNone) {
      L.expires[slot] = upd.expires[j];
      L.state[slot] = upd.state[j];
    }
  }
}

// ceil(max(n_ins, 1) / 256) workgroups, thread per insert, behind k_lease_delta_apply_old (a slot it
// erased may be taken again). The host has checked |L| <= max_leases <= cap / 2: every probe ends.
__global__ __launch_bounds__(256) void k_lease_delta_apply_new(LeaseCols L, LeaseState* st, LeasePacked ins,
                                                               uint32_t n_ins, unsigned long long next_id,
                                                               uint32_t n_leases) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_ins && i < ins.cap) lease_file(L, st, ins.id[i], ins.expires[i], ins.servant[i], ins.state[i]);
  if (i == 0) {
    st->next_id = next_id;
    st->n_leases = n_leases;
  }
}

}  // namespace ydc

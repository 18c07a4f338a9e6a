// stream_usage.h — slot-time and wait-time used per requestor of an open stream, kept on the device
// across ticks (ydc_stream_usage_begin / _get / _find / _load).
//
// requestor_index.h answers who holds the cluster NOW and is built again by each call, because a count
// kept inside the tick would need a decrement in every erase path. Usage is an integral, not a count:
// at the head of a tick, before anything of the tick changes them, every lease of L and every entry of
// W is charged for the quanta since the previous accepted tick,
//   dq = floor(now / quantum) - floor(last / quantum)          (usage_quanta.h; the host's, one word)
// so one read-only pass over L and W per tick is all there is, and no kernel of the tick is edited. A
// stream that never begins the capability launches what it launched before.
//
// The table is persistent: open addressing, keyed by requestor, in device memory,
//   word u64 | slot_time | zombie_time | prefetch_time | wait_time | wait_row_time   (u64 each, SoA)
// with requestor_index.h's slot word ((1 << 32) | requestor_ip, 0 for a free slot: all 2^32 ids are
// ordinary keys) and index_home.h's home slot, then linear probing. At least kIndexMinSlots slots, a
// power of two, at most half full: the host keeps a bound that errs high on the keys the next accrual
// can meet and files the table again into a larger one between ticks (k_usage_rehash), so a claim
// always finds room. Should one not, it is counted in `dropped` and the tick ends in an error: an
// addition is never lost silently. Beside the table, UsageState: `unattributed_time` (leases granted
// while inspection was off: never key 0xFFFFFFFF), `quanta` (the sum of dq), `ticks`, `n_keys`.
//
//   k_usage_accrue  the first launch of a tick's lease part. ceil(slots of L / kLeaseTile) workgroups
//                   read L as k_requestor_leases does (four slots per thread, one 16-byte load of
//                   their states; a slot counts while its state word is live, so erased slots whose
//                   records stay behind add nothing), `w_blocks` more cover W with a stride loop over
//                   min(ws->count, max_waiting) entries (an entry whose deadline has passed is charged
//                   while it is in W). dq == 0: every thread leaves before it touches the table.
//                   The workgroup that finishes last adds dq to `quanta`, 1 to `ticks` and stores the
//                   totals to the page-locked result block.
//   k_usage_find    thread per query; a miss is a row of zeros.
//   k_usage_fold    one ticket-ordered tile pass over the slots (slot_fold of slot_probe.h), as k_requestor_fold:
//                   THE ORDER OF THE ROWS IS UNSPECIFIED (the Python wrapper sorts them).
//   k_usage_load    thread per given row: its key claimed, its five sums added. Duplicates add together.
//   k_usage_rehash  thread per slot of the old table: the occupied ones filed into the new one.
//
// Hot key: one requestor that owns most of L is the normal case, and a plain pass would put 3 |L|
// 64-bit atomics on three addresses. Equal keys are combined inside the wave first (wave_combine of
// stream_tile.h: after kRequestorRounds distinct keys the lanes that are left add for themselves).
// The lead lane multiplies the combined COUNTS by dq once, so a wave issues at most three 64-bit atomics per key for leases and two for W. Over L a thread
// merges its four slots by requestor before the wave combines, and the four waves' first keys meet in
// LDS, so the hot key takes one set of atomics per workgroup (stream_depart.h's form). All sums are
// uint64 modulo 2^64 and all additions integer atomics in device memory: the result does not depend
// on their order. `combine` == false (YDC_TUNE requestor_combine=0, the switch requestor_index.h has):
// every lane adds for itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_home.h"
#include "kernels.h"
#include "lease_table.h"
#include "requestor_index.h"
#include "stream_inspect.h"
#include "stream_tile.h"
#include "wait_queue.h"

namespace ydc {

constexpr uint32_t kUsageCols = 5;  // slot_time | zombie_time | prefetch_time | wait_time | wait_row_time
constexpr uint32_t kUsageWaitBlocks = 64;  // workgroups of the accrual's stride part at the most
// (kIndexMinSlots and usage_slots: index_home.h)

struct UsageState {
  unsigned long long unattributed, quanta, ticks;
  uint32_t n_keys;       // occupied slots
  uint32_t dropped;      // additions that found no slot (never: the host grows the table first)
  uint32_t blocks_done;  // the accrual's workgroups that have finished (0 between ticks)
  uint32_t pad;
};

// Page-locked: what the host reads after the tick.
struct UsageDone {
  unsigned long long unattributed, quanta, ticks;
  uint32_t n_keys, dropped, tick_no, pad;
};

struct UsageTable {
  unsigned long long* word;  // [mask + 1]: 0, or kRequestorOccupied | requestor_ip
  unsigned long long* sum;   // [kUsageCols][mask + 1]
  UsageState* st;
  uint32_t mask;  // slots - 1
};

// ydc_usage_row.
struct UsageRow {
  uint32_t ip, pad;
  unsigned long long v[kUsageCols];
};
static_assert(sizeof(UsageRow) == 48, "ydc_usage_row is 48 bytes");

// The slot of `ip` (requestor_index.h's claim), claimed if nobody had it: the claim that publishes a new
// key bumps n_keys. kNone: the table is full, and the addition is counted in `dropped`.
__device__ __forceinline__ uint32_t usage_claim(const UsageTable& tb, uint32_t ip) {
  bool published;
  const uint32_t h = requestor_claim(tb.word, tb.mask, ip, &published);
  if (published) atomicAdd(&tb.st->n_keys, 1u);
  if (h == kNone) atomicAdd(&tb.st->dropped, 1u);
  return h;
}

// Columns col, col + 1, col + 2 of `ip`'s slot gain n | a | b (already multiplied by dq).
__device__ __forceinline__ void usage_add_one(const UsageTable& tb, uint32_t ip, uint32_t col, unsigned long long n,
                                              unsigned long long a, unsigned long long b) {
  const uint32_t h = usage_claim(tb, ip);
  if (h == kNone) return;
  const size_t slots = (size_t)tb.mask + 1;
  unsigned long long* const dst = tb.sum + (size_t)col * slots + h;
  atomicAdd(dst, n);
  if (a) atomicAdd(dst + slots, a);
  if (b) atomicAdd(dst + 2 * slots, b);
}

// Sum over the wave of one 32-bit value per lane, in 64 bits (the halves' sums fit 32 bits each).
__device__ __forceinline__ unsigned long long wave_sum_wide(uint32_t v) {
  if (!__ballot(v != 0)) return 0;  // (wave-uniform)
  return (unsigned long long)wave_sum_u32(v & 0xFFFFu) + ((unsigned long long)wave_sum_u32(v >> 16) << 16);
}

// A wave's first combined key of the pass over L, handed to the workgroup through LDS (n == 0: none).
struct UsageLead {
  uint32_t ip, n, a, b;
};

// Per active lane n | a | b entries of key `ip`: n dq | a dq | b dq into columns col, col + 1, col + 2.
// With `combine` every lane of the wave must get here (wave_combine).
// defer != NULL: the first round's key is not added here but left in *defer for the workgroup to add.
__device__ __forceinline__ void usage_add(const UsageTable& tb, bool combine, bool active, uint32_t ip, uint32_t col,
                                          uint32_t n, uint32_t a, uint32_t b, unsigned long long dq, UsageLead* defer) {
  if (combine)
    active = wave_combine(active, ip, [&](uint32_t ip0, bool mine, unsigned long long, bool leads, uint32_t round) {
      const unsigned long long sn = wave_sum_wide(mine ? n : 0u), sa = wave_sum_wide(mine ? a : 0u),
                               sb = wave_sum_wide(mine ? b : 0u);
      if (leads) {
        if (defer && round == 0) *defer = UsageLead{ip0, (uint32_t)sn, (uint32_t)sa, (uint32_t)sb};  // (at most 256 each)
        else usage_add_one(tb, ip0, col, sn * dq, sa * dq, sb * dq);
      }
    });
  if (active) usage_add_one(tb, ip, col, n * dq, a * dq, b * dq);
}

// l_blocks = ceil(slots of L / kLeaseTile) workgroups over L, thread i owning four consecutive slots;
// the workgroups behind them cover W (w_ip == NULL: the stream has none, and there are no such
// workgroups). n_imm == NULL (no rpc stream): an entry is one row. dq_word: page-locked, the host's.
// The hot requestor (requestor_index.h) would take an atomic per slot and column on three addresses;
// as in k_depart_leases a thread merges its four slots by requestor first, the wave combines, and the
// four waves' first keys meet in LDS, so the hot key costs one set of atomics per workgroup.
__global__ __launch_bounds__(256) void k_usage_accrue(LeaseCols L, const uint4* rec, const uint8_t* pre, uint32_t l_blocks,
                                                      const uint32_t* w_ip, const uint32_t* n_imm, const uint32_t* n_pre,
                                                      const WaitState* ws, uint32_t max_waiting, UsageTable tb,
                                                      const unsigned long long* dq_word, const LeaseHdr* lh,
                                                      UsageDone* done, uint32_t combine) {
  const unsigned long long dq = *dq_word;
  UsageState* const st = tb.st;
  if (dq == 0) {  // (nothing to add: the table is not touched; the tick still counts)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st->ticks += 1;
      *done = UsageDone{st->unattributed, st->quanta, st->ticks, st->n_keys, st->dropped, lh->tick_no, 0};
    }
    return;
  }
  __shared__ UsageLead s_lead[4];  // (256 threads: four waves)
  if (blockIdx.x < l_blocks) {
    const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const uint4 sv = lease_states4(L, i0);
    const uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
    // The thread's four slots merged by requestor: ng groups of gn leases, gz zombies, gp prefetched.
    uint32_t gip[4] = {0, 0, 0, 0}, gn[4] = {0, 0, 0, 0}, gz[4] = {0, 0, 0, 0}, gp[4] = {0, 0, 0, 0};
    uint32_t ng = 0, nobody = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(st4[k] & kLeaseLive)) continue;
      const uint4 r = rec[i0 + k];
      if (inspect_started(r) == kInspectNoTime) {
        ++nobody;
        continue;
      }
      const uint32_t ip = r.w, zombie = (st4[k] & kLeaseZombie) ? 1u : 0u, prefetch = pre[i0 + k] ? 1u : 0u;
      bool found = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool hit = !found && ((uint32_t)j < ng ? gip[j] == ip : (uint32_t)j == ng);
        if (hit) {
          gip[j] = ip;
          gn[j] += 1, gz[j] += zombie, gp[j] += prefetch;
          found = true;
        }
      }
      // (a hit at j == ng opened a group)
      uint32_t open = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) open += gn[j] ? 1u : 0u;
      ng = open;
    }
    const uint32_t wn = wave_sum_if_any(nobody);
    if (wn && lane_id() == 0) atomicAdd(&st->unattributed, (unsigned long long)wn * dq);
    const uint32_t wave = threadIdx.x >> 6;
    if (lane_id() == 0) s_lead[wave] = UsageLead{0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 4; ++g)
      usage_add(tb, combine != 0, (uint32_t)g < ng, gip[g], 0, gn[g], gz[g], gp[g], dq, g == 0 ? &s_lead[wave] : nullptr);
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < 4; ++w) {
        UsageLead m = s_lead[w];
        if (!m.n) continue;
        for (int v = w + 1; v < 4; ++v)
          if (s_lead[v].n && s_lead[v].ip == m.ip) {
            m.n += s_lead[v].n, m.a += s_lead[v].a, m.b += s_lead[v].b;
            s_lead[v].n = 0;
          }
        usage_add_one(tb, m.ip, 0, m.n * dq, m.a * dq, m.b * dq);
      }
    }
  } else {
    const uint32_t n = min(ws->count, max_waiting);
    const uint32_t w_blocks = gridDim.x - l_blocks;
    for (uint32_t base = (blockIdx.x - l_blocks) * blockDim.x; base < n; base += w_blocks * blockDim.x) {
      const uint32_t i = base + threadIdx.x;
      const bool mine = i < n;
      const uint32_t ip = mine ? w_ip[i] : 0u;
      const uint32_t rows = !mine ? 0u : n_imm ? n_imm[i] + n_pre[i] : 1u;
      usage_add(tb, combine != 0, mine, ip, 3, 1u, rows, 0u, dq, nullptr);
    }
  }
  // The workgroup that finishes last has everybody's additions behind it: every wave drains its own
  // atomics, the workgroup meets, one lane releases and takes the ticket; the last one acquires.
  __shared__ uint32_t s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(&st->blocks_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (s_last && threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st->blocks_done = 0;
    st->quanta += dq;
    st->ticks += 1;
    const unsigned long long un = __hip_atomic_load(&st->unattributed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t nk = __hip_atomic_load(&st->n_keys, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t dr = __hip_atomic_load(&st->dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *done = UsageDone{un, st->quanta, st->ticks, nk, dr, lh->tick_no, 0};
  }
}

__device__ __forceinline__ UsageRow usage_row_at(const UsageTable& tb, uint32_t ip, uint32_t h) {
  const size_t slots = (size_t)tb.mask + 1;
  UsageRow r{ip, 0u, {0, 0, 0, 0, 0}};
  if (h != kNone)
    for (uint32_t k = 0; k < kUsageCols; ++k) r.v[k] = tb.sum[k * slots + h];
  return r;
}

// ceil(n / 256) workgroups.
__global__ __launch_bounds__(256) void k_usage_find(const uint32_t* q, uint32_t n, UsageTable tb, UsageRow* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t ip = q[i];
  out[i] = usage_row_at(tb, ip, requestor_lookup(tb.word, tb.mask, ip));
}

// The fold's bookkeeping and tile: slot_probe.h's.
using UsageFoldState = SlotFoldState;
constexpr uint32_t kUsageTile = kSlotFoldTile;

// slot_fold's grid: ceil(slots / kUsageTile) workgroups of 256 threads. out: out_cap rows of room.
__global__ __launch_bounds__(256) void k_usage_fold(UsageTable tb, UsageFoldState* fs, unsigned long long* lookback,
                                                    UsageRow* out, uint32_t out_cap) {
  slot_fold(tb.word, tb.mask, fs, lookback, out_cap, [&](uint32_t dst, unsigned long long w, uint32_t h) {
    out[dst] = usage_row_at(tb, (uint32_t)w, h);
  });
}

// ceil(max(n, 1) / 256) workgroups. add: what the three totals gain (thread 0's).
__global__ __launch_bounds__(256) void k_usage_load(const UsageRow* rows, uint32_t n, UsageTable tb,
                                                    unsigned long long add_unattributed, unsigned long long add_quanta,
                                                    unsigned long long add_ticks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    atomicAdd(&tb.st->unattributed, add_unattributed);
    atomicAdd(&tb.st->quanta, add_quanta);
    atomicAdd(&tb.st->ticks, add_ticks);
  }
  if (i >= n) return;
  const UsageRow r = rows[i];
  const uint32_t h = usage_claim(tb, r.ip);
  if (h == kNone) return;
  const size_t slots = (size_t)tb.mask + 1;
  for (uint32_t k = 0; k < kUsageCols; ++k)
    if (r.v[k]) atomicAdd(&tb.sum[k * slots + h], r.v[k]);
}

// ceil(old slots / 256) workgroups: the growth. The new table: cleared by the host, its n_keys 0 (both
// tables share the UsageState; the claims count the keys again).
__global__ __launch_bounds__(256) void k_usage_rehash(UsageTable o, UsageTable n) {
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h > o.mask) return;
  const unsigned long long w = o.word[h];
  if (!w) return;
  const uint32_t to = usage_claim(n, (uint32_t)w);
  if (to == kNone) return;
  const size_t os = (size_t)o.mask + 1, ns = (size_t)n.mask + 1;
  for (uint32_t k = 0; k < kUsageCols; ++k) n.sum[k * ns + to] = o.sum[k * os + h];  // (a key has one old slot)
}

}  // namespace ydc

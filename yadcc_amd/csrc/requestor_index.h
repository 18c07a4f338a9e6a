// requestor_index.h — the load per requestor of an open stream, summed on the device from what the
// stream already keeps in HBM (ydc_stream_requestor_find / ydc_stream_requestor_get).
// Read-only for the stream: nothing here is state, no tick kernel knows about it, a stream that never
// asks launches what it launched before.
//
// With inspection on every slot of the lease table L carries its requestor_ip (stream_inspect.h: the
// 16-byte record beside the lease), and every entry of W carries its ip (wait_queue.h), in rpc mode
// its two row counts too. The index folds both by requestor: an open-addressing table of
//   slots = max(1024, the smallest power of two >= 2 (|L| + |W|))
// (load <= 1/2; sized by the entries when it is built, not by max_leases), per slot
//   word u64 | leases | zombies | prefetch_leases | waiting | waiting_rows   (u32 each, SoA)
// and ONE further counter, `unattributed`: leases granted while inspection was off.
//
// The slot word is (1 << 32) | requestor_ip; 0 marks a free slot. All 2^32 ids are ordinary keys —
// 0xFFFFFFFF is also YDC_INSPECT_NO_ID — and none of them makes the word 0, so no key needs a side
// record and the host clears the whole table with one memset. The home slot is book_index_mix of the
// id (addresses of one subnet are sequential), then linear probing.
//
// It is DERIVED state, built by each call: L and W change in every tick, and the tick's erase paths
// (free, sweep, orphan, k_lease_remap) leave the erased leases' records behind, so an index kept
// inside the tick would need a decrement in each of them. The build reads the table as it stands: a
// slot counts only while it holds a lease (its state word is live, which between ticks is the same as
// its key not being kLeaseEmpty: every erase path clears both).
//
//   k_requestor_leases   four slots of L per thread, as k_outlook_leases reads them. A lease whose
//                        record has started_at == kInspectNoTime goes to `unattributed`, not to key
//                        0xFFFFFFFF. A zombie counts in leases too.
//   k_requestor_waiting  a stride loop over min(ws->count, max_waiting) entries of W; an entry whose
//                        deadline has passed counts while it is in W.
//   k_requestor_find     thread per query: probe to the key or a free slot; a miss is a row of zeros.
//   k_requestor_fold     one ticket-ordered tile pass (stream_tile.h) over the SLOTS: the occupied ones
//                        go at their rank to the call's output rows. Its ticket and look-back words
//                        are the call's own. Which slot a key landed in depends on who won a CAS, so
//                        THE ORDER OF THE ROWS IS UNSPECIFIED (the Python wrapper sorts them).
// Claim, lookup and fold are slot_probe.h's: a slot is claimed and its key published by ONE 64-bit
// compare-and-swap, nobody waits for another thread's store, every probe ends after `slots` steps at
// the latest. All sums are integer atomics: the result does not depend on the order.
//
// Hot key: one requestor that owns most of L is the normal case (a farm's CI host), and a plain pass
// would put |L| atomics on one address. The two counting kernels therefore combine equal keys inside
// the wave first (wave_combine of stream_tile.h: kRequestorRounds distinct keys, then the lanes that
// are left add for themselves). `combine` == false (YDC_TUNE requestor_combine=0): every lane adds
// for itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_home.h"
#include "kernels.h"
#include "lease_table.h"
#include "slot_probe.h"
#include "stream_inspect.h"
#include "stream_tile.h"
#include "wait_queue.h"

namespace ydc {

constexpr uint32_t kRequestorCols = 5;    // leases | zombies | prefetch_leases | waiting | waiting_rows
constexpr uint32_t kRequestorUnknown = 0xFFFFFFFFu;  // YDC_REQUESTOR_UNKNOWN
constexpr unsigned long long kRequestorOccupied = 1ull << 32;

struct RequestorIndex {
  unsigned long long* word;  // [mask + 1]: 0, or kRequestorOccupied | requestor_ip
  uint32_t* sum;             // [kRequestorCols][mask + 1]
  uint32_t* unattributed;    // [1]
  uint32_t mask;             // slots - 1
};

// ydc_requestor_load.
struct RequestorLoad {
  uint32_t ip, leases, zombies, prefetch, waiting, rows;
};
static_assert(sizeof(RequestorLoad) == 24, "ydc_requestor_load is 24 bytes");

// (requestor_index_slots: index_home.h)

// The three tables keyed by requestor (this one, stream_quota.h's and stream_usage.h's) share the slot
// word, the home slot (slot_home of the id) and the probe (slot_probe.h).

// The slot of `ip`, claimed if nobody had it. kNone: the table is full (never: it has at least twice
// as many slots as there are entries).
__device__ __forceinline__ uint32_t requestor_claim(unsigned long long* word, uint32_t mask, uint32_t ip,
                                                    bool* published = nullptr) {
  return slot_claim(word, mask, slot_home(ip, mask), 0ull, kRequestorOccupied | ip, published);
}

// The slot of `ip`, or kNone.
__device__ __forceinline__ uint32_t requestor_lookup(const unsigned long long* word, uint32_t mask, uint32_t ip) {
  return slot_lookup(word, mask, slot_home(ip, mask), 0ull, kRequestorOccupied | ip);
}

// n entries of `ip` into columns col, col + 1, col + 2 of its slot: n | a | b.
__device__ __forceinline__ void requestor_add_one(const RequestorIndex& ix, uint32_t ip, uint32_t col, uint32_t n,
                                                  uint32_t a, uint32_t b) {
  const uint32_t h = requestor_claim(ix.word, ix.mask, ip);
  if (h == kNone) return;
  uint32_t* const dst = ix.sum + (size_t)col * ((size_t)ix.mask + 1) + h;
  atomicAdd(dst, n);
  if (a) atomicAdd(dst + ((size_t)ix.mask + 1), a);
  if (b) atomicAdd(dst + 2 * ((size_t)ix.mask + 1), b);
}

// Sum over the wave where any lane has something to add (every lane gets it).
__device__ __forceinline__ uint32_t wave_sum_if_any(uint32_t v) {
  return __ballot(v != 0) ? wave_sum_u32(v) : 0u;  // (wave-uniform)
}

// One entry per active lane: 1 | a | b for key `ip`. With `combine` every lane of the wave must get
// here (wave_combine).
__device__ __forceinline__ void requestor_add(const RequestorIndex& ix, bool combine, bool active, uint32_t ip,
                                              uint32_t col, uint32_t a, uint32_t b) {
  if (combine)
    active = wave_combine(active, ip, [&](uint32_t ip0, bool mine, unsigned long long same, bool leads, uint32_t) {
      const uint32_t sa = wave_sum_if_any(mine ? a : 0u), sb = wave_sum_if_any(mine ? b : 0u);
      if (leads) requestor_add_one(ix, ip0, col, (uint32_t)__popcll(same), sa, sb);
    });
  if (active) requestor_add_one(ix, ip, col, 1u, a, b);
}

// k_outlook_leases' shape: ceil(slots of L / kLeaseTile) workgroups, thread i owns four consecutive
// slots (one 16-byte load of their states). The table: cleared by the host.
__global__ __launch_bounds__(256) void k_requestor_leases(LeaseCols L, const uint4* rec, const uint8_t* pre,
                                                          RequestorIndex ix, uint32_t combine) {
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint4 sv = lease_states4(L, i0);
  const uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool live = (st4[k] & kLeaseLive) != 0;
    uint32_t ip = 0, zombie = 0, prefetch = 0;
    bool known = false;
    if (live) {
      const uint4 r = rec[i0 + k];
      known = inspect_started(r) != kInspectNoTime;
      ip = r.w;
      zombie = (st4[k] & kLeaseZombie) ? 1u : 0u;
      prefetch = pre[i0 + k];
    }
    wave_count(ix.unattributed, live && !known);
    requestor_add(ix, combine != 0, live && known, ip, 0, zombie, prefetch);
  }
}

// n_imm == NULL (no rpc stream): an entry is one row. |W| is the device's (ws->count), never more
// than max_waiting entries are read. The grid may be any size (a stride loop of whole workgroups
// covers W, so every lane of a wave makes the same number of rounds).
__global__ __launch_bounds__(256) void k_requestor_waiting(const uint32_t* w_ip, const uint32_t* n_imm,
                                                           const uint32_t* n_pre, const WaitState* ws,
                                                           uint32_t max_waiting, RequestorIndex ix, uint32_t combine) {
  const uint32_t n = min(ws->count, max_waiting);
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    const bool mine = i < n;
    const uint32_t ip = mine ? w_ip[i] : 0u;
    const uint32_t rows = !mine ? 0u : n_imm ? n_imm[i] + n_pre[i] : 1u;
    requestor_add(ix, combine != 0, mine, ip, 3, rows, 0u);
  }
}

// ceil(n / 256) workgroups. with_l == 0: the lease columns are unknown (no L, or inspection off).
__global__ __launch_bounds__(256) void k_requestor_find(const uint32_t* q, uint32_t n, RequestorIndex ix,
                                                        uint32_t with_l, RequestorLoad* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t ip = q[i], h = requestor_lookup(ix.word, ix.mask, ip);
  const size_t slots = (size_t)ix.mask + 1;
  RequestorLoad r{ip, 0u, 0u, 0u, 0u, 0u};
  if (h != kNone) {
    r.leases = ix.sum[h];
    r.zombies = ix.sum[slots + h];
    r.prefetch = ix.sum[2 * slots + h];
    r.waiting = ix.sum[3 * slots + h];
    r.rows = ix.sum[4 * slots + h];
  }
  if (!with_l) r.leases = r.zombies = r.prefetch = kRequestorUnknown;
  out[i] = r;
}

// The fold's bookkeeping and tile: slot_probe.h's.
using RequestorFoldState = SlotFoldState;
constexpr uint32_t kRequestorTile = kSlotFoldTile;

// slot_fold's grid: ceil(slots / kRequestorTile) workgroups of 256 threads. out: out_cap rows of room.
__global__ __launch_bounds__(256) void k_requestor_fold(RequestorIndex ix, uint32_t with_l, RequestorFoldState* fs,
                                                        unsigned long long* lookback, RequestorLoad* out,
                                                        uint32_t out_cap) {
  const size_t slots = (size_t)ix.mask + 1;
  slot_fold(ix.word, ix.mask, fs, lookback, out_cap, [&](uint32_t dst, unsigned long long w, uint32_t h) {
    RequestorLoad r{(uint32_t)w, ix.sum[h], ix.sum[slots + h], ix.sum[2 * slots + h], ix.sum[3 * slots + h],
                    ix.sum[4 * slots + h]};
    if (!with_l) r.leases = r.zombies = r.prefetch = kRequestorUnknown;
    out[dst] = r;
  });
}

}  // namespace ydc

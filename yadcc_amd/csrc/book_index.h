// book_index.h — a digest index over the running-task book B of an open stream
// (ydc_stream_book_find / ydc_stream_book_distinct). Read-only for the stream:
// nothing here is state, no tick kernel knows about it, a stream that never asks launches what it
// launched before.
//
// The reference's one consumer of GetRunningTasks is the daemons' RunningTaskKeeper
// (running_task_keeper.cc:55-60): one pass over the list, m[task_digest] = entry, so the LAST entry
// of a digest wins; TryFindTask (:67-75) then asks that map once per compile task. The index is that
// map in HBM, keyed by digest_key: an open-addressing table of
//   slots = max(1024, the smallest power of two >= 2 |B|)
// (load <= 1/2; sized by |B| when it is built, not by max_book), three columns per slot:
//   key u64 | last1 u32 (largest position of the key in B, + 1) | cnt u32 (entries with the key).
// kBookIndexEmpty (all ones) marks a free slot; it is an ordinary digest_key too, so the one key
// equal to it has a side record of its own (last1 | cnt) instead of a slot. The home slot is a full
// 64-bit mix of the key (callers' handles may be sequential, pointers, or multiples of 2^32),
// then linear probing.
//
// It is DERIVED state and rebuilt on demand rather than maintained: k_book_commit and k_book_remap
// compact B in place, so one report moves the position of every entry behind the reporter's — an
// incremental index would have to be rewritten as a whole anyway, and inside the tick.
//
//   k_book_index_build   thread per entry of B, the table cleared by the host in front of it. A slot
//                        is claimed and its key published by slot_claim (slot_probe.h: ONE 64-bit
//                        compare-and-swap, no thread ever waits for another's store); whoever finds
//                        the slot free or already holding its key adds itself with atomicMax /
//                        atomicAdd.
//   k_book_index_find    thread per query: probe to the key or a free slot, B's columns at last1 - 1.
//   k_book_distinct      one ticket-ordered tile pass (stream_tile.h) over B's positions: position p
//                        is kept iff its key's last1 == p + 1, and kept rows go at their rank to
//                        output columns of the call's own. Its ticket and look-back words are the
//                        call's own as well (the stream's belong to the tick); B is only read.
// Every probe ends after `slots` steps at the latest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_home.h"
#include "kernels.h"
#include "running_book.h"
#include "slot_probe.h"
#include "stream_tile.h"

namespace ydc {

constexpr unsigned long long kBookIndexEmpty = ~0ull;
constexpr uint32_t kBookNotFound = 0xFFFFFFFFu;  // YDC_BOOK_NOT_FOUND

struct BookIndex {
  unsigned long long* key;  // [mask + 1]
  uint32_t* last1;          // [mask + 1]
  uint32_t* cnt;            // [mask + 1]
  uint32_t* side;           // [2]: last1 | cnt of the key kBookIndexEmpty
  uint32_t mask;            // slots - 1
};

// ydc_book_hit.
struct BookHit {
  uint32_t pos, count, servant, reserved;
  unsigned long long grant, stid;
};
static_assert(sizeof(BookHit) == 32, "ydc_book_hit is 32 bytes");

// (book_index_slots and book_index_mix: index_home.h)

// What the index knows of key k: last1 (0: the key is not in B) and the count.
__device__ __forceinline__ uint2 book_index_lookup(const BookIndex& ix, unsigned long long k) {
  if (k == kBookIndexEmpty) return make_uint2(ix.side[0], ix.side[1]);
  const uint32_t h = slot_lookup(ix.key, ix.mask, slot_home(k, ix.mask), kBookIndexEmpty, k);
  return h == kNone ? make_uint2(0u, 0u) : make_uint2(ix.last1[h], ix.cnt[h]);
}

// ceil(n / 256) workgroups. n: |B| (the host's mirror, <= max_book).
__global__ __launch_bounds__(256) void k_book_index_build(const unsigned long long* dkey, uint32_t n, BookIndex ix) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const unsigned long long k = dkey[p];
  if (k == kBookIndexEmpty) {
    atomicMax(&ix.side[0], p + 1);
    atomicAdd(&ix.side[1], 1u);
    return;
  }
  const uint32_t h = slot_claim(ix.key, ix.mask, slot_home(k, ix.mask), kBookIndexEmpty, k);
  if (h == kNone) return;  // (never: the table has at least 2 n slots)
  atomicMax(&ix.last1[h], p + 1);
  atomicAdd(&ix.cnt[h], 1u);
}

// ceil(n / 256) workgroups; n_b: |B|. A last1 beyond |B| (there is none in a valid index) is a miss.
__global__ __launch_bounds__(256) void k_book_index_find(const unsigned long long* q, uint32_t n, BookIndex ix,
                                                         BookCols B, uint32_t n_b, BookHit* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint2 r = book_index_lookup(ix, q[i]);
  BookHit hit{kBookNotFound, 0u, 0u, 0u, 0ull, 0ull};
  if (r.x != 0 && r.x <= n_b) {
    const uint32_t p = r.x - 1;
    hit.pos = p;
    hit.count = r.y;
    hit.servant = B.servant[p];
    hit.grant = B.grant[p];
    hit.stid = B.stid[p];
  }
  out[i] = hit;
}

// The distinct pass's own bookkeeping, cleared by the host in front of the launch; its look-back
// words follow it.
struct BookDistinctState {
  uint32_t ticket;
  uint32_t n_rows;  // the result: distinct keys of B
};

struct BookDistinctOut {
  uint32_t* servant;
  unsigned long long* grant;
  unsigned long long* stid;
  unsigned long long* dkey;
  uint32_t* count;
};

// ceil(n_b / kBookTile) workgroups of 256 threads, thread i of a workgroup owning four consecutive
// positions of B. out: n_b rows of room.
__global__ __launch_bounds__(256) void k_book_distinct(BookCols B, uint32_t n_b, BookIndex ix, BookDistinctState* ds,
                                                       unsigned long long* lookback, BookDistinctOut out) {
  __shared__ uint32_t lds[17];
  __shared__ uint32_t s_bid, s_pre;
  if (threadIdx.x == 0) s_bid = atomicAdd(&ds->ticket, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const uint32_t p0 = bid * kBookTile + threadIdx.x * 4;
  bool keep[4];
  uint32_t cnt[4];
  uint32_t n_keep = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t p = p0 + i;
    keep[i] = false;
    cnt[i] = 0;
    if (p >= n_b) continue;
    const uint2 r = book_index_lookup(ix, B.dkey[p]);
    keep[i] = r.x == p + 1;
    cnt[i] = r.y;
    n_keep += keep[i] ? 1u : 0u;
  }
  uint32_t tot = 0;
  const uint32_t ex = block_exclusive_scan(n_keep, lds, &tot);
  if (threadIdx.x < 64) {
    LbWords<1> agg;
    agg.w[0] = lb_pack(tot);
    const LbWords<1> pre = tile_lookback<1>(lookback, bid, threadIdx.x, agg);
    if (threadIdx.x == 0) {
      s_pre = lb_lo(pre.w[0]);
      if (bid == gridDim.x - 1) ds->n_rows = s_pre + tot;
    }
  }
  __syncthreads();
  uint32_t dst = s_pre + ex;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!keep[i]) continue;
    const uint32_t p = p0 + i;
    if (dst < n_b) {  // (always: a rank among the kept is never larger than the position)
      out.servant[dst] = B.servant[p];
      out.grant[dst] = B.grant[p];
      out.stid[dst] = B.stid[p];
      out.dkey[dst] = B.dkey[p];
      out.count[dst] = cnt[i];
    }
    ++dst;
  }
}

}  // namespace ydc

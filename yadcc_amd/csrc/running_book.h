// running_book.h — the servants' running-task book B of a leased streaming context
// (ydc_stream_book_begin / ydc_stream_book_stage / ydc_stream_book_get).
//
// The reference's NotifyServantRunningTasks (task_dispatcher.cc:222-277) answers unknown_tasks —
// k_lease_report and k_lease_sweep do that — and hands the report minus the unknown ids to
// RunningTaskBookkeeper::SetServantRunningTasks, which replaces that servant's list; DropServant
// (servant expiry, task_dispatcher.cc:510) erases it and GetRunningTasks flattens what is left
// (running_task_bookkeeper.cc:24-43). B is that flattened list in HBM, four columns per entry:
// servant | task_grant_id | servant_task_id | digest_key (the caller's handle for the digest
// string, echoed like a tag). Its order is defined: the entries of the servants that did not report
// in the tick, in their previous order, then the tick's permitted ids in report order.
//
//   k_book_commit   in the tick, directly behind k_lease_report (it needs rep_tick and
//                   out_report_unknown, not the sweep): one ticket-ordered tile pass
//                   (stream_tile.h) over the positions [max_book slots of B | max_report_ids ids
//                   of the tick]. An old entry is kept when its servant did not report this tick;
//                   a new id is kept when k_lease_report answered 0 for it. The kept positions are
//                   counted through one look-back word per tile and stored to B at their rank.
//   k_book_remap    ydc_remove_servants: the same pass over B alone, kept: the servant's row
//                   stays; its index follows the registry's compaction (as k_lease_remap).
//
// The compaction is IN PLACE, and that is safe:
//   - a tile loads all its positions into registers and then passes a __syncthreads() (those of
//     block_exclusive_scan) before wave 0 publishes its aggregate; tile_lookback itself has no
//     barrier, the ones in front of its call are what counts;
//   - a tile learns its exclusive prefix only after every predecessor has published (an
//     aggregate or an inclusive word, both behind that barrier), so every predecessor has loaded;
//   - a tile's destinations [prefix, prefix + kept) lie at or below its own positions (a rank
//     among the kept is never larger than the position; a new id k sits at max_book + k and
//     lands below |B| + k), so they never reach a region a later tile has yet to read, and no two
//     tiles write the same slot.
// max_book + max_report_ids < 2^31 (the host checks), so one 31-bit count per word is enough.
//
// BookState: |B| and the pass's ticket. The last workgroup stores the new |B| (also to the
// page-locked BookOutcome) and puts the ticket back to 0: it learns its prefix only after every
// other workgroup has published, hence drawn its ticket and — thread 0 reads it first — read |B|.
// The look-back words are the tail of the stream's words, which k_lease_renew clears every tick;
// the host clears them in front of k_book_remap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_table.h"
#include "stream_tile.h"

namespace ydc {

constexpr uint32_t kBookTile = 1024;  // positions per workgroup (256 x 4)

struct BookCols {
  uint32_t* servant;
  unsigned long long* grant;  // task_grant_id
  unsigned long long* stid;   // servant_task_id
  unsigned long long* dkey;   // digest_key
};

struct BookState {
  uint32_t n_entries;  // |B|
  uint32_t ticket;     // workgroups of the pass started; 0 between passes
};

// Page-locked: what the host reads after the tick.
struct BookOutcome {
  uint32_t n_entries;
  uint32_t tick_no;
};

// A thread's four positions, loaded.
struct BookQuad {
  uint32_t servant[4];
  unsigned long long grant[4], stid[4], dkey[4];
  bool keep[4];
};

// The pass's ticket and |B| as it was before the pass, to every thread.
__device__ __forceinline__ uint32_t book_draw(BookState* bs, uint32_t* n_before) {
  __shared__ uint32_t s_bid, s_n;
  if (threadIdx.x == 0) {
    // (|B| before the ticket: the last workgroup changes it, stream_tile.h)
    s_n = __hip_atomic_load(&bs->n_entries, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_bid = atomicAdd(&bs->ticket, 1u);
  }
  __syncthreads();
  *n_before = s_n;
  return s_bid;
}

// The loaded quad's kept entries to B at their rank among all kept. Returns nothing; the last
// workgroup stores |B| (and the outcome block, when there is one).
__device__ __forceinline__ void book_store(BookCols B, BookState* bs, uint32_t max_book, unsigned long long* lookback,
                                           uint32_t bid, const BookQuad& q, BookOutcome* bout, uint32_t tick_no) {
  __shared__ uint32_t lds[17];
  __shared__ uint32_t s_pre;
  uint32_t n_keep = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) n_keep += q.keep[i] ? 1u : 0u;
  uint32_t tot = 0;
  // (its barriers stand between every load of the tile and the publication below)
  const uint32_t ex = block_exclusive_scan(n_keep, lds, &tot);
  if (threadIdx.x < 64) {
    LbWords<1> agg;
    agg.w[0] = lb_pack(tot);
    const LbWords<1> pre = tile_lookback<1>(lookback, bid, threadIdx.x, agg);
    if (threadIdx.x == 0) {
      const uint32_t p = lb_lo(pre.w[0]);
      s_pre = p;
      if (bid == gridDim.x - 1) {
        const uint32_t n = min(p + tot, max_book);
        __hip_atomic_store(&bs->n_entries, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bs->ticket = 0;
        if (bout) {
          bout->n_entries = p + tot;
          bout->tick_no = tick_no;
        }
      }
    }
  }
  __syncthreads();
  uint32_t dst = s_pre + ex;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!q.keep[i]) continue;
    if (dst < max_book) {  // (always: |B| + n_ids <= max_book is checked before the tick)
      B.servant[dst] = q.servant[i];
      B.grant[dst] = q.grant[i];
      B.stid[dst] = q.stid[i];
      B.dkey[dst] = q.dkey[i];
    }
    ++dst;
  }
}

// ceil((max_book + max_ids) / kBookTile) workgroups of 256 threads; thread i of a workgroup owns
// four consecutive positions. unknown: k_lease_report's answers, read back from the page-locked
// result block; stid / dkey: the payload columns the host staged beside rep_id.
__global__ __launch_bounds__(256) void k_book_commit(BookCols B, BookState* bs, uint32_t max_book, LeaseIn in,
                                                     const unsigned long long* stg_stid,
                                                     const unsigned long long* stg_dkey, uint32_t max_rep,
                                                     uint32_t max_ids, uint32_t n_servants, const uint32_t* rep_tick,
                                                     const uint8_t* unknown, unsigned long long* lookback,
                                                     BookOutcome* bout) {
  uint32_t n_b = 0;
  const uint32_t bid = book_draw(bs, &n_b);
  n_b = min(n_b, max_book);
  const uint32_t tick = in.hdr->tick_no;
  const uint32_t n_rep = min(in.hdr->n_rep, max_rep), n_ids = min(in.hdr->n_ids, max_ids);
  const uint32_t p0 = bid * kBookTile + threadIdx.x * 4;
  BookQuad q;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t p = p0 + i;
    q.keep[i] = false;
    q.servant[i] = 0;
    q.grant[i] = q.stid[i] = q.dkey[i] = 0;
    if (p < max_book) {
      if (p >= n_b) continue;
      const uint32_t s = B.servant[p];
      if (s < n_servants && rep_tick[s] == tick) continue;  // its servant reported: replaced
      q.keep[i] = true;
      q.servant[i] = s;
      q.grant[i] = B.grant[p];
      q.stid[i] = B.stid[p];
      q.dkey[i] = B.dkey[p];
    } else {
      const uint32_t k = p - max_book;
      if (k >= n_ids || n_rep == 0 || unknown[k]) continue;
      // The report k belongs to: the last r with rep_off[r] <= k (as k_lease_report finds it).
      uint32_t lo = 0, hi = n_rep;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (in.rep_off[mid] <= k) lo = mid; else hi = mid;
      }
      q.keep[i] = true;
      q.servant[i] = in.rep_srv[lo];
      q.grant[i] = in.rep_id[k];
      q.stid[i] = stg_stid[k];
      q.dkey[i] = stg_dkey[k];
    }
  }
  book_store(B, bs, max_book, lookback, bid, q, bout, tick);
}

// ydc_remove_servants with a book on (DropServant): ceil(max_book / kBookTile) workgroups.
// removed[]: ascending.
__global__ __launch_bounds__(256) void k_book_remap(BookCols B, BookState* bs, uint32_t max_book,
                                                    const uint32_t* removed, uint32_t n_removed,
                                                    unsigned long long* lookback) {
  uint32_t n_b = 0;
  const uint32_t bid = book_draw(bs, &n_b);
  n_b = min(n_b, max_book);
  const uint32_t p0 = bid * kBookTile + threadIdx.x * 4;
  BookQuad q;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t p = p0 + i;
    q.keep[i] = false;
    q.servant[i] = 0;
    q.grant[i] = q.stid[i] = q.dkey[i] = 0;
    if (p >= n_b) continue;
    const uint32_t s = B.servant[p];
    const uint32_t before = lower_bound_u32(removed, n_removed, s);
    if (before < n_removed && removed[before] == s) continue;
    q.keep[i] = true;
    q.servant[i] = s - before;
    q.grant[i] = B.grant[p];
    q.stid[i] = B.stid[p];
    q.dkey[i] = B.dkey[p];
  }
  book_store(B, bs, max_book, lookback, bid, q, nullptr, 0);
}

}  // namespace ydc

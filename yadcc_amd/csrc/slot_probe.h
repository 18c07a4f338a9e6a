// slot_probe.h — the device code the open-addressing tables of an open stream share: the digest index
// over the book (book_index.h), the load per requestor (requestor_index.h), the tick's quota table
// (stream_quota.h) and the usage per requestor (stream_usage.h). The arithmetic — the home slot and the
// slot counts — is index_home.h's, which stays free of HIP; here are the probe from the home slot and
// the fold of a table's occupied slots into rows.
//
// A table is an array of 64-bit slot words over mask + 1 = 2^k slots, one value of which (`empty`) marks
// a free slot. A slot is claimed and its word published by ONE 64-bit compare-and-swap, and a published
// word never changes while the table lives: nobody waits for another thread's store (the lanes of a wave
// run in lockstep: a claim-then-publish protocol with a spin hangs them). Linear probing, and every
// probe ends after mask + 1 steps at the latest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_home.h"
#include "kernels.h"
#include "stream_tile.h"

namespace ydc {

__device__ __forceinline__ uint32_t slot_home(uint64_t key, uint32_t mask) {
  return (uint32_t)book_index_mix(key) & mask;
}

// The slot that holds `w`, probing from `home`; the first free slot on the way is claimed for it.
// kNone: the table is full. *published (where asked for): this call put the word there.
__device__ __forceinline__ uint32_t slot_claim(unsigned long long* word, uint32_t mask, uint32_t home,
                                               unsigned long long empty, unsigned long long w,
                                               bool* published = nullptr) {
  uint32_t h = home;
  for (uint32_t it = 0; it <= mask; ++it) {
    // (a published word never changes: a plain look first spares the slot the CAS traffic of everybody
    // who shares the word or merely passes by)
    unsigned long long at = __hip_atomic_load(&word[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (at == empty) at = atomicCAS(&word[h], empty, w);
    if (at == empty || at == w) {
      if (published) *published = at == empty;
      return h;
    }
    h = (h + 1) & mask;
  }
  if (published) *published = false;
  return kNone;
}

// The slot that holds `w`, or kNone: the probe ends at the word or at a free slot. For a table nobody
// is claiming in (the launch behind the one that built it).
__device__ __forceinline__ uint32_t slot_lookup(const unsigned long long* word, uint32_t mask, uint32_t home,
                                                unsigned long long empty, unsigned long long w) {
  uint32_t h = home;
  for (uint32_t it = 0; it <= mask; ++it) {
    const unsigned long long at = word[h];
    if (at == w) return h;
    if (at == empty) break;
    h = (h + 1) & mask;
  }
  return kNone;
}

// The bookkeeping of one fold, cleared by the host in front of the launch; its look-back words follow it.
struct SlotFoldState {
  uint32_t ticket;
  uint32_t n_rows;  // the result: occupied slots
};

constexpr uint32_t kSlotFoldTile = 1024;  // slots per workgroup of a fold (256 x 4)

// One ticket-ordered tile pass (stream_tile.h) over the slot words of a table whose free slots are 0:
// ceil(slots / kSlotFoldTile) workgroups of 256 threads, thread i of a workgroup owning four consecutive
// slots (the slot count is a multiple of 1024). An occupied slot h is handed, with its word and its rank
// among the occupied slots, to emit(rank, word, h) while rank < out_cap; a rank beyond it is counted
// and not emitted. Which slot a key landed in depends on who won a CAS, so the order of the ranks is
// unspecified. Every thread of the workgroup must get here, once.
template <class Emit>
__device__ __forceinline__ void slot_fold(const unsigned long long* word, uint32_t mask, SlotFoldState* fs,
                                          unsigned long long* lookback, uint32_t out_cap, Emit&& emit) {
  __shared__ uint32_t lds[17];
  __shared__ uint32_t s_bid, s_pre;
  if (threadIdx.x == 0) s_bid = atomicAdd(&fs->ticket, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const uint32_t h0 = bid * kSlotFoldTile + threadIdx.x * 4;
  unsigned long long w4[4] = {0, 0, 0, 0};
  if (h0 <= mask) {
    const ulonglong2 w01 = *reinterpret_cast<const ulonglong2*>(word + h0);
    const ulonglong2 w23 = *reinterpret_cast<const ulonglong2*>(word + h0 + 2);
    w4[0] = w01.x, w4[1] = w01.y, w4[2] = w23.x, w4[3] = w23.y;
  }
  uint32_t n_keep = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) n_keep += w4[i] ? 1u : 0u;
  uint32_t tot = 0;
  const uint32_t ex = block_exclusive_scan(n_keep, lds, &tot);
  if (threadIdx.x < 64) {
    LbWords<1> agg;
    agg.w[0] = lb_pack(tot);
    const LbWords<1> pre = tile_lookback<1>(lookback, bid, threadIdx.x, agg);
    if (threadIdx.x == 0) {
      s_pre = lb_lo(pre.w[0]);
      if (bid == gridDim.x - 1) fs->n_rows = s_pre + tot;
    }
  }
  __syncthreads();
  uint32_t dst = s_pre + ex;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!w4[i]) continue;
    if (dst < out_cap) emit(dst, w4[i], h0 + i);
    ++dst;
  }
}

}  // namespace ydc

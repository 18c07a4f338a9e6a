// stream_select.h — the lease table filtered, counted and paged on the device
// (ydc_stream_inspect_select / ydc_stream_inspect_count).
//
// Read-only: no kernel here writes the table, the records or anything a tick reads. A call answers
// "the `cap` smallest ids among the leases that satisfy a filter, and how many satisfy it", so that
// min(matches, cap) records cross the bus and not |L|. The predicate is lease_filter.h's, evaluated
// per live slot (the live bit decides: an erased slot's stale record is never looked at).
//
//   k_select_count   one pass over L. n filters staged in LDS; per filter the matches, counted per
//                    wave by ballot, combined in LDS and added to HBM once per workgroup and filter.
//                    <true>: one filter, and the smallest and largest matching id beside the count.
//   k_select_hist    one round of the radix select on the 64-bit id, one pass over L: among the
//                    matches whose id agrees with the prefix chosen so far above byte b, the
//                    histogram of byte b, 256 bins in LDS per workgroup, flushed once.
//   k_select_digit   one workgroup: the round's bins scanned, the bin that holds the rank looked for
//                    chosen, prefix and remaining rank handed to the next round in HBM.
//   k_select_pack    k_inspect_pack with the predicate and id <= threshold.
//
// The select only runs when matches > cap, for the cap-th smallest matching id. Every matching id
// lies in [min, max], so all of them share the bytes above the highest byte in which min and max
// differ (`top`): the rounds go from byte `top` down to byte 0, and the host always launches eight,
// of which those above `top` return at once. Ids are unique, so after byte 0 the prefix IS the
// cap-th smallest matching id and the pack's `id <= threshold` lets exactly cap rows through.
//
// Every kernel has k_inspect_pack's shape: ceil(slots / kLeaseTile) workgroups of 256 threads, thread
// i owns four consecutive slots, `state` read as one uint4 and the other columns as vectors when one
// of the four is live. Indices: a slot index is < slots by the guard of lease_states4 (slots is a
// multiple of 4, and beyond the table nothing is live); a bin index is a byte; a filter index is < n <= kSelectMaxFilters; a packed
// position is guarded by out.cap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lease_filter.h"
#include "lease_table.h"
#include "stream_inspect.h"

namespace ydc {

constexpr uint32_t kSelectBins = 256, kSelectRounds = 8;

// The call's state in HBM, at the head of its scratch buffer; the host clears it, sets min_id to ~0
// and, before the pack, prefix / rank.
struct SelectState {
  uint32_t matches[kSelectMaxFilters];
  unsigned long long min_id, max_id;  // over the matches of filter 0 (k_select_count<true>)
  unsigned long long prefix;          // the id's bytes chosen so far; after byte 0: the threshold
  uint32_t rank;                      // 1-based, among the matches that agree with the prefix
  uint32_t n_packed;
  uint32_t hist[kSelectRounds][kSelectBins];
};

// The bits of an id above byte b.
__host__ __device__ __forceinline__ unsigned long long select_above(unsigned long long id, uint32_t b) {
  return b >= 7 ? 0ull : id >> (8 * (b + 1));
}

// The four slots [i0, i0 + 4) as rows. `need`: the columns to fetch, as a filter's `fields` names
// them (kSelAfterId: the id). Returns the live bits; rows of dead slots are not filled in. rec /
// pre NULL (inspection off): the sentinels.
__device__ __forceinline__ uint32_t select_tile(const LeaseCols& L, const uint4* rec, const uint8_t* pre, uint32_t i0,
                                                uint32_t need, LeaseRow (&row)[4], uint32_t (&st4)[4]) {
  const uint4 sv = lease_states4(L, i0);
  st4[0] = sv.x, st4[1] = sv.y, st4[2] = sv.z, st4[3] = sv.w;
  if (!((sv.x | sv.y | sv.z | sv.w) & kLeaseLive)) return 0;
  unsigned long long id4[4] = {0, 0, 0, 0};
  int64_t e4[4] = {0, 0, 0, 0};
  uint32_t s4[4] = {0, 0, 0, 0}, p4 = 0;
  if (need & kSelAfterId) {
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(L.key + i0);
    const ulonglong2 k23 = *reinterpret_cast<const ulonglong2*>(L.key + i0 + 2);
    id4[0] = k01.x, id4[1] = k01.y, id4[2] = k23.x, id4[3] = k23.y;
  }
  if (need & kSelExpiresBefore) {
    const longlong2 e01 = *reinterpret_cast<const longlong2*>(L.expires + i0);
    const longlong2 e23 = *reinterpret_cast<const longlong2*>(L.expires + i0 + 2);
    e4[0] = e01.x, e4[1] = e01.y, e4[2] = e23.x, e4[3] = e23.y;
  }
  if (need & kSelServant) {
    const uint4 srv = *reinterpret_cast<const uint4*>(L.servant + i0);
    s4[0] = srv.x, s4[1] = srv.y, s4[2] = srv.z, s4[3] = srv.w;
  }
  if ((need & kSelPrefetch) && pre) p4 = *reinterpret_cast<const uint32_t*>(pre + i0);
  uint32_t live = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(st4[k] & kLeaseLive)) continue;
    live |= 1u << k;
    uint4 r = inspect_rec(kInspectNoTime, kInspectNoId, kInspectNoId);
    if ((need & kSelRecord) && rec) r = rec[i0 + k];
    row[k].id = id4[k];
    row[k].expires_at = e4[k];
    row[k].started_at = inspect_started(r);
    row[k].servant = s4[k];
    row[k].env_id = r.z;
    row[k].requestor_ip = r.w;
    row[k].zombie = (st4[k] & kLeaseZombie) != 0;
    row[k].prefetch = ((p4 >> (8 * k)) & 0xFFu) != 0;
  }
  return live;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// n <= kSelectMaxFilters filters at `filters` (HBM). kMinMax: n == 1, and st->min_id / max_id too.
// Every lane stays to the end: the ballots and the barriers want the whole wave.
template <bool kMinMax>
__global__ __launch_bounds__(256) void k_select_count(LeaseCols L, const uint4* rec, const uint8_t* pre,
                                                      const LeaseFilter* filters, uint32_t n, SelectState* st) {
  __shared__ LeaseFilter s_f[kSelectMaxFilters];
  __shared__ uint32_t s_cnt[kSelectMaxFilters];
  __shared__ unsigned long long s_min, s_max;
  if (n > kSelectMaxFilters) n = kSelectMaxFilters;
  for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) {
    s_f[t] = filters[t];
    s_cnt[t] = 0;
  }
  if (threadIdx.x == 0) {
    s_min = ~0ull;
    s_max = 0ull;
  }
  __syncthreads();
  uint32_t need = kMinMax ? kSelAfterId : 0u;
  for (uint32_t q = 0; q < n; ++q) need |= s_f[q].fields;  // (uniform)
  LeaseRow row[4];
  uint32_t st4[4];
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint32_t live = select_tile(L, rec, pre, i0, need, row, st4);
  const uint32_t lane = lane_id();
  unsigned long long lo = ~0ull, hi = 0ull;
  if (__ballot(live != 0)) {  // (wave-uniform)
    for (uint32_t q = 0; q < n; ++q) {
      const LeaseFilter f = s_f[q];
      uint32_t c = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool hit = ((live >> k) & 1u) && lease_filter_match(f, row[k]);
        c += (uint32_t)__popcll(__ballot(hit));
        if (kMinMax && hit) {
          lo = row[k].id < lo ? row[k].id : lo;
          hi = row[k].id > hi ? row[k].id : hi;
        }
      }
      if (lane == 0 && c) atomicAdd(&s_cnt[q], c);
    }
    if (kMinMax) {
      lo = wave_min_u64(lo);
      hi = wave_max_u64(hi);
      if (lane == 0 && lo <= hi) {
        atomicMin(&s_min, lo);
        atomicMax(&s_max, hi);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < n && s_cnt[threadIdx.x]) atomicAdd(&st->matches[threadIdx.x], s_cnt[threadIdx.x]);
  if (kMinMax && threadIdx.x == 64 && s_min <= s_max) {
    atomicMin(&st->min_id, s_min);
    atomicMax(&st->max_id, s_max);
  }
}

// Round `b` of the select (byte b of the id), `top`: the highest byte that is not common to all
// matches. st->prefix holds the bytes above b.
__global__ __launch_bounds__(256) void k_select_hist(LeaseCols L, const uint4* rec, const uint8_t* pre,
                                                     const LeaseFilter* filter, uint32_t b, uint32_t top,
                                                     SelectState* st) {
  if (b > top || b >= kSelectRounds) return;  // (uniform)
  __shared__ uint32_t s_bin[kSelectBins];
  s_bin[threadIdx.x] = 0;  // (256 threads, 256 bins)
  __syncthreads();
  const LeaseFilter f = *filter;
  const unsigned long long above = select_above(st->prefix, b);
  LeaseRow row[4];
  uint32_t st4[4];
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint32_t live = select_tile(L, rec, pre, i0, f.fields | kSelAfterId, row, st4);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (((live >> k) & 1u) && lease_filter_match(f, row[k]) && select_above(row[k].id, b) == above)
      atomicAdd(&s_bin[(uint32_t)(row[k].id >> (8 * b)) & (kSelectBins - 1)], 1u);
  __syncthreads();
  const uint32_t mine = s_bin[threadIdx.x];
  if (mine) atomicAdd(&st->hist[b][threadIdx.x], mine);
}

// One workgroup of 256 threads, thread t owns bin t of round b: the smallest bin d whose inclusive
// prefix sum reaches the rank; the rank that remains inside it.
__global__ __launch_bounds__(256) void k_select_digit(uint32_t b, uint32_t top, SelectState* st) {
  if (b > top || b >= kSelectRounds) return;
  __shared__ uint32_t s_sum[kSelectBins];
  const uint32_t t = threadIdx.x, mine = st->hist[b][t], rank = st->rank;
  s_sum[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < kSelectBins; d <<= 1) {  // (Hillis-Steele, inclusive)
    const uint32_t add = t >= d ? s_sum[t - d] : 0u;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  const uint32_t upto = s_sum[t], before = upto - mine;
  if (before < rank && rank <= upto) {  // (exactly one bin when 1 <= rank <= the bins' total)
    st->prefix |= (unsigned long long)t << (8 * b);
    st->rank = rank - before;
  }
}

// k_inspect_pack with the predicate and id <= st->prefix. st->n_packed: cleared by the host; counts
// every row that passes, also those beyond out.cap (which are not written, and which do not exist
// when the threshold is right).
__global__ __launch_bounds__(256) void k_select_pack(LeaseCols L, const uint4* rec, const uint8_t* pre,
                                                     const LeaseFilter* filter, InspectPacked out, SelectState* st) {
  const LeaseFilter f = *filter;
  const unsigned long long threshold = st->prefix;
  LeaseRow row[4];
  uint32_t st4[4];
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint32_t live = select_tile(L, rec, pre, i0, f.fields | kSelAfterId, row, st4);
  bool hit[4];
  unsigned long long m4[4];
  uint32_t total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hit[k] = ((live >> k) & 1u) && lease_filter_match(f, row[k]) && row[k].id <= threshold;
    m4[k] = __ballot(hit[k]);
    total += (uint32_t)__popcll(m4[k]);
  }
  if (!total) return;  // (wave-uniform)
  const uint32_t lane = lane_id();
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&st->n_packed, total);
  base = (uint32_t)__shfl((int)base, 0, 64);
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (hit[k]) {
      const uint32_t at = base + (uint32_t)__popcll(m4[k] & below), slot = i0 + k;
      if (at < out.cap) {
        out.id[at] = row[k].id;
        out.expires[at] = L.expires[slot];
        out.rec[at] = rec ? rec[slot] : inspect_rec(kInspectNoTime, kInspectNoId, kInspectNoId);
        out.servant[at] = L.servant[slot];
        out.state[at] = st4[k];
        out.prefetch[at] = pre ? pre[slot] : (uint8_t)0;
      }
    }
    base += (uint32_t)__popcll(m4[k]);
  }
}

}  // namespace ydc

// stream_outlook.h — the outlook per request personality of an open stream, computed on the device
// from what the stream already keeps in HBM (ydc_stream_outlook_get). Read-only:
// nothing here is state, no tick kernel knows about it, a stream that never asks launches what it
// launched before.
//
// For a personality (env_id, min_version) the reference's grant call first lists the eligible
// servants (UnsafeEnumerateEligibleServants, task_dispatcher.cc:316-344), then the free ones among
// them (UnsafeEnumerateFreeServants, :346-360). Eligibility is the class test of the batch pipeline
// (host_tables.h: a class is one (environment set, version) signature among the servants with
// max_tasks != 0), so the supply side is summed per CLASS once and then per query over the classes:
// O(S + n * C), not O(n * S).
//
//   k_outlook_classes   thread per servant: six sums per class (members, free members, slots =
//                       servant_slot_count, running_tasks, max_tasks, capacity_available).
//   k_outlook_queries   wave per query: the sums of the classes that pass the query's test.
//   k_outlook_waiting   thread per entry of W: entries and rows per env id (dense histogram).
//   k_outlook_leases    four slots of L per thread: leases and zombies per env id of the inspection
//                       record (dense histograms; inspection on only).
//
// Histogram bins: env ids [0, 64 * env_words) and ONE further bin for everything else (an id no
// servant can advertise, or YDC_INSPECT_NO_ID), which no query reads.
//
// Contention: a registry has 1 - 30 classes and a few dozen digests, so thousands of atomics would
// meet on a handful of addresses. Each workgroup therefore counts in LDS first and adds its non-zero
// sums to the global table with one atomic each:
//   kOutlookLdsClasses = 256 classes x 6 x 8 B = 12 KB  (the lane-per-class kernels' bound,
//                        kMaxWaveClasses; 13 workgroups of a CU's 160 KB still fit)
//   kOutlookLdsBins    = 2048 bins x 2 x 4 B  = 16 KB  (32 mask words of digests)
// Above either bound the collisions are spread over that many addresses anyway, and the kernel uses
// plain global atomics. All sums are integers: the result does not depend on the order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch_core.h"
#include "kernels.h"
#include "lease_table.h"
#include "stream_inspect.h"
#include "wait_queue.h"

namespace ydc {

constexpr uint32_t kOutlookLdsClasses = 256;
constexpr uint32_t kOutlookLdsBins = 2048;
constexpr uint32_t kOutlookCols = 6;  // members | free members | slots | running | max_tasks | capacity_available

// agg: [C][kOutlookCols], cleared by the host. class_of == kNone (max_tasks == 0) contributes
// nothing; so does a class id >= C (there is none between ticks).
__global__ __launch_bounds__(256) void k_outlook_classes(const uint32_t* nproc, const uint32_t* load,
                                                         const uint32_t* max_tasks, const uint32_t* running,
                                                         const uint32_t* flags, const uint32_t* class_of, uint32_t n,
                                                         uint32_t C, unsigned long long* agg) {
  __shared__ unsigned long long s_agg[kOutlookLdsClasses * kOutlookCols];
  const bool lds = C <= kOutlookLdsClasses;  // (uniform)
  if (lds) {
    for (uint32_t i = threadIdx.x; i < C * kOutlookCols; i += blockDim.x) s_agg[i] = 0;
    __syncthreads();
  }
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) {
    const uint32_t c = class_of[s];
    if (c < C) {
      const uint32_t np = nproc[s], ld = load[s], mt = max_tasks[s], r = running[s], fl = flags[s];
      const uint32_t av = capacity_available(np, ld, mt, r, fl);
      const unsigned long long v[kOutlookCols] = {1ull, r < av ? 1ull : 0ull,  // (:354: running_tasks >= capacity: not free)
                                                  servant_slot_count(np, ld, mt, r, fl), r, mt, av};
      if (lds) {
        unsigned long long* dst = s_agg + c * kOutlookCols;
#pragma unroll
        for (uint32_t k = 0; k < kOutlookCols; ++k)
          if (v[k]) atomicAdd(&dst[k], v[k]);
      } else {
        unsigned long long* dst = agg + (size_t)c * kOutlookCols;
#pragma unroll
        for (uint32_t k = 0; k < kOutlookCols; ++k)
          if (v[k]) atomicAdd(&dst[k], v[k]);
      }
    }
  }
  if (lds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < C * kOutlookCols; i += blockDim.x) {
      const unsigned long long v = s_agg[i];
      if (v) atomicAdd(&agg[i], v);
    }
  }
}

// Four waves per workgroup, a wave per query; lane l takes classes l, l + 64, ... out: [n][kOutlookCols].
// An env id >= 64 * env_words is a digest no servant has: no class passes, the row is zeros.
__global__ __launch_bounds__(256) void k_outlook_queries(const uint32_t* env, const uint32_t* minv, uint32_t n,
                                                         const uint64_t* cls_env, const uint32_t* cls_ver, uint32_t C,
                                                         uint32_t env_words, const unsigned long long* agg,
                                                         unsigned long long* out) {
  const uint32_t q = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  if (q >= n) return;  // (wave-uniform)
  const uint32_t lane = lane_id(), e = env[q], mv = minv[q];
  unsigned long long v[kOutlookCols] = {0, 0, 0, 0, 0, 0};
  if (e / 64 < env_words) {
    for (uint32_t c = lane; c < C; c += 64) {
      if (!((cls_env[(size_t)c * env_words + e / 64] >> (e & 63)) & 1ull) || cls_ver[c] < mv) continue;
#pragma unroll
      for (uint32_t k = 0; k < kOutlookCols; ++k) v[k] += agg[(size_t)c * kOutlookCols + k];
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kOutlookCols; ++k) {
    const unsigned long long sum = wave_sum_u64(v[k]);
    if (lane == 0) out[(size_t)q * kOutlookCols + k] = sum;
  }
}

// hist: [2][bins] (entries | rows), cleared by the host; bins = 64 * env_words + 1. |W| is the
// device's (ws->count), never more than max_waiting entries are read. n_imm == NULL (no rpc stream):
// an entry is one row. The grid may be any size (a stride loop covers W).
__global__ __launch_bounds__(256) void k_outlook_waiting(const uint32_t* env, const uint32_t* n_imm,
                                                         const uint32_t* n_pre, const WaitState* ws,
                                                         uint32_t max_waiting, uint32_t bins, uint32_t* hist) {
  __shared__ uint32_t s_hist[2 * kOutlookLdsBins];
  const bool lds = bins <= kOutlookLdsBins;  // (uniform)
  if (lds) {
    for (uint32_t i = threadIdx.x; i < 2 * bins; i += blockDim.x) s_hist[i] = 0;
    __syncthreads();
  }
  const uint32_t n = min(ws->count, max_waiting);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t b = min(env[i], bins - 1);
    const uint32_t rows = n_imm ? n_imm[i] + n_pre[i] : 1u;
    if (lds) {
      atomicAdd(&s_hist[b], 1u);
      if (rows) atomicAdd(&s_hist[bins + b], rows);
    } else {
      atomicAdd(&hist[b], 1u);
      if (rows) atomicAdd(&hist[bins + b], rows);
    }
  }
  if (lds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * bins; i += blockDim.x) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(&hist[i], v);
    }
  }
}

// k_inspect_pack's shape: ceil(slots / kLeaseTile) workgroups, thread i owns four consecutive slots
// (one 16-byte load of their states). hist: [2][bins] (leases | zombies), cleared by the host. Live
// slots only; a zombie counts in both. A record without a digest (YDC_INSPECT_NO_ID) lands in the
// last bin.
__global__ __launch_bounds__(256) void k_outlook_leases(LeaseCols L, const uint4* rec, uint32_t bins, uint32_t* hist) {
  __shared__ uint32_t s_hist[2 * kOutlookLdsBins];
  const bool lds = bins <= kOutlookLdsBins;  // (uniform)
  if (lds) {
    for (uint32_t i = threadIdx.x; i < 2 * bins; i += blockDim.x) s_hist[i] = 0;
    __syncthreads();
  }
  const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const uint4 sv = lease_states4(L, i0);
  const uint32_t st4[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(st4[k] & kLeaseLive)) continue;
    const uint32_t b = min(rec[i0 + k].z, bins - 1);
    const bool zombie = (st4[k] & kLeaseZombie) != 0;
    if (lds) {
      atomicAdd(&s_hist[b], 1u);
      if (zombie) atomicAdd(&s_hist[bins + b], 1u);
    } else {
      atomicAdd(&hist[b], 1u);
      if (zombie) atomicAdd(&hist[bins + b], 1u);
    }
  }
  if (lds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * bins; i += blockDim.x) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(&hist[i], v);
    }
  }
}

}  // namespace ydc

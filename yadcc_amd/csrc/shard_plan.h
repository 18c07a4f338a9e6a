// shard_plan.h — the arithmetic of a sharded batch (ydc_dispatch_sharded) that every rank of a
// group has to decide identically: whether the slot sort is windowed, how large a window is, how
// many matching passes go out before the host looks, which pass was the first without a change,
// and how the replicated fallback slices the gathered batch. Plain integers in, plain integers
// out; host-only and free of HIP, so that a plain C++ program can drive it
// (tests/native/shard_plan_test.cc). A rank that computed any of these differently would issue
// other exchanges than its peers and the group would wait in-stream for ever.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace ydc {

// The sharded sort (k_key_count / k_window) is taken for integer keys, one part, a servant per
// host, at least 2 classes of a registry the wave path takes, in a group of several ranks — unless
// the registry is small enough for the bin sort and the group prefers that. Decided from the
// registry and the options alone, never from a rank's slice.
struct WindowedInputs {
  uint32_t n_ranks = 0, n_parts = 0, n_classes = 0;
  bool shard_sort = false;     // YDC_SHARD_SORT
  bool exact_keys = false;     // integer sort keys
  bool use_generic = false;    // > 256 classes: the replicated fallback
  bool any_shared = false;     // hosts with several servants
  bool binsort = false;        // the full plan bin-sorts the registry ...
  bool group_binsort = false;  // ... and YDC_GROUP_BINSORT lets a group do so
};
inline bool shard_windowed(const WindowedInputs& w) {
  return w.n_ranks > 1 && w.shard_sort && w.exact_keys && w.n_parts == 1 && !w.use_generic && w.n_classes >= 2 &&
         !w.any_shared && !(w.binsort && w.group_binsort);
}

// Slots of a rank's window: its requests + a margin on both sides (classes run ahead of or
// behind the global level) + the granularity of the thresholds, and never more than the registry
// has. tuned_margin < 0: unset, the margin is margin_scale * max(N / 8, 8192).
struct ShardWindow {
  uint32_t win_margin = 0;  // saturates at 0x7FFFFFFF
  uint32_t slot_bound = 0;
  uint32_t sort_items = 0;  // keys per sort thread: 2 / 4 / 8
  uint32_t n_tiles = 0;     // sort tiles of sort_threads * sort_items slots, at least 1
};
inline ShardWindow shard_window(uint32_t N, uint32_t margin_scale, int64_t tuned_margin, uint32_t full_slot_bound,
                                uint32_t sort_threads) {
  const uint64_t margin =
      tuned_margin >= 0 ? (uint64_t)tuned_margin : (uint64_t)margin_scale * std::max<uint64_t>(N / 8, 8192);
  const uint64_t bound =
      std::min<uint64_t>(full_slot_bound, (uint64_t)N + 2 * margin + full_slot_bound / 8 + 65536);
  ShardWindow w;
  w.win_margin = (uint32_t)std::min<uint64_t>(margin, 0x7FFFFFFFu);
  w.slot_bound = (uint32_t)bound;
  w.sort_items = w.slot_bound <= 300000 ? 2 : (w.slot_bound <= 700000 ? 4 : 8);
  const uint64_t tile = (uint64_t)sort_threads * w.sort_items;
  w.n_tiles = (uint32_t)std::max<uint64_t>(1, ((uint64_t)w.slot_bound + tile - 1) / tile);
  return w;
}

// A missed window doubles the margins of the batches to come, up to 64 times the default.
inline uint32_t shard_margin_after_miss(uint32_t margin_scale) { return std::min<uint32_t>(margin_scale * 2, 64u); }

// Matching passes pre-launched before the host looks at the outcome: as many as the last batch
// needed (2 .. 12) at first, 3 at a time after that.
inline uint32_t shard_pass_group(uint32_t launched, uint32_t pass_hint) {
  return launched == 0 ? std::max(2u, std::min(pass_hint, 12u)) : 3u;
}

// n_changed: DeviceParams' ring of 64 per-pass counts. Of the passes [first, first + count) — the
// last of which changed nothing — the number of passes up to and including the first in which no
// rank changed anything.
inline uint32_t shard_rounds(const uint32_t* n_changed, uint32_t first, uint32_t count) {
  for (uint32_t r = first; r < first + count; ++r)
    if (n_changed[r & 63] == 0) return r + 1;
  return first + count;
}

// Replicated fallback: from the ranks' slice sizes, the padded slice every rank sends (at least
// one word), the size of the whole batch and where this rank's slice begins in it.
struct ShardSlices {
  uint32_t max_n = 1, total = 0, my_off = 0;
};
inline ShardSlices shard_slices(const uint32_t* sizes, uint32_t n_ranks, uint32_t rank) {
  ShardSlices s;
  for (uint32_t r = 0; r < n_ranks; ++r) {
    s.max_n = std::max(s.max_n, sizes[r]);
    if (r < rank) s.my_off += sizes[r];
    s.total += sizes[r];
  }
  return s;
}

}  // namespace ydc

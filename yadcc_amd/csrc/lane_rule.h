// Which device lane a pipelined batch takes (ydc_dispatch_device_async). A lane is a stream plus
// everything one batch writes on the device; lane 0 is the context as it always was, lane 1 exists
// from the first batch sent to it. Two batches on different lanes run beside each other with no
// ordering between them on the device, so a batch only leaves lane 0 when nothing can tell the
// difference: the rule below, free of HIP (tests/native/lane_rule_test.cc).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ydc {

struct LaneOutput {
  const void* p = nullptr;  // NULL: not asked for
  size_t bytes = 0;
};

// What the rule needs to know of a batch.
struct LaneBatch {
  bool commit = false;    // YDC_DISPATCH_COMMIT
  bool enqueued = true;   // its launches are (or will be) in a stream: not left to be placed when waited for
  uint32_t lane = 0;      // (of an outstanding batch)
  LaneOutput out[3];      // out_idx, out_util, out_running
};

// ... and of the context.
struct LaneContext {
  bool lanes_on = true;       // YDC_TUNE lanes
  bool owns_stream = true;    // a caller's stream orders the caller's own work behind the batches: lane 0 only
  bool in_group = false;
  bool streaming = false;
  bool lane0_settled = false;  // a lane-0 batch was seen complete since the registry was last written
};

struct LaneChoice {
  uint32_t lane = 0;
  bool wait_first = false;  // the host waits for the outstanding batch's event before it enqueues
};

inline bool lane_ranges_overlap(const LaneOutput& a, const LaneOutput& b) {
  if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

inline bool lane_outputs_alias(const LaneBatch& a, const LaneBatch& b) {
  for (const LaneOutput& x : a.out)
    for (const LaneOutput& y : b.out)
      if (lane_ranges_overlap(x, y)) return true;
  return false;
}

// Whether `next` may run beside the outstanding batch `a`.
inline bool lane_independent(const LaneContext& c, const LaneBatch& a, const LaneBatch& next) {
  return c.lanes_on && c.owns_stream && !c.in_group && !c.streaming && c.lane0_settled && !a.commit &&
         !next.commit && a.enqueued && next.enqueued && !lane_outputs_alias(a, next);
}

// outstanding: the one batch that is outstanding when `next` is enqueued, or NULL.
inline LaneChoice lane_for(const LaneContext& c, const LaneBatch* outstanding, const LaneBatch& next) {
  LaneChoice r;
  if (!outstanding) return r;
  if (lane_independent(c, *outstanding, next)) {
    r.lane = outstanding->lane ^ 1u;
    return r;
  }
  // Behind it on lane 0, as ever; a batch on lane 1 is waited for first (no event between the lanes).
  r.wait_first = outstanding->lane == 1 && outstanding->enqueued;
  return r;
}

}  // namespace ydc

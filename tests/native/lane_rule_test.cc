// The lane-choice rule of the pipelined batches (yadcc_amd/csrc/lane_rule.h), row by row, as a
// program of its own: built with the host sanitizers (`make lanerule`; tests/test_lane_rule.py),
// no GPU, no HIP.
#include <cstdint>
#include <cstdio>

#include "lane_rule.h"

using namespace ydc;

static int g_failed = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    ++g_failed;
    std::printf("FAILED: %s\n", what);
  }
}

static bool is(const LaneChoice& c, uint32_t lane, bool wait_first) {
  return c.lane == lane && c.wait_first == wait_first;
}

// A batch of n requests on s servants with its three outputs at the given addresses.
static LaneBatch batch(uint32_t lane, uintptr_t idx, uintptr_t util, uintptr_t run, size_t n = 100, size_t s = 10) {
  LaneBatch b;
  b.lane = lane;
  b.out[0] = LaneOutput{(const void*)idx, n * 4};
  b.out[1] = LaneOutput{(const void*)util, n * 8};
  b.out[2] = LaneOutput{(const void*)run, s * 4};
  return b;
}

int main() {
  LaneContext ok;  // lanes on, own stream, no group, no streaming ...
  ok.lane0_settled = true;

  const LaneBatch a0 = batch(0, 0x10000, 0x20000, 0x30000);
  const LaneBatch a1 = batch(1, 0x10000, 0x20000, 0x30000);
  const LaneBatch b = batch(0, 0x50000, 0x60000, 0x70000);

  // Nothing outstanding: lane 0, whatever else holds.
  expect(is(lane_for(ok, nullptr, b), 0, false), "nothing outstanding -> lane 0");
  {
    LaneContext off = ok;
    off.lanes_on = false;
    LaneBatch commit = b;
    commit.commit = true;
    expect(is(lane_for(off, nullptr, commit), 0, false), "nothing outstanding, lanes off, COMMIT -> lane 0");
  }

  // Independent: the lane the outstanding batch is not on.
  expect(is(lane_for(ok, &a0, b), 1, false), "independent of a batch on lane 0 -> lane 1");
  expect(is(lane_for(ok, &a1, b), 0, false), "independent of a batch on lane 1 -> lane 0, no wait");

  // Every single reason not to be independent: lane 0; behind lane 1 the host waits first.
  struct Row {
    const char* name;
    LaneContext c;
    LaneBatch a, n;
  };
  auto row = [&](const char* name) { return Row{name, ok, a0, b}; };
  Row rows[12];
  int k = 0;
  rows[k] = row("outstanding has COMMIT"), rows[k++].a.commit = true;
  rows[k] = row("new has COMMIT"), rows[k++].n.commit = true;
  rows[k] = row("same out_idx"), rows[k++].n.out[0].p = a0.out[0].p;
  rows[k] = row("same out_util"), rows[k++].n.out[1].p = a0.out[1].p;
  rows[k] = row("same out_running"), rows[k++].n.out[2].p = a0.out[2].p;
  // (the new out_running starts inside the outstanding out_idx; the new out_idx ends inside its out_util)
  rows[k] = row("out_running inside the other's out_idx"), rows[k++].n.out[2].p = (const void*)(0x10000 + 396);
  rows[k] = row("out_idx overlapping the other's out_util"), rows[k++].n.out[0].p = (const void*)(0x20000 - 4);
  rows[k] = row("new is not enqueued (placed when waited for)"), rows[k++].n.enqueued = false;
  rows[k] = row("a caller's stream"), rows[k++].c.owns_stream = false;
  rows[k] = row("in a group"), rows[k++].c.in_group = true;
  rows[k] = row("streaming"), rows[k++].c.streaming = true;
  rows[k] = row("lane 0 not settled"), rows[k++].c.lane0_settled = false;
  for (int i = 0; i < k; ++i) {
    Row r = rows[i];
    r.a.lane = 0;
    expect(is(lane_for(r.c, &r.a, r.n), 0, false), r.name);
    r.a.lane = 1;
    expect(is(lane_for(r.c, &r.a, r.n), 0, true), r.name);
  }
  {
    LaneContext off = ok;
    off.lanes_on = false;
    expect(is(lane_for(off, &a0, b), 0, false), "lanes=0 -> lane 0");
    expect(is(lane_for(off, &a1, b), 0, true), "lanes=0 behind lane 1 (cannot arise) -> lane 0, waits");
  }
  {
    // The outstanding batch was never enqueued (it is placed when it is waited for): the new one
    // stays behind it on lane 0, and there is no event to wait for.
    LaneBatch r0 = a0, r1 = a1;
    r0.enqueued = r1.enqueued = false;
    expect(is(lane_for(ok, &r0, b), 0, false), "behind a batch that is to be replayed -> lane 0");
    expect(is(lane_for(ok, &r1, b), 0, false), "behind a replay that was on lane 1 -> lane 0, nothing to wait for");
  }

  // Outputs that do not alias: adjacent ranges, outputs not asked for, empty ranges.
  {
    LaneBatch n = b;
    n.out[0].p = (const void*)(0x10000 + 400);  // right behind the outstanding out_idx
    expect(is(lane_for(ok, &a0, n), 1, false), "adjacent ranges do not alias");
    n = b;
    n.out[1] = LaneOutput{};
    n.out[2] = LaneOutput{};
    LaneBatch a = a0;
    a.out[1] = LaneOutput{};
    expect(is(lane_for(ok, &a, n), 1, false), "outputs not asked for do not alias");
    n = b;
    n.out[0] = LaneOutput{a0.out[0].p, 0};
    expect(is(lane_for(ok, &a0, n), 1, false), "an empty range does not alias");
  }
  expect(lane_ranges_overlap(LaneOutput{(const void*)100, 10}, LaneOutput{(const void*)109, 1}), "last byte overlaps");
  expect(!lane_ranges_overlap(LaneOutput{(const void*)100, 10}, LaneOutput{(const void*)110, 1}), "one past the end does not");

  if (g_failed) return 1;
  std::printf("LANE-RULE-OK\n");
  return 0;
}

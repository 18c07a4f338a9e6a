// occupancy_plan.h — how much of a CU a batch's launches ask for, where the work leaves a choice:
// the width of a k_bin_sort workgroup. Pipelined batches run beside each other on two lanes
// (lane_rule.h), and these kernels are latency-bound: what slows them next to a neighbour is a
// workgroup waiting for wave slots, registers or LDS on a CU, so a batch that may
// have a neighbour takes no more than it needs. Plain integers in, plain integers out; free of
// HIP, so that a plain C++ program can drive it (tests/native/occupancy_plan_test.cc).
#pragma once

#include <cstdint>

namespace ydc {

// Threads of a k_bin_sort workgroup (bin_sort.h builds 512 and 1024; a bin holds <= 4096 records
// either way). Two wide workgroups are a CU's 32 wave slots: beside another batch the second one
// does not fit and whatever arrives behind them waits; two narrow ones fit next to the other
// lane's matching waves. On a device of its own the wide one is the faster by about a microsecond
// (half the rounds per thread). beside: the batch may have a neighbour on the other lane (enqueued
// by ydc_dispatch_device_async of a context that uses lanes). tuned: YDC_TUNE bin_threads; 0 or
// a width no build has: the rule.
constexpr uint32_t kBinThreadsNarrow = 512, kBinThreadsWide = 1024;
constexpr uint32_t bin_sort_threads(uint32_t tuned, bool beside) {
  return tuned == kBinThreadsNarrow || tuned == kBinThreadsWide ? tuned
                                                                 : (beside ? kBinThreadsNarrow : kBinThreadsWide);
}

}  // namespace ydc

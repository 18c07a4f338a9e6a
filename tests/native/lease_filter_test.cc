// The predicate of ydc_stream_inspect_select (yadcc_amd/csrc/lease_filter.h) against a second
// restatement of its rule, without a GPU: all 2^9 combinations of the nine predicates, each over
// every row of a grid of edge values (the sentinels, 0, the extremes, values one off the filter's).
// Includes only lease_filter.h; built with ASan + UBSan and run as a program of its own
// (tests/test_stream_select_binding.py, `make leasefilter`).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lease_filter.h"

using namespace ydc;

namespace {

// The rule, written the other way round: every reason to REJECT a row is collected, then counted.
bool restated(const LeaseFilter& f, const LeaseRow& r) {
  const bool attributed = r.started_at != INT64_MIN;
  int reasons = 0;
  for (uint32_t bit = 1; bit <= 0x100u; bit <<= 1) {
    if (!(f.fields & bit)) continue;
    switch (bit) {
      case 0x001u: reasons += r.servant == f.servant_idx ? 0 : 1; break;
      case 0x002u: reasons += (r.zombie ? 1 : 0) == f.zombie ? 0 : 1; break;
      case 0x004u: reasons += r.expires_at >= f.expires_before ? 1 : 0; break;
      case 0x008u: reasons += r.id <= f.after_id ? 1 : 0; break;
      case 0x010u: reasons += attributed && r.env_id == f.env_id ? 0 : 1; break;
      case 0x020u: reasons += attributed && r.requestor_ip == f.requestor_ip ? 0 : 1; break;
      case 0x040u: reasons += attributed && (r.prefetch ? 1 : 0) == f.prefetch ? 0 : 1; break;
      case 0x080u: reasons += attributed && r.started_at < f.started_before ? 0 : 1; break;
      case 0x100u: reasons += !attributed && !(f.fields & 0x0F0u) ? 0 : 1; break;
    }
  }
  return reasons == 0;
}

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    ++failures;
    printf("FAIL: %s\n", what);
  }
}

}  // namespace

int main() {
  const uint64_t ids[] = {0, 1, 255, 256, (1ull << 32) - 1, 1ull << 32, (1ull << 56) + 5, ~0ull - 1};
  const int64_t times[] = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, 1000, INT64_MAX - 1, INT64_MAX};
  const uint32_t keys[] = {0, 1, 7, 0xFFFFFFFEu, 0xFFFFFFFFu};
  std::vector<LeaseRow> grid;
  for (uint64_t id : ids)
    for (int64_t exp : {times[0], times[5], times[7]})
      for (int64_t started : {times[0], times[1], times[3], times[5], times[7]})
        for (uint32_t key : {keys[0], keys[2], keys[4]})
          for (int flags = 0; flags < 4; ++flags)
            grid.push_back(LeaseRow{id, exp, started, key, key ^ 1u, ~key, (flags & 1) != 0, (flags & 2) != 0});
  // Filters: every subset of the predicates, with values that sit on the grid's edges.
  std::vector<LeaseFilter> values;
  for (uint32_t key : {keys[0], keys[2], keys[4]})
    for (int64_t t : {times[0], times[1], times[5], times[7]})
      for (uint64_t after : {ids[0], ids[5], ~(uint64_t)0})
        for (uint8_t flag = 0; flag < 2; ++flag) {
          LeaseFilter f{};
          f.servant_idx = key;
          f.env_id = key ^ 1u;
          f.requestor_ip = ~key;
          f.zombie = flag;
          f.prefetch = (uint8_t)(1 - flag);
          f.expires_before = t;
          f.started_before = t;
          f.after_id = after;
          values.push_back(f);
        }
  unsigned long long checked = 0, matched = 0;
  for (uint32_t fields = 0; fields < 512; ++fields)
    for (LeaseFilter f : values) {
      f.fields = fields;
      if (!lease_filter_valid(f)) {
        expect(false, "a filter of known bits and flags 0 / 1 was called invalid");
        continue;
      }
      for (const LeaseRow& r : grid) {
        const bool got = lease_filter_match(f, r), want = restated(f, r);
        ++checked;
        matched += got;
        if (got != want) {
          ++failures;
          if (failures < 20)
            printf("FAIL: fields 0x%x id %llu started %lld: header %d restatement %d\n", fields, (unsigned long long)r.id,
                   (long long)r.started_at, (int)got, (int)want);
        }
      }
    }
  // What the header refuses.
  LeaseFilter bad{};
  bad.fields = 0x200u;
  expect(!lease_filter_valid(bad), "an unknown bit");
  bad.fields = 0x80000000u;
  expect(!lease_filter_valid(bad), "the top bit");
  bad = LeaseFilter{};
  bad.fields = kSelZombie;
  bad.zombie = 2;
  expect(!lease_filter_valid(bad), "zombie = 2 where selected");
  bad.fields = kSelServant;
  expect(lease_filter_valid(bad), "zombie = 2 where it is not selected");
  bad = LeaseFilter{};
  bad.fields = kSelPrefetch;
  bad.prefetch = 255;
  expect(!lease_filter_valid(bad), "prefetch = 255 where selected");
  // The rows of the issue, by hand.
  const LeaseRow un{5, 10, INT64_MIN, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, false, false};
  const LeaseRow at{6, 10, 3, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, false, true};
  LeaseFilter f{};
  expect(lease_filter_match(f, un) && lease_filter_match(f, at), "the empty filter matches every lease");
  f.fields = kSelRequestor;
  f.requestor_ip = 0xFFFFFFFFu;
  expect(!lease_filter_match(f, un) && lease_filter_match(f, at), "0xFFFFFFFF is an ordinary key; the sentinel record is nobody's");
  f.fields = kSelUnattributed;
  expect(lease_filter_match(f, un) && !lease_filter_match(f, at), "UNATTRIBUTED selects by started_at");
  f.fields = kSelUnattributed | kSelRequestor;
  expect(!lease_filter_match(f, un) && !lease_filter_match(f, at), "UNATTRIBUTED with REQUESTOR matches nothing");
  f.fields = kSelPrefetch;
  f.prefetch = 0;
  expect(!lease_filter_match(f, un), "an unattributed lease's prefetch = 0 says nothing");
  f.fields = kSelExpiresBefore;
  f.expires_before = INT64_MIN;
  expect(!lease_filter_match(f, at), "nothing expires before INT64_MIN");
  f.expires_before = INT64_MAX;
  expect(lease_filter_match(f, at), "10 < INT64_MAX");
  static_assert(sizeof(LeaseFilter) == 48 && alignof(LeaseFilter) == 8, "ydc_lease_filter");
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("LEASE-FILTER-OK %llu evaluations, %llu matches\n", checked, matched);
  return 0;
}

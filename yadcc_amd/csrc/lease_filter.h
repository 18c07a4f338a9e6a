// lease_filter.h — the predicate of ydc_stream_inspect_select / ydc_stream_inspect_count (DESIGN
// 3.3.16). Plain C++, no HIP, no context: the kernels of stream_select.h evaluate it per live slot of
// the lease table, the host checks a caller's filter with it, and a stand-alone host program sweeps it
// (tests/native/lease_filter_test.cc).
//
// A row of the lease table as ydc_stream_inspect_tasks reports it: id, servant, expires_at, the
// zombie bit, and the inspection record started_at | env_id | requestor_ip | prefetch (the sentinels
// of stream_inspect.h for a lease granted while inspection was off, or with inspection off). A filter
// is a conjunction: every predicate whose bit is set in `fields` has to hold.
//
//   SERVANT, ZOMBIE, EXPIRES_BEFORE, AFTER_ID   the table's own columns.
//   ENV, REQUESTOR, PREFETCH, STARTED_BEFORE    the record's columns. A lease whose started_at is
//                                               kFilterNoTime is unattributed and satisfies none of
//                                               them: its env_id / requestor_ip are not keys (all 2^32
//                                               values are ordinary keys of attributed leases), its
//                                               prefetch and started_at say nothing.
//   UNATTRIBUTED                                started_at == kFilterNoTime; together with any of the
//                                               four above it matches nothing.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YDC_FILTER_HD __host__ __device__
#else
#define YDC_FILTER_HD
#endif

namespace ydc {

constexpr uint32_t kSelServant = 0x001u, kSelZombie = 0x002u, kSelExpiresBefore = 0x004u, kSelAfterId = 0x008u,
                   kSelEnv = 0x010u, kSelRequestor = 0x020u, kSelPrefetch = 0x040u, kSelStartedBefore = 0x080u,
                   kSelUnattributed = 0x100u;
constexpr uint32_t kSelTable = kSelServant | kSelZombie | kSelExpiresBefore | kSelAfterId;
constexpr uint32_t kSelAttributed = kSelEnv | kSelRequestor | kSelPrefetch | kSelStartedBefore;
constexpr uint32_t kSelRecord = kSelAttributed | kSelUnattributed;
constexpr uint32_t kSelAll = kSelTable | kSelRecord;
constexpr uint32_t kSelectMaxFilters = 64;
constexpr int64_t kFilterNoTime = INT64_MIN;  // YDC_INSPECT_NO_TIME

// ydc_lease_filter.
struct LeaseFilter {
  uint32_t fields;
  uint32_t servant_idx, env_id, requestor_ip;
  uint8_t zombie, prefetch, pad[2];
  int64_t expires_before, started_before;
  uint64_t after_id;
};
static_assert(sizeof(LeaseFilter) == 48, "ydc_lease_filter is 48 bytes");

// One row of T.
struct LeaseRow {
  uint64_t id;
  int64_t expires_at, started_at;
  uint32_t servant, env_id, requestor_ip;
  bool zombie, prefetch;
};

// What a caller may not ask: an unknown bit, a flag that is neither 0 nor 1 where it is selected.
YDC_FILTER_HD inline bool lease_filter_valid(const LeaseFilter& f) {
  if (f.fields & ~kSelAll) return false;
  if ((f.fields & kSelZombie) && f.zombie > 1) return false;
  if ((f.fields & kSelPrefetch) && f.prefetch > 1) return false;
  return true;
}

// Columns a predicate does not select are not looked at: a caller may leave them unset.
YDC_FILTER_HD inline bool lease_filter_match(const LeaseFilter& f, const LeaseRow& r) {
  const uint32_t w = f.fields;
  if ((w & kSelServant) && r.servant != f.servant_idx) return false;
  if ((w & kSelZombie) && r.zombie != (f.zombie != 0)) return false;
  if ((w & kSelExpiresBefore) && !(r.expires_at < f.expires_before)) return false;
  if ((w & kSelAfterId) && !(r.id > f.after_id)) return false;
  if (w & kSelRecord) {
    const bool attributed = r.started_at != kFilterNoTime;
    if (w & kSelUnattributed) {
      if (attributed || (w & kSelAttributed)) return false;
    } else if (!attributed) {
      return false;
    }
    if ((w & kSelEnv) && r.env_id != f.env_id) return false;
    if ((w & kSelRequestor) && r.requestor_ip != f.requestor_ip) return false;
    if ((w & kSelPrefetch) && r.prefetch != (f.prefetch != 0)) return false;
    if ((w & kSelStartedBefore) && !(r.started_at < f.started_before)) return false;
  }
  return true;
}

}  // namespace ydc

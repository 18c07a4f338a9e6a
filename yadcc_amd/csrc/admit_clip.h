// admit_clip.h — the admission arithmetic that goes with the load per requestor (ydc_admit_clip;
// DESIGN 3.3.13). Plain C++, no HIP, no context: a scheduler calls it between assembling a tick and
// sending it, with the rows of ydc_stream_requestor_find beside the tick's requests.
//
// The reference answers a failed grant STATUS_NO_QUOTA_AVAILABLE (scheduler_service_impl.cc:266-269)
// but keeps no quota. Here requestor r may have `cap` grants outstanding:
//   room(r) = max(cap - min(cap, leases + waiting_rows), 0)
// (zombies are inside leases and count: they still hold slots). Rows are in arrival order. With
// pre_i the sum of n_immediate + n_prefetch over the EARLIER rows of the same requestor and want_i
// the row's own sum, row i is admitted
//   a_i = min(pre_i + want_i, room) - min(pre_i, room)
// grants: out_immediate = min(n_immediate, a_i), out_prefetch = a_i - out_immediate, so prefetch is
// clipped first. Rows of different requestors never interact.
//
// Sums are 64-bit. pre_i only ever enters as min(pre_i, room) with room < 2^32, so it is carried
// saturated at 2^62 (a row adds less than 2^33): no input makes an intermediate wrap.
//
// The rule itself — admit_room_of, admit_rows, admit_split — is written once, for the host loop below
// and for the tick's own clip on the device (stream_quota.h), which instantiates it
// with 32-bit sums: there pre + want < 2^31 (an accepted tick's rows) and held < 2^31.
#pragma once
#include <stdint.h>

#include <unordered_map>

#if defined(__HIPCC__)
#define YDC_ADMIT_HD __host__ __device__
#else
#define YDC_ADMIT_HD
#endif

namespace ydc {

// room = cap - min(cap, held).
template <class T>
YDC_ADMIT_HD inline T admit_room_of(T cap, T held) {
  return cap - (held < cap ? held : cap);
}

// a = min(pre + want, room) - min(pre, room). The caller sees to it that pre + want does not wrap.
template <class T>
YDC_ADMIT_HD inline T admit_rows(T pre, T want, T room) {
  const T before = pre < room ? pre : room;
  const T after = pre + want < room ? pre + want : room;
  return after - before;
}

// Prefetch is clipped first: of `a` admitted grants the immediate ones come first.
YDC_ADMIT_HD inline uint32_t admit_split(uint32_t n_immediate, uint64_t a) {
  return n_immediate < a ? n_immediate : (uint32_t)a;
}

// ydc_requestor_load.
struct AdmitLoad {
  uint32_t requestor_ip;
  uint32_t leases, zombies, prefetch_leases;
  uint32_t waiting, waiting_rows;
};
static_assert(sizeof(AdmitLoad) == 24, "ydc_requestor_load is 24 bytes");

constexpr uint32_t kAdmitUnknown = 0xFFFFFFFFu;  // YDC_REQUESTOR_UNKNOWN
constexpr uint64_t kAdmitSaturated = 1ull << 62;

inline uint64_t admit_room(const AdmitLoad& l, uint32_t cap) {
  return admit_room_of<uint64_t>(cap, (uint64_t)l.leases + (uint64_t)l.waiting_rows);
}

// false: a load with unknown lease columns (nothing is written then). n_prefetch == NULL: zeros.
inline bool admit_clip(const uint32_t* requestor_ip, const uint32_t* n_immediate, const uint32_t* n_prefetch, uint32_t n,
                       const AdmitLoad* load, uint32_t cap, uint32_t* out_immediate, uint32_t* out_prefetch) {
  for (uint32_t i = 0; i < n; ++i)
    if (load[i].leases == kAdmitUnknown) return false;
  std::unordered_map<uint32_t, uint64_t> asked;  // per requestor: pre_i, saturated
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t room = admit_room(load[i], cap);
    const uint64_t want = (uint64_t)n_immediate[i] + (n_prefetch ? (uint64_t)n_prefetch[i] : 0u);
    uint64_t& pre = asked[requestor_ip[i]];
    const uint64_t a = admit_rows<uint64_t>(pre, want, room);
    pre = pre + want < kAdmitSaturated ? pre + want : kAdmitSaturated;
    const uint32_t imm = admit_split(n_immediate[i], a);
    out_immediate[i] = imm;
    if (out_prefetch) out_prefetch[i] = (uint32_t)(a - imm);
  }
  return true;
}

}  // namespace ydc

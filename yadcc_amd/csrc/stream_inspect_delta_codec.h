// stream_inspect_delta_codec.h — the byte format of ydc_stream_delta_inspect / ydc_stream_inspect_restore /
// ydc_stream_delta_apply_inspected.
//
// Host only, no HIP: the layout of an inspection sidecar, the validation of a block of untrusted bytes
// and the building of one from columns. A sidecar lies beside a full snapshot (kind 0: the record of
// every lease of L) or beside a delta (kind 1: the records of the delta's inserted leases) and carries
// what those blobs leave out of a stream with inspection (stream_inspect.h). It is a header of 120
// bytes, then two sections, each a run of whole columns (SoA) padded with zero bytes to a multiple of 8:
//
//   records   id u64[n] | started_at i64[n] | env_id u32[n] | requestor_ip u32[n] | prefetch u8[n]
//             (ascending id)
//   servants  discovered_at i64[s] | ever_assigned u64[s], whole
//
// so a sidecar of n records over s servants weighs 120 + 8n + 8n + 4n + 4n + pad8(n) + 16s bytes. The
// header names the state the sidecar describes (lease_tick, next_id, |L|, last_now and the structure
// stamp of stream_delta_codec.h): for kind 1 the state that results from its delta. The inspection
// epoch counts the calls that rewrite records of leases that exist already (ydc_stream_inspect_begin,
// ydc_stream_inspect_load): a delta sidecar continues a full one only under the same epoch. The ids
// are carried and not implied, so that a sidecar can be read alone and checked against its delta byte
// for byte. One state has exactly one encoding.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "stream_snapshot_codec.h"

namespace ydc {
namespace insd {

constexpr uint64_t kMagic = 0x3144534E49434459ull;  // "YDCINSD1"
constexpr uint32_t kVersion = 1;
enum Kind : uint32_t { kFull = 0, kDelta = 1 };
enum Section { kRecords = 0, kServants, kSections };

struct Header {
  uint64_t magic;
  uint32_t version, header_bytes;
  uint64_t total_bytes;
  uint64_t checksum;  // snap::checksum of the whole block, this field read as 0 (word 3, as in a snapshot)
  uint32_t kind, n_servants, n, reserved;  // n: the records carried
  // The state the sidecar describes.
  uint64_t stamp;
  uint64_t next_id;
  int64_t last_now;
  uint32_t lease_tick, n_leases;  // |L|
  uint64_t epoch;
  struct {
    uint64_t offset, bytes;
  } dir[kSections];
};
static_assert(sizeof(Header) == 120, "inspection sidecar header layout");
static_assert(offsetof(Header, checksum) == offsetof(snap::Header, checksum), "snap::checksum skips this word");

using snap::get;
using snap::pad8;

// Bytes in use of every section, as the header's counts imply them (the section is that, padded to 8).
inline void section_used(const Header& h, uint64_t out[kSections]) {
  out[kRecords] = (uint64_t)h.n * 25;
  out[kServants] = (uint64_t)h.n_servants * 16;
}

// Fills the directory and total_bytes from the counts.
inline void layout(Header* h) {
  uint64_t used[kSections], off = sizeof(Header);
  section_used(*h, used);
  for (int s = 0; s < kSections; ++s) {
    h->dir[s].offset = off;
    h->dir[s].bytes = pad8(used[s]);
    off += pad8(used[s]);
  }
  h->header_bytes = sizeof(Header);
  h->total_bytes = off;
}

// The columns of a sidecar, at their places in it (read through get<>(): the base may be any address).
struct View {
  Header h;
  const uint8_t* base;
  const uint8_t *id, *started_at, *env_id, *requestor_ip, *prefetch;
  const uint8_t *discovered_at, *ever_assigned;
};

inline void place(View* v, const uint8_t* base) {
  const Header& h = v->h;
  v->base = base;
  const uint64_t n = h.n;
  const uint8_t* p = base + h.dir[kRecords].offset;
  v->id = p, p += n * 8;
  v->started_at = p, p += n * 8;
  v->env_id = p, p += n * 4;
  v->requestor_ip = p, p += n * 4;
  v->prefetch = p;
  p = base + h.dir[kServants].offset;
  v->discovered_at = p, p += (uint64_t)h.n_servants * 8;
  v->ever_assigned = p;
}

// Checks `bytes` untrusted bytes. nullptr: a well-formed sidecar, *out describes it. Otherwise the reason.
// Nothing outside [blob, blob + bytes) is read.
inline const char* validate(const void* blob, size_t bytes, View* out) {
  if (!blob || bytes < sizeof(Header)) return "shorter than a header";
  Header& h = out->h;
  memcpy(&h, blob, sizeof(Header));
  if (h.magic != kMagic) return "not an inspection sidecar (magic)";
  if (h.version != kVersion) return "unknown format version";
  if (h.header_bytes != sizeof(Header)) return "header size";
  if (h.total_bytes != bytes) return "total bytes differ from the block's size";
  if (bytes % 8) return "size is no multiple of 8";
  if (h.kind > kDelta) return "unknown kind";
  if (h.reserved) return "a reserved field is set";
  if (h.lease_tick && !(h.lease_tick & snap::kStamp)) return "a tick number whose stamp is 0";
  if (h.n > h.n_leases) return "more records than leases";
  if (h.kind == kFull && h.n != h.n_leases) return "a full sidecar whose records are not |L|";
  if (h.n_leases > h.next_id) return "more leases than ids handed out";
  // The directory is what the counts imply, inside the block.
  uint64_t used[kSections], off = sizeof(Header);
  section_used(h, used);
  for (int s = 0; s < kSections; ++s) {
    const uint64_t sz = pad8(used[s]);
    if (h.dir[s].offset != off || h.dir[s].bytes != sz) return "a section is not where its counts put it";
    if (sz > bytes - off) return "a section reaches past the end";
    off += sz;
  }
  if (off != bytes) return "bytes behind the last section";
  if (snap::checksum(blob, bytes) != h.checksum) return "checksum";
  place(out, (const uint8_t*)blob);
  const View& v = *out;
  for (uint64_t i = 0; i < h.n; ++i) {
    const uint64_t id = get<uint64_t>(v.id, i);
    if (i && id <= get<uint64_t>(v.id, i - 1)) return "ids not ascending";
    if (id >= h.next_id) return "an id >= next_id";
    if (v.prefetch[i] > 1) return "a prefetch flag that is neither 0 nor 1";
  }
  // Padding is zero (one encoding per state).
  for (int s = 0; s < kSections; ++s)
    for (uint64_t i = used[s]; i < h.dir[s].bytes; ++i)
      if (v.base[h.dir[s].offset + i]) return "padding is not zero";
  return nullptr;
}

// Seals a sidecar whose header fields and columns are in place: the header with its checksum stored.
inline void seal(uint8_t* blob, Header* h) {
  h->checksum = 0;
  memcpy(blob, h, sizeof *h);
  h->checksum = snap::checksum(blob, h->total_bytes);
  memcpy(blob, h, sizeof *h);
}

// The header of a sidecar of `n` records over `n_servants` servants, laid out; the identity is the caller's.
inline Header describe(uint32_t kind, uint32_t n_servants, uint32_t n) {
  Header h;
  memset(&h, 0, sizeof h);
  h.magic = kMagic;
  h.version = kVersion;
  h.kind = kind, h.n_servants = n_servants, h.n = n;
  layout(&h);
  return h;
}

// The columns a sidecar is built from (h.n and h.n_servants entries; any address).
struct Columns {
  const void *id, *started_at, *env_id, *requestor_ip, *prefetch;
  const void *discovered_at, *ever_assigned;
};

// The sidecar of the header `h` (kind, counts and identity set; describe()) with the columns `c`.
inline void build(Header h, const Columns& c, std::vector<uint8_t>* out) {
  layout(&h);
  out->assign((size_t)h.total_bytes, 0);
  View v;
  v.h = h;
  place(&v, out->data());
  auto put = [](const uint8_t* to, const void* from, uint64_t bytes) {
    if (bytes) memcpy(const_cast<uint8_t*>(to), from, (size_t)bytes);
  };
  const uint64_t n = h.n, s = h.n_servants;
  put(v.id, c.id, n * 8);
  put(v.started_at, c.started_at, n * 8);
  put(v.env_id, c.env_id, n * 4);
  put(v.requestor_ip, c.requestor_ip, n * 4);
  put(v.prefetch, c.prefetch, n);
  put(v.discovered_at, c.discovered_at, s * 8);
  put(v.ever_assigned, c.ever_assigned, s * 8);
  seal(out->data(), &h);
}

}  // namespace insd
}  // namespace ydc

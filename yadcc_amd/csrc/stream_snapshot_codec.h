// stream_snapshot_codec.h — the byte format of ydc_stream_snapshot / ydc_stream_restore.
//
// Host only, no HIP: the layout of a blob, its checksum, and the validation of a block of untrusted
// bytes. A blob is a header, then up to five sections laid end to end in a fixed order, every
// section a run of whole columns (SoA) padded with zero bytes to a multiple of 8:
//
//   registry  env_mask u64[n * env_words] | version, num_processors, current_load, max_tasks, flags,
//             ip_id, running_tasks, rep_tick u32[n] each | alias ip_id u32[a] | alias servant u32[a]
//   L         id u64[|L|] | expires_at i64[|L|] | servant u32[|L|] | state u32[|L|]     (ascending id)
//   W         deadline i64[|W|] | tag u64[|W|] | lease_for i64[|W|] (leased) | env, min_version,
//             requestor ip u32[|W|] | n_immediate, n_prefetch u32[|W|] (rpc)              (queue order)
//   B         grant u64[|B|] | servant task id u64[|B|] | digest key u64[|B|] | servant u32[|B|]
//   E         expires_at i64[n]                                                      (aliveness only)
//
// Everything is little-endian; there are no pointers, no slot numbers and nothing of the table's
// geometry. The layout is canonical: a given state has exactly one encoding (the sections follow
// each other without gaps, padding is zero, the directory is implied by the counts and checked).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace ydc {
namespace snap {

constexpr uint64_t kMagic = 0x3150414E53434459ull;  // "YDCSNAP1"
constexpr uint32_t kVersion = 1;
constexpr uint32_t kModeWaiting = 1, kModeLeased = 2, kModeRpc = 4, kModeBook = 8, kModeAlive = 16;
constexpr uint32_t kMaxEnvWords = 64;  // (the API checks its own, smaller bound as well)
constexpr uint32_t kLive = 1u << 31, kStamp = (1u << 30) - 1;
enum Section { kRegistry = 0, kL, kW, kB, kE, kSections };

// The ten bounds in ydc_stream_caps' order.
enum Cap { kUpdates = 0, kReleases, kTasks, kRows, kWaiting, kLeases, kRenewals, kFrees, kReports, kReportIds, kCaps };

struct Header {
  uint64_t magic;
  uint32_t version, header_bytes;
  uint64_t total_bytes;
  uint64_t checksum;  // of the whole block, this field read as 0
  uint32_t mode, env_words, n_servants, n_alias;
  uint32_t caps[kCaps];
  uint32_t max_book;
  uint32_t n_leases, n_waiting, n_wait_rows, n_book;  // |L|, |W|, rows(W), |B|
  uint32_t lease_tick;
  uint64_t next_id;
  int64_t last_now;
  int64_t alive_bound;
  struct {
    uint64_t offset, bytes;
  } dir[kSections];
};
static_assert(sizeof(Header) == 216, "blob header layout");

inline uint64_t pad8(uint64_t b) { return (b + 7) & ~7ull; }

// Bytes of every section as the header's counts imply them (64-bit: no product of two 32-bit counts
// and a width overflows).
inline void section_bytes(const Header& h, uint64_t out[kSections]) {
  const uint64_t n = h.n_servants, w = h.n_waiting, l = h.n_leases, b = h.n_book;
  const bool leased = h.mode & kModeLeased, rpc = h.mode & kModeRpc;
  out[kRegistry] = pad8(n * h.env_words * 8 + n * 8 * 4 + (uint64_t)h.n_alias * 2 * 4);
  out[kL] = leased ? l * 24 : 0;
  out[kW] = (h.mode & kModeWaiting) ? pad8(w * (16 + (leased ? 8 : 0) + 12 + (rpc ? 8 : 0))) : 0;
  out[kB] = (h.mode & kModeBook) ? pad8(b * 28) : 0;
  out[kE] = (h.mode & kModeAlive) ? n * 8 : 0;
}

// Fills the directory and total_bytes from the counts.
inline void layout(Header* h) {
  uint64_t sz[kSections], off = sizeof(Header);
  section_bytes(*h, sz);
  for (int s = 0; s < kSections; ++s) {
    h->dir[s].offset = off;
    h->dir[s].bytes = sz[s];
    off += sz[s];
  }
  h->header_bytes = sizeof(Header);
  h->total_bytes = off;
}

// Sum over the 8-byte words of mix(word ^ index * phi), the checksum's own word read as 0. Every
// word's term is a bijection of the word: a change of any single word changes the sum.
inline uint64_t checksum(const void* blob, uint64_t bytes) {
  const uint8_t* p = (const uint8_t*)blob;
  uint64_t sum = 0;
  for (uint64_t i = 0; i * 8 < bytes; ++i) {
    uint64_t w;
    memcpy(&w, p + i * 8, 8);
    if (i == offsetof(Header, checksum) / 8) w = 0;
    uint64_t z = w ^ (i * 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    sum += z ^ (z >> 31);
  }
  return sum;
}

// The columns of a blob, at their places in it (unaligned access is never made: the block's base
// may be any address, so readers go through get<>()).
struct View {
  Header h;
  const uint8_t* base;
  // registry
  const uint8_t *env_mask, *version, *nproc, *load, *max_tasks, *flags, *ip, *running, *rep_tick, *alias_ip, *alias_servant;
  // L
  const uint8_t *l_id, *l_exp, *l_srv, *l_state;
  // W
  const uint8_t *w_deadline, *w_tag, *w_for, *w_env, *w_minv, *w_ip, *w_nimm, *w_npre;
  // B
  const uint8_t *b_grant, *b_stid, *b_dkey, *b_srv;
  // E
  const uint8_t* e_exp;
};

template <typename T>
inline T get(const uint8_t* col, uint64_t i) {
  T v;
  memcpy(&v, col + i * sizeof(T), sizeof(T));
  return v;
}

// The column pointers for a header whose layout has been checked (or made by layout()).
inline void place(View* v, const uint8_t* base) {
  const Header& h = v->h;
  v->base = base;
  const uint64_t n = h.n_servants, a = h.n_alias, l = h.n_leases, w = h.n_waiting, b = h.n_book;
  const bool leased = h.mode & kModeLeased, rpc = h.mode & kModeRpc;
  const uint8_t* p = base + h.dir[kRegistry].offset;
  v->env_mask = p, p += n * h.env_words * 8;
  const uint8_t** reg[] = {&v->version, &v->nproc, &v->load, &v->max_tasks, &v->flags, &v->ip, &v->running, &v->rep_tick};
  for (auto** col : reg) *col = p, p += n * 4;
  v->alias_ip = p, p += a * 4;
  v->alias_servant = p;
  p = base + h.dir[kL].offset;
  v->l_id = p, p += l * 8;
  v->l_exp = p, p += l * 8;
  v->l_srv = p, p += l * 4;
  v->l_state = p;
  p = base + h.dir[kW].offset;
  v->w_deadline = p, p += w * 8;
  v->w_tag = p, p += w * 8;
  v->w_for = p, p += leased ? w * 8 : 0;
  v->w_env = p, p += w * 4;
  v->w_minv = p, p += w * 4;
  v->w_ip = p, p += w * 4;
  v->w_nimm = p, p += rpc ? w * 4 : 0;
  v->w_npre = p;
  p = base + h.dir[kB].offset;
  v->b_grant = p, p += b * 8;
  v->b_stid = p, p += b * 8;
  v->b_dkey = p, p += b * 8;
  v->b_srv = p;
  v->e_exp = base + h.dir[kE].offset;
}

// Checks `bytes` untrusted bytes. nullptr: a well-formed blob, *out describes it. Otherwise the reason.
// Nothing outside [blob, blob + bytes) is read.
inline const char* validate(const void* blob, size_t bytes, View* out) {
  if (!blob || bytes < sizeof(Header)) return "shorter than a header";
  Header& h = out->h;
  memcpy(&h, blob, sizeof(Header));
  if (h.magic != kMagic) return "not a stream snapshot (magic)";
  if (h.version != kVersion) return "unknown format version";
  if (h.header_bytes != sizeof(Header)) return "header size";
  if (h.total_bytes != bytes) return "total bytes differ from the block's size";
  if (bytes % 8) return "size is no multiple of 8";
  // Mode and counts.
  const uint32_t m = h.mode;
  if (m & ~(kModeWaiting | kModeLeased | kModeRpc | kModeBook | kModeAlive)) return "unknown mode bits";
  if (!(m & (kModeWaiting | kModeLeased))) return "a stream without device state";
  if ((m & kModeRpc) && (m & (kModeWaiting | kModeLeased)) != (kModeWaiting | kModeLeased)) return "rpc mode without W or L";
  if ((m & (kModeBook | kModeAlive)) && !(m & kModeLeased)) return "book or aliveness without L";
  if (h.env_words == 0 || h.env_words > kMaxEnvWords) return "env_words out of range";
  if (!h.caps[kTasks]) return "max_tasks is 0";
  if (!!(m & kModeWaiting) != !!h.caps[kWaiting]) return "max_waiting does not fit the mode";
  if (!!(m & kModeLeased) != !!h.caps[kLeases]) return "max_leases does not fit the mode";
  if (!!(m & kModeRpc) != !!h.caps[kRows]) return "max_rows does not fit the mode";
  if (!!(m & kModeBook) != !!h.max_book) return "max_book does not fit the mode";
  if (!(m & kModeLeased) && (h.caps[kRenewals] | h.caps[kFrees] | h.caps[kReports] | h.caps[kReportIds] | h.n_leases |
                             h.lease_tick | h.next_id))
    return "lease fields without L";
  if (h.n_leases > h.caps[kLeases]) return "|L| > max_leases";
  if (h.n_waiting > h.caps[kWaiting]) return "|W| > max_waiting";
  if (h.n_book > h.max_book) return "|B| > max_book";
  if (h.n_wait_rows > h.caps[kRows]) return "rows(W) > max_rows";
  if (h.lease_tick && !(h.lease_tick & kStamp)) return "a tick number whose stamp is 0";
  if (!(m & kModeAlive) && h.alive_bound != INT64_MAX) return "alive_bound without E";
  // The directory is what the counts imply, inside the block.
  uint64_t sz[kSections], off = sizeof(Header);
  section_bytes(h, sz);
  for (int s = 0; s < kSections; ++s) {
    if (h.dir[s].offset != off || h.dir[s].bytes != sz[s]) return "a section is not where its counts put it";
    if (sz[s] > bytes - off) return "a section reaches past the end";
    off += sz[s];
  }
  if (off != bytes) return "bytes behind the last section";
  if (checksum(blob, bytes) != h.checksum) return "checksum";
  place(out, (const uint8_t*)blob);
  const View& v = *out;
  // Contents.
  for (uint64_t i = 0; i < h.n_alias; ++i)
    if (get<uint32_t>(v.alias_servant, i) >= h.n_servants) return "an alias names no servant";
  uint64_t prev = 0;
  for (uint64_t i = 0; i < h.n_leases; ++i) {
    const uint64_t id = get<uint64_t>(v.l_id, i);
    if (i && id <= prev) return "lease ids not ascending";
    if (id >= h.next_id) return "a lease id >= next_id";
    if (!(get<uint32_t>(v.l_state, i) & kLive)) return "a lease without the live bit";
    if (get<uint32_t>(v.l_srv, i) >= h.n_servants) return "a lease names no servant";
    prev = id;
  }
  if (m & kModeRpc) {
    uint64_t rows = 0;
    for (uint64_t i = 0; i < h.n_waiting; ++i) {
      const uint64_t r = (uint64_t)get<uint32_t>(v.w_nimm, i) + get<uint32_t>(v.w_npre, i);
      if (!r) return "a waiting RPC of no rows";
      rows += r;
    }
    if (rows != h.n_wait_rows) return "rows(W) differs from the entries' sum";
  } else if (h.n_wait_rows) {
    return "rows(W) without rpc mode";
  }
  for (uint64_t i = 0; i < h.n_book; ++i)
    if (get<uint32_t>(v.b_srv, i) >= h.n_servants) return "a book entry names no servant";
  if (m & kModeAlive)
    for (uint64_t i = 0; i < h.n_servants; ++i)
      if (get<int64_t>(v.e_exp, i) < h.alive_bound) return "alive_bound above an expiry";
  // Padding is zero (one encoding per state).
  const uint64_t used[kSections] = {
      (uint64_t)h.n_servants * h.env_words * 8 + (uint64_t)h.n_servants * 32 + (uint64_t)h.n_alias * 8, sz[kL],
      (m & kModeWaiting) ? (uint64_t)h.n_waiting * (28 + ((m & kModeLeased) ? 8 : 0) + ((m & kModeRpc) ? 8 : 0)) : 0,
      (m & kModeBook) ? (uint64_t)h.n_book * 28 : 0, sz[kE]};
  for (int s = 0; s < kSections; ++s)
    for (uint64_t i = used[s]; i < sz[s]; ++i)
      if (v.base[h.dir[s].offset + i]) return "padding is not zero";
  return nullptr;
}

}  // namespace snap
}  // namespace ydc

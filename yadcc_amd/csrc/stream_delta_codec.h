// stream_delta_codec.h — the byte format of ydc_stream_delta / ydc_stream_delta_apply.
//
// Host only, no HIP: the layout of a delta blob, the structure stamp, the validation of a block of
// untrusted bytes, and the delta of two full snapshots (stream_snapshot_codec.h). A delta takes a
// leased, waiting-and-leased or rpc stream from its base state to a later one. It is a header, then
// up to seven sections laid end to end in a fixed order, every section a run of whole columns (SoA)
// padded with zero bytes to a multiple of 8:
//
//   inserted  id u64[i] | expires_at i64[i] | servant u32[i] | state u32[i]        (ascending id)
//   erased    id u64[e]                                                            (ascending id)
//   updated   id u64[u] | expires_at i64[u] | state u32[u]                         (ascending id)
//   registry  version, num_processors, current_load, max_tasks, flags, running_tasks, rep_tick
//             u32[n] each, whole: what a heartbeat or a tick changes without a structural turn
//   W         whole, as in the snapshot blob                                       (queue order)
//   E         expires_at i64[n], whole                                             (aliveness only)
//   B         whole, as in the snapshot blob; present only if B differs from the base's
//
// The header names the base it applies to (lease_tick, next_id, |L|, |W|, last_now and the structure
// stamp) and the values that result. The stamp covers what a delta does not carry: the mode bits, the
// ten bounds and max_book, n_servants, env_words, the alias count, every environment mask, ip_id and
// alias. A delta is a function of the two full snapshots alone (build, below): one state pair has
// exactly one encoding.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "stream_snapshot_codec.h"

namespace ydc {
namespace delta {

constexpr uint64_t kMagic = 0x3141544C44434459ull;  // "YDCDLTA1"
constexpr uint32_t kVersion = 1;
enum Section { kIns = 0, kEra, kUpd, kReg, kW, kE, kB, kSections };
constexpr int kRegCols = 7;  // version, num_processors, current_load, max_tasks, flags, running_tasks, rep_tick

struct Header {
  uint64_t magic;
  uint32_t version, header_bytes;
  uint64_t total_bytes;
  uint64_t checksum;  // snap::checksum of the whole block, this field read as 0 (word 3, as in a snapshot)
  uint32_t mode, env_words, n_servants;  // snap::kMode*
  uint32_t book_present;                 // 1: section B is carried
  uint32_t max_leases, max_waiting, max_rows, max_book;  // the bounds the counts are checked against
  uint64_t stamp;                        // the structure stamp of base and result alike
  // The base this delta applies to.
  uint64_t base_next_id;
  int64_t base_last_now;
  uint32_t base_lease_tick, base_n_leases, base_n_waiting, reserved;
  // What results.
  uint64_t next_id;
  int64_t last_now;
  int64_t alive_bound;
  uint32_t lease_tick, n_leases, n_waiting, n_wait_rows, n_book;  // |L|, |W|, rows(W), |B|
  uint32_t n_ins, n_era, n_upd;
  struct {
    uint64_t offset, bytes;
  } dir[kSections];
};
static_assert(sizeof(Header) == 272, "delta header layout");
static_assert(offsetof(Header, checksum) == offsetof(snap::Header, checksum), "snap::checksum skips this word");

using snap::get;
using snap::pad8;

inline uint64_t w_width(uint32_t mode) {
  return (mode & snap::kModeWaiting) ? 16 + 8 + 12 + ((mode & snap::kModeRpc) ? 8 : 0) : 0;
}

// Bytes in use of every section, as the header's counts imply them (the section is that, padded to 8).
inline void section_used(const Header& h, uint64_t out[kSections]) {
  const uint64_t n = h.n_servants;
  out[kIns] = (uint64_t)h.n_ins * 24;
  out[kEra] = (uint64_t)h.n_era * 8;
  out[kUpd] = (uint64_t)h.n_upd * 20;
  out[kReg] = n * 4 * kRegCols;
  out[kW] = (uint64_t)h.n_waiting * w_width(h.mode);
  out[kE] = (h.mode & snap::kModeAlive) ? n * 8 : 0;
  out[kB] = h.book_present ? (uint64_t)h.n_book * 28 : 0;
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

// The columns of a delta, at their places in it (read through get<>(): the base may be any address).
struct View {
  Header h;
  const uint8_t* base;
  const uint8_t *ins_id, *ins_exp, *ins_srv, *ins_state;
  const uint8_t* era_id;
  const uint8_t *upd_id, *upd_exp, *upd_state;
  const uint8_t* reg[kRegCols];
  const uint8_t *w_deadline, *w_tag, *w_for, *w_env, *w_minv, *w_ip, *w_nimm, *w_npre;
  const uint8_t* e_exp;
  const uint8_t *b_grant, *b_stid, *b_dkey, *b_srv;
};

inline void place(View* v, const uint8_t* base) {
  const Header& h = v->h;
  v->base = base;
  const uint64_t n = h.n_servants, w = h.n_waiting, b = h.book_present ? h.n_book : 0;
  const bool rpc = h.mode & snap::kModeRpc;
  const uint8_t* p = base + h.dir[kIns].offset;
  v->ins_id = p, p += (uint64_t)h.n_ins * 8;
  v->ins_exp = p, p += (uint64_t)h.n_ins * 8;
  v->ins_srv = p, p += (uint64_t)h.n_ins * 4;
  v->ins_state = p;
  v->era_id = base + h.dir[kEra].offset;
  p = base + h.dir[kUpd].offset;
  v->upd_id = p, p += (uint64_t)h.n_upd * 8;
  v->upd_exp = p, p += (uint64_t)h.n_upd * 8;
  v->upd_state = p;
  p = base + h.dir[kReg].offset;
  for (int k = 0; k < kRegCols; ++k) v->reg[k] = p, p += n * 4;
  p = base + h.dir[kW].offset;
  v->w_deadline = p, p += w * 8;
  v->w_tag = p, p += w * 8;
  v->w_for = p, p += w * 8;
  v->w_env = p, p += w * 4;
  v->w_minv = p, p += w * 4;
  v->w_ip = p, p += w * 4;
  v->w_nimm = p, p += rpc ? w * 4 : 0;
  v->w_npre = p;
  v->e_exp = base + h.dir[kE].offset;
  p = base + h.dir[kB].offset;
  v->b_grant = p, p += b * 8;
  v->b_stid = p, p += b * 8;
  v->b_dkey = p, p += b * 8;
  v->b_srv = p;
}

// The structure stamp: snap::checksum over the counts, the bounds and the mode bits (ten words, the
// fourth 0), every environment mask, then ip_id, alias ip and alias servant as they lie behind each
// other, zero-padded to a whole word. The columns may lie at any address.
inline uint64_t stamp(uint32_t mode, uint32_t env_words, uint32_t n, uint32_t n_alias, const uint32_t caps[snap::kCaps],
                      uint32_t max_book, const void* env_mask, const void* ip, const void* alias_ip,
                      const void* alias_servant) {
  const uint64_t env_bytes = (uint64_t)n * env_words * 8, tail = (uint64_t)n * 4 + (uint64_t)n_alias * 8;
  std::vector<uint64_t> buf(10 + env_bytes / 8 + pad8(tail) / 8, 0);
  buf[0] = kMagic;
  buf[1] = mode | (uint64_t)env_words << 32;
  buf[2] = n | (uint64_t)n_alias << 32;
  for (int i = 0; i < snap::kCaps; i += 2) buf[4 + i / 2] = caps[i] | (uint64_t)caps[i + 1] << 32;
  buf[9] = max_book;
  uint8_t* p = (uint8_t*)(buf.data() + 10);
  if (env_bytes) memcpy(p, env_mask, env_bytes);
  p += env_bytes;
  if (n) memcpy(p, ip, (uint64_t)n * 4);
  p += (uint64_t)n * 4;
  if (n_alias) memcpy(p, alias_ip, (uint64_t)n_alias * 4), memcpy(p + (uint64_t)n_alias * 4, alias_servant, (uint64_t)n_alias * 4);
  return snap::checksum(buf.data(), buf.size() * 8);
}

inline uint64_t stamp_of(const snap::View& v) {
  return stamp(v.h.mode, v.h.env_words, v.h.n_servants, v.h.n_alias, v.h.caps, v.h.max_book, v.env_mask, v.ip, v.alias_ip,
               v.alias_servant);
}

// Checks `bytes` untrusted bytes. nullptr: a well-formed delta, *out describes it. Otherwise the reason.
// Nothing outside [blob, blob + bytes) is read.
inline const char* validate(const void* blob, size_t bytes, View* out) {
  if (!blob || bytes < sizeof(Header)) return "shorter than a header";
  Header& h = out->h;
  memcpy(&h, blob, sizeof(Header));
  if (h.magic != kMagic) return "not a stream delta (magic)";
  if (h.version != kVersion) return "unknown format version";
  if (h.header_bytes != sizeof(Header)) return "header size";
  if (h.total_bytes != bytes) return "total bytes differ from the block's size";
  if (bytes % 8) return "size is no multiple of 8";
  // Mode, bounds and counts.
  const uint32_t m = h.mode;
  if (m & ~(snap::kModeWaiting | snap::kModeLeased | snap::kModeRpc | snap::kModeBook | snap::kModeAlive)) return "unknown mode bits";
  if (!(m & snap::kModeLeased)) return "a delta of a stream without L";
  if ((m & snap::kModeRpc) && !(m & snap::kModeWaiting)) return "rpc mode without W";
  if (h.env_words == 0 || h.env_words > snap::kMaxEnvWords) return "env_words out of range";
  if (h.book_present > 1 || h.reserved) return "a reserved field is set";
  if (h.book_present && !(m & snap::kModeBook)) return "B without the book";
  if (!h.max_leases) return "max_leases is 0";
  if (!!(m & snap::kModeWaiting) != !!h.max_waiting) return "max_waiting does not fit the mode";
  if (!!(m & snap::kModeRpc) != !!h.max_rows) return "max_rows does not fit the mode";
  if (!!(m & snap::kModeBook) != !!h.max_book) return "max_book does not fit the mode";
  if (h.n_leases > h.max_leases || h.base_n_leases > h.max_leases) return "|L| > max_leases";
  if (h.n_waiting > h.max_waiting || h.base_n_waiting > h.max_waiting) return "|W| > max_waiting";
  if (h.n_book > h.max_book) return "|B| > max_book";
  if (h.n_wait_rows > h.max_rows) return "rows(W) > max_rows";
  if (h.n_era > h.base_n_leases || h.n_upd > h.base_n_leases - h.n_era) return "more erased and updated leases than the base holds";
  if ((uint64_t)h.base_n_leases + h.n_ins - h.n_era != h.n_leases) return "|L| is not the base's + inserted - erased";
  if (h.next_id < h.base_next_id || h.n_ins > h.next_id - h.base_next_id) return "more inserted leases than ids handed out";
  if (h.last_now < h.base_last_now) return "the clock runs backwards";
  for (uint32_t t : {h.lease_tick, h.base_lease_tick})
    if (t && !(t & snap::kStamp)) return "a tick number whose stamp is 0";
  if (!(m & snap::kModeAlive) && h.alive_bound != INT64_MAX) return "alive_bound without E";
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
  // Contents: the three id lists ascending, in their ranges and pairwise disjoint (inserted ids lie
  // above the other two's range; erased and updated are walked together).
  for (uint64_t i = 0; i < h.n_ins; ++i) {
    const uint64_t id = get<uint64_t>(v.ins_id, i);
    if (i && id <= get<uint64_t>(v.ins_id, i - 1)) return "inserted ids not ascending";
    if (id < h.base_next_id || id >= h.next_id) return "an inserted id outside [base next_id, next_id)";
    if (!(get<uint32_t>(v.ins_state, i) & snap::kLive)) return "an inserted lease without the live bit";
    if (get<uint32_t>(v.ins_srv, i) >= h.n_servants) return "an inserted lease names no servant";
  }
  for (uint64_t i = 0; i < h.n_era; ++i) {
    const uint64_t id = get<uint64_t>(v.era_id, i);
    if (i && id <= get<uint64_t>(v.era_id, i - 1)) return "erased ids not ascending";
    if (id >= h.base_next_id) return "an erased id >= the base's next_id";
  }
  for (uint64_t i = 0, e = 0; i < h.n_upd; ++i) {
    const uint64_t id = get<uint64_t>(v.upd_id, i);
    if (i && id <= get<uint64_t>(v.upd_id, i - 1)) return "updated ids not ascending";
    if (id >= h.base_next_id) return "an updated id >= the base's next_id";
    if (!(get<uint32_t>(v.upd_state, i) & snap::kLive)) return "an updated lease without the live bit";
    while (e < h.n_era && get<uint64_t>(v.era_id, e) < id) ++e;
    if (e < h.n_era && get<uint64_t>(v.era_id, e) == id) return "a lease both erased and updated";
  }
  if (m & snap::kModeRpc) {
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
  for (uint64_t i = 0; h.book_present && i < h.n_book; ++i)
    if (get<uint32_t>(v.b_srv, i) >= h.n_servants) return "a book entry names no servant";
  if (m & snap::kModeAlive)
    for (uint64_t i = 0; i < h.n_servants; ++i)
      if (get<int64_t>(v.e_exp, i) < h.alive_bound) return "alive_bound above an expiry";
  // Padding is zero (one encoding per state pair).
  for (int s = 0; s < kSections; ++s)
    for (uint64_t i = used[s]; i < h.dir[s].bytes; ++i)
      if (v.base[h.dir[s].offset + i]) return "padding is not zero";
  return nullptr;
}

// Seals a delta whose header fields and columns are in place: the header with its checksum stored.
inline void seal(uint8_t* blob, Header* h) {
  h->checksum = 0;
  memcpy(blob, h, sizeof *h);
  h->checksum = snap::checksum(blob, h->total_bytes);
  memcpy(blob, h, sizeof *h);
}

// The header of the delta from a stream in the state of snapshot `a` to the one of snapshot `b`, its
// list counts still 0 (the caller fills them in and calls layout()).
inline Header describe(const snap::Header& a, const snap::Header& b, uint64_t structure_stamp) {
  Header h;
  memset(&h, 0, sizeof h);
  h.magic = kMagic;
  h.version = kVersion;
  h.mode = b.mode, h.env_words = b.env_words, h.n_servants = b.n_servants;
  h.max_leases = b.caps[snap::kLeases], h.max_waiting = b.caps[snap::kWaiting], h.max_rows = b.caps[snap::kRows];
  h.max_book = b.max_book;
  h.stamp = structure_stamp;
  h.base_next_id = a.next_id, h.base_last_now = a.last_now, h.base_lease_tick = a.lease_tick;
  h.base_n_leases = a.n_leases, h.base_n_waiting = a.n_waiting;
  h.next_id = b.next_id, h.last_now = b.last_now, h.alive_bound = b.alive_bound, h.lease_tick = b.lease_tick;
  h.n_leases = b.n_leases, h.n_waiting = b.n_waiting, h.n_wait_rows = b.n_wait_rows, h.n_book = b.n_book;
  return h;
}

// The delta of two validated snapshots of one stream, `a` the earlier. nullptr: *out is the blob.
// Otherwise why there is none: the structure stamps differ, or a lease changed its servant.
inline const char* build(const snap::View& a, const snap::View& b, std::vector<uint8_t>* out) {
  if (!(a.h.mode & snap::kModeLeased) || !(b.h.mode & snap::kModeLeased)) return "a snapshot without L";
  const uint64_t st = stamp_of(a);
  if (st != stamp_of(b)) return "the structure differs";
  Header h = describe(a.h, b.h, st);
  const uint64_t na = a.h.n_leases, nb = b.h.n_leases;
  std::vector<uint64_t> ins, era, upd;  // positions: ins and upd in b, era in a
  for (uint64_t i = 0, j = 0; i < na || j < nb;) {
    const uint64_t ia = i < na ? get<uint64_t>(a.l_id, i) : ~0ull, ib = j < nb ? get<uint64_t>(b.l_id, j) : ~0ull;
    if (i < na && (j == nb || ia < ib)) {
      era.push_back(i++);
    } else if (j < nb && (i == na || ib < ia)) {
      if (ib < a.h.next_id) return "a lease appeared below the base's next_id";
      ins.push_back(j++);
    } else {
      if (get<uint32_t>(a.l_srv, i) != get<uint32_t>(b.l_srv, j)) return "a lease changed its servant";
      if (get<int64_t>(a.l_exp, i) != get<int64_t>(b.l_exp, j) || get<uint32_t>(a.l_state, i) != get<uint32_t>(b.l_state, j))
        upd.push_back(j);
      ++i, ++j;
    }
  }
  h.n_ins = (uint32_t)ins.size(), h.n_era = (uint32_t)era.size(), h.n_upd = (uint32_t)upd.size();
  const bool book = b.h.mode & snap::kModeBook;
  h.book_present = book && (a.h.n_book != b.h.n_book ||
                            memcmp(a.base + a.h.dir[snap::kB].offset, b.base + b.h.dir[snap::kB].offset, b.h.dir[snap::kB].bytes));
  layout(&h);
  out->assign((size_t)h.total_bytes, 0);
  View v;
  v.h = h;
  place(&v, out->data());
  auto at = [](const uint8_t* col) { return const_cast<uint8_t*>(col); };
  for (size_t k = 0; k < ins.size(); ++k) {
    memcpy(at(v.ins_id) + k * 8, b.l_id + ins[k] * 8, 8);
    memcpy(at(v.ins_exp) + k * 8, b.l_exp + ins[k] * 8, 8);
    memcpy(at(v.ins_srv) + k * 4, b.l_srv + ins[k] * 4, 4);
    memcpy(at(v.ins_state) + k * 4, b.l_state + ins[k] * 4, 4);
  }
  for (size_t k = 0; k < era.size(); ++k) memcpy(at(v.era_id) + k * 8, a.l_id + era[k] * 8, 8);
  for (size_t k = 0; k < upd.size(); ++k) {
    memcpy(at(v.upd_id) + k * 8, b.l_id + upd[k] * 8, 8);
    memcpy(at(v.upd_exp) + k * 8, b.l_exp + upd[k] * 8, 8);
    memcpy(at(v.upd_state) + k * 4, b.l_state + upd[k] * 4, 4);
  }
  const uint8_t* reg[kRegCols] = {b.version, b.nproc, b.load, b.max_tasks, b.flags, b.running, b.rep_tick};
  for (int k = 0; k < kRegCols; ++k)
    if (h.n_servants) memcpy(at(v.reg[k]), reg[k], (size_t)h.n_servants * 4);
  uint64_t used[kSections];
  section_used(h, used);
  if (used[kW]) memcpy(out->data() + h.dir[kW].offset, b.base + b.h.dir[snap::kW].offset, used[kW]);
  if (used[kE]) memcpy(out->data() + h.dir[kE].offset, b.e_exp, used[kE]);
  if (used[kB]) memcpy(out->data() + h.dir[kB].offset, b.base + b.h.dir[snap::kB].offset, used[kB]);
  seal(out->data(), &h);
  return nullptr;
}

}  // namespace delta
}  // namespace ydc

// The delta codec (yadcc_amd/csrc/stream_delta_codec.h) under ASan + UBSan. Includes nothing but the two
// codec headers. Without arguments: deltas of seeded pairs of snapshots are built, validated, and handed
// to the validator again as seeded corruptions — truncations, flipped bits with and without the checksum
// made right, counts, offsets and ids overwritten with extremes, lists made unsorted or overlapping. No
// corrupted block whose checksum is wrong may be accepted, none may make the validator read outside the
// block (every block lives in a heap allocation of exactly its size, every other one at an odd address),
// and the named corruptions are refused also with the checksum made right.
//
//   delta_codec_test build BEFORE AFTER OUT   the delta of two snapshot files, written to OUT
//   delta_codec_test check DELTA              exit status 0 exactly if the validator accepts the file
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "stream_delta_codec.h"
#include "stream_snapshot_codec.h"

using namespace ydc;

static int g_failures = 0;
#define EXPECT(cond, ...)                                       \
  do {                                                          \
    if (!(cond)) {                                              \
      ++g_failures;                                             \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fprintf(stderr, "\n");                               \
    }                                                           \
  } while (0)

template <typename T>
static void put(const uint8_t* col, uint64_t i, T v) {
  std::memcpy(const_cast<uint8_t*>(col) + i * sizeof(T), &v, sizeof(T));
}

struct Lease {
  uint64_t id;
  int64_t exp;
  uint32_t srv, state;
};

// A stream's state, as far as a pair of snapshots needs one.
struct State {
  uint32_t mode = 0, n = 0, env_words = 1;
  std::vector<Lease> L;  // ascending id
  uint64_t next_id = 0;
  uint32_t tick = 0, nw = 0, nb = 0;
  int64_t now = 0;
  uint32_t fill = 0;  // seed of the carried columns (registry light, W, E)
  uint32_t book_fill = 0;
};

static std::vector<uint8_t> snapshot_of(const State& s) {
  snap::Header h{};
  h.magic = snap::kMagic, h.version = snap::kVersion, h.mode = s.mode, h.env_words = s.env_words, h.n_servants = s.n;
  h.n_alias = s.n ? 2 : 0;
  h.caps[snap::kUpdates] = 16, h.caps[snap::kReleases] = 16, h.caps[snap::kTasks] = 64;
  h.caps[snap::kLeases] = 4096, h.caps[snap::kRenewals] = 8, h.caps[snap::kFrees] = 8, h.caps[snap::kReports] = 4;
  h.caps[snap::kReportIds] = 32;
  if (s.mode & snap::kModeWaiting) h.caps[snap::kWaiting] = 64;
  if (s.mode & snap::kModeRpc) h.caps[snap::kRows] = 1024;
  if (s.mode & snap::kModeBook) h.max_book = 64;
  h.n_leases = (uint32_t)s.L.size(), h.n_waiting = s.nw, h.n_book = s.nb;
  h.lease_tick = s.tick, h.next_id = s.next_id, h.last_now = s.now, h.alive_bound = INT64_MAX;
  snap::layout(&h);
  std::vector<uint8_t> b(h.total_bytes, 0);
  snap::View v{};
  v.h = h;
  snap::place(&v, b.data());
  std::mt19937_64 structure(99), light(s.fill), book(s.book_fill);
  for (uint64_t i = 0; i < (uint64_t)s.n * s.env_words; ++i) put<uint64_t>(v.env_mask, i, structure());
  for (uint32_t k = 0; k < s.n; ++k) put<uint32_t>(v.ip, k, (uint32_t)structure());
  for (uint32_t a = 0; a < h.n_alias; ++a) put<uint32_t>(v.alias_ip, a, (uint32_t)structure()), put<uint32_t>(v.alias_servant, a, a % s.n);
  for (const uint8_t* col : {v.version, v.nproc, v.load, v.max_tasks, v.flags, v.running, v.rep_tick})
    for (uint32_t k = 0; k < s.n; ++k) put<uint32_t>(col, k, (uint32_t)light());
  for (size_t i = 0; i < s.L.size(); ++i) {
    put<uint64_t>(v.l_id, i, s.L[i].id), put<int64_t>(v.l_exp, i, s.L[i].exp);
    put<uint32_t>(v.l_srv, i, s.L[i].srv), put<uint32_t>(v.l_state, i, s.L[i].state);
  }
  uint32_t rows = 0;
  for (uint32_t i = 0; i < s.nw; ++i) {
    put<int64_t>(v.w_deadline, i, (int64_t)(light() % 1000)), put<uint64_t>(v.w_tag, i, light());
    put<int64_t>(v.w_for, i, (int64_t)(light() % 50));
    put<uint32_t>(v.w_env, i, (uint32_t)light() % 70), put<uint32_t>(v.w_minv, i, (uint32_t)light() % 5);
    put<uint32_t>(v.w_ip, i, (uint32_t)light());
    if (s.mode & snap::kModeRpc) {
      const uint32_t a = (uint32_t)(light() % 3), p = (uint32_t)(light() % 3) + (a ? 0 : 1);
      put<uint32_t>(v.w_nimm, i, a), put<uint32_t>(v.w_npre, i, p);
      rows += a + p;
    }
  }
  for (uint32_t i = 0; i < s.nb; ++i) {
    put<uint64_t>(v.b_grant, i, book()), put<uint64_t>(v.b_stid, i, book()), put<uint64_t>(v.b_dkey, i, book());
    put<uint32_t>(v.b_srv, i, (uint32_t)(book() % s.n));
  }
  if (s.mode & snap::kModeAlive)
    for (uint32_t k = 0; k < s.n; ++k) {
      const int64_t e = 2000 + (int64_t)(light() % 100);
      put<int64_t>(v.e_exp, k, e);
      if (e < h.alive_bound) h.alive_bound = e;
    }
  h.n_wait_rows = rows;
  std::memcpy(b.data(), &h, sizeof h);
  h.checksum = snap::checksum(b.data(), b.size());
  std::memcpy(b.data(), &h, sizeof h);
  return b;
}

static State first(uint32_t mode, uint32_t n, uint32_t nl, uint32_t seed) {
  std::mt19937_64 rng(seed);
  State s;
  s.mode = mode, s.n = n, s.env_words = 1 + seed % 3, s.tick = 12, s.now = 1234, s.fill = seed, s.book_fill = seed;
  s.nw = (mode & snap::kModeWaiting) ? 5 : 0, s.nb = (mode & snap::kModeBook) ? 7 : 0;
  for (uint32_t i = 0; i < nl; ++i)
    s.L.push_back({(1ull << 40) + 10ull * i + rng() % 10, (int64_t)(rng() % 100000) - 50, (uint32_t)(rng() % n),
                   snap::kLive | ((uint32_t)rng() & 0x7FFFFFFFu)});
  s.next_id = (1ull << 40) + 10ull * nl + 1;
  return s;
}

// A later state: every `drop`th lease gone, every `touch`th renewed or stamped, `add` new ones.
static State later(const State& a, uint32_t drop, uint32_t touch, uint32_t add, bool book_changes, uint32_t seed) {
  std::mt19937_64 rng(seed);
  State b = a;
  b.L.clear();
  for (size_t i = 0; i < a.L.size(); ++i) {
    if (drop && i % drop == 0) continue;
    Lease l = a.L[i];
    if (touch && i % touch == 1) (rng() & 1) ? (void)(l.exp += 77) : (void)(l.state ^= 1u << 30);
    b.L.push_back(l);
  }
  for (uint32_t i = 0; i < add; ++i)
    b.L.push_back({a.next_id + 2ull * i, (int64_t)(rng() % 1000), (uint32_t)(rng() % a.n), snap::kLive});
  b.next_id = a.next_id + 2ull * add + (add ? 3 : 0);
  b.tick = a.tick + (seed & 1 ? 1 : 20), b.now = a.now + 5, b.fill = seed * 7 + 1;
  if (a.mode & snap::kModeWaiting) b.nw = (uint32_t)(rng() % 9);
  if (book_changes) b.book_fill = seed * 3 + 2, b.nb = a.nb ? a.nb - (seed & 1) : 0;
  return b;
}

// validate() on a copy of exactly `bytes` bytes; odd: the copy starts at an odd address. An accepted
// block has every element of every column read, as an apply would.
static const char* check(const uint8_t* p, size_t bytes, bool odd) {
  const size_t size = bytes + (odd ? 1 : 0);
  uint8_t* block = (uint8_t*)std::malloc(size ? size : 1);
  uint8_t* at = block + (odd ? 1 : 0);
  if (bytes) std::memcpy(at, p, bytes);
  delta::View v{};
  const char* why = delta::validate(at, bytes, &v);
  uint64_t touched = 0;
  if (!why) {
    const delta::Header& h = v.h;
    for (uint32_t i = 0; i < h.n_ins; ++i)
      touched += snap::get<uint64_t>(v.ins_id, i) + (uint64_t)snap::get<int64_t>(v.ins_exp, i) + snap::get<uint32_t>(v.ins_srv, i) +
                 snap::get<uint32_t>(v.ins_state, i);
    for (uint32_t i = 0; i < h.n_era; ++i) touched += snap::get<uint64_t>(v.era_id, i);
    for (uint32_t i = 0; i < h.n_upd; ++i)
      touched += snap::get<uint64_t>(v.upd_id, i) + (uint64_t)snap::get<int64_t>(v.upd_exp, i) + snap::get<uint32_t>(v.upd_state, i);
    for (int k = 0; k < delta::kRegCols; ++k)
      for (uint32_t s = 0; s < h.n_servants; ++s) touched += snap::get<uint32_t>(v.reg[k], s);
    for (uint32_t i = 0; i < h.n_waiting; ++i) {
      touched += (uint64_t)snap::get<int64_t>(v.w_deadline, i) + snap::get<uint64_t>(v.w_tag, i) + (uint64_t)snap::get<int64_t>(v.w_for, i) +
                 snap::get<uint32_t>(v.w_env, i) + snap::get<uint32_t>(v.w_minv, i) + snap::get<uint32_t>(v.w_ip, i);
      if (h.mode & snap::kModeRpc) touched += snap::get<uint32_t>(v.w_nimm, i) + snap::get<uint32_t>(v.w_npre, i);
    }
    if (h.mode & snap::kModeAlive)
      for (uint32_t s = 0; s < h.n_servants; ++s) touched += (uint64_t)snap::get<int64_t>(v.e_exp, s);
    for (uint32_t i = 0; h.book_present && i < h.n_book; ++i)
      touched += snap::get<uint64_t>(v.b_grant, i) + snap::get<uint64_t>(v.b_stid, i) + snap::get<uint64_t>(v.b_dkey, i) +
                 snap::get<uint32_t>(v.b_srv, i);
  }
  if (touched == 0x0123456789ABCDEFull) std::printf("%s", "");  // (the reads above are not dead code)
  std::free(block);
  return why;
}

static void reseal(std::vector<uint8_t>& b) {
  if (b.size() < sizeof(delta::Header) || b.size() % 8) return;  // (the checksum is over whole words)
  const uint64_t sum = snap::checksum(b.data(), b.size());
  std::memcpy(b.data() + offsetof(delta::Header, checksum), &sum, 8);
}

static bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + k);
  std::fclose(f);
  return true;
}

static int tool(int argc, char** argv) {
  const std::string cmd = argv[1];
  if (cmd == "build" && argc == 5) {
    std::vector<uint8_t> a, b, d;
    if (!read_file(argv[2], &a) || !read_file(argv[3], &b)) return 2;
    snap::View va{}, vb{};
    if (const char* why = snap::validate(a.data(), a.size(), &va)) return std::fprintf(stderr, "before: %s\n", why), 3;
    if (const char* why = snap::validate(b.data(), b.size(), &vb)) return std::fprintf(stderr, "after: %s\n", why), 3;
    if (const char* why = delta::build(va, vb, &d)) return std::fprintf(stderr, "build: %s\n", why), 4;
    FILE* f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(d.data(), 1, d.size(), f) != d.size()) return 2;
    std::fclose(f);
    return 0;
  }
  if (cmd == "check" && argc == 3) {
    std::vector<uint8_t> d;
    if (!read_file(argv[2], &d)) return 2;
    const char* why = check(d.data(), d.size(), true);
    if (why) std::fprintf(stderr, "%s\n", why);
    return why ? 1 : 0;
  }
  return 2;
}

int main(int argc, char** argv) {
  if (argc > 1) return tool(argc, argv);
  const uint32_t L = snap::kModeLeased, WL = L | snap::kModeWaiting, R = WL | snap::kModeRpc;
  struct Pair {
    uint32_t mode, n, nl, drop, touch, add;
    bool book_changes;
  };
  const Pair pairs[] = {{L, 7, 40, 0, 0, 0, false},          {L, 7, 40, 0, 0, 9, false},   {L, 7, 40, 3, 0, 0, false},
                        {L, 7, 40, 1, 0, 0, false},          {L, 7, 40, 0, 2, 0, false},   {L, 5, 0, 0, 0, 3, false},
                        {L, 5, 1, 1, 0, 1, false},           {WL, 9, 65, 4, 3, 11, false}, {R, 9, 65, 4, 3, 11, false},
                        {R | snap::kModeBook | snap::kModeAlive, 11, 70, 5, 2, 6, true},
                        {R | snap::kModeBook | snap::kModeAlive, 11, 70, 5, 2, 6, false},
                        {L | snap::kModeAlive, 3, 12, 2, 2, 2, false}};
  uint32_t seed = 1, made = 0, tried = 0, refused_sealed = 0;
  for (const Pair& p : pairs) {
    ++seed;
    const State sa = first(p.mode, p.n, p.nl, seed), sb = later(sa, p.drop, p.touch, p.add, p.book_changes, seed);
    const std::vector<uint8_t> a = snapshot_of(sa), b = snapshot_of(sb);
    snap::View va{}, vb{};
    EXPECT(!snap::validate(a.data(), a.size(), &va) && !snap::validate(b.data(), b.size(), &vb), "pair %u: a snapshot is bad", seed);
    std::vector<uint8_t> d;
    const char* why = delta::build(va, vb, &d);
    EXPECT(!why, "pair %u: no delta: %s", seed, why ? why : "");
    if (why) continue;
    ++made;
    for (bool odd : {false, true}) {
      why = check(d.data(), d.size(), odd);
      EXPECT(!why, "pair %u: the delta is refused: %s", seed, why ? why : "");
    }
    delta::View v{};
    EXPECT(!delta::validate(d.data(), d.size(), &v), "pair %u", seed);
    const delta::Header h = v.h;
    EXPECT(h.book_present == (p.book_changes ? 1u : 0u), "pair %u: book_present %u", seed, h.book_present);
    EXPECT(h.n_leases == sb.L.size() && h.base_n_leases == sa.L.size() && h.stamp == delta::stamp_of(va), "pair %u: header", seed);
    // The reverse pair is no delta where a lease was dropped: its id would appear below the base's next_id.
    std::vector<uint8_t> rev;
    EXPECT((delta::build(vb, va, &rev) != nullptr) == (p.drop != 0 && p.nl != 0), "pair %u: the reverse pair", seed);
    // Truncations.
    for (size_t cut : {(size_t)0, (size_t)1, sizeof(delta::Header) - 1, sizeof(delta::Header), d.size() / 2, d.size() - 8, d.size() - 1}) {
      if (cut >= d.size()) continue;
      ++tried;
      EXPECT(check(d.data(), cut, cut & 1), "pair %u: cut at %zu accepted", seed, cut);
      std::vector<uint8_t> t(d.begin(), d.begin() + cut);
      reseal(t);
      EXPECT(check(t.data(), t.size(), true), "pair %u: cut at %zu, sealed, accepted", seed, cut);
    }
    // Flipped bits: with the checksum left wrong never accepted; with the checksum made right, no overread.
    std::mt19937_64 rng(seed * 1000);
    for (int k = 0; k < 300; ++k) {
      std::vector<uint8_t> t = d;
      const size_t at = k < 150 ? rng() % sizeof(delta::Header) : rng() % t.size();
      t[at] ^= (uint8_t)(1u << (rng() % 8));
      ++tried;
      EXPECT(check(t.data(), t.size(), k & 1), "pair %u: bit flip at %zu accepted with a wrong checksum", seed, at);
      reseal(t);
      if (check(t.data(), t.size(), !(k & 1))) ++refused_sealed;
    }
    // Header fields overwritten with extremes, the checksum made right.
    const size_t field32[] = {offsetof(delta::Header, mode),      offsetof(delta::Header, n_servants), offsetof(delta::Header, n_ins),
                              offsetof(delta::Header, n_era),     offsetof(delta::Header, n_upd),      offsetof(delta::Header, n_leases),
                              offsetof(delta::Header, n_waiting), offsetof(delta::Header, n_book),     offsetof(delta::Header, base_n_leases),
                              offsetof(delta::Header, n_wait_rows), offsetof(delta::Header, book_present)};
    for (size_t f : field32)
      for (uint32_t val : {0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu}) {
        std::vector<uint8_t> t = d;
        std::memcpy(t.data() + f, &val, 4);
        reseal(t);
        ++tried;
        EXPECT(check(t.data(), t.size(), true), "pair %u: field at %zu = %08x accepted", seed, f, val);
      }
    for (int s = 0; s < delta::kSections; ++s)
      for (uint64_t val : std::initializer_list<uint64_t>{~0ull, 1ull << 63, d.size(), d.size() - 8, 0}) {
        for (size_t f : {offsetof(delta::Header, dir) + 16 * s, offsetof(delta::Header, dir) + 16 * s + 8}) {
          std::vector<uint8_t> t = d;
          uint64_t was;
          std::memcpy(&was, t.data() + f, 8);
          if (was == val) continue;
          std::memcpy(t.data() + f, &val, 8);
          reseal(t);
          ++tried;
          EXPECT(check(t.data(), t.size(), false), "pair %u: directory word at %zu = %llx accepted", seed, f, (unsigned long long)val);
        }
      }
    {
      std::vector<uint8_t> t = d;
      const uint64_t big = ~0ull;
      std::memcpy(t.data() + offsetof(delta::Header, total_bytes), &big, 8);
      reseal(t);
      EXPECT(check(t.data(), t.size(), true), "pair %u: total_bytes 2^64 - 1 accepted", seed);
    }
    // Lists: ids out of range, unsorted, overlapping, without the live bit; a servant that is none.
    auto with = [&](const char* what, auto&& change) {
      std::vector<uint8_t> t = d;
      delta::View w{};
      w.h = h;
      delta::place(&w, t.data());
      change(w);
      reseal(t);
      ++tried;
      EXPECT(check(t.data(), t.size(), true), "pair %u: %s accepted", seed, what);
    };
    if (h.n_ins) {
      with("an inserted id below the base's next_id", [&](delta::View& w) { put<uint64_t>(w.ins_id, 0, h.base_next_id - 1); });
      with("an inserted id == next_id", [&](delta::View& w) { put<uint64_t>(w.ins_id, h.n_ins - 1, h.next_id); });
      with("an inserted id 2^64 - 1", [&](delta::View& w) { put<uint64_t>(w.ins_id, h.n_ins - 1, ~0ull); });
      with("an inserted servant == n_servants", [&](delta::View& w) { put<uint32_t>(w.ins_srv, 0, h.n_servants); });
      with("an inserted lease that is not live", [&](delta::View& w) { put<uint32_t>(w.ins_state, 0, 5u); });
    }
    if (h.n_ins > 1)
      with("inserted ids unsorted", [&](delta::View& w) { put<uint64_t>(w.ins_id, 1, snap::get<uint64_t>(w.ins_id, 0)); });
    if (h.n_era) with("an erased id >= the base's next_id", [&](delta::View& w) { put<uint64_t>(w.era_id, h.n_era - 1, h.base_next_id); });
    if (h.n_era > 1)
      with("erased ids unsorted", [&](delta::View& w) { put<uint64_t>(w.era_id, 0, snap::get<uint64_t>(w.era_id, 1) + 1); });
    if (h.n_upd) {
      with("an updated id >= the base's next_id", [&](delta::View& w) { put<uint64_t>(w.upd_id, h.n_upd - 1, ~0ull - 1); });
      with("an updated lease that is not live", [&](delta::View& w) { put<uint32_t>(w.upd_state, 0, 1u << 30); });
    }
    if (h.n_upd > 1)
      with("updated ids unsorted", [&](delta::View& w) { put<uint64_t>(w.upd_id, 1, snap::get<uint64_t>(w.upd_id, 0)); });
    if (h.n_era && h.n_upd)
      with("a lease both erased and updated", [&](delta::View& w) {
        // (the first updated id replaced by an erased one that keeps the list ascending, if there is one)
        const uint64_t next = h.n_upd > 1 ? snap::get<uint64_t>(w.upd_id, 1) : ~0ull;
        uint64_t pick = snap::get<uint64_t>(w.era_id, 0);
        for (uint32_t i = 0; i < h.n_era; ++i)
          if (snap::get<uint64_t>(w.era_id, i) < next) pick = snap::get<uint64_t>(w.era_id, i);
        put<uint64_t>(w.upd_id, 0, pick);
      });
    if ((h.mode & snap::kModeRpc) && h.n_waiting)
      with("an RPC of no rows", [&](delta::View& w) { put<uint32_t>(w.w_nimm, 0, 0u), put<uint32_t>(w.w_npre, 0, 0u); });
    if ((h.mode & snap::kModeAlive) && h.n_servants)
      with("E below alive_bound", [&](delta::View& w) { put<int64_t>(w.e_exp, 0, h.alive_bound - 1); });
    if (h.book_present && h.n_book) with("a book entry on no servant", [&](delta::View& w) { put<uint32_t>(w.b_srv, 0, h.n_servants); });
    if (h.dir[delta::kUpd].bytes != (uint64_t)h.n_upd * 20)
      with("padding not zero", [&](delta::View& w) { const_cast<uint8_t*>(w.base)[h.dir[delta::kUpd].offset + h.dir[delta::kUpd].bytes - 1] = 1; });
  }
  EXPECT(made == sizeof pairs / sizeof pairs[0], "%u deltas made", made);
  EXPECT(refused_sealed > 100, "only %u sealed bit flips refused", refused_sealed);
  if (g_failures) return std::fprintf(stderr, "%d failures\n", g_failures), 1;
  std::printf("DELTA-CODEC-OK %u deltas, %u corruptions, %u sealed flips refused\n", made, tried, refused_sealed);
  return 0;
}

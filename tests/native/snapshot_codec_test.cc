// The blob validator of ydc_stream_restore (yadcc_amd/csrc/stream_snapshot_codec.h) on good blobs and on
// seeded corruptions of them, under ASan + UBSan. Includes nothing but the codec: what the validator
// accepts is all a restore ever reads, so a validator that stays inside the block and refuses what does
// not add up keeps untrusted bytes away from the context.
//
// Every block handed to validate() lives in a heap allocation of exactly its size (an overread is an
// ASan report), every other one at an odd address (a misaligned access is a UBSan report).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "stream_snapshot_codec.h"

using namespace ydc::snap;

static int g_failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      ++g_failures;                       \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);  \
      std::fprintf(stderr, "\n");         \
    }                                     \
  } while (0)

template <typename T>
static void put(const uint8_t* col, uint64_t i, T v) {
  std::memcpy(const_cast<uint8_t*>(col) + i * sizeof(T), &v, sizeof(T));
}

static void seal(std::vector<uint8_t>& b) {
  const uint64_t sum = checksum(b.data(), b.size());
  std::memcpy(b.data() + offsetof(Header, checksum), &sum, 8);
}

// A well-formed blob of the given mode and counts, its columns filled from `seed`.
static std::vector<uint8_t> good(uint32_t mode, uint32_t n, uint32_t env_words, uint32_t n_alias, uint32_t nl,
                                 uint32_t nw, uint32_t nb, uint32_t seed) {
  std::mt19937_64 rng(seed);
  Header h{};
  h.magic = kMagic;
  h.version = kVersion;
  h.mode = mode;
  h.env_words = env_words;
  h.n_servants = n;
  h.n_alias = n_alias;
  h.caps[kUpdates] = 16, h.caps[kReleases] = 16, h.caps[kTasks] = 64;
  if (mode & kModeWaiting) h.caps[kWaiting] = nw + 5;
  if (mode & kModeLeased) {
    h.caps[kLeases] = nl + 9, h.caps[kRenewals] = 8, h.caps[kFrees] = 8, h.caps[kReports] = 4, h.caps[kReportIds] = 32;
    h.lease_tick = 12;
    h.next_id = (1ull << 40) + 10ull * nl + 1;
  }
  if (mode & kModeRpc) h.caps[kRows] = 64 + 6 * nw;
  if (mode & kModeBook) h.max_book = nb + 3;
  h.n_leases = nl, h.n_waiting = nw, h.n_book = nb;
  h.last_now = 1234;
  h.alive_bound = INT64_MAX;
  layout(&h);
  std::vector<uint8_t> b(h.total_bytes, 0);
  View v{};
  v.h = h;
  place(&v, b.data());
  for (uint64_t i = 0; i < (uint64_t)n * env_words; ++i) put<uint64_t>(v.env_mask, i, rng());
  for (const uint8_t* col : {v.version, v.nproc, v.load, v.max_tasks, v.flags, v.ip, v.running, v.rep_tick})
    for (uint32_t s = 0; s < n; ++s) put<uint32_t>(col, s, (uint32_t)rng());
  for (uint32_t a = 0; a < n_alias; ++a) put<uint32_t>(v.alias_ip, a, (uint32_t)rng()), put<uint32_t>(v.alias_servant, a, a % n);
  for (uint32_t i = 0; i < nl; ++i) {
    put<uint64_t>(v.l_id, i, (1ull << 40) + 10ull * i + rng() % 10);
    put<int64_t>(v.l_exp, i, (int64_t)(rng() % 100000) - 50);
    put<uint32_t>(v.l_srv, i, (uint32_t)(rng() % n));
    put<uint32_t>(v.l_state, i, kLive | ((uint32_t)rng() & 0x7FFFFFFFu));
  }
  uint32_t rows = 0;
  for (uint32_t i = 0; i < nw; ++i) {
    put<int64_t>(v.w_deadline, i, (int64_t)(rng() % 1000));
    put<uint64_t>(v.w_tag, i, rng());
    if (mode & kModeLeased) put<int64_t>(v.w_for, i, (int64_t)(rng() % 50));
    put<uint32_t>(v.w_env, i, (uint32_t)rng() % 70), put<uint32_t>(v.w_minv, i, (uint32_t)rng() % 5), put<uint32_t>(v.w_ip, i, (uint32_t)rng());
    if (mode & kModeRpc) {
      const uint32_t a = (uint32_t)(rng() % 3), p = (uint32_t)(rng() % 3) + (a ? 0 : 1);
      put<uint32_t>(v.w_nimm, i, a), put<uint32_t>(v.w_npre, i, p);
      rows += a + p;
    }
  }
  for (uint32_t i = 0; i < nb; ++i) {
    put<uint64_t>(v.b_grant, i, rng()), put<uint64_t>(v.b_stid, i, rng()), put<uint64_t>(v.b_dkey, i, rng());
    put<uint32_t>(v.b_srv, i, (uint32_t)(rng() % n));
  }
  if (mode & kModeAlive) {
    for (uint32_t s = 0; s < n; ++s) {
      const int64_t e = 2000 + (int64_t)(rng() % 100);
      put<int64_t>(v.e_exp, s, e);
      if (e < h.alive_bound) h.alive_bound = e;
    }
  }
  h.n_wait_rows = rows;
  std::memcpy(b.data(), &h, sizeof h);
  seal(b);
  return b;
}

// validate() on a copy of exactly `bytes` bytes; odd: the copy starts at an odd address.
static const char* check(const uint8_t* p, size_t bytes, bool odd, View* v) {
  uint8_t* block = (uint8_t*)std::malloc(bytes + (odd ? 1 : 0) + (bytes + (odd ? 1 : 0) == 0 ? 1 : 0));
  uint8_t* at = block + (odd ? 1 : 0);
  if (bytes) std::memcpy(at, p, bytes);
  const char* why = validate(at, bytes, v);
  uint64_t touched = 0;
  if (!why) {
    // What a restore reads: every element of every column.
    const Header& h = v->h;
    for (uint64_t i = 0; i < (uint64_t)h.n_servants * h.env_words; ++i) touched += get<uint64_t>(v->env_mask, i);
    for (const uint8_t* col : {v->version, v->nproc, v->load, v->max_tasks, v->flags, v->ip, v->running, v->rep_tick})
      for (uint32_t s = 0; s < h.n_servants; ++s) touched += get<uint32_t>(col, s);
    for (uint32_t a = 0; a < h.n_alias; ++a) touched += get<uint32_t>(v->alias_ip, a) + get<uint32_t>(v->alias_servant, a);
    for (uint32_t i = 0; i < h.n_leases; ++i)
      touched += get<uint64_t>(v->l_id, i) + (uint64_t)get<int64_t>(v->l_exp, i) + get<uint32_t>(v->l_srv, i) + get<uint32_t>(v->l_state, i);
    for (uint32_t i = 0; i < h.n_waiting; ++i) {
      touched += (uint64_t)get<int64_t>(v->w_deadline, i) + get<uint64_t>(v->w_tag, i) + get<uint32_t>(v->w_env, i) +
                 get<uint32_t>(v->w_minv, i) + get<uint32_t>(v->w_ip, i);
      if (h.mode & kModeLeased) touched += (uint64_t)get<int64_t>(v->w_for, i);
      if (h.mode & kModeRpc) touched += get<uint32_t>(v->w_nimm, i) + get<uint32_t>(v->w_npre, i);
    }
    for (uint32_t i = 0; i < h.n_book; ++i)
      touched += get<uint64_t>(v->b_grant, i) + get<uint64_t>(v->b_stid, i) + get<uint64_t>(v->b_dkey, i) + get<uint32_t>(v->b_srv, i);
    if (h.mode & kModeAlive)
      for (uint32_t s = 0; s < h.n_servants; ++s) touched += (uint64_t)get<int64_t>(v->e_exp, s);
  }
  if (touched == 0x0123456789ABCDEFull) std::printf("%s", "");  // (the reads above are not dead code)
  v->base = nullptr;  // (the copy is gone)
  std::free(block);
  return why;
}

int main() {
  const uint32_t WL = kModeWaiting | kModeLeased;
  std::vector<std::vector<uint8_t>> blobs = {
      good(kModeLeased, 5, 1, 0, 7, 0, 0, 1),
      good(kModeLeased, 0, 1, 0, 0, 0, 0, 2),
      good(kModeWaiting, 9, 1, 2, 0, 3, 0, 3),
      good(WL, 33, 2, 3, 65, 11, 0, 4),
      good(WL | kModeRpc, 12, 1, 0, 20, 6, 0, 5),
      good(WL | kModeRpc | kModeBook | kModeAlive, 17, 3, 1, 40, 5, 9, 6),
      good(kModeLeased | kModeAlive, 3, 1, 0, 1, 0, 0, 7),
  };
  unsigned cases = 0, accepted_after_fix = 0;
  View v;
  std::mt19937_64 rng(99);
  for (size_t k = 0; k < blobs.size(); ++k) {
    const std::vector<uint8_t>& g = blobs[k];
    const char* why = check(g.data(), g.size(), false, &v);
    EXPECT(!why, "good blob %zu refused: %s", k, why);
    why = check(g.data(), g.size(), true, &v);
    EXPECT(!why, "good blob %zu refused at an odd address: %s", k, why);
    Header h;
    std::memcpy(&h, g.data(), sizeof h);
    // Truncations: every length around the header and the sections' ends, and a stride through the rest.
    std::vector<size_t> cuts = {0, 1, 7, 8, sizeof(Header) - 1, sizeof(Header), g.size() - 1, g.size() - 8};
    for (int s = 0; s < kSections; ++s)
      for (int d = -1; d <= 1; ++d) cuts.push_back((size_t)(h.dir[s].offset + h.dir[s].bytes) + d);
    for (size_t c = 0; c < g.size(); c += 37) cuts.push_back(c);
    for (size_t c : cuts) {
      if (c >= g.size()) continue;
      ++cases;
      EXPECT(check(g.data(), c, c & 1, &v), "blob %zu cut to %zu bytes was accepted", k, c);
    }
    // One byte longer (the tail is not the block's).
    {
      std::vector<uint8_t> b = g;
      b.push_back(0);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with a byte behind it was accepted", k);
    }
    // Flipped bits: as they are (the checksum refuses every one), and with the checksum made right
    // again (whatever is then accepted is read in full above).
    for (int i = 0; i < 120; ++i) {
      std::vector<uint8_t> b = g;
      const size_t at = rng() % b.size();
      b[at] ^= (uint8_t)(1u << (rng() % 8));
      ++cases;
      EXPECT(check(b.data(), b.size(), i & 1, &v), "blob %zu with byte %zu flipped was accepted", k, at);
      if (at >= offsetof(Header, checksum) && at < offsetof(Header, checksum) + 8) continue;
      seal(b);
      ++cases;
      accepted_after_fix += check(b.data(), b.size(), i & 1, &v) == nullptr;
    }
    // Counts, sizes and offsets overwritten with extremes, the checksum made right: all refused.
    const size_t u32_fields[] = {offsetof(Header, version),    offsetof(Header, header_bytes), offsetof(Header, mode),
                                 offsetof(Header, env_words),  offsetof(Header, n_servants),   offsetof(Header, n_alias),
                                 offsetof(Header, n_leases),   offsetof(Header, n_waiting),    offsetof(Header, n_wait_rows),
                                 offsetof(Header, n_book)};
    for (size_t f : u32_fields) {
      uint32_t orig;
      std::memcpy(&orig, g.data() + f, 4);
      for (uint32_t x : {0u, 1u, 7u, 8u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, orig + 1, orig - 1, orig * 2 + 1}) {
        if (x == orig) continue;
        // (without servants no mask word exists: any env_words in range describes the same bytes)
        if (f == offsetof(Header, env_words) && h.n_servants == 0 && x >= 1 && x <= kMaxEnvWords) continue;
        std::vector<uint8_t> b = g;
        std::memcpy(b.data() + f, &x, 4);
        seal(b);
        ++cases;
        EXPECT(check(b.data(), b.size(), x & 1, &v), "blob %zu with the u32 at %zu set to %u was accepted", k, f, x);
      }
    }
    std::vector<size_t> u64_fields = {offsetof(Header, magic), offsetof(Header, total_bytes)};
    for (int s = 0; s < kSections; ++s) {
      u64_fields.push_back(offsetof(Header, dir) + 16 * s);
      u64_fields.push_back(offsetof(Header, dir) + 16 * s + 8);
    }
    for (size_t f : u64_fields) {
      uint64_t orig;
      std::memcpy(&orig, g.data() + f, 8);
      const uint64_t extremes[] = {0, 8, sizeof(Header), 1ull << 63, ~0ull, ~0ull - 7, orig + 8, orig - 8, g.size()};
      for (uint64_t x : extremes) {
        if (x == orig) continue;
        std::vector<uint8_t> b = g;
        std::memcpy(b.data() + f, &x, 8);
        seal(b);
        ++cases;
        EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with the u64 at %zu set to %llu was accepted", k, f,
               (unsigned long long)x);
      }
    }
    // Contents: ids out of order, an id at next_id, a lease without the live bit, indexes at n_servants.
    if (h.n_leases >= 2) {
      v.h = h;
      std::vector<uint8_t> b = g;
      place(&v, b.data());
      put<uint64_t>(v.l_id, 1, get<uint64_t>(v.l_id, 0));
      seal(b);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with two equal ids was accepted", k);
      b = g, v.h = h, place(&v, b.data());
      put<uint64_t>(v.l_id, h.n_leases - 1, h.next_id);
      seal(b);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with an id at next_id was accepted", k);
      b = g, v.h = h, place(&v, b.data());
      put<uint32_t>(v.l_state, 1, get<uint32_t>(v.l_state, 1) & ~kLive);
      seal(b);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with a lease that is not live was accepted", k);
      b = g, v.h = h, place(&v, b.data());
      put<uint32_t>(v.l_srv, 0, h.n_servants);
      seal(b);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with a lease on servant n_servants was accepted", k);
    }
    if (h.n_book) {
      std::vector<uint8_t> b = g;
      v.h = h, place(&v, b.data());
      put<uint32_t>(v.b_srv, h.n_book - 1, 0xFFFFFFFFu);
      seal(b);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with a book entry on no servant was accepted", k);
    }
    if (h.n_alias) {
      std::vector<uint8_t> b = g;
      v.h = h, place(&v, b.data());
      put<uint32_t>(v.alias_servant, 0, h.n_servants);
      seal(b);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with an alias of no servant was accepted", k);
    }
    if (h.mode & kModeRpc) {
      std::vector<uint8_t> b = g;
      v.h = h, place(&v, b.data());
      put<uint32_t>(v.w_nimm, 0, 0u), put<uint32_t>(v.w_npre, 0, 0u);
      seal(b);
      ++cases;
      EXPECT(check(b.data(), b.size(), false, &v), "blob %zu with an RPC of no rows was accepted", k);
    }
  }
  std::printf("%u corruptions of %zu blobs, %u still well-formed after the checksum was made right\n", cases,
              blobs.size(), accepted_after_fix);
  if (g_failures) {
    std::printf("SNAPSHOT-CODEC-FAILED (%d)\n", g_failures);
    return 1;
  }
  std::printf("SNAPSHOT-CODEC-OK\n");
  return 0;
}

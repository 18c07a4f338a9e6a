// inspect_delta_codec_test.cc — yadcc_amd/csrc/stream_inspect_delta_codec.h as a program of its own, built
// with ASan + UBSan by tests/test_stream_inspect_delta_codec.py. It includes only the codec headers.
//
//   (no argument)           good sidecars of every edge size validate; a few thousand seeded corruptions —
//                           flipped bytes, cuts, overwritten header fields and column entries, sealed again
//                           or not — are refused or, where a sealed one is accepted, are well-formed by an
//                           independent check. Every blob is validated out of a heap block of exactly its
//                           size, so a read beyond it is the sanitizer's to report. Prints INSPECT-CODEC-OK.
//   build <columns> <out>   the sidecar of a column file (nine u64 words kind, n_servants, n, stamp, next_id,
//                           last_now, lease_tick, n_leases, epoch; then the seven columns unpadded).
//   check <blob>            exit code 0: validate() accepts the file's bytes; 1: it refuses them.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "stream_inspect_delta_codec.h"

namespace insd = ydc::insd;
namespace snap = ydc::snap;

static int failures = 0;
#define EXPECT(cond, ...)                                \
  do {                                                   \
    if (!(cond)) {                                       \
      ++failures;                                        \
      fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);    \
      fprintf(stderr, __VA_ARGS__);                      \
      fprintf(stderr, "\n");                             \
    }                                                    \
  } while (0)

struct Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};

// validate() over a heap copy of exactly `bytes` bytes.
static const char* validate_exact(const uint8_t* p, size_t bytes, insd::View* v) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes ? bytes : 1]);
  if (bytes) memcpy(exact.get(), p, bytes);
  const char* why = insd::validate(bytes ? exact.get() : nullptr, bytes, v);
  if (!why) {  // (the view points into the copy: read what a caller would read, then forget it)
    uint64_t sum = 0;
    for (uint64_t i = 0; i < v->h.n; ++i)
      sum += insd::get<uint64_t>(v->id, i) + (uint64_t)insd::get<int64_t>(v->started_at, i) + insd::get<uint32_t>(v->env_id, i) +
             insd::get<uint32_t>(v->requestor_ip, i) + v->prefetch[i];
    for (uint64_t s = 0; s < v->h.n_servants; ++s)
      sum += (uint64_t)insd::get<int64_t>(v->discovered_at, s) + insd::get<uint64_t>(v->ever_assigned, s);
    volatile uint64_t sink = sum;
    (void)sink;
    v->base = nullptr;
  }
  return why;
}

// What a well-formed sidecar is, written down a second time.
static bool well_formed(const std::vector<uint8_t>& b) {
  if (b.size() < 120 || b.size() % 8) return false;
  auto u32 = [&](size_t at) { uint32_t x; memcpy(&x, &b[at], 4); return x; };
  auto u64 = [&](size_t at) { uint64_t x; memcpy(&x, &b[at], 8); return x; };
  const uint64_t kind = u32(32), S = u32(36), n = u32(40), next_id = u64(56), L = u32(76);
  if (u64(0) != insd::kMagic || u32(8) != 1 || u32(12) != 120 || u64(16) != b.size() || kind > 1 || u32(44)) return false;
  const uint64_t rec = (n * 25 + 7) & ~7ull, srv = S * 16;
  if (b.size() != 120 + rec + srv || n > L || (kind == 0 && n != L) || L > next_id) return false;
  if (u64(88) != 120 || u64(96) != rec || u64(104) != 120 + rec || u64(112) != srv) return false;
  if (u32(72) && !(u32(72) & snap::kStamp)) return false;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t id = u64(120 + i * 8);
    if (id >= next_id || (i && id <= u64(120 + (i - 1) * 8)) || b[120 + n * 24 + i] > 1) return false;
  }
  for (uint64_t i = n * 25; i < rec; ++i)
    if (b[120 + i]) return false;
  return snap::checksum(b.data(), b.size()) == u64(24);
}

static std::vector<uint8_t> good(Rng& r, uint32_t kind, uint32_t n, uint32_t S, uint64_t first_id) {
  std::vector<uint64_t> id(n), ever(S);
  std::vector<int64_t> at(n), disc(S);
  std::vector<uint32_t> env(n), ip(n);
  std::vector<uint8_t> pre(n);
  uint64_t next = first_id;
  for (uint32_t i = 0; i < n; ++i) {
    next += 1 + r.below(3);
    id[i] = next - 1;
    const bool none = r.below(5) == 0;
    at[i] = none ? INT64_MIN : (int64_t)r.below(1 << 20);
    env[i] = none ? 0xFFFFFFFFu : (uint32_t)r.below(70);
    ip[i] = none ? 0xFFFFFFFFu : (uint32_t)r.next();
    pre[i] = (uint8_t)r.below(2);
  }
  for (uint32_t s = 0; s < S; ++s) disc[s] = (int64_t)r.below(1000), ever[s] = r.next();
  insd::Header h = insd::describe(kind, S, n);
  h.stamp = r.next(), h.next_id = next + r.below(4), h.last_now = (int64_t)r.below(1000), h.lease_tick = 1 + (uint32_t)r.below(1000);
  h.n_leases = kind == insd::kFull ? n : n + (uint32_t)r.below(100), h.epoch = 1 + r.below(5);
  if (h.next_id < h.n_leases) h.next_id = h.n_leases;
  std::vector<uint8_t> out;
  insd::build(h, insd::Columns{id.data(), at.data(), env.data(), ip.data(), pre.data(), disc.data(), ever.data()}, &out);
  return out;
}

static void reseal(std::vector<uint8_t>& b) {
  if (b.size() < 32 || b.size() % 8) return;
  memset(&b[24], 0, 8);
  const uint64_t c = snap::checksum(b.data(), b.size());
  memcpy(&b[24], &c, 8);
}

static int self_test() {
  Rng r{20240611};
  const uint32_t ns[] = {0, 1, 63, 64, 65, 1000}, servants[] = {1, 63, 64, 65, 257};
  std::vector<std::vector<uint8_t>> goods;
  for (uint32_t n : ns)
    for (uint32_t S : servants)
      for (uint32_t kind : {0u, 1u}) goods.push_back(good(r, kind, n, S, n == 65 ? 1ull << 40 : 0));
  insd::View v;
  for (const auto& g : goods) {
    const char* why = validate_exact(g.data(), g.size(), &v);
    EXPECT(!why, "a good sidecar is refused: %s", why ? why : "");
    EXPECT(well_formed(g), "a good sidecar is not well-formed by the second check");
    const uint64_t n = v.h.n, S = v.h.n_servants;
    EXPECT(g.size() == 120 + 8 * n + 8 * n + 4 * n + 4 * n + ((n + 7) & ~7ull) + 16 * S, "size of %llu records, %llu servants",
           (unsigned long long)n, (unsigned long long)S);
  }
  int refused = 0, accepted = 0;
  for (int k = 0; k < 6000; ++k) {
    std::vector<uint8_t> b = goods[r.below(goods.size())];
    const int what = (int)r.below(6);
    bool sealed_again = false;
    if (what == 0) {  // a flipped bit, as it is
      b[r.below(b.size())] ^= (uint8_t)(1u << r.below(8));
    } else if (what == 1) {  // cut anywhere
      b.resize(r.below(b.size()));
    } else if (what == 2) {  // a header word overwritten, sealed again
      const size_t at = 32 + 4 * r.below(22);
      uint32_t x = (uint32_t)(r.below(3) ? r.below(2000) : r.next());
      memcpy(&b[at], &x, 4);
      reseal(b), sealed_again = true;
    } else if (what == 3) {  // a byte behind the header overwritten, sealed again
      if (b.size() > 120) b[120 + r.below(b.size() - 120)] = (uint8_t)r.next();
      reseal(b), sealed_again = true;
    } else if (what == 4) {  // words appended or dropped, total_bytes following, sealed again
      if (r.below(2)) b.resize(b.size() + 8 * (1 + r.below(3)), 0);
      else if (b.size() >= 128) b.resize(b.size() - 8);
      const uint64_t t = b.size();
      memcpy(&b[16], &t, 8);
      reseal(b), sealed_again = true;
    } else {  // the counts swapped for huge ones, sealed again
      const uint32_t x = 0xFFFFFFFFu - (uint32_t)r.below(8);
      memcpy(&b[r.below(2) ? 36 : 40], &x, 4);
      reseal(b), sealed_again = true;
    }
    const char* why = validate_exact(b.data(), b.size(), &v);
    const bool wf = well_formed(b);
    EXPECT(!why == wf, "corruption %d (kind %d): validate says '%s', the second check says %d", k, what, why ? why : "ok", (int)wf);
    if (!sealed_again && what == 0) EXPECT(why, "a flipped bit was accepted (corruption %d)", k);
    why ? ++refused : ++accepted;
  }
  EXPECT(refused > 3000, "only %d corruptions were refused", refused);
  // A null block, and every length below a header.
  EXPECT(insd::validate(nullptr, 0, &v) && insd::validate(nullptr, 4096, &v), "a null block was accepted");
  for (size_t len = 0; len < 120; ++len) EXPECT(validate_exact(goods[0].data(), len, &v), "%zu bytes were accepted", len);
  if (failures) return 1;
  printf("INSPECT-CODEC-OK %zu good, %d refused, %d accepted and well-formed\n", goods.size(), refused, accepted);
  return 0;
}

static bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + k);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_test();
  const std::string cmd = argv[1];
  std::vector<uint8_t> in;
  if (cmd == "check" && argc == 3) {
    if (!read_file(argv[2], &in)) return 2;
    insd::View v;
    const char* why = validate_exact(in.data(), in.size(), &v);
    if (why) fprintf(stderr, "%s\n", why);
    return why ? 1 : 0;
  }
  if (cmd == "build" && argc == 4) {
    if (!read_file(argv[2], &in) || in.size() < 72) return 2;
    uint64_t w[9];
    memcpy(w, in.data(), 72);
    const uint64_t n = w[2], S = w[1];
    if (in.size() != 72 + n * 25 + S * 16) return 2;
    insd::Header h = insd::describe((uint32_t)w[0], (uint32_t)S, (uint32_t)n);
    h.stamp = w[3], h.next_id = w[4], h.last_now = (int64_t)w[5], h.lease_tick = (uint32_t)w[6], h.n_leases = (uint32_t)w[7];
    h.epoch = w[8];
    const uint8_t* p = in.data() + 72;
    const insd::Columns c{p, p + n * 8, p + n * 16, p + n * 20, p + n * 24, p + n * 25, p + n * 25 + S * 8};
    std::vector<uint8_t> out;
    insd::build(h, c, &out);
    FILE* f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: %s [build <columns> <out> | check <blob>]\n", argv[0]);
  return 2;
}

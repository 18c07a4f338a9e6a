// The host mirror of the registry (yadcc_amd/csrc/registry_mirror.h) against a naive model — a vector
// of per-servant structs — through seeded sequences of uploads, heartbeat lists (with appends, with
// and without masks, masks narrower and wider than the table), removals and alias changes, under
// ASan + UBSan. Includes nothing but the mirror. After every step every column, env_words and the
// alias lists are compared; for every heartbeat row `structural` is compared with the rule written
// out below from its description.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "registry_mirror.h"

using ydc::RegistryMirror;

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

struct Servant {
  uint32_t version = 0, nproc = 0, load = 0, max_tasks = 0, flags = 0, ip = 0;
  std::vector<uint64_t> env;  // Model::words words
};
struct Model {
  std::vector<Servant> sv;
  uint32_t words = 1;
  std::vector<std::pair<uint32_t, uint32_t>> alias;  // (ip, servant)
};

// Row i of a heartbeat list: its masks (empty: the list carries none).
static std::vector<uint64_t> row_masks(const uint64_t* masks, uint32_t words, uint32_t i) {
  if (!masks) return {};
  return std::vector<uint64_t>(masks + (size_t)i * words, masks + (size_t)(i + 1) * words);
}

// The rule: a new servant is structural; so is another version, host or capacity bound
// min(max_tasks, nproc), and max_tasks going to or from 0; an environment set differs when the
// shorter mask, extended with zero words, is unequal; a row without masks on a wider table keeps
// its environments.
static bool rule(const Model& m, uint32_t s, const ydc_servant_row& r, const uint64_t* masks, uint32_t words,
                 uint32_t i) {
  if (s >= m.sv.size()) return true;
  const Servant& v = m.sv[s];
  if (v.version != r.version || v.ip != r.ip_id) return true;
  if (std::min(v.max_tasks, v.nproc) != std::min(r.max_tasks, r.num_processors)) return true;
  if ((v.max_tasks == 0) != (r.max_tasks == 0)) return true;
  if (masks) {
    std::vector<uint64_t> have = v.env, want = row_masks(masks, words, i);
    have.resize(std::max(have.size(), want.size()), 0);
    want.resize(have.size(), 0);
    return have != want;
  }
  if (m.words == 1) return v.env[0] != r.env_mask;
  return false;
}

static void model_store(Model& m, uint32_t s, const ydc_servant_row& r, const uint64_t* masks, uint32_t words,
                        uint32_t i) {
  Servant& v = m.sv[s];
  v.version = r.version, v.nproc = r.num_processors, v.load = r.current_load, v.max_tasks = r.max_tasks;
  v.flags = r.flags, v.ip = r.ip_id;
  if (masks) {
    v.env = row_masks(masks, words, i);
    v.env.resize(m.words, 0);
  } else if (m.words == 1) {
    v.env[0] = r.env_mask;
  }
}

static void compare(const RegistryMirror& g, const Model& m, const char* after, uint32_t seq) {
  const size_t n = m.sv.size();
  EXPECT(g.n == n && g.env_words == m.words, "seq %u after %s: n %u / %zu, env_words %u / %u", seq, after, g.n, n,
         g.env_words, m.words);
  EXPECT(g.version.size() == n && g.nproc.size() == n && g.load.size() == n && g.max_tasks.size() == n &&
             g.flags.size() == n && g.ip.size() == n && g.env.size() == n * m.words,
         "seq %u after %s: column lengths", seq, after);
  if (g_failures) return;
  for (size_t s = 0; s < n; ++s) {
    const Servant& v = m.sv[s];
    EXPECT(g.version[s] == v.version && g.nproc[s] == v.nproc && g.load[s] == v.load && g.max_tasks[s] == v.max_tasks &&
               g.flags[s] == v.flags && g.ip[s] == v.ip,
           "seq %u after %s: row %zu", seq, after, s);
    for (uint32_t w = 0; w < m.words; ++w)
      EXPECT(g.env[s * m.words + w] == v.env[w], "seq %u after %s: mask word %u of row %zu", seq, after, w, s);
  }
  EXPECT(g.alias_ip.size() == m.alias.size() && g.alias_servant.size() == m.alias.size(), "seq %u after %s: %zu aliases / %zu",
         seq, after, g.alias_ip.size(), m.alias.size());
  for (size_t a = 0; a < m.alias.size() && a < g.alias_ip.size(); ++a)
    EXPECT(g.alias_ip[a] == m.alias[a].first && g.alias_servant[a] == m.alias[a].second, "seq %u after %s: alias %zu", seq,
           after, a);
}

struct Coverage {
  unsigned structural = 0, light = 0, appended = 0, widened = 0, wider_rows = 0, narrower_rows = 0, maskless_wide = 0;
  unsigned removed_first = 0, removed_last = 0, removed_all = 0, removed_none = 0, renumbered = 0, light_lists = 0;
};

static uint64_t mask_word(std::mt19937_64& rng) { return rng() & rng() & 0xFFFFull; }

static void upload(RegistryMirror& g, Model& m, std::mt19937_64& rng, uint32_t n, uint32_t words) {
  std::vector<uint32_t> col[7];
  for (auto& c : col) c.resize(n);
  std::vector<uint64_t> env((size_t)n * words);
  m.sv.assign(n, Servant{});
  m.words = words;
  m.alias.clear();
  for (uint32_t s = 0; s < n; ++s) {
    Servant& v = m.sv[s];
    v.version = col[0][s] = 1 + rng() % 3;
    v.nproc = col[1][s] = rng() % 9;
    v.load = col[2][s] = rng() % 5;
    v.max_tasks = col[3][s] = rng() % 7;
    col[4][s] = (uint32_t)rng();  // running_tasks: not mirrored
    v.flags = col[5][s] = rng() % 4;
    v.ip = col[6][s] = rng() % 40;
    v.env.resize(words);
    for (uint32_t w = 0; w < words; ++w) v.env[w] = env[(size_t)s * words + w] = mask_word(rng);
  }
  const ydc_servant_soa sv{col[0].data(), col[1].data(), col[2].data(), col[3].data(), col[4].data(),
                           col[5].data(), env.data(),    col[6].data(), rng() % 2 && words == 1 ? 0u : words};
  const bool no_table = !n && rng() % 2;  // (an upload of nothing may bring no table at all: one word then)
  g.assign(no_table ? nullptr : &sv, n);
  if (no_table) m.words = 1;
}

// One heartbeat list, applied the way ydc_update_servants_wide applies it (widen, append, row by row)
// or — when no row of it is structural — the way the small-batch path does (the four light columns).
static void update(RegistryMirror& g, Model& m, std::mt19937_64& rng, uint32_t seq, Coverage* cov) {
  const bool with_masks = rng() % 3 != 0;
  const uint32_t words = with_masks ? 1 + rng() % 3 : 1;
  const uint32_t k = rng() % 7;
  std::vector<uint32_t> idx;
  std::vector<ydc_servant_row> rows;
  std::vector<uint64_t> masks;
  uint32_t new_n = (uint32_t)m.sv.size();
  const bool may_append = (with_masks || m.words == 1) && rng() % 3 == 0;
  const bool quiet = rng() % 3 == 0;  // a list of light rows only
  for (uint32_t i = 0; i < k; ++i) {
    const bool append = !quiet && may_append && (new_n == 0 || rng() % 3 == 0);
    if (!append && new_n == 0) break;
    const uint32_t s = append ? new_n : rng() % new_n;
    if (append) ++new_n, ++cov->appended;
    ydc_servant_row r{};
    std::vector<uint64_t> e(words, 0);
    if (s < m.sv.size()) {  // an existing servant: its row, changed a little
      const Servant& v = m.sv[s];
      r = ydc_servant_row{v.version, v.nproc, v.load, v.max_tasks, v.flags, v.ip, v.env[0]};
      for (uint32_t w = 0; w < words && w < m.words; ++w) e[w] = v.env[w];
      switch (quiet ? rng() % 3 : rng() % 10) {
        case 0: r.current_load = rng() % 5; break;
        case 1: r.flags = rng() % 4; break;
        case 2:  // the larger of the two capacities moves: the bound stays
          if (r.max_tasks && r.max_tasks < r.num_processors) r.num_processors += 1;
          else if (r.num_processors < r.max_tasks) r.max_tasks += 1;
          break;
        case 3: r.version += 1; break;
        case 4: r.ip_id = rng() % 40; break;
        case 5: r.max_tasks = r.max_tasks ? 0 : 1 + rng() % 6; break;
        case 6: r.max_tasks = rng() % 7, r.num_processors = rng() % 9; break;
        case 7: e[rng() % words] ^= 1ull << (rng() % 16), r.env_mask = e[0]; break;
        case 8: e[words - 1] = mask_word(rng), r.env_mask = e[0]; break;
        default: break;  // the same row again
      }
    } else {
      r = ydc_servant_row{(uint32_t)(1 + rng() % 3), (uint32_t)(rng() % 9), (uint32_t)(rng() % 5), (uint32_t)(rng() % 7),
                          (uint32_t)(rng() % 4), (uint32_t)(rng() % 40), 0};
      for (auto& w : e) w = mask_word(rng);
      r.env_mask = e[0];
    }
    idx.push_back(s);
    rows.push_back(r);
    if (with_masks) masks.insert(masks.end(), e.begin(), e.end());
  }
  const uint32_t n_upd = (uint32_t)idx.size();
  const uint64_t* mp = with_masks ? masks.data() : nullptr;
  if (with_masks && n_upd && words > m.words) ++cov->wider_rows;
  if (with_masks && n_upd && words < m.words) ++cov->narrower_rows;
  if (!with_masks && n_upd && m.words > 1) ++cov->maskless_wide;
  // What a tick asks before anything is applied: every row against the registry as it stands
  // (new servants beyond its end, masks wider than the table).
  bool any = false;
  for (uint32_t i = 0; i < n_upd; ++i) {
    const bool got = g.structural(idx[i], rows[i], mp, words, i), want = rule(m, idx[i], rows[i], mp, words, i);
    EXPECT(got == want, "seq %u: structural(row %u of the list, servant %u) %d, the rule %d (before)", seq, i, idx[i], (int)got,
           (int)want);
    any |= want;
  }
  if (!any && n_upd && rng() % 2) {
    ++cov->light_lists;
    for (uint32_t i = 0; i < n_upd; ++i) {
      g.store_light(idx[i], rows[i]);
      Servant& v = m.sv[idx[i]];
      v.nproc = rows[i].num_processors, v.load = rows[i].current_load, v.max_tasks = rows[i].max_tasks, v.flags = rows[i].flags;
    }
    return compare(g, m, "light rows", seq);
  }
  if (with_masks) {
    const bool widened = g.widen_env(words);
    EXPECT(widened == (words > m.words), "seq %u: widen_env(%u) on %u words said %d", seq, words, m.words, (int)widened);
    if (words > m.words) {
      ++cov->widened;
      for (auto& v : m.sv) v.env.resize(words, 0);
      m.words = words;
    }
  }
  g.resize(new_n);
  while (m.sv.size() < new_n) {
    m.sv.push_back(Servant{});
    m.sv.back().env.assign(m.words, 0);
  }
  compare(g, m, "widen and append", seq);
  for (uint32_t i = 0; i < n_upd; ++i) {
    const bool got = g.structural(idx[i], rows[i], mp, words, i), want = rule(m, idx[i], rows[i], mp, words, i);
    EXPECT(got == want, "seq %u: structural(row %u of the list, servant %u) %d, the rule %d", seq, i, idx[i], (int)got, (int)want);
    ++(want ? cov->structural : cov->light);
    g.store_row(idx[i], rows[i], mp, words, i);
    model_store(m, idx[i], rows[i], mp, words, i);
  }
  compare(g, m, "an update list", seq);
}

static void set_aliases(RegistryMirror& g, Model& m, std::mt19937_64& rng) {
  m.alias.clear();
  g.clear_aliases();
  if (m.sv.empty()) return;
  for (uint32_t a = 0, k = rng() % 6; a < k; ++a) {
    m.alias.emplace_back(100 + (uint32_t)(rng() % 50), (uint32_t)(rng() % m.sv.size()));
    g.alias_ip.push_back(m.alias.back().first);
    g.alias_servant.push_back(m.alias.back().second);
  }
}

static void remove(RegistryMirror& g, Model& m, std::mt19937_64& rng, uint32_t seq, Coverage* cov) {
  const uint32_t n = (uint32_t)m.sv.size();
  std::vector<uint32_t> gone;
  switch (rng() % 5) {
    case 0: if (n) gone = {0}, ++cov->removed_first; break;
    case 1: if (n) gone = {n - 1}, ++cov->removed_last; break;
    case 2: for (uint32_t s = 0; s < n; ++s) gone.push_back(s); ++cov->removed_all; break;
    case 3: ++cov->removed_none; break;
    default: for (uint32_t s = 0; s < n; ++s) if (rng() % 4 == 0) gone.push_back(s); break;
  }
  const bool in_tick = rng() % 2;
  // The model: rows erased from the back, aliases of erased rows dropped, the others shifted down.
  std::vector<std::pair<uint32_t, uint32_t>> alias;
  if (in_tick) {
    for (auto& a : m.alias) {
      if (std::binary_search(gone.begin(), gone.end(), a.second)) continue;
      uint32_t below = 0;
      for (uint32_t s : gone) below += s < a.second;
      alias.emplace_back(a.first, a.second - below);
    }
    if (!m.alias.empty() && !gone.empty()) ++cov->renumbered;
  }
  m.alias = alias;
  for (size_t j = gone.size(); j-- > 0;) m.sv.erase(m.sv.begin() + gone[j]);
  g.compact(gone.data(), (uint32_t)gone.size());
  if (in_tick) g.renumber_aliases(gone.data(), (uint32_t)gone.size());
  else g.clear_aliases();
  compare(g, m, "a removal", seq);
}

int main() {
  Coverage cov;
  const uint32_t sizes[] = {0, 1, 70};
  uint32_t sequences = 0;
  for (uint32_t seed = 1; seed <= 300 && !g_failures; ++seed, ++sequences) {
    std::mt19937_64 rng(seed);
    RegistryMirror g;
    Model m;
    upload(g, m, rng, sizes[seed % 3], seed % 2 ? 1 : 3);
    compare(g, m, "an upload", seed);
    for (uint32_t step = 0; step < 24 && !g_failures; ++step) {
      switch (rng() % 8) {
        case 0: remove(g, m, rng, seed, &cov); break;
        case 1:
          set_aliases(g, m, rng);
          compare(g, m, "aliases", seed);
          break;
        case 2:
          if (rng() % 4 == 0) {
            upload(g, m, rng, sizes[rng() % 3], rng() % 2 ? 1 : 3);
            compare(g, m, "an upload", seed);
            break;
          }
          [[fallthrough]];
        default: update(g, m, rng, seed, &cov); break;
      }
    }
  }
  // Every kind of step and both verdicts were met (a generator that stopped producing one would
  // leave the comparison above vacuous).
  EXPECT(cov.structural > 100 && cov.light > 100 && cov.appended > 20 && cov.widened > 5 && cov.wider_rows > 5 &&
             cov.narrower_rows > 20 && cov.maskless_wide > 20 && cov.light_lists > 20,
         "coverage: structural %u light %u appended %u widened %u wider %u narrower %u maskless-on-wide %u light lists %u",
         cov.structural, cov.light, cov.appended, cov.widened, cov.wider_rows, cov.narrower_rows, cov.maskless_wide,
         cov.light_lists);
  EXPECT(cov.removed_first > 5 && cov.removed_last > 5 && cov.removed_all > 5 && cov.removed_none > 5 && cov.renumbered > 5,
         "coverage: removals first %u last %u all %u none %u, renumbered %u", cov.removed_first, cov.removed_last,
         cov.removed_all, cov.removed_none, cov.renumbered);
  if (g_failures) {
    std::fprintf(stderr, "%d failure(s)\n", g_failures);
    return 1;
  }
  std::printf("REGISTRY-MIRROR-OK %u sequences: %u structural and %u light rows, %u appended, %u light lists\n", sequences,
              cov.structural, cov.light, cov.appended, cov.light_lists);
  return 0;
}

// registry_mirror.h — the host's copy of the registry: the columns the derived tables
// (host_tables.h) are built from and the small-batch path reads its limits from, the host
// aliases, and the rule that says which heartbeat rows change those tables. Host-only and
// free of HIP, so that a plain C++ program can drive it (tests/native/registry_mirror_test.cc).
// running_tasks is not here: it lives on the device alone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/yadcc_dispatch.h"

namespace ydc {

struct RegistryMirror {
  uint32_t n = 0;          // servants (rows of every column)
  uint32_t env_words = 1;  // mask words per servant in `env`
  std::vector<uint32_t> version, nproc, load, max_tasks, flags, ip;
  std::vector<uint64_t> env;
  std::vector<uint32_t> alias_ip, alias_servant;  // ydc_set_host_aliases: further ip table entries

  // The whole registry replaced by an upload (sv == NULL: by nothing). The aliases named rows
  // of the old table and go with it.
  void assign(const ydc_servant_soa* sv, uint32_t rows) {
    n = sv ? rows : 0;
    env_words = sv && sv->env_words ? sv->env_words : 1;
    auto col = [&](std::vector<uint32_t>& to, const uint32_t* from) {
      if (n) to.assign(from, from + n);
      else to.clear();
    };
    col(version, sv ? sv->version : nullptr);
    col(nproc, sv ? sv->num_processors : nullptr);
    col(load, sv ? sv->current_load : nullptr);
    col(max_tasks, sv ? sv->max_tasks : nullptr);
    col(flags, sv ? sv->flags : nullptr);
    col(ip, sv ? sv->ip_id : nullptr);
    if (n) env.assign(sv->env_mask, sv->env_mask + (size_t)n * env_words);
    else env.clear();
    clear_aliases();
  }

  // Rows [n, rows) appear zeroed, rows [rows, n) go.
  void resize(uint32_t rows) {
    for (auto* c : {&version, &nproc, &load, &max_tasks, &flags, &ip}) c->resize(rows);
    env.resize((size_t)rows * env_words);
    n = rows;
  }

  // Lays the masks out for `words` words per servant; true if that widened them (the device holds
  // per-class masks only, which are derived from this copy: the tables are to be rebuilt).
  bool widen_env(uint32_t words) {
    if (words <= env_words) return false;
    std::vector<uint64_t> wide((size_t)n * words, 0);
    for (uint32_t s = 0; s < n; ++s)
      for (uint32_t w = 0; w < env_words; ++w) wide[(size_t)s * words + w] = env[(size_t)s * env_words + w];
    env.swap(wide);
    env_words = words;
    return true;
  }

  // A heartbeat row for servant s that changes what the derived tables are built from (classes,
  // the ip table, the slot bound): a new servant, another version / host / capacity bound, or (row
  // i of env_masks, words words each) another environment set, the shorter of the two masks
  // extended with zero words. A row without masks on a table of several mask words cannot say what
  // the servant advertises: it keeps its environments.
  bool structural(uint32_t s, const ydc_servant_row& r, const uint64_t* env_masks, uint32_t words, uint32_t i) const {
    if (s >= n) return true;
    bool env_changed = false;
    if (env_masks) {
      for (uint32_t w = 0; w < std::max(env_words, words); ++w) {
        const uint64_t have = w < env_words ? env[(size_t)s * env_words + w] : 0;
        const uint64_t want = w < words ? env_masks[(size_t)i * words + w] : 0;
        env_changed |= have != want;
      }
    } else if (env_words == 1) {
      env_changed = env[s] != r.env_mask;
    }
    return env_changed || version[s] != r.version || ip[s] != r.ip_id || (max_tasks[s] == 0) != (r.max_tasks == 0) ||
           std::min(max_tasks[s], nproc[s]) != std::min(r.max_tasks, r.num_processors);
  }

  // The four columns a heartbeat that changes no structure replaces.
  void store_light(uint32_t s, const ydc_servant_row& r) {
    nproc[s] = r.num_processors;
    load[s] = r.current_load;
    max_tasks[s] = r.max_tasks;
    flags[s] = r.flags;
  }

  // The whole row (s < n; words <= env_words: widen_env first). Mask words the row does not carry
  // are zero; a row without masks is its one word, and on a wider table keeps its environments.
  void store_row(uint32_t s, const ydc_servant_row& r, const uint64_t* env_masks, uint32_t words, uint32_t i) {
    store_light(s, r);
    version[s] = r.version;
    ip[s] = r.ip_id;
    uint64_t* e = &env[(size_t)s * env_words];
    if (env_masks)
      for (uint32_t w = 0; w < env_words; ++w) e[w] = w < words ? env_masks[(size_t)i * words + w] : 0;
    else if (env_words == 1)
      e[0] = r.env_mask;
  }

  // Order-preserving removal of the rows removed[0 .. k) (ascending, < n) from every column. The
  // aliases are the caller's: renumber_aliases or clear_aliases.
  void compact(const uint32_t* removed, uint32_t k) {
    uint32_t w = 0, next = 0;
    for (uint32_t s = 0; s < n; ++s) {
      if (next < k && removed[next] == s) {
        ++next;
        continue;
      }
      if (w != s) {
        for (auto* c : {&version, &nproc, &load, &max_tasks, &flags, &ip}) (*c)[w] = (*c)[s];
        std::copy_n(&env[(size_t)s * env_words], env_words, &env[(size_t)w * env_words]);
      }
      ++w;
    }
    resize(w);
  }

  // The aliases after the same removal: those of removed rows go, the others name their servant
  // by its new number.
  void renumber_aliases(const uint32_t* removed, uint32_t k) {
    size_t wa = 0;
    for (size_t a = 0; a < alias_servant.size(); ++a) {
      const uint32_t s = alias_servant[a];
      const uint32_t before = (uint32_t)(std::lower_bound(removed, removed + k, s) - removed);
      if (before < k && removed[before] == s) continue;
      alias_ip[wa] = alias_ip[a];
      alias_servant[wa++] = s - before;
    }
    alias_ip.resize(wa);
    alias_servant.resize(wa);
  }

  void clear_aliases() {
    alias_ip.clear();
    alias_servant.clear();
  }
};

}  // namespace ydc

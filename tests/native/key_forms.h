// tests/native/key_forms.h — TEST TOOL, not product code.
//
// One case of the closed forms of dispatch_core.h (the keys of a slot, first_slot_not_below in its
// three forms, servant_slots_before in both key formats) evaluated from a table row. Compiled for
// the host by tests/model (model_check_key_forms) and for gfx950 by tests/native/key_forms_gpu.hip;
// the table is written by tests/key_edge_cases.py (FORM_DTYPE / FORM_OUT_DTYPE: same layout).
#ifndef YADCC_AMD_TESTS_KEY_FORMS_H_
#define YADCC_AMD_TESTS_KEY_FORMS_H_

#include "../../yadcc_amd/csrc/dispatch_core.h"

namespace ydc {

struct KeyFormCase {
  uint32_t nproc, load, max_tasks, running, flags, s, head_servant, cap_bits, r, fp64;
  uint64_t part_key, K;
};
struct KeyFormOut {
  uint64_t key_exact, key_fp64;  // of slot r (0 when r is no slot of the servant)
  uint32_t first, first_direct, first_direct32, before_exact, before_fp64, pad;
};
static_assert(sizeof(KeyFormCase) == 56 && sizeof(KeyFormOut) == 40, "layout of tests/key_edge_cases.py");

constexpr uint32_t kKeyFormNotRun = 0xFFFFFFFFu;  // first_direct32 outside its domain

YDC_HD bool key_form_direct32_applies(const KeyFormCase& c) {
  return c.cap_bits <= 10 && c.K < (1ull << 32) && c.part_key < (1ull << 32);
}

YDC_HD void key_forms_eval(const KeyFormCase& c, KeyFormOut& o) {
  const uint32_t n = servant_slot_count(c.nproc, c.load, c.max_tasks, c.running, c.flags);
  const bool has = n && c.r >= c.running && c.r < c.running + n;
  o.key_exact = o.key_fp64 = 0;
  if (has) {
    const uint32_t cap = slot_capacity(c.nproc, c.load, c.max_tasks, c.r), tier = slot_tier(c.nproc, c.flags, c.r);
    o.key_exact = slot_key_exact(tier, c.r, cap, c.cap_bits);
    o.key_fp64 = slot_key_fp64(tier, c.r, cap);
  }
  o.first = first_slot_not_below(c.nproc, c.load, c.max_tasks, c.running, c.flags, c.part_key, c.K, c.cap_bits);
  o.first_direct =
      first_slot_not_below_direct(c.nproc, c.load, c.max_tasks, c.running, c.flags, c.part_key, c.K, c.cap_bits);
  o.first_direct32 = key_form_direct32_applies(c)
                         ? first_slot_not_below_direct32(c.nproc, c.load, c.max_tasks, c.running, c.flags,
                                                         (uint32_t)c.part_key, (uint32_t)c.K, c.cap_bits)
                         : kKeyFormNotRun;
  o.before_exact = servant_slots_before(c.nproc, c.load, c.max_tasks, c.running, c.flags, c.s, c.part_key, c.K,
                                        c.head_servant, true, c.cap_bits);
  // (registries with fp64 keys are one part: no part id rides on a double)
  o.before_fp64 = servant_slots_before(c.nproc, c.load, c.max_tasks, c.running, c.flags, c.s, 0ull, c.K,
                                       c.head_servant, false, c.cap_bits);
  o.pad = 0;
}

}  // namespace ydc
#endif  // YADCC_AMD_TESTS_KEY_FORMS_H_

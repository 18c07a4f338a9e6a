"""Many-class matching at its thresholds, on the CPU: every case of tests/class_edge_cases.py —
a class count on each side of every threshold of the planner, eligible-class rows of every
staged length, 16 and 17 versions, the table of 2^20 words, the two LDS bounds and the bit budget
of k_walk_groups, and the hand-made blocks for its commit rule — is verified BEFORE a GPU sees
it: the oracle's literal restatement equals its slot-order form, the CPU model (tests/model, built
from the headers the kernels use) and the verbatim reference (oracle/_ref, where it is built) —
placement, utilisation doubles and running_tasks, all EQUAL —; plan_of names the path the case
was made for; and the counts the case promises hold in the oracle's answer."""
import numpy as np
import pytest

from oracle import oraclebind as O
from oracle import refbind as R
from tests import class_edge_cases as K
from tests.model import modelbind as M

CASES = K.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_what_it_claims_and_every_cpu_reference_agrees(case):
    sv, tk = case.data()
    n = len(tk["env_id"])
    want, wutil, wrun = O.dispatch(sv, tk, "scan")
    got, gutil, grun = O.dispatch(sv, tk, "sorted")
    assert np.array_equal(got, want) and np.array_equal(gutil, wutil) and np.array_equal(grun, wrun)
    for chunk in (64, 256):
        got, gutil, grun, st = M.dispatch(sv, tk, chunk)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (case, chunk, bad[:5], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(gutil, wutil) and np.array_equal(grun, wrun), (case, chunk)
        assert st.n_classes == case.promise.get("C", st.n_classes)
    if R.available():
        d = R.RefDispatcher()
        d.load_servants(sv)
        ref_idx, _, _, _ = d.dispatch_batch(tk)
        d.close()
        assert np.array_equal(ref_idx, want), (case, np.nonzero(ref_idx != want)[0][:5])
    # ---- the path
    plan = K.plan_of(sv, n)
    assert plan["kernel"] == case.path, (case, {k: v for k, v in plan.items() if k != "row_len"})
    # ---- the promises
    pr = case.promise
    for key in ("C", "V", "rows_exist", "table_words", "walk_cbits"):
        if key in pr:
            assert plan[key] == pr[key], (case, key, plan[key])
    if pr.get("oversubscribed"):
        assert (want == K.TIMEOUT).sum() > 0
    if case.kind in ("count", "rows", "budget"):
        # own hosts, hosts with several servants, unknown digests, min_version on both sides
        assert (want == K.ENF).sum() > 0 and np.isin(tk["requestor_ip"], sv["ip"]).sum() > 20
        assert len(np.unique(sv["ip"])) < len(sv["ip"])
        assert tk["min_version"].min() < sv["version"].min() and tk["min_version"].max() > sv["version"].max()
        if case.kind == "count":
            assert (1000 <= n <= 2048 and plan["C"] <= K.MAX_WIDE_CLASSES) or n == 1024
    if "dense" in pr and pr["C"] > K.MAX_WAVE_CLASSES:  # (every row <= 64 classes / some row longer)
        assert (plan["elig_max_len"] > 64) == pr["dense"] and plan["lists_exist"]
    if pr.get("row_lens"):
        E = K.pair_digests(pr["C"])[0]
        assert tuple(plan["row_len"][E:E + len(pr["row_lens"]), 0]) == pr["row_lens"]
        for j in range(len(pr["row_lens"])):  # every made row is asked for, with the version threshold below all
            assert ((tk["env_id"] == E + j) & (tk["min_version"] == 0)).sum() >= 5, (case, j)
    if pr.get("slot_bound_plus_1"):
        assert plan["slot_bound"] + 1 == pr["slot_bound_plus_1"]
        assert (plan["slot_bound"] + 1 < 1 << (32 - plan["walk_cbits"])) == (case.path == K.WALK_PACKED)
        assert plan["walk_lds_packed"] <= K.GROUP_WALK_MAX_LDS  # (the LDS allows packing: the bits decide)
        free = np.minimum(sv["max_tasks"], sv["num_processors"]).astype(np.int64) - sv["running_tasks"]
        assert free[len(free) - 1] == K.BALLAST_FREE and sv["max_tasks"].max() < 1 << 21
    if case.kind == "commit":
        at, ln = pr["block_at"], pr["block_len"]
        blk = want[at:at + ln]
        assert n == pr["size"] and plan["C"] > K.MAX_WAVE_CLASSES and plan["elig_max_len"] <= 23
        first = case.info["first"]
        if ln == 64 and "timeouts" in pr:
            assert (blk == K.TIMEOUT).sum() == pr["timeouts"], (case, blk)
        if "servants" in pr:
            assert blk.tolist() == [first[c] for c in pr["servants"]][:ln]
        if "finals" in pr:
            assert (blk[3::4] >= K.ENF).all() and set(blk[3::4].tolist()) == {K.ENF, K.TIMEOUT}
        for lane in pr.get("barrier_lanes", ()):
            if lane < ln:  # (not its own servant at the head of the class: the other one)
                assert tk["requestor_ip"][at + lane] == sv["ip"][first[0]] and blk[lane] == first[0] + 1


def test_the_pinned_boundaries_are_the_formulas_own():
    assert K.lds_boundaries() == (K.LAST_PACKED_C, K.LAST_WALK_C)
    for C, want in ((K.LAST_PACKED_C, (True, True)), (K.LAST_PACKED_C + 1, (False, True)),
                    (K.LAST_WALK_C, (False, True)), (K.LAST_WALK_C + 1, (False, False))):
        _, n_rows, n_list = K.family_shape(C)
        fits = tuple(K.group_walk_lds_bytes(C, n_rows, n_list, p) <= K.GROUP_WALK_MAX_LDS for p in (True, False))
        assert fits == want, (C, fits)
        plan = K.plan_of(K.class_pool(C, n_tasks_hint=1200, shared_ip_frac=0.05, seed=C), 1200)
        assert (plan["n_rows"], plan["n_list"]) == (n_rows, n_list)


def test_every_path_and_each_side_of_every_threshold_has_a_case():
    plans = {c.name: K.plan_of(c.data()[0], len(c.data()[1]["env_id"])) for c in CASES if c.kind != "commit"}
    by_path = {p: [n for n, pl in plans.items() if pl["kernel"] == p] for p in K.PATHS}
    assert all(len(v) >= 2 for v in by_path.values()), by_path
    seen = lambda f: {f(pl) for pl in plans.values()}
    assert seen(lambda p: p["match_words"] if p["kernel"] == K.MATCH else 0) == {0, 1, 2, 4}
    assert seen(lambda p: p["fused_class_pass"]) == {True, False}
    assert seen(lambda p: p["init_fill_class"]) == {8, 16, 0}
    assert seen(lambda p: p["tick_takes_classes"]) == {True, False}
    assert {64, 65, 128, 129, 192, 193, 256, 257, 3072, 3073, 4096, 4097} <= seen(lambda p: p["C"])
    assert seen(lambda p: p["W8"]) >= {8, 16, 24, 32, 40, 48, 56, 64, 72}
    assert seen(lambda p: p["walk_cbits"]) >= set(range(3, 14))
    assert seen(lambda p: p["V"]) >= {1, 16, 17}
    assert seen(lambda p: p["elig_max_len"]) >= {64, 65}
    assert seen(lambda p: p["table_words"] <= K.ELIG_MAX_WORDS) == {True, False}
    walks = [p for p in plans.values() if p["wide_lists"]]
    assert {p["group_walk"] for p in walks} == {True, False}
    assert {(p["packed_bits_fit"], p["walk_lds_packed"] <= K.GROUP_WALK_MAX_LDS) for p in walks if p["group_walk"]} == {
        (True, True), (False, True), (True, False)}

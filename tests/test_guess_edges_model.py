"""The start states of k_match_pass, on the CPU: every case of tests/guess_edge_cases.py is verified
BEFORE a GPU sees it.

Exact pools: both forms of the oracle, the CPU model (tests/model) and — on the small cases — the
verbatim reference (oracle/_ref, where it is built) agree; the model needs ONE round and replays
every chunk once, and its deviation hook finds the level guess equal to the true start state at
every chunk (so a device that replays a chunk twice has computed a wrong guess); guess_plan names
the form of the guesses the case was made for. The control pools (own hosts) are not exact.

Walk pools: the restated T0 is the one the pool was built for; row 0 of the restated walk is the
level guess of its start; every later row EQUALS the class cursors that the oracle's placement
implies at the request where that chunk's replay starts — a condition on the inputs (seeds are
chosen so that it holds), which makes the device's rows comparable with the truth; where the plan
or the restatement finds no zone, there is none."""
import ctypes as C

import numpy as np
import pytest

from oracle import oraclebind as O
from oracle import refbind as R
from tests import guess_edge_cases as G
from tests.model import modelbind as M

EXACT = G.exact_cases() + G.disjoint_cases()
CONTROL = G.control_cases()
WALK = G.walk_cases()
ids = lambda cases: [c.name for c in cases]


def model_with_deviation(sv, tk, cs):
    k = -(-len(tk["env_id"]) // cs)
    dev = np.full(k, 0xFFFFFFFF, np.uint32)
    M.lib().model_set_deviation_out(dev.ctypes.data_as(C.c_void_p), None)
    try:
        got, util, run, st = M.dispatch(sv, tk, cs)
    finally:
        M.lib().model_set_deviation_out(None, None)
    return got, util, run, st, dev


def agree(sv, tk, cs, small):
    want, wutil, wrun = O.dispatch(sv, tk, "scan")
    got, gutil, grun = O.dispatch(sv, tk, "sorted")
    assert np.array_equal(got, want) and np.array_equal(gutil, wutil) and np.array_equal(grun, wrun)
    got, gutil, grun, st, dev = model_with_deviation(sv, tk, cs)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(gutil, wutil) and np.array_equal(grun, wrun)
    if small and R.available():
        d = R.RefDispatcher()
        d.load_servants(sv)
        ref_idx, _, _, _ = d.dispatch_batch(tk)
        d.close()
        assert np.array_equal(ref_idx, want), np.nonzero(ref_idx != want)[0][:5]
    return want, st, dev


@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_exact_pool_needs_one_replay_per_chunk(case):
    plan = case.plan()
    assert plan["form"] == case.path, (case, plan)
    assert plan["C"] == case.promise["C"] and plan["cs"] == case.cs
    assert 4096 <= plan["n_tasks"] <= 16384 and len(case.data()[0]["version"]) <= 2000
    for sv, tk in G.stages(case):
        n = len(tk["env_id"])
        assert not np.isin(tk["requestor_ip"], sv["ip"]).any()
        want, st, dev = agree(sv, tk, case.cs, small=n <= 4200)
        assert st.n_classes == case.promise["C"] and st.n_chunks == -(-n // case.cs)
        assert (st.rounds, st.chunk_sims) == (1, st.n_chunks), (case, st.rounds, st.chunk_sims)
        assert not dev.any(), (case, np.nonzero(dev)[0][:5])
        assert 0.01 * n < (want == G.ENF).sum() < 0.3 * n  # unknown digests among the requests
        if case.promise["over"]:
            assert (want == G.TIMEOUT).sum() > 0
            if case.promise["levels"]:  # the last chunks only time out
                assert (want[-case.cs:] >= G.ENF).all()
    sv, tk = case.data()
    if case.promise["slots"]:
        lists, _, m = G.class_lists(sv)
        assert sorted(len(l) for l in lists) == sorted(case.promise["slots"]) and m == sum(case.promise["slots"])


@pytest.mark.parametrize("case", CONTROL, ids=ids(CONTROL))
def test_control_pool_is_not_exact(case):
    sv, tk = case.data()
    assert case.plan()["form"] == case.path
    assert np.isin(tk["requestor_ip"], sv["ip"]).sum() > 0.05 * len(tk["env_id"])
    _, st, dev = agree(sv, tk, case.cs, small=True)
    assert st.chunk_sims > st.n_chunks and dev.any(), (case, st.chunk_sims, st.n_chunks)


def test_every_form_has_exact_cases_and_a_control():
    forms = {c.path for c in EXACT}
    assert forms == set(G.FORMS), forms
    assert {c.path for c in CONTROL} == set(G.FORMS)
    plans = [c.plan() for c in EXACT]
    assert {p["warm_len"] for p in plans} >= {0, 1, 16, 17, 32, 64}
    assert {p["cs"] for p in plans} >= {64, 128, 256, 512}
    assert {p["W"] for p in plans} == {1, 2, 4}
    assert {(p["binsort"], p["tile_tab"]) for p in plans} == {(True, False), (False, True), (False, False)}
    assert {p["rounds"] for p in plans} == {1, 2}


def walk_facts(case):
    """(servants and requests of the batch under test, the oracle's placement, the restatement)."""
    sv, tk = G.stages(case)[-1]
    pr = case.promise
    z = G.zone_restate(sv, tk, case.cs, pr["lead"], pr["trail"], case.plan(len(tk["env_id"]))["warm_len"])
    return sv, tk, z


@pytest.mark.parametrize("case", WALK, ids=ids(WALK))
def test_restated_walk_is_the_truth(case):
    sv0, _ = case.data()
    pr = case.promise
    assert G.slot_counts(sv0) == (pr["T0"], pr["M"])
    sv, tk, z = walk_facts(case)
    n = len(tk["env_id"])
    plan = case.plan(n)
    assert plan["walk"] == (case.path == "walk"), (case, plan)
    assert plan["C"] == pr["C"] and n <= 16384 and len(sv["version"]) <= 2000
    assert not np.isin(tk["requestor_ip"], sv["ip"]).any()
    want, st, _ = agree(sv, tk, case.cs, small=False)
    if not pr["first"]:
        assert (z["T0"], z["M"]) == (pr["T0"], pr["M"])  # slot_tier's rule on the oracle's order == the builder's
    assert (z["T0"], z["M"]) == G.slot_counts(sv)
    lists, _, _ = G.class_lists(sv)
    order_cls = G.servant_classes(sv)[G.global_order(sv)]
    off = 0
    for j, row in enumerate(z["cursors"]):
        at = z["t_start"] + j * case.cs
        if j == 0:  # the level guess: the class's slots among the first `level` of the global order
            assert np.array_equal(row, np.bincount(order_cls[:z["level0"]], minlength=len(lists))), case
        else:
            true = G.true_cursors(sv, tk, want, at)
            assert np.array_equal(row, true), (case, j, np.nonzero(row != true)[0], row - true)
            before = int(G.consuming(sv, tk)[:at].sum())
            off = max(off, int(np.abs(G.level_cursors(lists, before) - true).max()))
    print(case.name, "T0", z["T0"], "M", z["M"], "z_lo", z["z_lo"], "z_hi", z["z_hi"], "rows", z["rows"],
          "level guesses off by up to", off)
    assert len(z["cursors"]) == (z["rows"] if z["rows"] >= 2 else 0)


def test_walk_cases_cover_what_they_name():
    z = {c.name: walk_facts(c)[2] for c in WALK}
    rows = {k: v["rows"] for k, v in z.items()}
    for name in ("W-T0-0", "W-T0-M", "W-batch-ends-before", "W-batch-starts-behind", "W-second-batch-behind"):
        assert rows[name] == 0, (name, rows[name])
    assert rows["W-header-only"] == 1
    assert rows["W-cap-32-default-lead"] == G.ZONE_MAX_ROWS
    for name in ("W-T0-1", "W-T0-63", "W-T0-64", "W-T0-65"):  # T0 <= lead: the zone starts with chunk 1
        assert z[name]["z_lo"] == 1 and z[name]["t_start"] == 64 - G.WARM_UP and rows[name] >= 2, (name, z[name])
    assert rows["W-T0-M-1"] >= 2 and rows["W-second-batch"] >= 2
    c = G.case("W-reaches-last-chunk")
    n = len(c.data()[1]["env_id"])
    assert n % 64 and z[c.name]["z_hi"] == -(-n // 64)
    assert {G.case(k).plan()["zone_ring"] for k in ("W-C9", "W-C16-chunks-128")} == {256}
    assert {G.case(k).plan()["zone_ring"] for k in ("W-C17", "W-C32-chunks-128")} == {128}
    assert not G.case("W-C33-refused").plan()["walk"] and G.case("W-C64-rings-4096").plan()["walk"]
    assert G.case("W-chunks-96").plan()["cs"] == 128 and rows["W-chunks-96"] >= 2
    # one class wins 200 times in a row inside the zone; lists end inside it; every class runs dry
    c = G.case("W-one-class-200-in-a-row")
    zz = z[c.name]
    assert zz["t_start"] < 1400 and 1600 <= zz["t_start"] + (zz["rows"] - 1) * 64
    sv, tk, zz = walk_facts(G.case("W-lists-end-and-empty"))
    ends = np.array([len(l) for l in G.class_lists(sv)[0]])
    assert (ends == 0).sum() >= 1
    inside = (zz["cursors"][0] < ends) & (zz["cursors"][-1] == ends)
    assert inside.sum() >= 2, (zz["cursors"][0], zz["cursors"][-1], ends)
    sv, tk, zz = walk_facts(G.case("W-all-exhausted"))
    ends = np.array([len(l) for l in G.class_lists(sv)[0]])
    assert (zz["cursors"][0] < ends).any() and (zz["cursors"][-1] == ends).all()
    zz = z["W-unknown-block"]
    assert zz["t_start"] <= 1472 and 1472 + 64 <= zz["t_start"] + (zz["rows"] - 1) * 64

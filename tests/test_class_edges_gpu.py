"""Many-class matching at its thresholds, on the device: every case of tests/class_edge_cases.py
(verified on the CPU by tests/test_class_edges_model.py) through ydc_dispatch with profiling on.
Placement, utilisation doubles, the returned running_tasks and get_running() must EQUAL the
oracle's literal restatement; stats()["n_classes"] must be the case's class count; and the
matching kernel named by kernel_profile() must be the one plan_of predicts — k_match_pass,
k_walk_groups, k_sim_wide (with or without its walk) or k_sim_generic — so that a case made for
one side of a threshold cannot quietly run on the other. The commit-rule blocks also run with head
ranks and class ids in two arrays (YDC_WALK_PACKED=0) and with the plain parked fetch
(YDC_WALK_PARK=0); the class counts above 256 also without the group walk, without the
eligible-class lists and (up to 1025 classes) with the thread-per-chunk kernel; two cases per
path as two committed halves cut inside a block of 64; 4096 and 4097 classes through
ydc_dispatch_tick; and one child process on the measurement build reads the counts k_walk_groups
leaves behind (iterations, general steps, commits, losers, blocked; packed or not).

Wall time of the whole file on one MI355X, measured once: 8.3 s for its 231 tests (0.8 s of them the
child process on the measurement build, which was built beforehand)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (the witness child runs this file as a program)
    sys.path.insert(0, ROOT)

from oracle import oraclebind as O  # noqa: E402
from tests import class_edge_cases as K  # noqa: E402
from tests.test_tick_gpu import took_the_tick_kernel  # noqa: E402
from yadcc_amd import binding, pack  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = K.all_cases()
MATCHING_KERNELS = ("k_match_pass", "k_walk_groups", "k_sim_wide", "k_sim_wide(walk)", "k_sim_generic")
PROFILE_OF = {K.MATCH: "k_match_pass", K.WALK_PACKED: "k_walk_groups", K.WALK_UNPACKED: "k_walk_groups",
              K.WIDE: "k_sim_wide", K.GENERIC: "k_sim_generic"}


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    sv, tk = K.case(name).data()
    return O.dispatch(sv, tk, "scan")


def ran(profile):
    """The matching kernels of the last dispatch (the lone walker counts as k_sim_wide)."""
    names = {k for k in MATCHING_KERNELS if k in profile}
    if "k_sim_wide(walk)" in names:
        assert "k_sim_wide" in names, profile  # (rounds first, then the walker)
        names.discard("k_sim_wide(walk)")
    return names


def place(c, case, kernel=None, want=None, tk=None, commit=False):
    """One dispatch of the case (or of the requests tk, expecting `want`) on context c."""
    sv, all_tk = case.data()
    if want is None:
        want = oracle_of(case.name)
    tk = all_tk if tk is None else tk
    got, gutil, grun = c.dispatch(tk, commit=commit)
    st, prof = c.stats(), c.kernel_profile()
    bad = np.nonzero(got != want[0])[0]
    assert bad.size == 0, (case, bad[:5], got[bad[:5]], want[0][bad[:5]], st, sorted(prof))
    assert np.array_equal(gutil, want[1]), case
    assert np.array_equal(grun, want[2]), case
    assert st["n_classes"] == K.plan_of(sv, len(got))["C"] == case.promise.get("C", st["n_classes"]), (case, st)
    assert st["small_batch"] == 0, (case, st)
    assert ran(prof) == {kernel or PROFILE_OF[case.path]}, (case, sorted(prof))
    return st


def context(case, monkeypatch, **switches):
    for k, v in switches.items():
        monkeypatch.setenv("YDC_" + k, str(v))
    if case.kind == "commit":
        monkeypatch.setenv("YDC_SMALL_BATCH", "0")  # (64 requests: not the tick kernel's, the walk's)
    c = binding.Context(device=0)
    c.set_profiling(True)
    c.upload_servants(pack.to_abi_columns(case.data()[0]))
    return c


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_on_the_path_it_was_made_for(case, monkeypatch):
    sv, tk = case.data()
    assert K.plan_of(sv, len(tk["env_id"]))["kernel"] == case.path
    c = context(case, monkeypatch)
    try:
        place(c, case)
        assert np.array_equal(c.get_running(), sv["running_tasks"])  # (not committed)
        place(c, case, commit=True)
        assert np.array_equal(c.get_running(), oracle_of(case.name)[2])
    finally:
        c.close()


@pytest.mark.parametrize("switch", ["WALK_PACKED", "WALK_PARK"])
@pytest.mark.parametrize("scenario", [sc.__name__[3:] for sc in K.SCENARIOS])
def test_commit_rule_blocks_in_the_other_forms_of_the_walk(scenario, switch, monkeypatch):
    for size in K.COMMIT_SIZES:
        case = K.case("%s-%d" % (scenario, size))
        c = context(case, monkeypatch, **{switch: 0})
        try:
            place(c, case, commit=True)
            assert np.array_equal(c.get_running(), oracle_of(case.name)[2])
        finally:
            c.close()


ABOVE_256 = [c for c in CASES if c.kind == "count" and c.promise["C"] > K.MAX_WAVE_CLASSES]
OTHER_WAYS = ([("GROUP_WALK", c) for c in ABOVE_256] + [("WIDE_LISTS", c) for c in ABOVE_256] +
              [("WIDE", c) for c in ABOVE_256 if c.promise["C"] <= 1025])


@pytest.mark.parametrize("switch,case", OTHER_WAYS, ids=["%s=0-%s" % (s, c.name) for s, c in OTHER_WAYS])
def test_class_counts_with_a_path_switched_off(switch, case, monkeypatch):
    """Without the group walk and without the eligible-class lists, k_sim_wide's rounds (and the lone
    walker) place what k_walk_groups placed; without the wide kernel, k_sim_generic does."""
    if switch == "WIDE" or case.path == K.GENERIC:
        kernel = "k_sim_generic"
    else:
        kernel = "k_sim_wide"
    c = context(case, monkeypatch, **{switch: 0})
    try:
        place(c, case, kernel=kernel, commit=True)
        assert np.array_equal(c.get_running(), oracle_of(case.name)[2])
    finally:
        c.close()


HALVES = {K.MATCH: ("C65", "C256"), K.WALK_PACKED: ("C257", "rows-every-length"),
          K.WALK_UNPACKED: ("lds-first-unpacked", "bits-first-unpacked"), K.WIDE: ("C3072", "rows-one-of-65"),
          K.GENERIC: ("C3073", "C4097-dense")}


@pytest.mark.parametrize("name", [n for names in HALVES.values() for n in names])
def test_two_committed_halves_cut_inside_a_block(name, monkeypatch):
    case = K.case(name)
    assert name in HALVES[case.path]
    sv, tk = case.data()
    want, wutil, wrun = oracle_of(name)
    n = len(want)
    cut = n // 2 // 64 * 64 + 29
    c = context(case, monkeypatch)
    try:
        first = {k: v[:cut] for k, v in tk.items()}
        mid = O.dispatch(sv, first, "scan")
        assert np.array_equal(mid[0], want[:cut])
        place(c, case, want=mid, tk=first, commit=True)
        assert np.array_equal(c.get_running(), mid[2])
        place(c, case, want=(want[cut:], wutil[cut:], wrun), tk={k: v[cut:] for k, v in tk.items()}, commit=True)
        assert np.array_equal(c.get_running(), wrun)
    finally:
        c.close()


@pytest.mark.parametrize("C,takes", [(4096, True), (4097, False)])
def test_tick_kernel_up_to_4096_classes(C, takes, monkeypatch):
    """A small RPC through ydc_dispatch_tick: the tick kernel's eligible-class mask holds 4096 classes;
    one more and the batch pipeline places it (k_sim_generic)."""
    monkeypatch.setenv("YDC_RESIDENT", "0")
    case = K.case("C%d" % C)
    sv, tk = case.data()
    rpc = {k: v[100:109] for k, v in tk.items()}
    want, wutil, wrun = O.dispatch(sv, rpc, "scan")
    c = binding.Context(device=0)
    try:
        c.set_profiling(True)
        c.upload_servants(pack.to_abi_columns(sv))
        got, gutil = c.dispatch_tick(rpc, commit=True, want_util=True)
        st = c.stats()
        assert np.array_equal(got, want) and np.array_equal(gutil, wutil), (got, want, st)
        assert np.array_equal(c.get_running(), wrun)
        assert st["n_classes"] == C and took_the_tick_kernel(st) == takes, st
        if not takes:
            assert ran(c.kernel_profile()) == {"k_sim_generic"}
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# A witness that the intended form of the walk ran
# ---------------------------------------------------------------------------------------------
WITNESS = ("disjoint-64", "one_class-64", "dry-64", "dry_second_choice-64", "short_lists-64", "chain-64", "chain_up-64",
           "barrier_lane0-64", "barrier_lane63-64", "barrier_adjacent-64", "barrier_all-64", "holes-64",
           "self_shared-64", "finals-64", "lds-last-packed", "lds-first-unpacked", "bits-last-packed",
           "bits-first-unpacked")
WORDS = ("iters", "gens", "rounds", "commits", "losers", "blocked", "pending", "form")  # words 23 .. 30


def _witness_child():
    """Runs in a process of its own on the measurement build (YDC_LIB): one dispatch per case,
    checked against the oracle, then the stamps k_walk_groups left in words 16 .. 31."""
    import ctypes as C
    L = binding.lib()
    L.ydc_debug_phase_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.ydc_debug_phase_probe.restype = C.c_int
    out = {}
    for name in WITNESS:
        case = K.case(name)
        sv, tk = case.data()
        want, wutil, wrun = O.dispatch(sv, tk, "scan")
        c = binding.Context(device=0)
        c.set_profiling(True)
        c.upload_servants(pack.to_abi_columns(sv))
        assert L.ydc_debug_phase_probe(None, 0, 1) == 0
        got, gutil, grun = c.dispatch(tk)
        buf = np.zeros(32, np.uint64)
        assert L.ydc_debug_phase_probe(buf.ctypes.data, buf.size, 0) == 0
        assert np.array_equal(got, want) and np.array_equal(gutil, wutil) and np.array_equal(grun, wrun), name
        assert ran(c.kernel_profile()) == {"k_walk_groups"}, (name, c.kernel_profile())
        c.close()
        assert buf[22] != 0 and buf[31] == 0, (name, buf[16:32])
        out[name] = dict(zip(WORDS, (int(w) for w in buf[23:31])))
    print("WITNESS " + json.dumps(out))


def test_witness_that_the_intended_walk_ran():
    """The measurement build counts what k_walk_groups does (wide_kernel.h, words 23 .. 29 of the
    phase probe) and stamps its form into word 30 (1: two arrays, 2: packed). Asserted is what follows
    from the commit rule as written there; the rest is printed."""
    subprocess.check_call(["make", "-s", "probe"], cwd=ROOT)
    env = dict(os.environ, YDC_LIB=os.path.join(ROOT, "yadcc_amd", "libydc_probe.so"), YDC_SMALL_BATCH="0")
    env.pop("YDC_TUNE", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "witness"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("WITNESS ")][-1]
    w = json.loads(line[len("WITNESS "):])
    for name in WITNESS:
        print(name, w[name])
    sub = lambda name, *keys: tuple(w[name][k] for k in keys)
    # 64 one-class rows: every lane is the only claimant of its class, nobody marks anything
    assert sub("disjoint-64", "iters", "gens", "commits", "losers", "blocked") == (1, 0, 64, 0, 0), w["disjoint-64"]
    # one class: the lowest unresolved lane wins the claim, the others wait: 63 + 62 + ... + 1 losers
    assert sub("one_class-64", "iters", "gens", "commits", "losers") == (64, 0, 64, 2016), w["one_class-64"]
    # 40 slots: 40 iterations of one commit, and one in which the other 24 see an exhausted row
    assert sub("dry-64", "iters", "gens", "commits") == (41, 0, 40), w["dry-64"]
    assert sub("dry_second_choice-64", "iters", "gens", "commits") == (64, 0, 64), w["dry_second_choice-64"]
    # the second of two equal requests loses; its marks block the lane behind it, whose marks ...
    assert w["chain-64"]["blocked"] > 0 and w["chain-64"]["iters"] > 1 and w["chain-64"]["gens"] == 0, w["chain-64"]
    assert sub("chain_up-64", "iters", "gens", "commits", "losers", "blocked") == (1, 0, 64, 0, 0), w["chain_up-64"]
    for name, n in (("barrier_lane0-64", 1), ("barrier_lane63-64", 1), ("barrier_adjacent-64", 2),
                    ("barrier_all-64", 64)):
        assert sub(name, "gens", "commits") == (n, 64 - n), (name, w[name])
    assert w["short_lists-64"]["gens"] == 0 and w["short_lists-64"]["commits"] == 40, w["short_lists-64"]
    assert w["holes-64"]["gens"] >= 2 and w["self_shared-64"]["gens"] >= 4
    for name in WITNESS:  # packed wherever the bits and the LDS allow it, and only there
        assert w[name]["form"] == (2 if K.case(name).path == K.WALK_PACKED else 1), (name, w[name])
    assert sub("lds-last-packed", "form") + sub("lds-first-unpacked", "form") == (2, 1)
    assert sub("bits-last-packed", "form") + sub("bits-first-unpacked", "form") == (2, 1)


if __name__ == "__main__":
    if sys.argv[1:] == ["witness"]:
        _witness_child()

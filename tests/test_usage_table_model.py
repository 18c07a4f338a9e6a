"""tests/usage_table_cases.py rehearsed without a GPU: every crafted input of tests/test_usage_table_gpu.py
is on the path it was made for (the chains form and lie where the cases say, every lease id is alone in
its home slot, each thread, wave and workgroup of the accrual is given the pattern it is meant to see,
the table grows at the sizes the cases expect), and the closed-form expectations add up. The slot count
of the table (usage_slots, index_home.h) is compared with the restatement through
tests/native/hash_home_test.cc under ASan + UBSan (`make hashhome`).

Displacements the usage suites reach (the table of DESIGN 3.3.20) are printed by
test_displacements_of_the_suites_ids_and_of_the_crafted_chains."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import hash_index_cases as H
from tests import lease_table_cases as LT
from tests import usage_table_cases as UC
from tests.test_hash_index_model import bound
from tests.usage_table_cases import BITS, SIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the expectation itself ---------------------------------------------------------------------------

def test_expect_is_the_written_rule():
    e = UC.Expect(quantum=3)
    L = [(7, False, False), (7, True, False), (9, False, True), (None, False, False)]
    W = [(7, 5), (11, 1)]
    assert e.tick(4, L, W) == 0 and e.rows == {} and e.ticks == 1  # (the first tick: no interval behind it)
    assert e.tick(5, L, W) == 0 and e.rows == {}
    assert e.tick(6, L, W) == 1
    assert e.rows == {7: [2, 1, 0, 1, 5], 9: [1, 0, 1, 0, 0], 11: [0, 0, 0, 1, 1]} and e.unattributed == 1
    assert e.tick(14, L, ()) == 2 and e.rows[7] == [6, 3, 0, 1, 5] and e.quanta == 3 and e.ticks == 4
    e.load([(7, UC.M64, 0, 0, 0, 1), (12, 0, 0, 0, 0, 0)], {"unattributed_time": 2, "quanta": 1, "ticks": 1})
    assert e.rows[7] == [5, 3, 0, 1, 6] and e.rows[12] == [0] * 5 and (e.unattributed, e.quanta, e.ticks) == (5, 4, 5)
    rows, tot = e.get()
    assert rows["requestor_ip"].tolist() == [7, 9, 11, 12] and tot["n_keys"] == 4
    assert e.find([12, 13])["slot_time"].tolist() == [0, 0]
    e.reset()
    assert e.get()[1] == {"unattributed_time": 0, "quanta": 0, "ticks": 0, "n_keys": 0}


# ---- A. chains ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", H.HOMES)
def test_chains_and_the_ids_around_them(h):
    for n in H.LENGTHS:
        ids = UC.chain(h, n)
        run = H.one_chain(ids, BITS, h)
        assert (SIZE - 1 in run and 0 in run) == (h + n > SIZE)
        absent = H.absent_around(BITS, h, n, ids, ids=True)
        assert sum(H.home(x, BITS) == h for x in absent) >= 16 and not set(absent) & set(ids)
        assert {H.home(x, BITS) for x in absent} >= {(h + n) % SIZE}
        rows = UC.sums_for(ids, n)
        flat = [v for r in rows for v in r[1:]]
        assert all(flat) and len(set(flat)) == len(flat), "the sums are not distinct and non-zero"
        # the load's own room: one call of n rows, then one of 3 n (every row may be a new key)
        assert H.slots_usage(n) == SIZE
        assert H.slots_usage(n + 3 * n) == (SIZE if n <= 65 else 4096), n
        e = UC.Expect()
        e.load(UC.permuted(rows, h))
        e.load(UC.permuted(rows * 3, h + 1))
        assert all(e.rows[r[0]] == [(4 * v) & UC.M64 for v in r[1:]] for r in rows) and len(e.rows) == n


def test_ends_and_touching_chains():
    zero, ones, hf = UC.ends()
    assert zero[0] == 0 and ones[0] == 0xFFFFFFFF and H.home(0, BITS) == 0 and len(set(zero + ones)) == 128
    a, b, absent = UC.touching()
    assert not set(absent) & set(a + b) and {H.home(x, BITS) for x in absent} == {1021, 0, (1021 + 80) % SIZE}
    hist = H.histogram(a + b, BITS)
    assert hist.get("wrap", 0) >= 37 and max(d for d in hist if d != "wrap") >= 40


@pytest.mark.parametrize("kind", ["stay0", "stay1", "split"])
@pytest.mark.parametrize("h", H.HOMES)
def test_chains_when_the_table_doubles(h, kind):
    ids, homes = UC.doubled(h, kind)
    occ, md = H.layout(ids, BITS + 1)
    assert occ == frozenset().union(*[H.run_of(hh, n, BITS + 1) for hh, n in homes.items()]) and md == max(homes.values()) - 1
    # both ways to 2048 slots: a begin that asks for 600, a load of 300 further keys
    assert H.slots_usage(257) == SIZE and H.slots_usage(600) == 2 * SIZE and H.slots_usage(257 + 300) == 2 * SIZE
    more = UC.further_keys(300, ids)
    assert len(set(more) | set(ids)) == 557
    for hh, n in homes.items():
        absent = H.absent_around(BITS + 1, hh, n, ids + more, ids=True)
        assert not set(absent) & set(ids + more) and sum(H.home(x, BITS + 1) == hh for x in absent) >= 16


def test_fold_chains_cross_the_tile_boundary_and_the_wrap():
    a, b, c = UC.fold_chains()
    assert H.slots_usage(600) == 2048 and H.slots_usage(195 + 195) == 1024  # (the loads alone would not grow it)
    tiles = [{s // 1024 for s in H.layout(x, BITS + 1)[0]} for x in (a, b, c)]
    assert tiles == [{0, 1}, {0, 1}, {0}]


def test_displacements_of_the_suites_ids_and_of_the_crafted_chains():
    """The two columns of the table in DESIGN 3.3.20."""
    suites = [("0x0C000000 + 13 i, i < 513", [0x0C000000 + 13 * i for i in range(513)], 2048),
              ("0x0D000000 + 7 i, i < 3000", [0x0D000000 + 7 * i for i in range(3000)], 8192),
              ("0x0C000000 + 31 i, i < 74", [0x0C000000 + 31 * i for i in range(74)], 1024)]
    for name, ids, slots in suites:
        hist = H.histogram(ids, H.bits_of(slots))
        most = max(d for d in hist if d != "wrap")
        print("%-30s %5d slots: largest displacement %3d, at home %5.1f %%, crossed the wrap %d" % (
            name, slots, most, 100.0 * hist[0] / len(ids), hist.get("wrap", 0)))
        # (what random keys at this load reach, tests/test_hash_index_model.py's bound; a wrap by one slot at the most)
        assert most <= bound(len(ids), slots) < 64 and hist.get("wrap", 0) <= 1, (name, most, hist)
    for name, ids in (("257 ids of home 1021", UC.chain(1021, 257)), ("40 + 40 at 1021 and 0", sum(UC.touching()[:2], []))):
        hist = H.histogram(ids, BITS)
        most = max(d for d in hist if d != "wrap")
        print("%-30s %5d slots: largest displacement %3d, crossed the wrap %d" % (name, SIZE, most, hist.get("wrap", 0)))
        assert most >= 40 and hist.get("wrap", 0) >= 37


# ---- B. the upper half ----------------------------------------------------------------------------------

def test_wide_wave_needs_the_upper_half():
    wave = UC.wide_wave()
    assert len(wave) == 64
    heavy = [(i, a + b) for i, (ip, a, b) in enumerate(wave) if ip == UC.HEAVY]
    assert [i for i, _ in heavy] == list(UC.WIDE_LANES) and [r for _, r in heavy] == list(UC.WIDE_ROWS)
    rows = [r for _, r in heavy]
    low, high = sum(r & 0xFFFF for r in rows), sum(r >> 16 for r in rows)
    assert low == 0x20000 and high == 3 and low + (high << 16) == sum(rows) == 327680
    assert low != sum(rows), "a sum of the lower halves alone would pass"
    assert sum(a + b for ip, a, b in wave if ip == UC.LIGHT) == 59
    assert all(a + b > 0 and a > 0 for _, a, b in wave) and any(a > 65535 for _, a, _ in wave)
    total = sum(a + b for _, a, b in wave)
    assert total < 1 << 19, "rows(W) fits max_rows and max_leases of 2^19"
    e = UC.Expect()
    W = [(ip, a + b) for ip, a, b in wave]
    for now in (10, 11, 14):
        e.tick(now, (), W)
    assert e.rows[UC.HEAVY] == [0, 0, 0, 4 * 5, 4 * 327680] and e.rows[UC.LIGHT] == [0, 0, 0, 4 * 59, 4 * 59]


# ---- C. leases at exact slots -----------------------------------------------------------------------------

def test_one_id_per_slot_of_a_whole_table():
    """1024 ids, one per slot of a 1024-slot table: distinct, each at displacement 0; and of a 2048-slot one."""
    for bits in (BITS, BITS + 1):
        ids = UC.exact_ids(bits, range(1 << bits))
        assert len(set(ids)) == 1 << bits and max(ids) < LT.NEXT_ID


def _check_plan(plan, bits=BITS):
    ls, caps, at = UC.exact_stream(plan, bits)
    assert sorted(at) == sorted(plan) and LT.layout([at[s] for s in sorted(at)], bits) == (frozenset(plan), 0)
    assert len(ls.table.L) == len(plan) and caps["max_leases"] == 1 << (bits - 1)
    rec = UC.records(plan, at)
    assert len(rec["task_id"]) == sum(le.ip is not None for le in plan.values())
    return at


@pytest.mark.parametrize("pattern", UC.THREAD_PATTERNS)
def test_what_one_thread_sees(pattern):
    plan = UC.thread_plan(pattern)
    _check_plan(plan)
    letters = []
    for c in pattern:
        if c != "." and c not in letters:
            letters.append(c)
    for wg, t in UC.THREADS:
        groups, nobody = UC.thread_groups(plan, t, wg)
        assert [g[0] for g in groups] == [UC.KEY[c] for c in letters] and nobody == 0
        assert [g[1] for g in groups] == [pattern.count(c) for c in letters]
        assert sum(g[2] for g in groups) == 1 and sum(g[3] for g in groups) == 1
        if len(groups) > 1:  # (neither mark on the first group: crediting group 0 gives another answer)
            assert groups[0][2] == 0 and groups[0][3] == 0
            assert groups[min(2, len(groups) - 1)][2] == 1
        zi, pi = UC._marks(pattern)
        assert (zi != pi) == (len(pattern.replace(".", "")) > 1)
        assert UC.thread_groups(plan, t + 1, wg) == ([(UC.KEY["A"], 1, 0, 0)], 1)
    assert 0 in {le.ip for le in plan.values()}


def test_what_one_wave_sees():
    for distinct in (None, UC.chain(1021, 64)):
        plan = UC.wave_plan(distinct)
        _check_plan(plan)
        seconds = set()
        for t in range(64):
            groups, nobody = UC.thread_groups(plan, t)
            assert len(groups) == 2 and groups[0][0] == UC.HOT and groups[0][1] == (2 if t % 5 == 0 else 1) and nobody == 0
            seconds.add(groups[1][0])
        assert seconds == set(UC.SIX) and len(seconds) > UC.ROUNDS
        lead = UC.wave_lead(plan, 0)
        assert lead[0] == UC.HOT and lead[1] == 64 + 13 and lead[2] == 7 and lead[3] == 8
        assert sum(UC.thread_groups(plan, t)[0][1][2] for t in range(64)) > 0
        firsts = [UC.thread_groups(plan, 64 + t)[0] for t in range(64)]
        assert all(len(g) == 1 for g in firsts) and len({g[0][0] for g in firsts}) == 64
        assert UC.wave_lead(plan, 1)[:2] == (firsts[0][0][0], 1) and UC.wave_lead(plan, 2) is None
        if distinct is not None:
            assert {H.home(g[0][0], BITS) for g in firsts} == {1021}


@pytest.mark.parametrize("name", sorted(UC.LEADS))
def test_what_the_four_leads_are(name):
    keys = UC.LEADS[name]
    plan = UC.leads_plan(keys)
    _check_plan(plan)
    for w, key in enumerate(keys):
        lead = UC.wave_lead(plan, w)
        if key is None:
            assert lead is None and not any(UC.slots_of(64 * w)[0] <= s < UC.slots_of(64 * w + 64)[0] for s in plan)
        else:
            assert lead == (key, 7, w % 2, 1)
    e = UC.Expect()
    for now in (1, 2):
        e.tick(now, UC.triples(plan))
    for key in set(keys) - {None}:
        k = sum(x == key for x in keys)
        assert e.rows[key] == [7 * k, sum(w % 2 for w, x in enumerate(keys) if x == key), k, 0, 0]


def test_what_the_two_workgroups_see():
    plan = UC.two_workgroups_plan()
    _check_plan(plan, BITS + 1)
    seam = sorted(s for s, le in plan.items() if le.ip == UC.ONLY_AT_THE_SEAM)
    assert seam == list(range(1020, 1028)) and UC.slots_of(255, 0) == seam[:4] and UC.slots_of(0, 1) == seam[4:]
    assert UC.thread_groups(plan, 255, 0)[0] == [(UC.ONLY_AT_THE_SEAM, 4, 1, 0)]
    assert UC.thread_groups(plan, 0, 1)[0] == [(UC.ONLY_AT_THE_SEAM, 4, 0, 1)]
    for wg in (0, 1):
        assert sum(1 for s, le in plan.items() if le.ip == UC.HOT and s // 1024 == wg) >= 8
        assert UC.wave_lead(plan, 0, wg)[0] == (UC.HOT if wg == 0 else UC.ONLY_AT_THE_SEAM)
    assert UC.wave_lead(plan, 3, 0)[0] == UC.HOT and UC.wave_lead(plan, 3, 1)[0] == UC.HOT


# ---- D. the host's bound --------------------------------------------------------------------------------

def test_the_ramp_keeps_the_floor_and_the_strangers_need_the_bump():
    """The host's arithmetic (usage_bound, `fresh` in stream_tick_finish) replayed: every tick of the ramp
    accrues (dq > 0), so behind it n_keys is what L held in front of it and fresh the tick's requests."""
    n_keys = fresh = holders = 0
    seen = set()
    for reqs in UC.ramp():
        assert H.slots_usage(UC.bound(n_keys, fresh, holders)) == SIZE
        n_keys, fresh = len(seen), len(reqs)  # (the accrual claims what L held; the grants join behind it)
        seen |= set(reqs)
        holders += len(reqs)
    assert H.slots_usage(UC.bound(n_keys, fresh, holders)) == SIZE
    n_keys, fresh = len(seen), 0  # (one more accruing tick without requests)
    assert (n_keys, holders) == (UC.RAMP_KEYS, UC.RAMP_LEASES) and H.slots_usage(n_keys) == SIZE
    strangers = UC.strangers()
    assert len(set(strangers)) == UC.STRANGERS <= holders and not set(strangers) & seen
    assert H.slots_usage(UC.bound(n_keys, fresh + len(strangers), holders)) == 2 * SIZE
    # (a full sidecar files every record of L: the bound takes all of them for new)
    assert H.slots_usage(UC.bound(n_keys, fresh + holders, holders)) == 4 * SIZE
    # without the bump the table stays, and the accrual files more keys than half of it
    assert H.slots_usage(UC.bound(n_keys, fresh, holders)) == SIZE and n_keys + len(strangers) > SIZE // 2
    assert n_keys + len(strangers) <= SIZE, "every claim still finds a slot: an error, not a walk without end"


# ---- against the library's own header ---------------------------------------------------------------------

def test_usage_slots_against_the_librarys_header_under_sanitizers(tmp_path):
    """usage_slots for n = 0 .. 5000 and around 2^30, 2^31 and 2^32 (the cap of 2^31 slots)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "hash_home_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "hash_home_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    sizes = list(range(5001)) + [(1 << k) + d for k in (20, 29, 30, 31) for d in (-1, 0, 1)] + [(1 << 32) - 1, 1 << 32]
    out = subprocess.run([exe], input="".join("u %d\n" % n for n in sizes), capture_output=True, text=True, timeout=600)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and lines[len(sizes)] == "HASH-HOME-OK %d" % len(sizes), (out.stdout[-500:], out.stderr[-4000:])
    for n, line in zip(sizes, lines):
        assert int(line) == H.slots_usage(n), "usage_slots(%d): the library %s, the restatement %d" % (n, line, H.slots_usage(n))
    assert H.slots_usage(1 << 32) == 1 << 31 and H.slots_usage((1 << 30) + 1) == 1 << 31 and H.slots_usage(1 << 30) == 1 << 31
    assert np.all([H.slots_usage(n) >= 2 * n for n in sizes if n <= 1 << 30])

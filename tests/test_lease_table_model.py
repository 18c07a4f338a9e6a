"""tests/lease_table_cases.py on the CPU: the arithmetic that makes ids collide, the two facts about
linear probing the GPU tests rest on, and every scripted tick sequence through the model alone, so
that each case is known to meet the events it was written for before a device is touched."""
import os
import random
import re

import pytest

from tests import lease_table_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bits,h", [(10, 0), (10, 100), (10, 1021), (10, 1023), (11, 2043), (13, 8191), (20, 12345)])
def test_colliders_collide(bits, h):
    ids = C.colliders(bits, h, 300)
    assert len(ids) == len(set(ids)) == 300 and ids == sorted(ids) and 0 <= ids[0] and ids[-1] < 1 << 62
    assert {C.home(t, bits) for t in ids} == {h}
    assert len({C.home(t, bits + 1) for t in ids}) == 2, "the ids fall into one half of the slot's interval only"
    few = C.colliders(bits, h, 5, below=1 << 50)
    assert len(few) == 5 and few[-1] < 1 << 50 and {C.home(t, bits) for t in few} == {h}


def test_the_constant_is_the_librarys():
    src = open(os.path.join(ROOT, "yadcc_amd", "csrc", "lease_table.h")).read()
    assert "id * 0x%Xull) >> L.shift" % C.K in src
    api = open(os.path.join(ROOT, "yadcc_amd", "csrc", "ydc_api.hip")).read()
    assert re.search(r"size_t cap = 1024;\s*uint32_t cap_bits = 10;\s*while \(cap < 2 \* \(size_t\)k\.max_leases\)", api)


@pytest.mark.parametrize("max_leases,slots", [(1, 1024), (512, 1024), (513, 2048), (1024, 2048), (1025, 4096)])
def test_cap_is_what_the_bounds_imply(max_leases, slots):
    assert C.cap(max_leases) == slots == 1 << C.cap_bits(max_leases)
    assert slots >= 2 * max_leases and (slots == 1024 or slots < 4 * max_leases)


@pytest.mark.parametrize("case", C.SHAPES, ids=[c.name for c in C.SHAPES])
def test_layout_does_not_depend_on_the_order(case):
    occ, md = C.layout(case.ids, case.bits)
    rng = random.Random(7)
    for _ in range(3):
        ids = list(case.ids)
        rng.shuffle(ids)
        occ2, md2 = C.layout(ids, case.bits)
        assert occ2 == occ
        if len(case.chains) == 1:
            assert md2 == md == case.n - 1
    assert len(occ) == case.n
    if case.bits == 10 and len(case.chains) == 1:
        h = case.chains[0][0]
        assert case.wraps() == (h + case.n > C.SIZE)
    # (in the larger table of the reserve cases too)
    for _ in range(2):
        ids = list(case.ids)
        rng.shuffle(ids)
        assert C.layout(ids, 11)[0] == C.layout(case.ids, 11)[0]


def test_the_wrap_cases_wrap():
    for name in ("wrap3_2", ):
        assert not C.BY_NAME[name].wraps()  # (two of the three slots before the end)
    for name in ("wrap3_63", "wrap3_257", "wrap1_2", "wrap1_257", "touching", "whole_2048", "split_2048"):
        occ = C.BY_NAME[name].run_slots()
        assert C.SIZE - 1 in occ and 0 in occ, name
    assert not any(c.wraps() for c in C.SHAPES if c.name.startswith("mid") or c.name == "touching_mid")
    occ = C.BY_NAME["wrap3_257"].run_slots()
    assert occ == {(C.SIZE - 3 + d) % C.SIZE for d in range(257)} and max(o for o in occ if o < 500) == 253
    # The touching chains make one run of 257 slots whose bound is that of the longer chain alone.
    for c in (C.TOUCHING, C.TOUCHING_MID):
        (h, a), (h2, b) = c.chains
        occ, md = C.layout(c.ids, c.bits)
        assert h2 == (h + a) % C.SIZE and occ == {(h + d) % C.SIZE for d in range(a + b)}
        assert b - 1 <= md < a + b - 1
    # After the reserve: one chain of 257 across the larger table's wrap, or two chains that touch.
    occ, md = C.layout(C.WHOLE_2048.ids, 11)
    assert md == 256 and 2047 in occ and 0 in occ
    occ, md = C.layout(C.SPLIT_2048.ids, 11)
    assert occ == {(2 * (C.SIZE - 3) + d) % 2048 for d in range(257)} and md >= 128  # (md depends on the order here)


def test_new_ids_fall_into_the_run():
    """The conditions of scripts 3, 4 and 8, from the ids alone."""
    for c in C.LONG:
        assert len(c.hits(C.GRANTS)) >= 20, (c.name, len(c.hits(C.GRANTS)))
        assert len(c.hits(64)) >= 8, (c.name, len(c.hits(64)))
    for c in (C.TOUCHING, C.TOUCHING_MID):
        assert len(c.past_bound(64)) >= 3, (c.name, len(c.past_bound(64)))
    for c in C.SHAPES:
        if c.n >= 63:
            assert len(c.hits(C.GRANTS)) >= 3, c.name


def test_displacements_the_suite_reached_before_and_reaches_now():
    """The replay behind the table in DESIGN 3.3.2. The streams' own consecutive ids stay at displacement
    0 or 1 and never cross the wrap displaced (asserted loosely: this documents the hole, the numbers may
    move with the streams); the crafted tables reach 256 and cross it (asserted exactly)."""
    before = [C.replay_consecutive(10, 8, 200, keep=(0, 1024)), C.replay_consecutive(13, 20, 1500)]
    for hist in before:
        assert max(d for d in hist if d != "wrap") <= 2 and hist.get("wrap", 0) <= 1, hist
    top = 0
    for c in C.SHAPES:
        hist = C.histogram(c.ids, c.bits)
        assert sum(v for k, v in hist.items() if k != "wrap") == c.n
        top = max(top, max(d for d in hist if d != "wrap"))
        if len(c.chains) == 1:
            assert sorted(d for d in hist if d != "wrap") == list(range(c.n))
        if c.wraps():
            assert hist["wrap"] >= 1, c.name
    assert top == 256
    assert sum(1 for c in C.SHAPES if max(d for d in C.histogram(c.ids, c.bits) if d != "wrap") >= 64) >= 10
    assert C.histogram(C.BY_NAME["wrap1_257"].ids, 10)["wrap"] == 256


PLAYS = [(script, make, case) for script, make, shapes in C.SCRIPTS for case in shapes]


@pytest.mark.parametrize("script,make,case", PLAYS, ids=["%s-%s" % (s.__name__, c.name) for s, _, c in PLAYS])
def test_scripts_meet_their_events_in_the_model(script, make, case):
    ls, caps = C.crafted_stream(make(case))
    assert len(ls.table.L) == case.n and int(ls.es.running.sum()) == case.n and ls.table.next_id == C.NEXT_ID
    d = C.ModelDriver(ls, caps)
    script(d, case)
    assert 2 <= d.t < 10
    want = {"found_at_every_displacement": ("renewed", "renew_refused"),
            "holes_inside_the_chain": ("renewed", "freed", "ignored_frees", "granted"),
            "contended_inserts": ("renewed", "renew_refused", "freed", "granted"),
            "expiry_and_sweep": () if case.n == 1 else ("renewed", "renew_refused", "expired", "swept"),
            "reserve_with_a_chain": ("renewed", "renew_refused", "freed", "granted"),
            "snapshot_and_restore": ("renewed", "renew_refused", "freed", "granted"),
            "delta_to_a_standby": ("renewed", "renew_refused", "freed", "expired", "granted"),
            "remove_servants_with_a_chain": ("renewed", "renew_refused", "freed", "granted")}[script.__name__]
    for k in want:
        assert d.seen[k] > 0, "%s on %s never saw %s" % (script.__name__, case.name, k)


def test_the_blob_of_a_crafted_state_is_well_formed():
    from yadcc_amd import snapshot
    case = C.BY_NAME["wrap3_257"]
    ls, caps = C.crafted_stream(C.expiry_entries(case))
    p = snapshot.parse(snapshot.build(C.state(ls, caps)))
    assert p["next_id"] == C.NEXT_ID and list(p["l_id"]) == case.ids and p["lease_tick"] == 0
    assert int(p["running_tasks"].sum()) == 257 and p["max_leases"] == C.MAX_LEASES

"""The usage model (tests/stream_usage_model.py) on the CPU: the yardstick of tests/test_stream_usage_gpu.py.

Hand vectors of the interval rule; the telescoped identity on seeded streams in all three modes, checked
after every tick against the BASE model's own counts (pinned to the verbatim reference by the existing model
tests); the conditions the GPU tests put on their inputs, met by the model's side of their rig alone; and
the constants and the struct's layout against the header text."""
import os
import re

import numpy as np
import pytest

from tests import stream_inspect_model as IM
from tests import stream_usage_model as U
from tests import test_stream_usage_gpu as G
from tests.conftest import ROOT
from tests.test_stream_depart_model import A, B, MODELS, new_stream, small_pool, spread, tiny_pool
from yadcc_amd import binding

M64 = U.M64
MODES = ("leased", "wl", "rpc")


# ---- the interval rule -----------------------------------------------------------------------------

def test_quanta_by_hand():
    q = 10
    assert [U.quanta(q - 1, now, q) for now in (q, q + 1, 2 * q - 1)] == [1, 1, 1]
    assert U.quanta(7, 7, q) == 0 and U.quanta(0, 9, q) == 0
    assert [U.quanta(-1, 0, q), U.quanta(0, 1, q), U.quanta(-q, -1, q), U.quanta(-q - 1, -q, q), U.quanta(-1, 1, q)] == [1, 0, 0, 1, 1]
    assert [U.quanta(a, b, 1) for a, b in ((-3, -3), (-3, 0), (0, 1), (5, 12))] == [0, 3, 1, 7]
    assert U.quanta(-(1 << 63), (1 << 63) - 1, 1) == M64 and U.quanta((1 << 63) - 1, -(1 << 63), 1) == 1
    chain = [-25, -25, -11, -10, -1, 0, 3, 9, 10, 41]
    assert sum(U.quanta(a, b, q) for a, b in zip(chain, chain[1:])) == U.quanta(chain[0], chain[-1], q) == 7


def test_clock_hand_vectors_in_the_model():
    """A lease granted at q - 1 and freed at q, q + 1, 2q - 1; two ticks with the same now; clocks at -1, 0, 1
    and -q: the list tests/test_stream_usage_gpu.py runs on the device."""
    assert G._clock_vectors(device=False) == [1, 1, 1, 0, 1, 0, 1, 2, 0]


# ---- the telescoped identity -----------------------------------------------------------------------

@pytest.mark.parametrize("quantum", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_telescoped_identity(mode, quantum):
    """Sum of slot_time + unattributed_time == sum over ticks of dq_t |L|_{t-1}, and sum of wait_time == sum of
    dq_t |W|_{t-1}, with |L| and |W| the base model's own; a lease granted before the capability began its
    details are kept for is nobody's until inspection is attached."""
    M = MODELS[mode]
    ws = new_stream(mode, small_pool())
    rng, crng = np.random.default_rng(11), np.random.default_rng(5)
    for _ in range(3):  # (leases without details)
        ev = spread(ws.next_tick(), rng)
        M.model_tick(ws, ev)
    IM.attach(ws)
    u = U.Usage(ws, quantum)
    assert u.last == ws.table.last_now
    want_l = want_w = 0
    for t in range(40):
        ws.es.tick_no += int(crng.choice([0, 1, 1, 2, 4])) - 1
        ev = spread(ws.next_tick(), rng)
        n_l = len(ws.table.L)
        n_w = len(ws.state.q) if getattr(ws, "state", None) is not None else 0
        dq = U.quanta(u.last, int(ev["now"]), quantum)
        u.tick(ev, lambda e: IM.model_tick(M, ws, e))
        assert u.dq == dq
        want_l, want_w = want_l + dq * n_l, want_w + dq * n_w
        assert sum(r[0] for r in u.rows.values()) + u.unattributed == want_l, t
        assert sum(r[3] for r in u.rows.values()) == want_w, t
        assert all(r[1] <= r[0] and r[2] <= r[0] and r[4] >= r[3] for r in u.rows.values())
    assert want_l > 100 and (mode == "leased" or want_w > 100) and u.unattributed > 0 and u.ticks == 40


def test_a_refused_tick_adds_nothing_and_keeps_last():
    ws = new_stream("leased", tiny_pool(1, 4))
    IM.attach(ws)
    u = U.Usage(ws, 2)
    M = MODELS["leased"]
    ev = ws.next_tick()
    ev["tasks"] = dict(ev["tasks"], requestor_ip=np.full(len(ev["tasks"]["env_id"]), A, np.uint32))
    u.tick(ev, lambda e: IM.model_tick(M, ws, e))
    assert u.last == 0 and u.dq == 0 and u.rows == {}

    def refuse(e):
        raise OverflowError("capacity")
    ws.es.tick_no = 6
    with pytest.raises(OverflowError):
        u.tick(ws.next_tick(), refuse)
    assert u.last == 0 and u.rows == {} and u.ticks == 1
    ws.es.tick_no = 9
    held = len(ws.table.L)
    u.tick(ws.next_tick(), lambda e: IM.model_tick(M, ws, e))
    assert u.dq == 4 and u.rows[A][0] == 4 * held and held > 0


def test_get_reset_find_and_load():
    ws = new_stream("leased", tiny_pool(1, 4))
    IM.attach(ws)
    u = U.Usage(ws, 1)
    u.load(G.rows_of([(A, 1, 2, 3, 4, 5), (B, M64 - 4, 0, 0, 0, 0), (A, 1, 0, 0, 0, M64)]), {"quanta": 3, "ticks": 2})
    u.load(G.rows_of([(B, 10, 0, 0, 0, 0), (7, 0, 0, 0, 0, 0)]))
    rows, tot = u.get()
    assert rows["requestor_ip"].tolist() == [7, A, B] and rows["slot_time"].tolist() == [0, 2, 5]  # (2^64 - 5 + 10 reads 5)
    assert rows["wait_row_time"].tolist() == [0, 4, 0] and tot == {"unattributed_time": 0, "quanta": 3, "ticks": 2, "n_keys": 3}
    found = u.find([B, 99, A])
    assert found["requestor_ip"].tolist() == [B, 99, A] and found["slot_time"].tolist() == [5, 0, 2]
    assert u.get(reset=True)[1]["n_keys"] == 3 and len(u.get()[0]) == 0
    assert u.get()[1] == {"unattributed_time": 0, "quanta": 0, "ticks": 0, "n_keys": 0}
    with pytest.raises(ValueError):
        u.begin(2)
    with pytest.raises(ValueError):
        U.Usage(ws, 0)
    with pytest.raises(ValueError):
        U.Usage(new_stream("leased", tiny_pool(1, 4)), 1)  # (inspection is off)


# ---- the conditions of the GPU tests, met by the model alone ---------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_the_differential_meets_its_conditions(mode):
    """At least 50 rows in the final table, every column the mode has and unattributed_time non-zero in total,
    a tick with dq == 0, a reset and a load on the way."""
    G.differential_conditions(*G._differential(mode, device=False), mode=mode)


@pytest.mark.parametrize("mode", MODES)
def test_the_scripted_route_meets_its_conditions(mode):
    G._scripted_route(mode, device=False, ticks=20)


def test_the_scenarios_meet_their_conditions():
    G._lease_pattern((A + np.arange(300) % 5).astype(np.uint32), device=False)
    for n in (511, 512, 513):
        G.test_distinct_requestors_on_the_1024_slot_floor(n, device=False)
    G.test_3000_requestors_brought_by_blocked_calls(device=False)
    G.test_requestors_that_arrive_inside_one_quantum(device=False)
    G.test_a_requestor_that_left_keeps_its_row_and_reset_drops_it(device=False)
    G.test_load_with_duplicates_then_an_accrual_and_a_wrap(device=False)
    for mode in ("wl", "rpc"):
        G.test_with_departure_and_a_quota(mode, device=False)
    for mode in MODES:
        G.test_a_structural_heartbeat(mode, device=False)
    G._alive_run("wl", device=False)
    for case in (G.test_zombies_after_an_expiry_tick, G.test_prefetch_leases_in_rpc_mode, G.test_inspection_switched_on_late,
                 G.test_erased_leases_whose_records_stay_behind):
        case(device=False)


# ---- the header ------------------------------------------------------------------------------------

def test_constants_and_layout_against_the_header():
    text = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define\s+YDC_USAGE_RESET\s+1u", text) and binding.USAGE_RESET == 1
    assert re.search(r"#define\s+YDC_ABI_VERSION\s+8u", text)
    row = re.search(r"typedef struct ydc_usage_row \{[^}]*\} ydc_usage_row;", text).group(0)
    names = re.findall(r"\b(requestor_ip|pad|slot_time|zombie_time|prefetch_time|wait_time|wait_row_time)\b", row)
    assert tuple(names) == U.DTYPE.names and "48 bytes" in row
    assert U.DTYPE.itemsize == 48 and [U.DTYPE.fields[k][1] for k in U.DTYPE.names] == [0, 4, 8, 16, 24, 32, 40]
    tot = re.search(r"typedef struct ydc_usage_totals \{[^}]*\} ydc_usage_totals;", text).group(0)
    assert re.findall(r"\b(unattributed_time|quanta|ticks|n_keys|slots)\b", tot) == ["unattributed_time", "quanta", "ticks",
                                                                                      "n_keys", "slots"]
    src = open(os.path.join(ROOT, "yadcc_amd", "csrc", "index_home.h")).read()  # (the slot functions' common place)
    assert re.search(r"kIndexMinSlots = (\d+)", src).group(1) == str(U.MIN_SLOTS)  # (one minimum for the four tables)
    assert re.search(r"uint32_t usage_slots\(uint64_t n\) \{ return index_slots\(n\); \}", src)
    assert [U.slots_for(n) for n in (0, 1, 512, 513, 1024, 1025, 3001)] == [1024, 1024, 1024, 2048, 2048, 4096, 8192]

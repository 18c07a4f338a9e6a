"""The fair-share level per tick on the device (ydc_stream_quota_fair / _fair_result; stream_fair.h:
k_fair_sums, k_fair_level, k_fair_done): every tick of a waiting-and-leased or rpc stream with the quota
and the level on is compared with the model (tests/stream_fair_model.py, pinned on the CPU by
tests/test_stream_fair_model.py):

  - ydc_stream_quota_fair_result integer for integer (the tick's number apart: it counts up);
  - everything the quota's own test compares, by that test's own rig (tests/test_stream_quota_gpu.Rig):
    the admitted counts, the label, the modes' check_tick with the label taken back, the inspection check
    and the invariant on the device's own state — against the model of the stream with the STATIC quota
    whose default_cap is, tick by tick, what the level came to.
"""
import copy

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_fair_model as F
from tests import stream_quota_model as Q
from tests import stream_wait_lease_model as WL
from tests import test_stream_inspect_gpu as ist
from tests import test_stream_quota_gpu as TQ
from tests import test_stream_rpc_gpu as TR
from tests import test_stream_wait_lease_gpu as TWL
from yadcc_amd import binding, pack, streaming

pytestmark = pytest.mark.gpu
MODES = TQ.MODES
OQ, WAITING, UNL = TQ.OQ, TQ.WAITING, TQ.UNL
A, B, INVALID = TQ.A, TQ.B, TQ.INVALID
C_, Z = 0x0A000003, 0x0A0000FF
REG, FIX, OFF = F.REGISTRY, F.FIXED, F.OFF


class Rig(TQ.Rig):
    """The quota's rig with the level on both sides: self.q is the Fair model over the rig's Quota."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.q = F.Fair(self.q)
        self.last_no = 0

    def fair(self, mode, pool=0, floor=0):
        self.ctx.stream_quota_fair(mode, pool, floor)
        self.q.fair(mode, pool, floor)

    def check_result(self, ctx=None, want=None):
        got = (ctx or self.ctx).stream_quota_fair_result()
        want = self.q.level_result if want is None else want
        for k in F.RESULT_FIELDS:
            if k != "tick_no" and k in want:
                assert got[k] == want[k], "tick %d: %s gpu %d model %d (%s)" % (self.t, k, got[k], want[k], got)
        return got

    def tick(self, ev, **kw):
        r = super().tick(ev, **kw)
        got = self.check_result()
        assert got["tick_no"] > self.last_no, (got, self.last_no)
        self.last_no = got["tick_no"]
        if self.q.mode != OFF and self.q.floor == 0:
            assert self.q.invariant(), (self.t, self.q.level_result)
        return dict(r, fair=got)


def new_ids(rig, base):
    return [t for t in rig.held() if t not in base]


def reqs(mode, ip, rows):
    """`rows` rows of requestor ip: single requests outside rpc mode, RPCs of up to 2 + 1 rows in it."""
    if mode == "wl":
        return [(ip, 1, 0)] * rows
    out = [(ip, 2, 1)] * (rows // 3)
    return out + ([(ip, rows % 3, 0)] if rows % 3 else [])


# ---- the hand vector and the boundaries ---------------------------------------------------------------

def hand_rig(mode, per_tick=40, slots=64):
    """One servant of `slots` slots; Z holds 2, B 3 and C_ 8 for good: O = 2 when A, B and C_ ask."""
    rig = Rig(mode, TQ.tiny_pool(1, slots), 64, per_tick, max_rows=512)
    rig.tick(rig.event(reqs(mode, Z, 2) + reqs(mode, B, 3) + reqs(mode, C_, 8)))
    assert rig.load([Z, B, C_]) == {Z: 2, B: 3, C_: 8}
    return rig, set(rig.held())


def ask(rig, base, mode):
    """A asks 10 rows, B 10 and C_ 4, nobody may wait; what the tick before granted goes back first."""
    ev = rig.event(reqs(mode, A, 10) + reqs(mode, B, 10) + reqs(mode, C_, 4), wait=0, free=new_ids(rig, base))
    return rig.tick(ev, snapshot=False)


@pytest.mark.parametrize("mode", MODES)
def test_the_hand_vector(mode):
    rig, base = hand_rig(mode)
    rig.fair(FIX, 20)
    r = ask(rig, base, mode)
    f = r["fair"]
    assert (f["level"], f["cap_default_effective"], f["pool"], f["held_total"], f["held_others"]) == (5, 5, 20, 13, 2)
    assert (f["n_askers"], f["n_override_askers"], f["asked_rows"], f["capacity_now"], f["mode"]) == (3, 0, 24, 64, FIX)
    a_imm, a_pre, clipped, refused = rig.ctx.stream_quota_result()
    adm = {}
    for ip, a in zip(rig.q.last_ips.tolist(), (a_imm.astype(np.int64) + a_pre).tolist()):
        adm[ip] = adm.get(ip, 0) + a
    assert adm == {A: 5, B: 2, C_: 0} and clipped == 24 - 7
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_boundaries_of_the_level(mode):
    """f(D) == P and P + 1, f(0) == P and P + 1, no fair asker, floor 0 and 3, an override above and below
    the level, default_cap below it, 50 / 100 / 150 percent of the registry, a pool that saturates."""
    rig, base = hand_rig(mode)
    steps = [  # (default, overrides), (mode, pool, floor) -> (level, effective default, pool)
        ((UNL, {}), (FIX, 37, 0), (UNL, UNL, 37)), ((UNL, {}), (FIX, 36, 0), (12, 12, 36)),
        ((UNL, {}), (FIX, 13, 0), (0, 0, 13)), ((UNL, {}), (FIX, 12, 0), (0, 0, 12)),
        ((UNL, {}), (FIX, 13, 3), (0, 3, 13)), ((UNL, {}), (FIX, 20, 3), (5, 5, 20)),
        ((9, {A: 1, B: 20, C_: 0}), (FIX, 13, 0), (UNL, 9, 13)),       # no fair asker
        ((UNL, {C_: 20}), (FIX, 32, 0), (9, 9, 32)), ((UNL, {C_: 2}), (FIX, 32, 0), (12, 12, 32)),
        ((4, {}), (FIX, 20, 0), (5, 4, 20)),                            # default_cap below the level
        ((UNL, {}), (REG, 50, 0), (10, 10, 32)), ((UNL, {}), (REG, 100, 0), (UNL, UNL, 64)),
        ((UNL, {}), (REG, 150, 0), (UNL, UNL, 96)), ((UNL, {}), (REG, 31, 0), (4, 4, 19)),
        ((UNL, {}), (FIX, 0xFFFFFFFF, 0), (UNL, UNL, 0xFFFFFFFE)),     # a saturating pool
    ]
    for caps, fair, want in steps:
        rig.set(*caps)
        rig.fair(*fair)
        f = ask(rig, base, mode)["fair"]
        assert (f["level"], f["cap_default_effective"], f["pool"]) == want, (caps, fair, f)
        assert (f["held_total"], f["held_others"], f["asked_rows"]) == (13, 2, 24), f
    rig.close()


# ---- both modes, every route ------------------------------------------------------------------------------

@pytest.mark.parametrize("stream_graph", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_randomised_differential(mode, stream_graph, monkeypatch):
    """200 servants with at most two slots, 300 requests a tick, 40 ticks, six requestors of which three
    have overrides; the pool's mode and numbers and the static settings change on the way. With the
    captured step and with the step enqueued kernel by kernel (stream_graph=0)."""
    TQ._graph(monkeypatch, stream_graph)
    rig = Rig(mode, TQ.crowded_pool(), 6000, 300, frees=60, renewals=20, n_envs=2, scripted=False, max_rows=1 << 14,
              requestors=TQ.REQUESTORS)
    rig.set(*TQ.THREE_CLASSES)
    rig.fair(REG, 60, 2)
    refused = waited = 0
    levels = set()
    for t in range(40):
        if t == 12:
            rig.fair(FIX, 250, 0)
        if t == 20:
            rig.set(150, {A: 200, B: 5})
        if t == 26:
            rig.fair(OFF)
        if t == 30:
            rig.fair(REG, 110, 0)
        r = rig.tick(rig.next(), snapshot=t % 8 == 0)
        refused += rig.q.result[3]
        waited += r["n_waiting"]
        levels.add(r["fair"]["level"])
    assert refused > 300 and waited > 100 and len(levels - {UNL, 0}) > 3, (refused, waited, levels)
    rig.close()


def _eager_rig(mode, quota=True):
    r = TQ._eager_rig(mode, quota=quota)
    r.__class__ = Rig
    r.q, r.last_no = F.Fair(r.q), 0
    return r


@pytest.mark.parametrize("mode", MODES)
def test_more_than_256_classes_runs_eagerly(mode):
    """eager_only: every tick is enqueued, the three launches with it, once; both modes of the pool. (The
    profile of the eager route names the launches from the batch's front on: of the three, k_fair_done.)"""
    rig = _eager_rig(mode)
    rig.set(30 if mode == "rpc" else 200, {A: 400, 0xFFFFFFFF: 0})
    rig.ctx.set_profiling(True)
    levels = set()
    for t in range(4):
        rig.fair(*((REG, 40, 0) if t < 2 else (FIX, 900 if mode == "wl" else 120, 1)))
        r = rig.tick(rig.next(), snapshot=t == 3)
        levels.add(r["fair"]["level"])
        prof = rig.ctx.kernel_profile()
        assert "k_fair_done" in prof and "k_quota_label" in prof, sorted(prof)
    assert levels - {UNL}, levels
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_mode_off_launches_nothing(mode):
    """The eager route names its launches: a stream with the quota on and the mode off (never set, or set
    and switched off again) names no k_fair_*."""
    rig = _eager_rig(mode)
    rig.set(30 if mode == "rpc" else 200, {A: 400})
    rig.ctx.set_profiling(True)
    for t in range(3):
        if t == 1:
            rig.fair(FIX, 50)
        if t == 2:
            rig.fair(OFF)
        rig.tick(rig.next(), snapshot=False)
        prof = rig.ctx.kernel_profile()
        assert "k_quota_label" in prof
        assert bool([k for k in prof if k.startswith("k_fair")]) == (t == 1), sorted(prof)
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_twin_with_a_pool_nobody_fills(mode):
    """The mode on with a huge pool answers like the quota-only stream: identical answers, lease snapshot,
    running_tasks and snapshot bytes."""
    rig = Rig(mode, TQ.crowded_pool(60, seed=7), 2000, 150, frees=30, renewals=10, n_envs=2, scripted=False,
              requestors=TQ.REQUESTORS)
    twin = TQ.uploaded(rig.ws.es.sv)
    twin = TR.begin(rig.ws, 150, max_leases=1 << 15, ctx=twin) if mode == "rpc" else TWL.begin(rig.ws, 1 << 15, 150, ctx=twin)
    twin.stream_inspect_begin()
    twin.stream_quota_begin(8)
    caps = (40, {A: 70, B: 3})
    twin.stream_quota_set(*caps)
    rig.set(*caps)
    rig.fair(FIX, 0xFFFFFFFF, 0)
    refused = 0
    for t in range(10):
        if t == 5:
            rig.fair(REG, 100000, 5)
        ev = rig.next()
        other = rig.G.gpu_tick(twin, rig.ws, ev)
        r = rig.tick(ev, snapshot=False)
        assert r["fair"]["level"] == UNL
        mine = other["status"] if mode == "rpc" else other[0]
        assert np.array_equal(mine, r["label"]), t
        for x, y in zip(rig.ctx.stream_quota_result(), twin.stream_quota_result()):
            assert np.array_equal(x, y), t
        for a, b in zip(rig.ctx.stream_leases(), twin.stream_leases()):
            assert np.array_equal(a, b), t
        assert np.array_equal(rig.ctx.get_running(), twin.get_running()), t
        refused += rig.q.result[3]
    assert refused > 10 and rig.ws.state.q.tag.size > 20
    assert rig.ctx.stream_snapshot() == twin.stream_snapshot(), "the level left a trace in the snapshot"
    twin.stream_end()
    twin.close()
    rig.close()


# ---- the askers and the table ---------------------------------------------------------------------------

def _crowd(mode, n, held_every=0):
    """n distinct askers in one tick: asker i sends 1 + i % 3 rows (rpc: one RPC with 1 + i % 2 immediate and
    i % 3 prefetch rows)."""
    if mode == "wl":
        return [(0x0B000000 + i, 1, 0) for i in range(n) for _ in range(1 + i % 3)]
    return [(0x0B000000 + i, 1 + i % 2, i % 3) for i in range(n)]


@pytest.mark.parametrize("sizes", [(1, 2, 63, 64, 65), (256, 257), (1025,)])
@pytest.mark.parametrize("mode", MODES)
def test_distinct_askers_in_one_tick(mode, sizes):
    """1 .. 1025 distinct askers in one tick, the table from its smallest size (1024 slots) to beyond the
    8192 slots at 1025 askers. Half of what is held goes back
    in every tick, so the askers come with loads of their own; the pool is two thirds of what they hold
    and ask."""
    per_tick = len(_crowd(mode, max(sizes)))
    rig = Rig(mode, TQ.tiny_pool(8, 1200), per_tick + 64, per_tick, max_rows=8192, max_leases=1 << 14)
    if mode == "wl":  # (an rpc tick has one request per asker: 1024, 1024 and 4096 slots)
        assert binding_slots(per_tick) == {65: 1024, 257: 2048, 1025: 8192}[max(sizes)]
    rig.set(UNL, {0x0B000001: 1, 0x0B000040: 2, 0x0B000100: 0})
    levels = set()
    for n in sizes:
        for rep in range(2):
            ev = rig.event(_crowd(mode, n), wait=0, free=rig.held()[::2])
            rows = len(ev["tags"]) if mode == "wl" else int(ev["n_immediate"].sum() + ev["n_prefetch"].sum())
            rig.fair(FIX, (len(rig.held()) - len(rig.held()[::2]) + rows) * 2 // 3, 0)
            r = rig.tick(ev, snapshot=False)
            assert r["fair"]["n_askers"] == n
            levels.add(r["fair"]["level"])
    assert levels - {UNL}, levels
    rig.close()


def binding_slots(max_tasks):
    """quota_slots of stream_quota.h."""
    s = 1024
    while s < 2 * max_tasks:
        s <<= 1
    return s


@pytest.mark.parametrize("n", [4096, 4097])
def test_the_fair_askers_at_both_sides_of_the_register_threshold(n):
    """Up to 4096 fair askers k_fair_level keeps their pairs in registers, above that it reads the list again in
    every round. n fair askers of one or two rows and 60 askers with overrides, which are not in the list."""
    over = {0x0C000000 + i: i % 5 for i in range(60)}
    crowd = [(0x0B000000 + i, 1, 0) for i in range(n) for _ in range(1 + i % 2)] + [(ip, 1, 0) for ip in over]
    rig = Rig("wl", TQ.tiny_pool(8, 1200), len(crowd) + 64, len(crowd), max_overrides=64, max_leases=1 << 14)
    rig.set(UNL, over)
    levels = []
    for pool in (n + 100, 5, 1 << 20, 2 * n):
        rig.fair(FIX, pool, 0)
        r = rig.tick(rig.event(crowd, wait=0, free=rig.held()[::3]), snapshot=False)
        assert (r["fair"]["n_askers"], r["fair"]["n_override_askers"]) == (n + 60, 60)
        levels.append(r["fair"]["level"])
    assert levels[:3] == [1, 0, UNL] and 0 < levels[3] < UNL, levels
    rig.close()


def test_one_asker_owns_every_request_of_a_tick():
    """2049 requests of one requestor: the wants are combined inside the waves before they reach ask[]."""
    rig = Rig("wl", TQ.tiny_pool(8, 1200), 2049 + 64, 2049, max_leases=1 << 14)
    rig.fair(FIX, 1000, 0)
    r = rig.tick(rig.event([(A, 1, 0)] * 2049, wait=0), snapshot=False)
    f = r["fair"]
    assert (f["n_askers"], f["asked_rows"], f["level"]) == (1, 2049, 1000) and int((r["label"] == OQ).sum()) == 1049
    rig.fair(FIX, 1500, 0)
    r = rig.tick(rig.event([(A, 1, 0)] * 2049, wait=0), snapshot=False)  # (it holds 1000 now)
    assert r["fair"]["level"] == 1500 and int((r["label"] == OQ).sum()) == 1549
    rig.close()


@pytest.mark.parametrize("d,level", [(1, 40), (4, 10), (5, 8), (64, 0)])
def test_one_wave_of_requests_of_d_askers(d, level):
    """64 requests, one wave of the pass that sums the wants, dealt round to d askers that hold nothing: one
    key, as many as a wave combines (4), one more (the lanes of the fifth add for themselves), and a key for
    every lane. A pool of 40 rows: the level is where sum min(a_r, level) <= 40 last holds."""
    rig = Rig("wl", TQ.tiny_pool(8, 1200), 128, 64, max_leases=1 << 14)
    rig.fair(FIX, 40, 0)
    r = rig.tick(rig.event([(0x0B000000 + i % d, 1, 0) for i in range(64)], wait=0), snapshot=False)
    f = r["fair"]
    assert (f["n_askers"], f["asked_rows"], f["held_total"], f["level"]) == (d, 64, 0, level), f
    assert int((r["label"] == OQ).sum()) == 64 - sum(min(len(range(j, 64, d)), level) for j in range(d))
    rig.close()


# ---- the totals: L, W, the registry ---------------------------------------------------------------------

def test_a_large_lease_table_with_a_hot_requestor_and_erased_leases():
    """|L| = 4 097 with one requestor holding 90 %; then 200 of its leases are freed (their records stay
    behind in the slots) in the tick that asks again: T counts what is live, and a third requestor's leases
    are the others'."""
    rig = Rig("wl", TQ.tiny_pool(8, 600), 2112, 2049, max_leases=1 << 14)
    n = 4097
    ips = np.where(np.arange(n) % 10 == 9, B, np.where(np.arange(n) % 10 == 8, Z, A)).astype(np.uint32)
    for lo in (0, 2049):
        rig.tick(rig.event([(int(ip), 1, 0) for ip in ips[lo:lo + 2049][:n - lo]]), snapshot=False)
    hot, quiet = int((ips == A).sum()), int((ips == Z).sum())
    assert len(rig.held()) == n
    mine = [t for t in rig.held() if rig.x.I.details[t][2] == A][:200]
    rig.fair(FIX, n - 200 + 60, 0)
    r = rig.tick(rig.event([(A, 1, 0)] * 150 + [(B, 1, 0)] * 50, free=mine))
    f = r["fair"]
    assert (f["held_total"], f["held_others"], f["asked_rows"]) == (n - 200, quiet, 200)
    # (60 rows are left: B, far below A, gets its 50 first; the other 10 raise the level above what A holds)
    assert f["level"] == hot - 200 + 10 and int((r["label"][:150] == OQ).sum()) == 140 and not (r["label"][150:] == OQ).any()
    rig.close()


@pytest.mark.parametrize("size", [0, 1, 1023, 1024, 1025])
@pytest.mark.parametrize("mode", MODES)
def test_waiting_entries_count_while_they_live(mode, size):
    """|W| == size when the tick finds it, a saturated pool: a third of the entries expire in that tick and
    another third is withdrawn; the rows of what is left are in T, and in O where their requestor does not ask."""
    rows = (1, 1) if mode == "rpc" else (1, 0)
    rig = Rig(mode, TQ.tiny_pool(1, 1), 2100, 1100, withdraw=2048, max_rows=8192)
    rig.tick(rig.event([(B, 1, 0)]))  # (the only slot is taken)
    i = np.arange(size)
    wait = np.where(i % 3 == 0, 1, 1000)
    ev = rig.event([(A if k % 5 else B, rows[0], rows[1]) for k in range(size)], wait=wait)
    rig.tick(ev, snapshot=False)
    assert len(rig.ws.state.q) == size
    gone = ev["tags"][i % 3 == 1]
    live = int((i % 3 == 2).sum()) * sum(rows)
    live_a = int(((i % 3 == 2) & (i % 5 != 0)).sum()) * sum(rows)
    rig.fair(FIX, 1 + live + 3 * sum(rows), 0)
    r = rig.tick(rig.event([(A, rows[0], rows[1])] * 5 + [(C_, rows[0], rows[1])] * 5), stage=gone)
    f = r["fair"]
    assert (f["held_total"], f["held_others"]) == (1 + live, 1 + live - live_a), f
    assert int((r["label"] == OQ).sum()) > 0 and int((r["label"] == WAITING).sum()) > 0
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_heartbeats_of_the_tick_move_the_pool(mode):
    """A heartbeat that sets a servant short of memory and one that sets max_tasks = 0: the pool of that
    same tick follows; then a structural heartbeat (a servant appended) and ydc_remove_servants."""
    rig = Rig(mode, TQ.tiny_pool(4, 4), 64, 24, max_rows=256)
    es = rig.ws.es
    rig.fair(REG, 100, 0)
    r = rig.tick(rig.event(reqs(mode, A, 6) + reqs(mode, B, 3)))
    assert (r["fair"]["capacity_now"], r["fair"]["pool"], r["fair"]["level"]) == (16, 16, UNL)
    es.sv["memory_available"][1] = 1 << 20
    es.abi["flags"][1] |= pack.SERVANT_LOW_MEMORY
    r = rig.tick(rig.event(reqs(mode, A, 6) + reqs(mode, B, 6)))
    assert (r["fair"]["capacity_now"], r["fair"]["held_total"], r["fair"]["level"]) == (12, 9, 6), r["fair"]  # (A holds 6 already; B 3 -> 6)
    es.sv["max_tasks"][2] = 0
    r = rig.tick(rig.event(reqs(mode, A, 3) + reqs(mode, C_, 3), wait=0))
    assert r["fair"]["capacity_now"] == 8 and r["fair"]["level"] == 0 and (r["label"] == OQ).all()
    ev = rig.event(reqs(mode, A, 3) + reqs(mode, C_, 3), wait=0)
    row, s_new = AM.append_servant(rig.ws, 0, 0x0A636363)
    ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
    ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
    r = rig.tick(ev)
    assert r["fair"]["capacity_now"] == 12 and r["fair"]["n_askers"] == 2
    removed = np.array([0], np.uint32)
    rig.ctx.remove_servants(removed)
    ist.lease.drop_rows(rig.ws, removed)
    rig.x.check()
    r = rig.tick(rig.event(reqs(mode, A, 3) + reqs(mode, C_, 3), wait=0))
    assert r["fair"]["capacity_now"] == 8
    rig.close()


@pytest.mark.parametrize("short", MODES)
def test_a_servant_expiring_in_the_tick_parks_its_leases(short):
    """Aliveness on: the leases of a servant that expires in this tick are parked when the sums are taken
    and count neither in T nor for their requestors; its slots leave the pool of the same tick."""
    sv = TQ.synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    first = AM.first_expiries(70, life=4)
    rig = Rig(short, sv, 1100 if short == "wl" else 400, 400 if short == "wl" else 40, frees=30, renewals=10, n_envs=2,
              scripted=False, alive=first, requestors=TQ.REQUESTORS, rpc_mix=TQ.BIG if short == "rpc" else None, max_rows=1536)
    rig.set(60, {A: 80, B: 3})
    rig.fair(REG, 150, 0)
    gen = AM.AliveGen(rig.ws, life=4, p_stop=0.3, p_short=0.3, seed=3)
    both, caps = 0, set()
    for t in range(12):
        ev = gen.next_tick()
        n, k = len(ev["tags"]), len(TQ.REQUESTORS)
        pick = np.where(rig.rng.random(n) < 0.5, 0, rig.rng.integers(0, k, n))
        ev["tasks"] = dict(ev["tasks"], requestor_ip=np.asarray(TQ.REQUESTORS, np.uint32)[pick])
        r = rig.tick(ev)
        both += bool(len(rig.q.base["removed"]) and r["fair"]["level"] != UNL)
        caps.add(r["fair"]["capacity_now"])
    assert both and len(caps) > 2, (both, caps)
    rig.close()


def test_after_reserve_and_restore():
    """The setting is carried over ydc_stream_reserve and the begins; after ydc_stream_restore + inspect_load +
    quota_begin the mode is off until it is set again. The restored stream is loaded with the records of
    two thirds of the leases only: the others are nobody's, in T all the same."""
    rig = Rig("wl", TQ.tiny_pool(6, 4), 64, 32)
    ctx = rig.ctx
    rig.set(UNL, {B: 2})
    rig.fair(FIX, 9, 1)
    r = rig.tick(rig.event([(A, 1, 0)] * 5 + [(B, 1, 0)] * 3 + [(C_, 1, 0)] * 6))
    assert r["fair"]["level"] == 3 and int((r["label"] == OQ).sum()) == 2 + 1 + 3
    ctx.stream_reserve(max_tasks=64, max_leases=1 << 16)
    ctx.stream_book_begin(64)
    ctx.stream_withdraw_begin(8)
    ctx.stream_depart_begin(4)
    ctx.stream_quota_begin(32)
    rig.q.begin(32)
    r = rig.tick(rig.event([(A, 1, 0), (C_, 1, 0), (Z, 1, 0)] * 4))
    assert r["fair"]["mode"] == FIX and r["fair"]["pool"] == 9 and r["fair"]["level"] == 1
    assert list(r["label"][:2]) == [OQ, OQ] and r["label"][2] < WAITING  # (Z, who holds nothing, gets one)
    blob, sv_cols, tk_cols = ctx.stream_snapshot(), ctx.stream_inspect_servants(), ctx.stream_inspect_tasks()
    b = binding.Context(device=0, max_servants=TQ.BOUND)
    b.stream_restore(blob)
    with pytest.raises(binding.YdcError, match=INVALID):
        b.stream_quota_fair(FIX, 9)
    b.stream_inspect_begin(sv_cols["discovered_at"], sv_cols["ever_assigned"])
    keep = np.arange(len(tk_cols["task_id"])) % 3 != 0
    b.stream_inspect_load(**{k: v[keep] for k, v in tk_cols.items()})
    b.stream_quota_begin(4)
    b.stream_quota_set(UNL, {B: 2})
    assert b.stream_quota_fair_result()["mode"] == OFF
    ev = rig.event([(A, 1, 0), (C_, 1, 0)] * 4, wait=0)
    ws_b = copy.deepcopy(rig.ws)  # the model of the restored stream: the records that were not loaded are gone
    for t in np.asarray(tk_cols["task_id"])[~keep].tolist():
        del ws_b.table.inspect.details[int(t)]
    qb = Q.Quota(WL, ws_b)
    qb.begin(4)
    qb.set(UNL, {B: 2})
    fb = F.Fair(qb)
    for fair in ((OFF, 0, 0), (FIX, 12, 0)):  # (off until it is set again)
        evb = copy.deepcopy(ev)
        evb["now"] = ev["now"] + fair[0]
        b.stream_quota_fair(*fair)
        fb.fair(*fair)
        got_b = TWL.gpu_tick(b, ws_b, evb)
        want = fb.tick(evb)
        assert np.array_equal(got_b[0], want["out"])
        got = b.stream_quota_fair_result()
        for k in F.RESULT_FIELDS:
            if k != "tick_no":
                assert got[k] == fb.level_result[k], (fair, k, got, fb.level_result)
        for x, y in zip(b.stream_quota_result(), qb.result):
            assert np.array_equal(x, y)
    n_l = len(tk_cols["task_id"])
    # (the first of the two ticks granted eight more; the others are B, Z and the three leases that are nobody's)
    assert got["held_total"] == n_l + 8 and got["held_others"] == 2 + int((~keep).sum()) and (want["out"] == OQ).all()
    b.stream_end()
    b.close()
    rig.tick(ev)
    rig.close()


# ---- conventions -------------------------------------------------------------------------------------------

def test_conventions_and_refusals():
    rig = Rig("wl", TQ.tiny_pool(1, 8), 8, 8, max_overrides=2)
    ctx = rig.ctx
    for bad in ((3, 1, 0), (0xFFFFFFFF, 1, 0), (REG, 0, 0), (REG, 0, 5)):
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_quota_fair(*bad)
    # a refused call leaves the setting: still off, nothing of the level in the answers
    r = rig.tick(rig.event([(A, 1, 0)] * 3, wait=0))
    assert r["fair"]["mode"] == OFF and r["fair"]["level"] == 0 and not (r["label"] == OQ).any()
    # fixed mode takes a pool of 0, the convenience sets the common case, a change of numbers alone holds at once
    rig.fair(FIX, 0, 0)
    r = rig.tick(rig.event([(A, 1, 0)] * 3, wait=0, free=rig.held()))
    assert r["fair"]["level"] == 0 and (r["label"] == OQ).all()
    result = streaming.fair_share(ctx, percent=50, floor=1)
    rig.q.fair(REG, 50, 1)
    r = rig.tick(rig.event([(A, 1, 0)] * 6 + [(B, 1, 0)] * 2, wait=0))
    assert result() == r["fair"] and (r["fair"]["pool"], r["fair"]["level"]) == (4, 2)
    # a refused tick leaves the setting and the last result
    before = ctx.stream_quota_fair_result()
    with pytest.raises(binding.YdcError, match=TQ.CAPACITY):
        rig.G.gpu_tick(ctx, rig.ws, rig.event([(A, 1, 0)] * 9))
    assert ctx.stream_quota_fair_result() == before
    r = rig.tick(rig.event([(A, 1, 0)] * 2, wait=0, free=rig.held()))
    assert r["fair"]["mode"] == REG and r["fair"]["pool"] == 4
    # end switches it off with the quota; a stream without the quota cannot have it
    ctx.stream_end()
    for begin in (None, lambda: ctx.stream_begin_waiting_leased(8, 8, 8, 8, 64, 8, 8, 8, 8)):
        if begin:
            begin()
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_quota_fair(FIX, 5)
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_quota_fair_result()
    ctx.stream_inspect_begin()
    with pytest.raises(binding.YdcError, match=INVALID):  # (inspection alone is not the quota)
        ctx.stream_quota_fair(FIX, 5)
    ctx.stream_quota_begin(4)
    ctx.stream_quota_fair(FIX, 5)
    ctx.stream_begin_waiting_leased(8, 8, 8, 8, 64, 8, 8, 8, 8)  # (the next begin call switches it off)
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_quota_fair(FIX, 5)
    ctx.stream_end()
    ctx.close()

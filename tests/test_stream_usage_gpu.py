"""Usage per requestor on the device (ydc_stream_usage_begin / _get / _find / _load; stream_usage.h:
k_usage_accrue, k_usage_find, k_usage_fold, k_usage_load, k_usage_rehash): every tick of a leased,
waiting-and-leased or rpc stream with the capability on goes through the modes' own check_tick with
inspection on (the rig of tests/test_stream_depart_gpu.py and its helpers), and ydc_stream_usage_get and
ydc_stream_usage_find are compared with the model (tests/stream_usage_model.py, pinned on the CPU by
tests/test_stream_usage_model.py) integer for integer after every tick. No test asserts a time.

URig(device=False) runs the model's side alone: the conditions the tests put on their inputs can be
rehearsed without a GPU (tests/test_stream_usage_model.py does)."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_usage_model as U
from tests import test_stream_inspect_gpu as ist
from tests.test_stream_depart_gpu import (BOUND, CAPACITY, INVALID, MODES, Rig, _eager_rig, _graph, crowded_pool, one)
from tests.test_stream_depart_model import A, B, C as CC, NOBODY, REQUESTORS, tiny_pool
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, streaming, synth

pytestmark = pytest.mark.gpu
M64 = U.M64


class URig(Rig):
    """The departure tests' rig (departure off unless asked for) with the usage capability on both sides."""

    def __init__(self, mode, sv, per_tick, quantum=1, usage=True, want=0, **kw):
        kw.setdefault("depart", False)
        self.u, self.quantum = None, quantum
        super().__init__(mode, sv, per_tick, **kw)
        if usage and getattr(self.ws.table, "inspect", None) is not None:
            self.usage_begin(want)

    def usage_begin(self, want=0):
        if self.u is None:
            self.u = U.Usage(self.ws, self.quantum)
        else:
            self.u.begin(self.quantum)
        if self.ctx:
            self.ctx.stream_usage_begin(self.quantum, want)

    def event(self, reqs=(), now=None, **kw):
        if now is not None:  # (the clock is the stream's tick number)
            self.ws.es.tick_no = int(now)
        return super().event(reqs, **kw)

    def next(self, step=1):
        """The seeded stream's next tick, `step` clock units after the previous one."""
        self.ws.es.tick_no += step - 1
        return super().next()

    def tick(self, ev, **kw):
        if self.u is None:
            return super().tick(ev, **kw)
        r = self.u.tick(ev, lambda e: Rig.tick(self, e, **kw))
        self.compare()
        return r

    def compare(self, ask=()):
        """ydc_stream_usage_get and _find against the model, integer for integer."""
        if not self.ctx:
            return
        t = self.t
        got, tot = streaming.usage(self.ctx)
        want, wtot = self.u.get()
        assert len(got) == len(want), "tick %d: %d rows, the model has %d" % (t, len(got), len(want))
        for k in U.DTYPE.names:
            assert np.array_equal(got[k], want[k]), "tick %d: usage %s gpu %s model %s" % (t, k, got[k], want[k])
        for k, v in wtot.items():
            assert tot[k] == v, "tick %d: totals %s gpu %d model %d" % (t, k, tot[k], v)
        s = tot["slots"]
        assert s >= U.MIN_SLOTS and s & (s - 1) == 0 and 2 * tot["n_keys"] <= s, tot
        ips = np.array(sorted(self.u.rows)[:40] + [NOBODY, 0, 0xFFFFFFFF] + [int(x) for x in ask], np.uint64).astype(np.uint32)
        found, model = self.ctx.stream_usage_find(ips), self.u.find(ips)
        for k in U.DTYPE.names:
            assert np.array_equal(found[k], model[k]), "tick %d: usage_find %s gpu %s model %s" % (t, k, found[k], model[k])

    def slots(self):
        return self.ctx.stream_usage_get()[1]["slots"] if self.ctx else U.slots_for(len(self.u.rows))

    def get(self, reset=False):
        """get on both sides (compared) -> the model's (rows, totals)."""
        want, wtot = self.u.get(reset)
        if self.ctx:
            got, tot = streaming.usage(self.ctx, reset=reset)
            assert got.tobytes() == want.tobytes() and all(tot[k] == v for k, v in wtot.items()), (got, want, tot, wtot)
        return want, wtot

    def load(self, rows, totals=None):
        self.u.load(rows, totals)
        if self.ctx:
            self.ctx.stream_usage_load(rows, totals)
        self.compare()

    def row(self, ip):
        return tuple(int(x) for x in self.u.rows.get(int(ip), [0] * 5))


def rows_of(pairs):
    """Rows of U.DTYPE from (requestor, slot, zombie, prefetch, wait, wait_row) tuples."""
    out = np.zeros(len(pairs), U.DTYPE)
    for i, p in enumerate(pairs):
        out[i] = (p[0], 0) + tuple(p[1:])
    return out


# ---- routes ----------------------------------------------------------------------------------------

def _scripted_route(mode, device=True, ticks=10):
    """A saturated tiny pool: leases that expire and turn zombie, a queue where the mode has one, prefetch
    rows in rpc mode, frees, clock steps of 0, 1 and 5 with quantum 3."""
    rig = URig(mode, tiny_pool(4, 2), 16, quantum=3, mw=64, max_leases=1 << 10, device=device)
    now, zero = 0, 0
    steps = [0, 1, 1, 5, 0, 2, 1, 7, 1, 3, 1, 1, 4, 0, 1, 2, 9, 1, 1, 1]
    for t in range(ticks):
        now += steps[t % len(steps)]
        reqs = [(int(REQUESTORS[(t + i) % 4]), 1 + i % 2, i % 3) if mode == "rpc" else (int(REQUESTORS[(t + i) % 4]), 1, 0)
                for i in range(3 + t % 4)]
        held = rig.held()
        rig.tick(rig.event(reqs, now=now, wait=4, lease_for=2 if t % 3 else 30, free=held[:2] if t % 4 == 3 else ()),
                 snapshot=False)
        zero += rig.u.dq == 0
    tot = rig.u.totals()
    assert zero >= 2 and tot["quanta"] == now // 3 and tot["ticks"] == ticks
    cols = [sum(r[k] for r in rig.u.rows.values()) for k in range(5)]
    assert cols[0] and cols[1] and (mode == "leased" or (cols[3] and cols[4])) and (mode != "rpc" or cols[2]), cols
    rig.close()


@pytest.mark.parametrize("stream_graph,ticks", [("1", 20), ("0", 8)])
@pytest.mark.parametrize("mode", MODES)
def test_scripted_ticks(mode, stream_graph, ticks, monkeypatch):
    """The three modes with the captured step and with the step enqueued kernel by kernel (stream_graph=0)."""
    _graph(monkeypatch, stream_graph)
    _scripted_route(mode, ticks=ticks)


@pytest.mark.parametrize("mode", MODES)
def test_more_than_256_classes_runs_eagerly(mode):
    """eager_only (more than 256 servant classes need the registry of the modes' own eager test): every tick is
    enqueued, the accrual with it, exactly once: the sums are the model's."""
    rig = _eager_rig(mode, depart=False)
    rig.__class__ = URig
    rig.u, rig.quantum = None, 1
    rig.usage_begin()
    for t in range(8):
        rig.tick(rig.next(step=1 + t % 2), snapshot=False)
    assert rig.u.totals()["quanta"] > 8 and len(rig.u.rows) >= 4
    rig.close()


# ---- the clock -------------------------------------------------------------------------------------

Q = 50


def _clock_vectors(device=True):
    """One lease per requestor, granted at `start` and freed at `end`: charged floor(end / q) - floor(start / q)."""
    out = []
    for start, end in ((Q - 1, Q), (Q - 1, Q + 1), (Q - 1, 2 * Q - 1), (-Q, -1), (-1, 0), (0, 1), (-Q - 1, -Q), (-1, Q), (7, 7)):
        rig = URig("leased", tiny_pool(2, 4), 8, quantum=Q, device=device)
        rig.tick(rig.event(one(A), now=start), snapshot=False)
        tid = rig.held()[0]
        if start == Q - 1:  # (two ticks with the same now in between)
            rig.tick(rig.event(one(B), now=start), snapshot=False)
        rig.tick(rig.event(free=[tid], now=end), snapshot=False)
        rig.tick(rig.event(now=end + 3 * Q), snapshot=False)  # (freed: nothing more)
        want = end // Q - start // Q
        assert rig.row(A) == (want, 0, 0, 0, 0), (start, end, rig.row(A))
        assert rig.u.totals()["quanta"] == (end + 3 * Q) // Q - start // Q
        out.append(want)
        rig.close()
    return out


def test_clock_hand_vectors():
    assert _clock_vectors() == [1, 1, 1, 0, 1, 0, 1, 2, 0]


def test_quantum_one_and_a_large_quantum():
    for q, clocks in ((1, (-3, -3, 0, 1, 10)), (1 << 40, (-(1 << 41) - 1, -1, 0, (1 << 40) - 1, 1 << 40, 5 << 40))):
        rig = URig("leased", tiny_pool(2, 4), 8, quantum=q)
        for t, now in enumerate(clocks):
            rig.ws.es.tick_no = 0  # (the seeds of the drawn tick stay small; the clock is written below)
            ev = rig.event(one(A) if t == 0 else ())
            ev["now"] = now
            ev["lease_expires_at"] = np.full(len(ev["lease_expires_at"]), 1 << 62, np.int64)
            rig.tick(ev, snapshot=False)
        assert rig.row(A)[0] == clocks[-1] // q - clocks[0] // q > 0
        rig.close()


def test_a_tick_with_dq_zero_leaves_the_table_as_it_is():
    rig = URig("wl", tiny_pool(1, 2), 8, quantum=10, mw=16)
    rig.tick(rig.event(one(A, 3) + one(B, 2), now=5), snapshot=False)
    rig.tick(rig.event(now=12), snapshot=False)
    before, tb = rig.ctx.stream_usage_get()
    rig.tick(rig.event(one(CC), now=19), snapshot=False)  # (floor(19 / 10) == floor(12 / 10))
    after, ta = rig.ctx.stream_usage_get()
    assert rig.u.dq == 0 and before.tobytes() == after.tobytes() and len(before) == 2
    assert (ta["ticks"], ta["quanta"], ta["n_keys"]) == (tb["ticks"] + 1, tb["quanta"], tb["n_keys"])
    rig.tick(rig.event(now=20), snapshot=False)
    assert rig.row(CC) == (0, 0, 0, 1, 1) and rig.row(A) == (4, 0, 0, 2, 2)
    rig.close()


# ---- columns ---------------------------------------------------------------------------------------

def test_zombies_after_an_expiry_tick(device=True):
    rig = URig("leased", tiny_pool(2, 4), 8, device=device)
    rig.tick(rig.event(one(A, 3) + one(B), lease_for=1))
    rig.tick(rig.event())
    rig.tick(rig.event())  # (now 2: overdue, zombies from here on)
    rig.tick(rig.event())
    rig.tick(rig.event())
    assert rig.row(A) == (12, 6, 0, 0, 0) and rig.row(B) == (4, 2, 0, 0, 0)
    rig.close()


def test_prefetch_leases_in_rpc_mode(device=True):
    rig = URig("rpc", tiny_pool(2, 4), 8, mw=16, device=device)
    # (8 slots: CC's immediate row and one of its prefetch rows are granted, the other prefetch rows are dropped)
    rig.tick(rig.event([(A, 2, 3), (B, 1, 0), (CC, 1, 4)], wait=50))
    rig.tick(rig.event())
    rig.tick(rig.event())
    assert rig.row(A) == (10, 0, 6, 0, 0) and rig.row(B) == (2, 0, 0, 0, 0) and rig.row(CC) == (4, 0, 2, 0, 0)
    rig.close()


def test_inspection_switched_on_late(device=True):
    """Half the leases were granted while inspection was off: they are nobody's, beside requestors 0 and
    0xFFFFFFFF, which are ordinary keys."""
    rig = URig("leased", tiny_pool(4, 8), 16, inspect=False, device=device)
    rig.tick(rig.event(one(A, 5) + one(0xFFFFFFFF, 3)))
    rig.inspect()
    rig.usage_begin()
    rig.tick(rig.event(one(0xFFFFFFFF, 2) + one(0, 3) + one(A, 3)))
    rig.tick(rig.event())
    rig.tick(rig.event())
    assert rig.u.totals()["unattributed_time"] == 24  # (8 leases, 3 ticks since the begin call)
    assert rig.row(0xFFFFFFFF) == (4, 0, 0, 0, 0) and rig.row(0) == (6, 0, 0, 0, 0) and rig.row(A) == (6, 0, 0, 0, 0)
    rig.close()


def test_erased_leases_whose_records_stay_behind(device=True):
    rig = URig("leased", tiny_pool(8, 64), 320, max_leases=1 << 10, device=device)
    rig.tick(rig.event(one(A, 200) + one(B, 100)), snapshot=False)
    rig.tick(rig.event(free=rig.held()[:200]), snapshot=False)
    rig.tick(rig.event(), snapshot=False)
    rig.tick(rig.event(), snapshot=False)
    assert rig.row(A) == (200, 0, 0, 0, 0) and rig.row(B) == (300, 0, 0, 0, 0)
    rig.close()


# ---- wave combining --------------------------------------------------------------------------------

def _lease_pattern(ips, device=True):
    """The given requestors' leases, one each, in one tick; three ticks of accrual."""
    rig = URig("leased", tiny_pool(8, 64), 512, max_leases=1 << 10, device=device)
    rig.tick(rig.event([(int(ip), 1, 0) for ip in ips]), snapshot=False)
    for _ in range(3):
        rig.tick(rig.event(), snapshot=False)
    assert sum(r[0] for r in rig.u.rows.values()) == 3 * len(ips)
    rig.close()


@pytest.mark.parametrize("combine", [None, "0"])
@pytest.mark.parametrize("pattern", ["one requestor", "64 distinct", "rounds", "rounds + 1", "300 of 7"])
def test_wave_patterns_over_the_lease_table(pattern, combine, monkeypatch):
    """The leases' slots are where their ids hash to, so a wave of the pass meets these mixes in some lanes:
    one key for every lane, all keys distinct, exactly kRequestorRounds (4) and one more; with the
    combining on (the default) and off (YDC_REQUESTOR_COMBINE=0, the switch requestor_index.h has)."""
    if combine is not None:
        monkeypatch.setenv("YDC_REQUESTOR_COMBINE", combine)
    n = 300
    ips = {"one requestor": np.full(n, A), "64 distinct": 0x0C000000 + np.arange(64), "rounds": A + np.arange(n) % 4,
           "rounds + 1": A + np.arange(n) % 5, "300 of 7": 0x0C000000 + 977 * (np.arange(n) % 7)}[pattern]
    _lease_pattern(ips.astype(np.uint32))


@pytest.mark.parametrize("combine", [None, "0"])
@pytest.mark.parametrize("size", [0, 1, 1023, 1024, 1025])
@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_waiting_queue_sizes_and_waves(mode, size, combine, monkeypatch):
    """|W| == size on a saturated pool; entry i is thread i's: runs of one requestor that change in mid-wave,
    64 distinct requestors in a wave, exactly 4 and 5 distinct keys in a wave; 1 ... 5 rows in rpc mode."""
    if combine is not None:
        monkeypatch.setenv("YDC_REQUESTOR_COMBINE", combine)
    rig = URig(mode, tiny_pool(1, 1), 1100, mw=1100, max_rows=8192, max_leases=1 << 14)
    rig.tick(rig.event(one(B)), snapshot=False)  # (the only slot is taken)
    i = np.arange(size)
    ip = np.where(i < 100, A + (i >= 37), np.where(i < 164, 0x0C000000 + i, np.where(i < 228, A + i % 4, A + i % 5)))
    reqs = [(int(ip[k]), 1 + (k % 5) // 2, (k % 5) - (k % 5) // 2) if mode == "rpc" else (int(ip[k]), 1, 0) for k in range(size)]
    rig.tick(rig.event(reqs), snapshot=False)
    assert len(rig.ws.state.q) == size
    rig.tick(rig.event(), snapshot=False)
    rig.tick(rig.event(), snapshot=False)
    want_rows = int((1 + i % 5).sum()) if mode == "rpc" else size
    assert sum(r[3] for r in rig.u.rows.values()) == 2 * size and sum(r[4] for r in rig.u.rows.values()) == 2 * want_rows
    rig.close()


# ---- growth ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [511, 512, 513])
def test_distinct_requestors_on_the_1024_slot_floor(n, device=True):
    rig = URig("leased", tiny_pool(8, 128), 600, max_leases=1 << 11, device=device)
    ips = (0x0C000000 + 13 * np.arange(n)).astype(np.uint32)
    rig.tick(rig.event([(int(x), 1, 0) for x in ips]), snapshot=False)
    assert rig.slots() == 1024
    rig.tick(rig.event(), snapshot=False)  # (claims n keys; behind it the bound is n)
    assert len(rig.u.rows) == n and rig.slots() == (1024 if n <= 512 else 2048)
    rig.tick(rig.event(one(A)), snapshot=False)
    rig.tick(rig.event(), snapshot=False)
    assert rig.slots() == (1024 if n < 512 else 2048) and rig.row(int(ips[-1])) == (3, 0, 0, 0, 0)
    rig.close()


def test_3000_requestors_brought_by_blocked_calls(device=True):
    """A saturated pool: the requestors arrive in W, 300 a tick, and the table doubles on the way; every
    row is carried across each growth (the comparison with the model after every tick)."""
    rig = URig("wl", tiny_pool(1, 1), 300, mw=3100, max_leases=1 << 12, device=device)
    rig.tick(rig.event(one(B)), snapshot=False)
    seen = [rig.slots()]
    for k in range(10):
        ips = 0x0D000000 + 7 * (300 * k + np.arange(300))
        rig.tick(rig.event([(int(x), 1, 0) for x in ips], wait=1000), snapshot=False)
        seen.append(rig.slots())
    rig.tick(rig.event(), snapshot=False)
    seen.append(rig.slots())
    assert len(rig.u.rows) == 3001 and seen[0] == 1024 and seen[-1] == 8192 and sorted(set(seen)) == [1024, 2048, 4096, 8192]
    assert all(b in (a, 2 * a) for a, b in zip(seen, seen[1:])), seen
    rig.close()


def test_requestors_that_arrive_inside_one_quantum(device=True):
    """Quantum 1000 on a clock that advances by one: ten ticks with dq == 0 claim nothing while 600 distinct
    requestors arrive in W, 60 a tick, on the 1024-slot floor. The bound keeps their allowance over those
    ticks, so the table has grown before the tick that accrues claims all of them at once; then 600 more in
    the next quantum, and a reset followed by ticks with dq == 0."""
    rig = URig("wl", tiny_pool(1, 1), 64, mw=1400, max_leases=1 << 11, quantum=1000, device=device)
    rig.tick(rig.event(one(B), now=1), snapshot=False)
    for k in range(10):
        ips = 0x0D000000 + 7 * (60 * k + np.arange(60))
        rig.tick(rig.event([(int(x), 1, 0) for x in ips], now=2 + k, wait=100000, lease_for=100000), snapshot=False)
        assert rig.u.dq == 0 and len(rig.u.rows) == 0
    # (the table has grown by now: in front of the tick whose bound, 1 + 60 k, first passed 512)
    rig.tick(rig.event(now=1000), snapshot=False)
    assert rig.u.dq == 1 and len(rig.u.rows) == 601 and rig.slots() == 2048
    for k in range(10, 20):
        ips = 0x0D000000 + 7 * (60 * k + np.arange(60))
        rig.tick(rig.event([(int(x), 1, 0) for x in ips], now=1001 + k, wait=100000, lease_for=100000), snapshot=False)
    rig.get(reset=True)
    rig.tick(rig.event(now=1500), snapshot=False)
    rig.tick(rig.event(now=1600), snapshot=False)
    assert len(rig.u.rows) == 0
    rig.tick(rig.event(now=2000), snapshot=False)
    assert len(rig.u.rows) == 1201 and rig.slots() == 4096 and rig.row(0x0D000000) == (0, 0, 0, 1, 1)
    rig.close()


def test_begin_again_grows_and_another_quantum_is_refused():
    rig = URig("leased", tiny_pool(2, 4), 8, quantum=5)
    rig.tick(rig.event(one(A, 2), now=4), snapshot=False)
    rig.tick(rig.event(now=11), snapshot=False)
    rig.usage_begin(want=3000)
    assert rig.slots() == 8192
    rig.compare()
    rig.usage_begin(want=10)  # (smaller: nothing happens)
    assert rig.slots() == 8192
    with pytest.raises(binding.YdcError, match=INVALID):
        rig.ctx.stream_usage_begin(6, 0)
    rig.tick(rig.event(now=15), snapshot=False)
    assert rig.row(A) == (6, 0, 0, 0, 0)
    rig.close()


# ---- persistence -----------------------------------------------------------------------------------

def test_a_requestor_that_left_keeps_its_row_and_reset_drops_it(device=True):
    rig = URig("wl", tiny_pool(1, 2), 8, mw=16, device=device)
    rig.tick(rig.event(one(A, 2) + one(B, 2)), snapshot=False)
    rig.tick(rig.event(free=rig.held()), snapshot=False)  # (A's leases go; B's requests take the slots)
    rig.tick(rig.event(), snapshot=False)
    assert rig.row(A) == (2, 0, 0, 0, 0) and rig.row(B) == (2, 0, 0, 2, 2)
    rig.tick(rig.event(), snapshot=False)
    assert rig.row(A) == (2, 0, 0, 0, 0) and sorted(rig.u.rows) == [A, B]
    rows, tot = rig.get(reset=True)
    assert len(rows) == 2 and tot["quanta"] == 3 and tot["ticks"] == 4
    assert rig.get()[1] == {"unattributed_time": 0, "quanta": 0, "ticks": 0, "n_keys": 0}
    rig.tick(rig.event(), snapshot=False)  # (claims today's holders only)
    assert sorted(rig.u.rows) == [B] and rig.row(B) == (2, 0, 0, 0, 0) and rig.u.totals()["quanta"] == 1
    rig.close()


def test_load_with_duplicates_then_an_accrual_and_a_wrap(device=True):
    rig = URig("wl", tiny_pool(1, 2), 8, mw=16, device=device)
    rig.tick(rig.event(one(A, 3)), snapshot=False)
    rig.load(rows_of([(A, 5, 1, 0, 7, 9), (NOBODY, 1, 2, 3, 4, 5), (A, 10, 0, 2, 0, 1), (CC, 0, 0, 0, 0, 0),
                      (B, M64 - 4, M64, 0, M64 - 9, 1 << 63)]),
             {"unattributed_time": M64, "quanta": 11, "ticks": 100})
    assert rig.row(A) == (15, 1, 2, 7, 10) and rig.row(CC) == (0, 0, 0, 0, 0) and sorted(rig.u.rows) == sorted([A, B, CC, NOBODY])
    rig.load(rows_of([]), None)
    for t in range(5):
        rig.tick(rig.event(one(B, 2) if t == 0 else (), wait=1000), snapshot=False)
    # (A: two leases and a waiting request for five ticks; B: two waiting requests for four)
    assert rig.row(A) == (25, 1, 2, 12, 15) and rig.row(B) == (M64 - 4, M64, 0, M64 - 1, (1 << 63) + 8)
    rig.load(rows_of([(B, 10, 1, 0, 10, 0)]))
    assert rig.row(B)[:2] == (5, 0) and rig.row(B)[3] == 8  # (2^64 - 5 + 10 reads 5)
    tot = rig.u.totals()
    assert (tot["unattributed_time"], tot["quanta"], tot["ticks"]) == (M64, 16, 106)
    rig.close()


def test_carrying_usage_across_a_restart():
    """get on the old side, a restore of the stream (which leaves the capability off, like inspection),
    begin and load on the new: the next accruals land on the loaded rows."""
    rig = URig("wl", tiny_pool(1, 2), 8, mw=16)
    rig.tick(rig.event(one(A, 2) + one(B)), snapshot=False)
    rig.tick(rig.event(), snapshot=False)
    ctx = rig.ctx
    rows, tot = streaming.usage(ctx)
    blob, sv_cols, tk_cols = ctx.stream_snapshot(), ctx.stream_inspect_servants(), ctx.stream_inspect_tasks()
    b = binding.Context(device=0, max_servants=BOUND)
    b.stream_restore(blob)
    for call in (b.stream_usage_get, lambda: b.stream_usage_find([A]), lambda: b.stream_usage_load(rows),
                 lambda: b.stream_usage_begin(1)):
        with pytest.raises(binding.YdcError, match=INVALID):  # (off, and inspection is off after a restore)
            call()
    b.stream_inspect_begin(sv_cols["discovered_at"], sv_cols["ever_assigned"])
    b.stream_inspect_load(**{k: tk_cols[k] for k in ("task_id", "started_at", "env_id", "requestor_ip", "prefetch")})
    b.stream_usage_begin(1)
    b.stream_usage_load(rows, tot)
    ev = rig.event(one(CC))
    rig.G.gpu_tick(b, rig.ws, ev)
    rig.tick(ev, snapshot=False)
    mine, theirs = streaming.usage(ctx), streaming.usage(b)
    assert mine[0].tobytes() == theirs[0].tobytes() and mine[1] == theirs[1] and rig.row(A) == (4, 0, 0, 0, 0)
    # ... and restoring into a context with the capability on switches it off
    ctx2_blob = b.stream_snapshot()
    b.stream_restore(ctx2_blob)
    with pytest.raises(binding.YdcError, match=INVALID):
        b.stream_usage_get()
    b.stream_end()
    b.close()
    rig.close()


# ---- composition -----------------------------------------------------------------------------------

def test_a_refused_tick_accrues_nothing():
    rig = URig("wl", tiny_pool(1, 2), 8, mw=8, quantum=2)
    rig.tick(rig.event(one(A, 2) + one(B), now=1), snapshot=False)
    before = rig.ctx.stream_usage_get()
    with pytest.raises(binding.YdcError, match=CAPACITY):
        rig.G.gpu_tick(rig.ctx, rig.ws, rig.event(one(A, 9), now=6))
    after = rig.ctx.stream_usage_get()
    assert before[0].tobytes() == after[0].tobytes() and before[1] == after[1]
    rig.tick(rig.event(now=9), snapshot=False)  # (the accepted tick spans the whole interval: floor(9/2) - floor(1/2))
    assert rig.u.dq == 4 and rig.row(A) == (8, 0, 0, 0, 0) and rig.row(B) == (0, 0, 0, 4, 4)
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_structural_heartbeat(mode, device=True):
    rig = URig(mode, tiny_pool(2, 1), 8, mw=16, quantum=2, device=device)
    rig.tick(rig.event(one(A, 2) + one(B, 2), now=1))
    ev = rig.event(one(CC), now=4)
    row, s_new = AM.append_servant(rig.ws, 0, 0x0A636363)
    ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
    ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
    rig.tick(ev)
    assert rig.u.dq == 2
    rig.tick(rig.event(now=9))
    assert rig.row(A) == (8, 0, 0, 0, 0) and rig.u.totals()["ticks"] == 3 and rig.u.totals()["quanta"] == 4
    rig.close()


def _alive_run(mode, device=True):
    """The removal route runs in front of the step and parks the expired servants' leases: they are charged
    for the interval that ends in the tick that orphans them, and the accrual runs once."""
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    first = AM.first_expiries(70, life=4)
    per_tick, mw = {"leased": (120, 64), "wl": (300, 1100), "rpc": (40, 400)}[mode]
    rig = URig(mode, sv, per_tick, mw=mw, frees=30, renewals=10, n_envs=2, scripted=False, alive=first, requestors=REQUESTORS,
               rpc_mix=BIG if mode == "rpc" else None, max_rows=1536, max_leases=1 << 14, quantum=3, device=device)
    gen = AM.AliveGen(rig.ws, life=4, p_stop=0.3, p_short=0.3, seed=3)
    removed, dqs, clocks = 0, [], []
    for t in range(12):
        ev = rig.spread(gen.next_tick())
        r = rig.tick(ev, snapshot=False)
        removed += len(np.asarray(r["removed"]))
        dqs.append(rig.u.dq)
        clocks.append(int(ev["now"]))
    # (quantum 3 on a clock that advances by one: ticks that accrue between ticks that do not)
    assert removed > 3 and 0 in dqs and 1 in dqs and rig.u.totals()["quanta"] == clocks[-1] // 3 - clocks[0] // 3 == sum(dqs)
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_servants_expire_through_aliveness(mode):
    _alive_run(mode)


def test_remove_servants_reserve_and_book_begin_keep_the_table():
    rig = URig("wl", tiny_pool(4, 2), 16, mw=16, quantum=2)
    ctx = rig.ctx
    rig.tick(rig.event(one(A, 5) + one(B, 5), now=1), snapshot=False)
    rig.tick(rig.event(now=2), snapshot=False)
    removed = np.array([1], np.uint32)
    ctx.remove_servants(removed)
    ist.lease.drop_rows(rig.ws, removed)
    rig.x.check()
    rig.compare()
    rig.tick(rig.event(now=5), snapshot=False)
    assert rig.u.dq == 1
    grows = (lambda: ctx.stream_reserve(max_tasks=32, max_leases=1 << 13), lambda: ctx.stream_book_begin(32),
             lambda: ctx.stream_depart_begin(4), lambda: ctx.stream_quota_begin(4))
    for grow, now in zip(grows, (6, 9, 10, 15)):  # (dq 1, 1, 1, 2)
        grow()
        rig.compare()
        rig.x.check()
        rig.tick(rig.event(one(CC), now=now), snapshot=False)
    assert rig.u.totals()["ticks"] == 7 and rig.u.totals()["quanta"] == 7 and rig.row(CC)[0] + rig.row(CC)[3] == 4 + 3 + 2
    rig.close()


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_with_departure_and_a_quota(mode, device=True):
    """A departed requestor is charged up to its departure tick and not after."""
    rig = URig(mode, tiny_pool(1, 4), 8, mw=16, depart=True, quota=True, quantum=2, device=device)
    rig.q.set(3)
    if device:
        rig.ctx.stream_quota_set(3)
    # (A: three leases and one over quota; B: one lease, two waiting. The clock: dq 2, 1, 1, 2)
    rig.tick(rig.event(one(A, 4) + one(B, 3), now=1), snapshot=False)
    rig.tick(rig.event(now=4), snapshot=False)
    rig.tick(rig.event(now=7), stage=[A], snapshot=False)
    at_departure = rig.row(A)
    assert at_departure == (9, 0, 0, 0, 0)
    rig.tick(rig.event(now=8), snapshot=False)
    rig.tick(rig.event(now=13), snapshot=False)
    assert rig.row(A) == at_departure and rig.row(B) == (12, 0, 0, 6, 6)
    rig.close()


def test_delta_apply_switches_it_off():
    rig = URig("wl", tiny_pool(1, 2), 8, mw=16)
    rig.tick(rig.event(one(A, 2) + one(B)), snapshot=False)
    base, side = streaming.standby_base(rig.ctx)
    b = binding.Context(device=0, max_servants=BOUND)
    streaming.standby_restore(b, base, side)
    b.stream_usage_begin(1)
    rig.tick(rig.event(one(CC)), snapshot=False)
    streaming.standby_step(rig.ctx, b)
    with pytest.raises(binding.YdcError, match=INVALID):
        b.stream_usage_get()
    rig.compare()  # (the primary's stays on)
    b.stream_end()
    b.close()
    rig.close()


# ---- the twin that never begins usage --------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_a_twin_that_never_begins_usage(mode):
    rig = URig(mode, crowded_pool(60, seed=7), 150, mw=2000, frees=30, renewals=10, n_envs=2, scripted=False,
               max_leases=1 << 14, requestors=REQUESTORS, quantum=2)
    twin = rig.new_context()
    twin.stream_inspect_begin()
    for t in range(20):
        ev = rig.next()
        other = rig.G.gpu_tick(twin, rig.ws, ev)
        r = rig.tick(ev, snapshot=False)
        assert np.array_equal(other["status"] if mode == "rpc" else other[0], r["label"]), t
        for a, b in zip(rig.ctx.stream_leases(), twin.stream_leases()):
            assert np.array_equal(a, b), t
        assert np.array_equal(rig.ctx.get_running(), twin.get_running()), t
    assert len(rig.held()) > 20 and len(rig.u.rows) >= 4
    assert rig.ctx.stream_snapshot() == twin.stream_snapshot(), "the capability left a trace in the snapshot"
    twin.stream_end()
    twin.close()
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_feature_off_means_untouched(mode):
    """A stream that never calls ydc_stream_usage_begin launches no kernel of the feature (the eager route
    names its launches); one that does names the accrual's followers as before."""
    rig = _eager_rig(mode, depart=False)
    rig.ctx.set_profiling(True)
    for t in range(2):
        rig.tick(rig.next(), snapshot=False)
        prof = rig.ctx.kernel_profile()
        assert prof and not [k for k in prof if k.startswith("k_usage")], sorted(prof)
        behind = {"leased": "k_lease_grant_inspect", "wl": "k_wait_lease_commit_inspect", "rpc": "k_rpc_settle"}[mode]
        assert behind in prof, sorted(prof)
    rig.close()


# ---- refusals --------------------------------------------------------------------------------------

def test_refusals_leave_their_outputs_untouched():
    lib = binding.lib()
    rig = URig("wl", tiny_pool(1, 2), 8, mw=8, usage=False)
    ctx = rig.ctx
    rows = np.full(4, 0xAB, U.DTYPE)
    n, tot = C.c_uint32(77), binding.UsageTotals(1, 2, 3, 4, 5)
    q = np.array([A, B], np.uint32)

    def untouched():
        return (n.value == 77 and (tot.unattributed_time, tot.quanta, tot.ticks, tot.n_keys, tot.slots) == (1, 2, 3, 4, 5)
                and rows.tobytes() == np.full(4, 0xAB, U.DTYPE).tobytes())
    # the capability off
    assert lib.ydc_stream_usage_get(ctx._h, rows.ctypes.data, 4, C.byref(n), C.byref(tot), 0) == -1 and untouched()
    assert lib.ydc_stream_usage_find(ctx._h, q.ctypes.data, 2, rows.ctypes.data) == -1 and untouched()
    assert lib.ydc_stream_usage_load(ctx._h, rows.ctypes.data, 2, None) == -1
    for bad in (0, -1, -(1 << 63)):
        assert lib.ydc_stream_usage_begin(ctx._h, bad, 0) == -1
    assert lib.ydc_stream_usage_begin(ctx._h, 1, (1 << 30) + 1) == -1
    rig.usage_begin()
    rig.tick(rig.event(one(A, 2) + one(B) + one(CC)), snapshot=False)
    rig.tick(rig.event(), snapshot=False)
    # more rows than cap: *out_n set, nothing written, nothing reset
    n.value = 77
    assert lib.ydc_stream_usage_get(ctx._h, rows.ctypes.data, 2, C.byref(n), C.byref(tot), binding.USAGE_RESET) == -4
    assert n.value == 3 and tot.quanta == 2 and rows.tobytes() == np.full(4, 0xAB, U.DTYPE).tobytes()
    rig.compare()
    n.value = 77
    assert lib.ydc_stream_usage_get(ctx._h, None, 4, C.byref(n), None, 0) == -1 and n.value == 77
    assert lib.ydc_stream_usage_get(ctx._h, rows.ctypes.data, 4, C.byref(n), None, 2) == -1 and n.value == 77
    assert lib.ydc_stream_usage_get(ctx._h, rows.ctypes.data, 4, None, None, 0) == -1
    assert lib.ydc_stream_usage_find(ctx._h, None, 2, rows.ctypes.data) == -1 and untouched()
    assert lib.ydc_stream_usage_find(ctx._h, q.ctypes.data, 2, None) == -1
    assert lib.ydc_stream_usage_load(ctx._h, None, 2, None) == -1
    rig.compare()
    # a plain stream and a stream without inspection have no such capability
    ctx.stream_end()
    assert lib.ydc_stream_usage_begin(ctx._h, 1, 0) == -1
    assert lib.ydc_stream_usage_get(ctx._h, rows.ctypes.data, 4, C.byref(n), None, 0) == -1 and n.value == 77
    ctx.stream_begin(8, 8, 8)
    assert lib.ydc_stream_usage_begin(ctx._h, 1, 0) == -1
    ctx.stream_end()
    ctx.close()
    bare = URig("leased", tiny_pool(1, 2), 8, inspect=False, usage=False)
    assert lib.ydc_stream_usage_begin(bare.ctx._h, 1, 0) == -1
    bare.ctx.stream_end()
    bare.ctx.close()


# ---- randomised differential -----------------------------------------------------------------------

def _differential(mode, ticks=40, device=True):
    """200 servants x 300 requests x `ticks` ticks, 80 requestors, random clock steps including 0, quantum 3;
    a late inspection begin (unattributed leases), resets and loads on the way."""
    sv = synth.make_servants(200, n_tasks_hint=4000, n_envs=2, seed=42)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    requestors = np.concatenate([REQUESTORS, 0x0C000000 + 31 * np.arange(74)]).astype(np.uint32)
    # (every row of W and of a tick's requests may become a lease: max_leases bounds their sum)
    rig = URig(mode, sv, 300, quantum=3, mw=3000, frees=60, renewals=20, n_envs=2, scripted=False, max_rows=1 << 15,
               max_leases=1 << 16, requestors=requestors, inspect=False, device=device)
    rng = np.random.default_rng(29)
    zero = resets = loads = 0
    for t in range(ticks):
        if t == 2:
            rig.inspect()
            rig.usage_begin()
        rig.tick(rig.next(step=int(rng.choice([0, 1, 1, 2, 5]))), snapshot=False)
        if rig.u is None:
            continue
        zero += rig.u.dq == 0
        if t in (15, 28):  # (a periodic export; the exported rows come back, half of them twice, with their totals)
            rows, old = rig.get(reset=True)
            rig.load(np.concatenate([rows, rows[::2]]), old)
            resets, loads = resets + 1, loads + 1
    rows, tot = rig.get()
    rig.close()
    return rows, tot, zero, resets, loads


def differential_conditions(rows, tot, zero, resets, loads, mode):
    """At least 50 rows, a tick with dq == 0, a reset and a load, unattributed_time and every column non-zero
    in total. All five columns are asked of the rpc stream. A waiting-and-leased stream has no prefetch
    leases and a leased one no W either, so those columns are zero there by construction and only the
    columns the mode has are asked for: narrower than "every one of the five" for those two modes."""
    assert len(rows) >= 50, len(rows)
    need = U.COLUMNS if mode == "rpc" else ("slot_time", "zombie_time", "wait_time", "wait_row_time") if mode == "wl" else \
        ("slot_time", "zombie_time")
    for k in need:
        assert int(rows[k].astype(object).sum()) > 0, k
    assert tot["unattributed_time"] > 0 and zero >= 1 and resets >= 1 and loads >= 1


@pytest.mark.parametrize("mode", MODES)
def test_randomised_differential(mode):
    differential_conditions(*_differential(mode), mode=mode)

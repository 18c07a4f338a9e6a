"""The servants' expiry on the device (ydc_stream_alive_begin / _stage / _removed / _get; k_alive_beat,
k_alive_due, k_alive_remap, k_alive_orphans): every tick of a leased, waiting-and-leased or rpc stream
with aliveness on is compared with the model (tests/stream_alive_model.py, pinned against the verbatim
reference's timer by tests/test_stream_alive_model.py) through the modes' own gpu_tick / check_tick —
outputs, running_tasks, the lease snapshot, the tick's counts — and on the expiry column, the removed
list with its orphan count, the host's bound and the book."""
import numpy as np
import pytest

from tests import stream_alive_cases as acases
from tests import stream_alive_model as AM
from tests import stream_book_model as BM
from tests import stream_lease_cases as cases
from tests import stream_lease_model as L
from tests import stream_rpc_cases as rcases
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WM
from tests import test_stream_lease_gpu as lease
from tests import test_stream_rpc_gpu as rpc
from tests import test_stream_wait_lease_gpu as wl
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu
MODS = {"leased": (L, lease), "wait_leased": (WM, wl), "rpc": (RM, rpc)}
BOOK_COLS = ("servant_idx", "task_grant_id", "servant_task_id", "digest_key")
FAR = acases.FAR


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def new_ctx(sv):
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(sv))
    return ctx


class Lively:
    """A stream `ws` of `mode` on `ctx` with aliveness on (and a book of max_book entries), and the
    model's side of both."""

    def __init__(self, mode, ws, ctx, expires, max_book=0, masks=False):
        self.M, self.G = MODS[mode]
        self.ws, self.ctx, self.masks, self.t = ws, ctx, masks, 0
        self.book = None
        if max_book:
            ctx.stream_book_begin(max_book)
            self.book = BM.Book(max_book)
        self.A = AM.attach(ws, expires, self.book)
        ctx.stream_alive_begin(expires)

    def check_alive(self, want=None):
        ctx, A = self.ctx, self.A
        assert np.array_equal(ctx.stream_alive(), A.expires), "tick %d: the expiry column differs" % self.t
        bound, alarms, _ = ctx.debug_alive()
        assert (bound, alarms) == (A.bound, A.alarms), (self.t, bound, alarms, A.bound, A.alarms)
        if want is not None:
            removed, orphans = ctx.stream_alive_removed()
            assert np.array_equal(removed, want["removed"]), (self.t, removed, want["removed"])
            assert orphans == want["orphans"], (self.t, orphans, want["orphans"])
        if self.book is not None:
            got, exp = ctx.stream_book(), self.book.columns()
            assert len(got[0]) == len(exp[0]), "tick %d: |B| gpu %d model %d" % (self.t, len(got[0]), len(exp[0]))
            for name, a, b in zip(BOOK_COLS, got, exp):
                assert np.array_equal(a, b), "tick %d: book %s differs" % (self.t, name)

    def tick(self, ev, snapshot=True, stage=True):
        if self.book is not None:
            p = BM.payload(ev)
            self.ctx.stream_book_stage(*p)
            self.book.stage(*p)
        if stage:  # (False: the expiries were staged before, and the staging is still pending)
            self.ctx.stream_alive_stage(ev["upd_expires_at"])
        # (the GPU first: gpu_tick reads the heartbeats' masks by the numbering the tick came with)
        got = self.G.gpu_tick(self.ctx, self.ws, ev, self.masks)
        want = AM.model_tick(self.M, self.ws, ev)
        self.G.check_tick(self.t, self.ctx, self.ws, got, want, snapshot=snapshot)
        self.check_alive(want)
        self.t += 1
        return want

    def state(self):
        c = self.ctx
        return (c.stream_alive(), c.get_running()) + c.stream_leases() + (c.stream_book() if self.book is not None else ())

    def refused(self, ev, match, stage=True):
        """The library refuses `ev`; column, leases, book and running_tasks stay."""
        before = self.state()
        if stage is not None:
            self.ctx.stream_alive_stage(ev["upd_expires_at"] if stage is True else stage)
        with pytest.raises(binding.YdcError, match=match):
            self.G.gpu_tick(self.ctx, self.ws, ev, self.masks)
        for x, y in zip(before, self.state()):
            assert np.array_equal(x, y), "a refused tick changed something"

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def proves(rec, A, removals=2, empty=2):
    """What a stream with aliveness must contain to prove anything, asserted from the model."""
    n_rm = sum(1 for r in rec if len(r["removed"]))
    orphans = sum(r["orphans"] for r in rec)
    assert n_rm >= removals and A.empty_alarms >= empty and orphans, (n_rm, A.empty_alarms, orphans)


HB, LIFE = 24, 4  # heartbeats per tick (of 70 servants: one every third tick) and the life each grants


def begun(mode, sv):
    """A stream of `mode` over the pool sv whose servants beat every third tick, and its context. The
    host's bound is the smallest expiry at the last alarm; its holder has beaten again by the time the
    clock passes it, so every few ticks an alarm ends empty."""
    if mode == "leased":
        ws = L.LeaseStream(sv, 400, 250, 60, L.LeaseTable(), n_envs=2, report_frac=0.3)
        ws.es.hb = HB
        return ws, lease.begin(ws, 1 << 14, 400)
    if mode == "wait_leased":
        ws = WM.new_stream(sv, 400, 250, 60, 3000, n_envs=2, rate=lambda now: 1.0 if now % 12 < 8 else 0.125,
                           report_frac=0.3)
        ws.es.hb = HB
        return ws, wl.begin(ws, 1 << 14, 400)
    ws = RM.new_stream(sv, 40, 300, 100, 1000, 1 << 12, n_envs=2, report_frac=0.3, **BIG)
    ws.es.hb = HB
    return ws, rpc.begin(ws, 40)


def seeded(mode, ticks=12, max_book=0, seed=3):
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    ws, ctx = begun(mode, sv)
    x = Lively(mode, ws, ctx, AM.first_expiries(70, life=LIFE), max_book)
    gen = AM.AliveGen(ws, life=LIFE, p_stop=0.2, p_short=0.2, seed=seed)
    rec = [x.tick(gen.next_tick()) for _ in range(ticks)]
    return x, rec


@pytest.mark.parametrize("mode,stream_graph", [("leased", "1"), ("leased", "0"), ("wait_leased", "1"), ("rpc", "1")])
def test_each_mode_with_aliveness(mode, stream_graph, monkeypatch):
    """70 servants, 12 ticks; some servants stop beating, some heartbeats carry a short life."""
    _graph(monkeypatch, stream_graph)
    x, rec = seeded(mode)
    proves(rec, x.A)
    assert x.ctx.debug_alive()[2] == sum(len(r["removed"]) for r in rec)
    x.close()


def test_leased_stream_with_a_book_and_aliveness():
    x, rec = seeded("leased", max_book=6000)
    proves(rec, x.A)
    assert len(x.book)
    x.close()


def beaters(ws, who, expires):
    """The stream's next tick with the heartbeats of exactly the servants `who`."""
    es = ws.es
    load_before = es.sv["current_load"].copy()
    ev = ws.next_tick()
    es.sv["current_load"][:] = load_before
    who = np.asarray(who, np.uint32)
    es.sv["current_load"][who] = np.minimum(es.foreign[who] + es.running[who], 0xFFFFFFFF).astype(np.uint32)
    rows = np.zeros(len(who), dtype=binding.ROW_DTYPE)
    for k in ("version", "num_processors", "current_load", "max_tasks"):
        rows[k] = es.sv[k][who]
    rows["flags"], rows["ip_id"], rows["env_mask"] = es.abi["flags"][who], es.abi["ip_id"][who], es.abi["env_mask"][who]
    ev.update(upd_idx=who, upd_rows=rows, upd_expires_at=np.asarray(expires, np.int64))
    return ev


def wide_pool():
    """300 servants (two workgroups of k_alive_due, five waves), leases on most of them."""
    sv = synth.make_servants(300, n_tasks_hint=3000, n_envs=2, seed=13)
    ls = L.LeaseStream(sv, 500, 200, 50, L.LeaseTable(), n_envs=2, report_frac=0.1)
    ctx = new_ctx(sv)
    ctx.stream_begin_leased(300, 16, 500, 1 << 14, 4096, 8192, ls.n_rep, 1 << 17)
    return Lively("leased", ls, ctx, np.full(300, FAR, np.int64))


def test_alive_beat_with_0_1_and_257_heartbeats():
    x = wide_pool()
    for t, who in enumerate([np.empty(0, np.uint32), np.array([299], np.uint32), np.arange(20, 277, dtype=np.uint32)]):
        ev = beaters(x.ws, who, FAR + 10 * (t + 1) + np.arange(len(who)))
        x.tick(ev)
        assert len(ev["upd_idx"]) == (0, 1, 257)[t]
    assert x.A.expires[299] == FAR + 20 and x.A.expires[276] == FAR + 30 + 256 and x.A.expires[277] == FAR
    x.close()


def reset_column(x, rows, value):
    """A second ydc_stream_alive_begin: the column replaced, `rows` expiring at `value`."""
    x.A.expires[np.asarray(rows, np.int64)] = value
    x.A.bound = int(x.A.expires.min())
    x.ctx.stream_alive_begin(x.A.expires)


def test_alive_due_across_waves_and_workgroups():
    x = wide_pool()
    gen = AM.AliveGen(x.ws, life=FAR, p_stop=0, p_short=0)
    for _ in range(3):
        x.tick(gen.next_tick())
    now = int(x.ws.es.tick_no)
    # (none of them beats in the next tick: the heartbeats are rows 90 .. 119)
    reset_column(x, [0, 63, 64, 255, 256, 299], now - 1)
    r = x.tick(gen.next_tick())
    assert list(r["removed"]) == [0, 63, 64, 255, 256, 299] and r["orphans"] > 0
    # every servant of one wave
    now = int(x.ws.es.tick_no)
    reset_column(x, np.arange(192, 256), now - 1)
    beat_next = set(((x.ws.es.hb_pos + np.arange(x.ws.es.hb)) % x.ws.es.n).tolist())
    assert not beat_next & set(range(192, 256))
    r = x.tick(gen.next_tick())
    assert list(r["removed"]) == list(range(192, 256)) and x.ws.es.n == 230
    # nobody due with the bound low: the beaters' old expiry is behind the clock, their heartbeat saves them
    now = int(x.ws.es.tick_no)
    beat_next = ((x.ws.es.hb_pos + np.arange(x.ws.es.hb)) % x.ws.es.n)
    reset_column(x, beat_next, now - 1)
    r = x.tick(gen.next_tick())
    assert r["alarm"] and len(r["removed"]) == 0 and x.A.empty_alarms == 1
    r = x.tick(gen.next_tick())
    assert not r["alarm"]
    x.close()


class GpuPlayer(acases.Player):
    """A hand-written case on the model and, mirrored call by call, on the device."""

    def __init__(self, make_stream, book):
        super().__init__(make_stream, False)
        ctx = new_ctx(self.ls.es.sv)
        ctx.stream_begin_leased(self.ls.es.hb + 8, 16, cases.MAX_TASKS, 64, 64, 64, self.ls.es.n, 64)
        table, self.ls.table.__class__ = self.ls.table, L.LeaseTable  # (Lively attaches again, with its book)
        del table.alive
        self.x = Lively("leased", self.ls, ctx, np.full(self.ls.es.n, FAR, np.int64), 256 if book else 0)
        self.A, self.book = self.x.A, self.x.book

    def on_set_expiry(self, row, value):
        self.x.ctx.stream_alive_begin(self.A.expires)

    def tick(self, beat=FAR, append=None, tasks=None, **kw):
        ev = self.make_ev(self.ls, beat, append, tasks, kw)
        x = self.x
        if self.book is not None:
            stid, dkey = ev["stid"], np.zeros(len(ev["stid"]), np.uint64)
            x.ctx.stream_book_stage(stid, dkey)
            self.book.stage(stid, dkey)
        x.ctx.stream_alive_stage(ev["upd_expires_at"])
        got = lease.gpu_tick(x.ctx, self.ls, ev)
        want = AM.model_tick(L, self.ls, ev)
        lease.check_tick(x.t, x.ctx, self.ls, got, want)
        x.check_alive(want)
        x.t += 1
        return want


@pytest.mark.parametrize("case", acases.CASES, ids=acases.IDS)
def test_hand_written_ticks(case):
    """tests/stream_alive_cases.py: a parked lease renewed, freed by id, freed twice, overdue, already a
    zombie, listed in its removed servant's own report; a removed servant with book entries; a
    heartbeat that saves and one that does not; an appended servant; a digest's last servant."""
    fn, make_stream, book = case
    p = GpuPlayer(make_stream, book)
    fn(p)
    assert p.x.t >= 2
    p.x.close()


def test_lease_table_at_exactly_max_leases_loses_servants():
    """max_leases 512 (1024 slots), filled to the brim; three servants with leases expire, with
    leases on the rows behind them."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=5)
    ls = L.LeaseStream(sv, 200, 0, 0, L.LeaseTable(512), n_envs=2)
    x = Lively("leased", ls, lease.begin(ls, 512, 200), np.full(60, FAR, np.int64))
    gen = AM.AliveGen(ls, life=FAR, p_stop=0, p_short=0)
    for n in (200, 200, 112):
        ev = lease.quiet(gen.next_tick())
        ev["tasks"] = {k: v[:n] for k, v in ev["tasks"].items()}
        ev["lease_expires_at"] = np.full(len(ev["tasks"]["env_id"]), 500, np.int64)
        x.tick(ev)
    assert len(ls.table) == 512, "the table is not at exactly max_leases"
    on = sorted({e[0] for e in ls.table.L.values()})
    beat_next = set(((ls.es.hb_pos + np.arange(ls.es.hb)) % ls.es.n).tolist())
    gone = [s for s in on if s not in beat_next][1:8:3]
    assert len(gone) == 3 and max(on) > gone[-1]
    reset_column(x, gone, 0)
    ev = lease.quiet(gen.next_tick())
    ev["tasks"] = {k: v[:0] for k, v in ev["tasks"].items()}
    ev["lease_expires_at"] = np.empty(0, np.int64)
    r = x.tick(ev)
    assert list(r["removed"]) == gone and r["orphans"] > 3
    ev = lease.quiet(gen.next_tick(), free_ids=np.array(sorted(ls.table.L)[:5] + [3], np.uint64))
    ev["tasks"] = {k: v[:0] for k, v in ev["tasks"].items()}
    ev["lease_expires_at"] = np.empty(0, np.int64)
    x.tick(ev)
    x.close()


def test_rpc_blocked_on_servants_that_expire():
    """An RPC waits for the one (loaded) servant of its digest; the servant expires: the RPC resolves
    as the model says, with EnvironmentNotFound."""
    sv = acases.two_digest_stream().es.sv
    ws = RM.new_stream(sv, rcases.MAX_REQUESTS, 0, 0, rcases.MAX_WAITING, rcases.MAX_ROWS, n_envs=2,
                       rate=lambda now: 1.0)
    x = Lively("rpc", ws, rpc.begin(ws, rcases.MAX_REQUESTS, max_leases=1 << 10, reports=ws.es.n),
               np.full(ws.es.n, FAR, np.int64))

    def tick(**kw):
        ev = rcases.scripted(ws, ws.next_tick(), **kw)
        ev["upd_expires_at"] = np.full(len(ev["upd_idx"]), FAR, np.int64)
        return x.tick(ev)

    r = tick(rpcs=[(1, 0, 9, 50, 1), (2, 0, 9, 50, 0)])
    assert r["status"][0] == RM.IDX_WAITING and r["n_waiting"] == 1 and r["n_granted"][1] == 2
    reset_column(x, [5], 0)
    r = tick()
    assert list(r["removed"]) == [5] and r["n_waiting"] == 0
    assert list(r["res_status"]) == [RM.IDX_ENV_NOT_FOUND]
    tick(rpcs=[(1, 0, 9, 50, 0)])
    x.close()


def test_more_than_256_classes_runs_eagerly_with_removals():
    """~600 servant classes (eager_only): every tick is enqueued, k_alive_beat with it, and the
    removal route runs in front of the enqueued step."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    ls = L.LeaseStream(sv, 1000, 500, 100, L.LeaseTable(), n_envs=n_envs)
    first = AM.first_expiries(700)
    first[[5, 300, 699]] = 2
    x = Lively("leased", ls, lease.begin(ls, 1 << 13, 1000), first, masks=True)
    gen = AM.AliveGen(ls, p_stop=0.5, p_short=0.5)
    rec = [x.tick(gen.next_tick(), snapshot=t % 3 == 0) for t in range(6)]
    proves(rec, x.A, removals=1, empty=0)
    x.close()


def test_bin_overflow_with_a_removal_in_the_tick_that_takes_the_exit():
    """The first eager exit (tests/test_stream_wait_lease_gpu.py: the registry that overflows a bin in
    tick 4) on a waiting-and-leased stream; a servant with leases expires in that very tick."""
    from tests.test_binsort_gpu import _context, _crowded_bin_pool
    sv = _crowded_bin_pool()
    sv["max_tasks"][48:] = 0
    sv["version"][47], sv["num_processors"][47], sv["max_tasks"][47] = 30, 1, 1
    ws = wl.Picky(sv, 3000, 1000, 200, WM.WaitLeaseState(6000), rate=lambda now: 1.0)
    c = _context(True)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        c.stream_begin_waiting_leased(4096 + 8, 16, 3000, 6000, 1 << 15, 4096, 8192, ws.n_rep, 1 << 17)
        x = Lively("wait_leased", ws, c, np.full(ws.es.n, FAR, np.int64))

        def alive(ev):
            ev["upd_expires_at"] = np.full(len(ev["upd_idx"]), FAR, np.int64)
            return ev

        for _ in range(4):
            x.tick(alive(ws.next_tick()))
        assert c.stats()["radix_passes"] == 0
        ev = ws.next_tick()
        es = ws.es
        es.sv["max_tasks"][48:96], es.sv["max_tasks"][96:] = 2047, 1
        es.abi = pack.to_abi_columns(es.sv)
        who = np.union1d(ev["upd_idx"], np.arange(48, 4096)).astype(np.uint32)
        rows = np.zeros(len(who), dtype=binding.ROW_DTYPE)
        for k in ("version", "num_processors", "current_load", "max_tasks"):
            rows[k] = es.sv[k][who]
        rows["flags"], rows["ip_id"], rows["env_mask"] = es.abi["flags"][who], es.abi["ip_id"][who], es.abi["env_mask"][who]
        ev = alive(dict(ev, upd_idx=who, upd_rows=rows))
        holders = sorted({e[0] for e in ws.table.L.values()} - set(who.tolist()))
        assert holders, "no lease on a servant that stays silent"
        reset_column(x, holders[:1], 0)
        r = x.tick(ev)
        assert c.stats()["radix_passes"] >= 1 and list(r["removed"]) == holders[:1] and r["orphans"]
        for _ in range(2):
            x.tick(alive(ws.next_tick()))
        c.stream_end()
    finally:
        c.close()


def test_reserve_and_book_begin_carry_the_column():
    """Twins: A begun large, B begun small and grown in mid-stream (ydc_stream_reserve) with a staging
    pending; then both gain a book (ydc_stream_book_begin), again with a staging pending. Both equal
    the model throughout and each other at the end."""
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    xs = []
    for max_leases in (1 << 14, 3000):
        ls = L.LeaseStream(sv, 400, 250, 60, L.LeaseTable(), n_envs=2, report_frac=0.3)
        ctx = new_ctx(sv)
        ctx.stream_begin_leased(HB + 8, 16, 400, max_leases, 4096, 8192, ls.n_rep, 1 << 17)
        ls.es.hb = HB
        xs.append((Lively("leased", ls, ctx, AM.first_expiries(70, life=LIFE)), AM.AliveGen(ls, life=LIFE)))
    for x, gen in xs:
        for _ in range(5):
            x.tick(gen.next_tick())
    (a, ga), (s, gs) = xs
    assert np.array_equal(a.A.expires, s.A.expires) and len(a.A.expires) < 70
    ev = gs.next_tick()
    s.ctx.stream_alive_stage(ev["upd_expires_at"])
    s.ctx.stream_reserve(max_leases=1 << 14, max_tasks=500)
    s.check_alive()
    s.tick(ev, stage=False)
    a.tick(ga.next_tick())
    for x, gen in xs:
        ev = gen.next_tick()
        x.ctx.stream_alive_stage(ev["upd_expires_at"])
        x.ctx.stream_book_begin(6000)
        x.check_alive()
        x.book = x.A.book = BM.Book(6000)
        x.tick(ev, stage=False)
        for _ in range(3):
            x.tick(gen.next_tick())
    assert len(a.book) and a.book.B == s.book.B
    assert np.array_equal(a.ctx.stream_alive(), s.ctx.stream_alive())
    for p, q in zip(a.ctx.stream_leases(), s.ctx.stream_leases()):
        assert np.array_equal(p, q)
    a.close()
    s.close()


def test_remove_servants_by_the_caller_compacts_the_column():
    x, rec = seeded("leased", ticks=5, max_book=6000)
    on = sorted({e[0] for e in x.ws.table.L.values()})
    removed = np.array(on[1:8:3], np.uint32)
    x.ctx.remove_servants(removed)
    x.A.remove(removed)
    x.check_alive()
    gen = AM.AliveGen(x.ws, life=LIFE, seed=9)
    for _ in range(4):
        x.tick(gen.next_tick())
    x.close()


def alias_checked(es, batch, out, aliased):
    """The placement `out` of `batch`, after asserting that it EQUALS the reference's on address
    strings (tests/alias_reference.py) for the registry `es` holds at this moment. aliased: requestor
    id -> the rows that answer to it through the alias list. A row's location is "<alias>:<ip>:<row>"
    (it answers to "<alias>" and to nothing shorter than its whole host part), or "<ip>:<row>"."""
    from tests import alias_reference as AR
    sv = es.registry_snapshot()
    alias_of = {s: ip for ip, rows in aliased.items() for s in rows}
    locations = [("%d:" % alias_of[s] if s in alias_of else "") + "%d:%d" % (int(sv["ip"][s]), s)
                 for s in range(len(sv["ip"]))]
    assert not set(int(x) for x in sv["ip"]) & set(aliased), "an alias id that is also a primary id"
    assert not {int(sv["ip"][s]) for s in alias_of} & {int(r) for r in batch["requestor_ip"]}  # (see the locations)
    want = AR.dispatch(locations, sv, [str(int(r)) for r in batch["requestor_ip"]], batch)[0]
    assert np.array_equal(np.asarray(out, np.uint32), want), (out, want, aliased)
    return out


def test_host_aliases_of_survivors_outlive_a_removal_tick():
    """Requests from an aliased host count as the aliased servant's own (they are not placed there).
    The alias still does after a row in front of that servant was erased inside a tick. Every tick
    frees the previous one's grants, so the pool looks the same to each."""
    p = GpuPlayer(cases.small_stream, False)
    ctx = p.x.ctx
    alias_ip = (192 << 24) + 77
    z = np.zeros(4, np.uint32)
    ask = {"env_id": z, "min_version": z, "requestor_ip": z + np.uint32(alias_ip)}
    last = []

    def placed_on():
        ev = p.make_ev(p.ls, FAR, None, ask, dict(n=4, lease=[100] * 4, free=list(last)))
        ctx.stream_alive_stage(ev["upd_expires_at"])
        out, ids = lease.gpu_tick(ctx, p.ls, ev)[:2]
        # (the lease model does not know the alias; the placement it is handed is checked against
        # the reference on address strings, on the registry as it is when the batch is placed)
        p.A.stage(ev["upd_expires_at"])
        held = set(p.ls.table.L)
        r = p.ls.table.tick(p.ls.es.running, ev, lambda batch: alias_checked(p.ls.es, batch, out, aliased))
        p.ls.commit(held, r["out"])
        assert np.array_equal(ids, r["task_id"]) and int((out < L.IDX_ENV_NOT_FOUND).sum()) == 4
        assert np.array_equal(ctx.get_running(), p.ls.es.running.astype(np.uint32))
        last[:] = ids.tolist()
        return out.tolist(), p.A.removed_last.tolist()

    aliased = {}  # requestor id -> the rows that answer to it through the alias list
    out, _ = placed_on()
    target = max(out)  # where such requests go when nothing keeps them away
    assert target > 0, "the favourite is row 0: no row in front of it can be erased"
    ctx.set_host_aliases(np.array([alias_ip], np.uint32), np.array([target], np.uint32))
    aliased[alias_ip] = {target}
    out, _ = placed_on()
    assert target not in out, "the alias does not keep its servant's own requests away"
    p.set_expiry(0, 0)
    aliased[alias_ip] = {target - 1}  # (row 0 leaves inside the tick, before the batch is placed)
    out, removed = placed_on()
    assert removed == [0] and target - 1 not in out, "the alias did not follow its servant to row %d" % (target - 1)
    # (set again by the caller: without the entry the same requests do reach it)
    ctx.set_host_aliases(np.empty(0, np.uint32), np.empty(0, np.uint32))
    aliased.clear()
    out, _ = placed_on()
    assert target - 1 in out
    p.x.close()


def test_refusals_leave_everything_untouched():
    x, rec = seeded("leased", ticks=4, max_book=6000)
    gen = AM.AliveGen(x.ws, life=LIFE, p_stop=0, p_short=0)
    ev = gen.next_tick()
    n = len(ev["upd_idx"])
    assert n >= 2
    p = BM.payload(ev)
    x.ctx.stream_book_stage(*p)
    x.refused(ev, "staged with ydc_stream_alive_stage", stage=ev["upd_expires_at"][:-1])  # count mismatch
    twice = dict(ev, upd_idx=np.concatenate([ev["upd_idx"][:-1], ev["upd_idx"][:1]]))
    x.refused(twice, "a second time")  # a servant twice in upd_idx
    with pytest.raises(binding.YdcError, match="expiries for"):
        x.ctx.stream_alive_begin(np.zeros(x.ws.es.n + 1, np.int64))  # n differs from the servant count
    # (the staging of the refused ticks is still there and is consumed by the accepted one)
    got = lease.gpu_tick(x.ctx, x.ws, ev)
    x.book.stage(*p)
    want = AM.model_tick(L, x.ws, ev)
    lease.check_tick(x.t, x.ctx, x.ws, got, want)
    x.check_alive(want)
    # nothing staged with heartbeats
    ev = gen.next_tick()
    x.ctx.stream_book_stage(*BM.payload(ev))
    x.refused(ev, "staged with ydc_stream_alive_stage", stage=None)
    x.tick(ev)
    # cap too small
    r = None
    while r is None or not len(r["removed"]):
        ev = gen.next_tick()
        ev["upd_expires_at"][0] = int(ev["now"]) - 1
        r = x.tick(ev)
    n_rm, orphans = binding.C.c_uint32(0), binding.C.c_uint32(0)
    rc = binding.lib().ydc_stream_alive_removed(x.ctx._h, None, 0, binding.C.byref(n_rm), binding.C.byref(orphans))
    assert rc != 0 and n_rm.value == len(r["removed"])
    x.close()


def test_wrong_mode_and_a_stream_without_aliveness():
    sv = synth.make_servants(20, n_tasks_hint=400, n_envs=1, seed=2)
    ctx = new_ctx(sv)
    with pytest.raises(binding.YdcError, match="ydc_stream_alive_begin"):
        ctx.stream_alive_begin(np.zeros(20, np.int64))  # no stream
    ctx.stream_begin(8, 8, 64)
    with pytest.raises(binding.YdcError, match="ydc_stream_alive_begin"):
        ctx.stream_alive_begin(np.zeros(20, np.int64))  # a plain stream keeps no leases
    ctx.stream_end()
    ctx.stream_begin(8, 8, 64, max_waiting=64)
    with pytest.raises(binding.YdcError, match="ydc_stream_alive_begin"):
        ctx.stream_alive_begin(np.zeros(20, np.int64))
    ctx.stream_end()
    # a leased stream that never switches it on answers as before and has no column
    ls = L.LeaseStream(sv, 60, 30, 10, L.LeaseTable(), n_envs=1)
    ctx.stream_begin_leased(ls.es.hb + 8, 16, 60, 1 << 10, 64, 256, ls.n_rep, 1 << 12)
    lease.drive(ctx, ls, 4)
    for call in (ctx.stream_alive, ctx.stream_alive_removed, lambda: ctx.stream_alive_stage(np.zeros(1, np.int64))):
        with pytest.raises(binding.YdcError, match="keeps no servant expiries"):
            call()
    # switched on, then off again by the next begin
    ctx.stream_alive_begin(None, n=20)
    assert np.array_equal(ctx.stream_alive(), np.full(20, AM.NEVER, np.int64))
    ctx.stream_begin_leased(ls.es.hb + 8, 16, 60, 1 << 10, 64, 256, ls.n_rep, 1 << 12)
    with pytest.raises(binding.YdcError, match="keeps no servant expiries"):
        ctx.stream_alive()
    ctx.stream_end()
    ctx.close()

"""ydc_stream_snapshot / ydc_stream_restore: everything an open stream keeps on the device leaves
context A as one block of bytes and enters a fresh context B, which never saw the registry.

Every twin case has one shape: A runs some ticks against the mode's model (tests/stream_lease_model.py,
stream_wait_lease_model.py, stream_rpc_model.py, stream_alive_model.py, stream_book_model.py — all
pinned against the verbatim reference) and is snapshotted; B is restored from the blob; both get the
same further ticks. Every tick of each is compared with the model through the modes' own check_tick
(outputs, running_tasks, the lease snapshot, the tick's counts in ydc_get_stats), plus the expiry
column, the removed list and the book where they are on, and A and B are compared with each other,
exactly, as the twins of tests/test_stream_reserve_gpu.py are. The blob itself is read with
yadcc_amd/snapshot.py and compared with the model's state section by section. Every test fails
without the feature: the entry points are missing."""
import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_book_model as BM
from tests import stream_lease_model as L
from tests import stream_rpc_cases as rcases
from tests import stream_rpc_model as RM
from tests import stream_snapshot_model as SM
from tests import stream_wait_lease_cases as wcases
from tests import stream_wait_lease_model as WM
from tests import test_stream_alive_gpu as alive
from tests import test_stream_lease_gpu as lease
from tests import test_stream_reserve_gpu as reserve
from tests import test_stream_rpc_gpu as rpc
from tests import test_stream_wait_lease_gpu as wl
from tests.test_stream_reserve_gpu import all_granted, new_ctx, requests, roomy_pool, same_outputs, same_state
from yadcc_amd import binding, snapshot, synth

pytestmark = pytest.mark.gpu
BOOK_COLS = alive.BOOK_COLS
INVALID, CAPACITY = "invalid argument", "capacity"


class Run:
    """The stream `ws` of `mode` on one context or on two; with a book and aliveness where given."""
    MODS = {"leased": (L, lease), "wait_leased": (WM, wl), "rpc": (RM, rpc)}

    def __init__(self, mode, ws, ctx, masks=False, A=None, book=None):
        self.mode, self.ws, self.ctxs, self.masks, self.A, self.book, self.t = mode, ws, [ctx], masks, A, book, 0
        self.M, self.G = self.MODS[mode]
        self.aliases = ((), ())

    def extras(self, ctx):
        out = ()
        if self.A is not None:
            out += (ctx.stream_alive(),) + ctx.stream_alive_removed()
        if self.book is not None:
            out += ctx.stream_book()
        return out

    def check_extras(self, ctx, want):
        if self.A is not None:
            assert np.array_equal(ctx.stream_alive(), self.A.expires), "tick %d: the expiry column differs" % self.t
            removed, orphans = ctx.stream_alive_removed()
            assert np.array_equal(removed, want["removed"]) and orphans == want["orphans"], (self.t, removed, orphans)
        if self.book is not None:
            got, exp = ctx.stream_book(), self.book.columns()
            assert len(got[0]) == len(exp[0]), "tick %d: |B| gpu %d model %d" % (self.t, len(got[0]), len(exp[0]))
            for name, a, b in zip(BOOK_COLS, got, exp):
                assert np.array_equal(a, b), "tick %d: book %s differs" % (self.t, name)

    def tick(self, ev):
        """The same tick on every context (the GPU first: gpu_tick reads the heartbeats' masks by the
        numbering the tick came with), then the model's; every context against the model, and the
        twins against each other. -> the model's record."""
        got = []
        for c in self.ctxs:
            if self.book is not None:
                c.stream_book_stage(*BM.payload(ev))
            if self.A is not None:
                c.stream_alive_stage(ev["upd_expires_at"])
            got.append(self.G.gpu_tick(c, self.ws, ev, self.masks))
        if self.book is not None:
            self.book.stage(*BM.payload(ev))
        if self.A is not None:
            want = AM.model_tick(self.M, self.ws, ev)
        elif self.book is not None:
            want = BM.model_tick(self.M, self.ws, self.book, ev)
        else:
            want = self.M.model_tick(self.ws, ev)
        for c, g in zip(self.ctxs, got):
            self.G.check_tick(self.t, c, self.ws, g, want)
            self.check_extras(c, want)
        if len(self.ctxs) == 2:
            same_outputs(self.t, self.mode, *got)
            same_state(self.t, *self.ctxs)
            for x, y in zip(self.extras(self.ctxs[0]), self.extras(self.ctxs[1])):
                assert np.array_equal(x, y), "tick %d: book or expiry column differs between the twins" % self.t
        self.t += 1
        return want

    def drive(self, ticks, gen=None):
        return [self.tick((gen or self.ws).next_tick()) for _ in range(ticks)]

    def state(self, caps=None):
        """The model's state as the blob must show it."""
        return SM.state_of(self.mode, self.ws, caps or self.ctxs[0].stream_caps(), self.t, self.book, self.A,
                           self.book.max_book if self.book is not None else 0, self.aliases)

    def fork(self, drop_a=False, **want):
        """Snapshot of A, compared with the model's state; B restored from it into a fresh context.
        drop_a: A is destroyed before B ticks, so that nothing is shared. -> the blob."""
        a = self.ctxs[0]
        blob = a.stream_snapshot()
        SM.same(snapshot.parse(blob), self.state())
        b = binding.Context(device=0)
        caps = b.stream_restore(blob, **want)
        if not want:
            assert caps == a.stream_caps()
        if drop_a:
            a.stream_end()
            a.close()
            self.ctxs = [b]
        else:
            self.ctxs = [a, b]
            # (same_state without the last tick's counters: B has not ticked yet)
            for name, x, y in zip(reserve.SNAP, a.stream_leases(), b.stream_leases()):
                assert np.array_equal(x, y), "lease snapshot %s differs right after the restore" % name
            assert np.array_equal(a.get_running(), b.get_running()), "running differs right after the restore"
            for x, y in zip(self.extras(a)[:1] + self.extras(a)[3:], self.extras(b)[:1] + self.extras(b)[3:]):
                assert np.array_equal(x, y), "book or expiry column differs right after the restore"
        if self.A is not None:  # (the last tick's result lists are not state)
            removed, orphans = b.stream_alive_removed()
            assert len(removed) == 0 and orphans == 0
        return blob

    def end(self):
        if self.mode != "leased":  # W itself, one tag per entry, in queue order
            w = self.ws.state.take()
            for c in self.ctxs:
                assert np.array_equal(c.stream_waiting_take(), w)
        for c in self.ctxs:
            c.stream_end()
            c.close()


def leased_run(sv, ls, caps, masks=False):
    ctx = new_ctx(sv)
    ctx.stream_begin_leased(ls.es.hb + 8, 16, caps["tasks"], caps["leases"], caps["renewals"], caps["frees"],
                            caps["reports"], caps["report_ids"])
    return Run("leased", ls, ctx, masks)


def report(lists):
    off = np.cumsum([0] + [len(ids) for _, ids in lists]).astype(np.uint32)
    return dict(report_servants=np.array([s for s, _ in lists], np.uint32), report_off=off,
                report_ids=np.array([t for _, ids in lists for t in ids], np.uint64))


def zombies_of(T):
    of = {}
    for t, e in sorted(T.L.items()):
        if e[2]:
            of.setdefault(e[0], []).append(t)
    return of


def test_leased_full_table_with_state_that_straddles_the_snapshot():
    """max_leases 1024 (a table of 2048 slots: two tiles of k_lease_pack) filled exactly: 90 zombies, 30
    renewed expiries, 100 ids freed out of the middle of the id range, heartbeats that changed
    current_load in every tick. In the tick before the snapshot a servant lists its zombies (they carry
    that tick's stamp); the last requests' leases end at the snapshot's clock and at the next tick's.
    First tick after the restore: that servant reports without one of its zombies — exactly that one is
    swept; the servants of the leases that just ran out report — those are swept in the tick that makes
    them zombies; the leases with expires_at == now are not overdue. Then every old live id renews,
    every zombie refuses, and a free of each old id gives its servant's slot back."""
    sv = roomy_pool(40, 40)
    ls = L.LeaseStream(sv, 300, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 4
    run = leased_run(sv, ls, dict(tasks=300, leases=1024, renewals=1024, frees=1024, reports=40, report_ids=1024))
    T = ls.table
    exp0 = np.full(300, 1000, np.int64)
    exp0[:100] = 2  # (overdue from now == 3 on)
    assert all_granted(run.tick(requests(ls, 300, exp0, 1)))                 # now 0: ids 0 .. 299
    assert all_granted(run.tick(requests(ls, 300, 1000, 2)))                 # now 1: ids 300 .. 599
    ren = np.concatenate([np.arange(10), np.arange(250, 270)]).astype(np.uint64)
    want = run.tick(requests(ls, 0, 0, 3, free_ids=np.arange(150, 250, dtype=np.uint64), renew_ids=ren,
                             renew_expires_at=np.full(30, 5000, np.int64)))  # now 2
    assert want["freed"] == 100 and want["renewed"].all() and len(T) == 500
    want = run.tick(requests(ls, 300, 1000, 4))                              # now 3: ids 600 .. 899; 10 .. 99 overdue
    assert all_granted(want) and want["expired"] == 90
    zo = zombies_of(T)
    sa = max(zo, key=lambda s: len(zo[s]))
    assert len(zo[sa]) >= 2
    exp4 = np.full(224, 1000, np.int64)
    exp4[:20], exp4[20:40] = 4, 5  # (overdue from now == 5 on; not overdue at now == 5)
    want = run.tick(requests(ls, 224, exp4, 5, **report([(sa, zo[sa])])))    # now 4: ids 900 .. 1123, sa's zombies stamped
    assert all_granted(want) and want["swept"] == 0 and len(T) == 1024 and T.next_id == 1124
    late = {t: T.L[t][0] for t in range(900, 920)}
    blob = run.fork()
    p = snapshot.parse(blob)
    assert len(p["l_id"]) == 1024 and p["l_zombie"].sum() == 90 and p["lease_tick"] == 5 and p["last_now"] == 4
    assert set(p["l_stamp"][np.isin(p["l_id"], zo[sa])].tolist()) == {5}, "the report stamps are not in the blob"
    assert len(blob) == 216 + snapshot._pad8(40 * 8 + 40 * 32) + 1024 * 24
    a, b = run.ctxs
    before = b.stream_leases()
    late_servants = sorted(set(late.values()) - {sa})
    want = run.tick(requests(ls, 0, 0, 6, **report([(sa, zo[sa][1:])] + [(s, []) for s in late_servants])))  # now 5
    # (sa's report names neither its first zombie nor what just ran out on it; the others name nothing)
    assert want["expired"] == 20 and want["swept"] == 1 + 20 + sum(len(zo.get(s, [])) for s in late_servants)
    assert zo[sa][0] not in T.L and all(t in T.L for t in zo[sa][1:]) and all(t in T.L for t in range(920, 940))
    assert not any(T.L[t][2] for t in range(920, 940)), "a lease with expires_at == now is not overdue"
    # Every id the blob held: the live ones renew, the zombies refuse; then each is freed.
    old = [t for t in before[0].tolist() if t in T.L]
    zombie = np.array([T.L[t][2] for t in old])
    want = run.tick(requests(ls, 0, 0, 7, renew_ids=np.array(old, np.uint64),
                             renew_expires_at=np.full(len(old), 7000, np.int64)))                            # now 6
    assert np.array_equal(want["renewed"], (~zombie).astype(np.uint8)) and want["renew_refused"] == zombie.sum() > 0
    held = np.bincount([T.L[t][0] for t in old], minlength=40)
    run_before = b.get_running().astype(np.int64)
    want = run.tick(requests(ls, 0, 0, 8, free_ids=np.array(old, np.uint64)))                              # now 7
    assert want["freed"] == len(old) and want["n_leases"] == 0
    assert np.array_equal(run_before - b.get_running(), held)
    assert all_granted(run.tick(requests(ls, 300, 1000, 9)))  # ids go on from 1124
    assert min(T.L) == 1124
    run.end()


@pytest.mark.parametrize("n_leases", [0, 1, 63, 65, 1000])
def test_ragged_ends_of_the_load_and_an_empty_table(n_leases):
    """|L| of 0 (snapshotted before the first tick: no clock, tick number 0), 1, 63, 65 and 1000:
    k_lease_load's last wave and workgroup partly filled. A is destroyed before B ticks."""
    sv = roomy_pool(30, 40)
    ls = L.LeaseStream(sv, 500, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 3
    run = leased_run(sv, ls, dict(tasks=500, leases=2000, renewals=1024, frees=1024, reports=30, report_ids=2048))
    left, seed = n_leases, 1
    while left:
        k = min(left, 500)
        assert all_granted(run.tick(requests(ls, k, 50 + np.arange(k), seed)))
        left, seed = left - k, seed + 1
    blob = run.fork(drop_a=True)
    p = snapshot.parse(blob)
    assert len(p["l_id"]) == n_leases and p["next_id"] == n_leases and p["lease_tick"] == run.t
    assert p["last_now"] == (snapshot.I64_MIN if n_leases == 0 else run.t - 1)
    ids = np.arange(n_leases, dtype=np.uint64)
    want = run.tick(requests(ls, 40, 1000, 7, renew_ids=ids, renew_expires_at=np.full(n_leases, 900, np.int64)))
    assert all_granted(want) and want["renewed"].all() and list(want["task_id"]) == list(range(n_leases, n_leases + 40))
    want = run.tick(requests(ls, 0, 0, 8, free_ids=ids[::2]))
    assert want["freed"] == (n_leases + 1) // 2
    run.drive(2)
    run.end()


def wait_leased_run(ws, tasks, waiting, leases):
    ctx = new_ctx(ws.es.sv)
    ctx.stream_begin_waiting_leased(ws.es.hb + 8, 16, tasks, waiting, leases, 16, 64, ws.es.n, 64)
    return Run("wait_leased", ws, ctx)


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_queue_with_leases(stream_graph, monkeypatch):
    """Three servants with few slots; W holds entries with distinct deadlines, tags and lease
    durations. First tick after the restore: some deadlines lapse, slots come back and the queue's
    front is granted — its ids in front of the new requests', its leases of its own durations from
    the granting tick. With the captured step and with the step enqueued kernel by kernel."""
    reserve._graph(monkeypatch, stream_graph)
    sv = wcases.small_stream().es.sv
    ws = WM.new_stream(sv, 48, 0, 0, 64, n_envs=1, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    run = wait_leased_run(ws, 48, 64, 256)
    S = ws.state
    k = np.arange(48)
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=48, lease_for=20 + 3 * k, wait=2 + k % 5))   # now 0
    assert want["n_waiting"] >= 8 and int((want["out"] < WM.IDX_WAITING).sum()) >= 8
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=10, lease_for=7 + np.arange(10), wait=3))   # now 1
    n_w = want["n_waiting"]
    assert n_w >= 18 and int((S.q.deadline == 2).sum()) >= 1 and len(set(S.lease_for.tolist())) > 8
    blob = run.fork()
    p = snapshot.parse(blob)
    assert len(p["w_tag"]) == n_w and p["waiting"] and p["leased"] and not p["rpc"]
    first = S.T.next_id
    held = sorted(S.T.L)[:6]
    front_for = S.lease_for[S.q.deadline > 2][:6].copy()
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=5, lease_for=9, wait=2, free=held))         # now 2
    gw = want["res_idx"] < WM.IDX_ENV_NOT_FOUND
    assert want["w_expired"] >= 1 and gw.sum() == 6 and list(want["res_ids"][gw]) == list(range(first, first + 6))
    assert [S.T.L[t][1] for t in range(first, first + 6)] == (2 + front_for).tolist()
    new_ids = want["task_id"][want["out"] < WM.IDX_WAITING]
    assert (new_ids >= first + 6).all()
    rec = [run.tick(wcases.scripted(ws, ws.next_tick(), n=0)) for _ in range(5)]                     # now 3 .. 7
    assert sum(r["w_expired"] for r in rec) > 0 and rec[-1]["n_waiting"] == 0
    run.end()


def test_waiting_queue_without_leases():
    """A stream begun with ydc_stream_begin_waiting: W alone (requests, deadlines, tags) and the clock.
    A is destroyed; B goes on against the model of tests/stream_wait_model.py, and a tick before the
    carried clock is refused."""
    from tests import stream_wait_model as QM
    from tests import test_stream_waiting_gpu as waiting
    sv = synth.make_servants(20, n_tasks_hint=300, n_envs=2, seed=42)
    ws, q = QM.WaitingStream(sv, 200, 40, 600, n_envs=2), QM.WaitQueue(600)
    a = waiting.begin(ws.es, 600, 40, 200)
    waiting.drive(a, ws, q, 5)
    assert 0 < len(q) == ws.n_waiting
    blob = a.stream_snapshot()
    p = snapshot.parse(blob)
    assert p["waiting"] and not p["leased"] and p["last_now"] == 4 and p["next_id"] == 0 and p["lease_tick"] == 0
    for k, v in (("w_tag", q.tag), ("w_deadline", q.deadline), ("w_env_id", q.cols["env_id"]),
                 ("w_min_version", q.cols["min_version"]), ("w_requestor_ip", q.cols["requestor_ip"]),
                 ("running_tasks", ws.es.running.astype(np.uint32)), ("current_load", ws.es.sv["current_load"])):
        assert np.array_equal(p[k], v), k
    b = binding.Context(device=0)
    assert b.stream_restore(blob) == a.stream_caps()
    a.stream_end()
    a.close()
    none = np.empty(0, np.uint32)
    with pytest.raises(binding.YdcError, match="before the previous"):
        b.stream_tick_waiting(none, np.empty(0, binding.ROW_DTYPE), none,
                              {"env_id": none, "min_version": none, "requestor_ip": none}, np.empty(0, np.int64),
                              np.empty(0, np.uint64), 3)
    waiting.drive(b, ws, q, 6)
    assert np.array_equal(b.stream_waiting_take(), q.take())
    b.stream_end()
    b.close()


def rpc_run(ws, requests_, max_leases=4096):
    ctx = new_ctx(ws.es.sv)
    ctx.stream_begin_rpc(ws.es.hb + 8, 16, requests_, ws.state.max_rows, ws.state.max_waiting, max_leases, 16, 64,
                         ws.es.n, 64)
    return Run("rpc", ws, ctx)


def test_rpc_rows_of_the_queue_are_carried():
    """Blocked RPCs of 1 .. 5 rows in W; rows(W) is what it was; straight after the restore four slots
    come back: the front RPC is granted in full, the next one in part."""
    ws = rcases.small_stream(max_rows=3000, max_waiting=64)
    run = rpc_run(ws, 24)
    state = ws.state
    shapes = [(1, 2), (3, 0), (0, 2), (2, 3), (1, 0), (4, 1), (0, 1)]
    want = run.tick(rcases.scripted(ws, ws.next_tick(), rpcs=[(200, 100, 30, 5)] +
                                    [(a, b, 10 + a, 20 + b) for a, b in shapes]))                      # now 0
    assert want["status"][0] == 0 and want["n_waiting"] == 7
    rows_w = want["n_waiting_rows"]
    assert rows_w == sum(a + b for a, b in shapes) and sorted(a + b for a, b in shapes) == [1, 1, 2, 3, 3, 5, 5]
    blob = run.fork()
    p = snapshot.parse(blob)
    assert p["rpc"] and p["n_wait_rows"] == rows_w and list(p["w_n_immediate"]) == [a for a, _ in shapes]
    held = sorted(state.T.L)[:4]
    want = run.tick(rcases.scripted(ws, ws.next_tick(), rpcs=[(1, 1, 7, 15)] * 3, free=held))           # now 1
    assert len(want["res_servants"]) == 4 and want["partial"] >= 1 and list(want["res_n_granted"][:2]) == [3, 1]
    assert want["n_waiting_rows"] == rows_w - 6 + 6
    rec = [run.tick(rcases.scripted(ws, ws.next_tick(), free=sorted(state.T.L)[:5])) for _ in range(4)]
    assert sum(len(r["res_servants"]) for r in rec) >= 10
    run.end()


def alive_rpc_run(max_book=6000):
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    ws, ctx = alive.begun("rpc", sv)
    ctx.stream_book_begin(max_book)
    book = BM.Book(max_book)
    expires = np.full(70, alive.FAR, np.int64)
    A = AM.attach(ws, expires, book)
    ctx.stream_alive_begin(expires)
    return Run("rpc", ws, ctx, A=A, book=book)


def test_book_and_aliveness_on_an_rpc_stream():
    """E holds a servant that expires in the first tick after the restore and one whose expiry is that
    tick's clock itself (not due). The removal route fires from the carried alive_bound: the due
    servant's book entries and leases go (the leases as orphans), ydc_stream_alive_removed on B equals
    A's, and the servant at the boundary stays."""
    run = alive_rpc_run()
    ws, A, a = run.ws, run.A, run.ctxs[0]
    gen = AM.AliveGen(ws, life=alive.FAR, p_stop=0, p_short=0)
    run.drive(5, gen)
    now = int(ws.es.tick_no)
    beat_next = set(((ws.es.hb_pos + np.arange(ws.es.hb)) % ws.es.n).tolist())
    booked = {e[0] for e in run.book.B}
    leased = {e[0] for e in ws.table.L.values()}
    quiet = sorted((booked & leased) - beat_next)
    assert len(quiet) >= 2, "no servant with book entries and leases that keeps quiet in the next tick"
    s_due, s_edge = quiet[0], quiet[1]
    A.expires[s_due], A.expires[s_edge] = now - 1, now
    A.bound = int(A.expires.min())
    a.stream_alive_begin(A.expires)
    blob = run.fork()
    p = snapshot.parse(blob)
    assert p["book"] and p["alive"] and p["alive_bound"] == now - 1 and len(p["b_servant"]) == len(run.book.B) > 0
    b = run.ctxs[1]
    assert b.debug_alive()[0] == now - 1
    n_book = len(run.book.B)
    lost = sum(1 for e in run.book.B if e[0] == s_due)
    r = run.tick(gen.next_tick())
    assert list(r["removed"]) == [s_due] and r["orphans"] > 0 and r["alarm"]
    assert lost > 0 and n_book > lost and ws.es.n == 69
    assert b.debug_alive()[2] == 1, "B's removal route did not fire"
    run.drive(4, gen)
    run.end()


def test_host_aliases_and_wide_masks():
    """An alias pair decides a self-avoidance after the restore (the model does not know the alias: it
    follows A's placement, and B must place exactly as A does); and a registry of 70 digests
    (env_words == 2), whose heartbeats carry their masks."""
    sv = roomy_pool(6, 8)
    ls = L.LeaseStream(sv, 4, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 2
    run = leased_run(sv, ls, dict(tasks=8, leases=64, renewals=16, frees=16, reports=6, report_ids=64))
    a = run.ctxs[0]
    alias_ip = (192 << 24) + 77
    z = np.zeros(4, np.uint32)
    ask = {"env_id": z, "min_version": z, "requestor_ip": z + np.uint32(alias_ip)}
    last = []

    def placed_on():
        ev = lease.quiet(ls.next_tick(), tasks=ask, release_idx=np.empty(0, np.uint32),
                         lease_expires_at=np.full(4, 1000, np.int64), free_ids=np.array(last, np.uint64))
        got = [lease.gpu_tick(c, ls, ev) for c in run.ctxs]
        out, ids = got[0][:2]
        held = set(ls.table.L)
        # (the lease model does not know the alias; the placement it is handed must equal the
        # reference's on address strings)
        r = ls.table.tick(ls.es.running, ev, lambda batch: alive.alias_checked(ls.es, batch, out, aliased))
        ls.commit(held, r["out"])
        run.t += 1
        assert np.array_equal(ids, r["task_id"]) and int((out < L.IDX_ENV_NOT_FOUND).sum()) == 4
        for c in run.ctxs:
            assert np.array_equal(c.get_running(), ls.es.running.astype(np.uint32))
        if len(got) == 2:
            same_outputs(run.t, "leased", *got)
            same_state(run.t, *run.ctxs)
        last[:] = ids.tolist()
        return out.tolist()

    aliased = {}
    target = max(placed_on())  # where such requests go when nothing keeps them away
    a.set_host_aliases(np.array([alias_ip], np.uint32), np.array([target], np.uint32))
    aliased[alias_ip] = {target}
    run.aliases = ([alias_ip], [target])
    assert target not in placed_on(), "the alias does not keep its servant's own requests away"
    blob = run.fork()
    assert list(snapshot.parse(blob)["alias_servant"]) == [target]
    for _ in range(2):
        assert target not in placed_on(), "the alias did not survive the restore"
    run.ctxs[1].set_host_aliases(np.empty(0, np.uint32), np.empty(0, np.uint32))
    out_b = lease.gpu_tick(run.ctxs[1], ls, lease.quiet(ls.next_tick(), tasks=ask, release_idx=np.empty(0, np.uint32),
                                                        lease_expires_at=np.full(4, 1000, np.int64),
                                                        free_ids=np.array(last, np.uint64)))[0]
    assert target in out_b.tolist()  # (without the entry the same requests do reach it)
    for c in run.ctxs:
        c.stream_end()
        c.close()
    # env_words == 2
    n_envs = 70
    sv = synth.make_servants(40, n_tasks_hint=2000, n_envs=n_envs, seed=31)
    ls = L.LeaseStream(sv, 300, 150, 40, L.LeaseTable(), n_envs=n_envs)
    run = leased_run(sv, ls, dict(tasks=300, leases=4096, renewals=4096, frees=8192, reports=ls.n_rep, report_ids=1 << 15),
                     masks=True)
    run.drive(5)
    blob = run.fork()
    assert snapshot.parse(blob)["env_words"] == 2
    rec = run.drive(6)
    assert sum(r["expired"] for r in rec) and sum(r["freed"] for r in rec)
    run.end()


def test_more_than_256_classes_runs_eagerly():
    """~600 servant classes: every tick is enqueued instead of replayed (eager_only), before and after
    the restore."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=3000, n_envs=n_envs, seed=23)
    ls = L.LeaseStream(sv, 300, 150, 40, L.LeaseTable(), n_envs=n_envs)
    run = leased_run(sv, ls, dict(tasks=300, leases=4096, renewals=4096, frees=8192, reports=ls.n_rep, report_ids=1 << 15),
                     masks=True)
    run.drive(3)
    run.fork()
    rec = run.drive(4)
    assert sum(r["expired"] for r in rec) and len(ls.table) > 0
    run.end()


def test_larger_bounds_and_a_reserve_after_the_restore():
    """Restored with a want that doubles max_leases and max_waiting: a tick the blob's own bounds would
    refuse is taken. Restored as it is, then grown with ydc_stream_reserve: the same."""
    sv = wcases.small_stream().es.sv
    ws = WM.new_stream(sv, 48, 0, 0, 96, n_envs=1, max_leases=256, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    run = wait_leased_run(ws, 48, 48, 128)
    k = np.arange(48)
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=48, lease_for=20 + k, wait=6 + k % 5))      # now 0
    assert want["n_waiting"] >= 8
    a = run.ctxs[0]
    blob = a.stream_snapshot()
    small = a.stream_caps()
    assert (small["max_waiting"], small["max_leases"]) == (48, 128)
    b, c = binding.Context(device=0), binding.Context(device=0)
    caps = b.stream_restore(blob, max_leases=256, max_waiting=96)
    assert caps == dict(small, max_leases=256, max_waiting=96)
    assert c.stream_restore(blob) == small
    ev = wcases.scripted(ws, ws.next_tick(), n=48, lease_for=50 + k, wait=4 + k % 3)                 # now 1
    for ctx in (a, c):
        with pytest.raises(binding.YdcError, match="max_waiting"):
            wl.gpu_tick(ctx, ws, ev)
    assert c.stream_reserve(max_leases=256, max_waiting=96) == caps
    # (blobs of the same state and bounds are the same bytes, restored or reserved)
    assert b.stream_snapshot() == c.stream_snapshot() != blob
    a.stream_end()
    a.close()
    run.ctxs = [b, c]
    want = run.tick(ev)
    assert want["n_waiting"] > 48
    held = sorted(ws.state.T.L)[:6]
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=0, free=held))                              # now 2
    assert want["w_granted"] == 6
    rec = [run.tick(wcases.scripted(ws, ws.next_tick(), n=0)) for _ in range(9)]
    assert rec[-1]["n_waiting"] == 0
    run.end()
    # A want that names a part the blob's mode lacks.
    d = binding.Context(device=0)
    for bad in (dict(max_rows=100),):
        with pytest.raises(binding.YdcError, match=INVALID):
            d.stream_restore(blob, **bad)
    d.close()


def test_format_round_trips_and_grown_twin():
    """Snapshot, restore, snapshot: the same bytes. A stream begun large and its twin begun small and
    grown by ydc_stream_reserve (another table size, other slots): the same bytes."""
    sv = synth.make_servants(80, n_tasks_hint=3000, n_envs=2, seed=11)
    ls = L.LeaseStream(sv, 500, 300, 80, L.LeaseTable(), n_envs=2)
    big = dict(tasks=500, leases=1 << 15, renewals=4096, frees=8192, reports=ls.n_rep, report_ids=1 << 15)
    tw = reserve.leased_twin(sv, ls, dict(big, leases=2500), big)
    tw.drive(4)
    tw.b.stream_reserve(max_leases=1 << 15)
    tw.drive(3)
    assert sum(1 for e in ls.table.L.values() if e[2]) > 0 and len(ls.table) > 500
    blob_a, blob_b = tw.a.stream_snapshot(), tw.b.stream_snapshot()
    assert blob_a == blob_b, "the blob depends on the table's history"
    c = binding.Context(device=0)
    c.stream_restore(blob_a)
    assert c.stream_snapshot() == blob_a, "snapshot, restore, snapshot changed the bytes"
    assert tw.a.stream_snapshot() == blob_a, "a snapshot changed the stream"
    c.stream_end()
    c.close()
    tw.drive(2)
    tw.end()


def test_a_blob_built_from_the_model_with_ids_beyond_2_to_the_40():
    """The model alone runs a leased stream whose ids start at 2^40; snapshot.build makes the blob from
    its state (no C writer involved); a fresh context restored from it matches the model from then on."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=5)
    ls = L.LeaseStream(sv, 300, 150, 40, L.LeaseTable(), n_envs=2)
    ls.table.next_id = 1 << 40
    rec = [L.model_tick(ls, ls.next_tick()) for _ in range(5)]
    assert sum(r["expired"] for r in rec) and len(ls.table) > 100 and min(ls.table.L) >= 1 << 40
    caps = dict(max_updates=ls.es.hb + 8, max_releases=16, max_tasks=300, max_leases=4096, max_renewals=4096,
                max_frees=8192, max_reports=ls.n_rep, max_report_ids=1 << 15)
    blob = snapshot.build(SM.state_of("leased", ls, caps, 5))
    ctx = binding.Context(device=0)
    assert ctx.stream_restore(blob) == dict(caps, max_rows=0, max_waiting=0)
    assert ctx.stream_snapshot() == blob, "the C writer and snapshot.build disagree"
    run = Run("leased", ls, ctx)
    run.t = 5
    rec = run.drive(6)
    assert sum(r["swept"] for r in rec) and sum(r["freed"] for r in rec) and max(ls.table.L) > (1 << 40) + 500
    run.end()


def corrupt(blob, at, value=None, fix=False):
    """`blob` with the byte at `at` flipped (or the u32 there set to value); fix: checksum made right."""
    b = bytearray(blob)
    if value is None:
        b[at] ^= 0x40
    else:
        b[at:at + 4] = int(value).to_bytes(4, "little")
    if fix:
        b[24:32] = snapshot.checksum(bytes(b)).to_bytes(8, "little")
    return bytes(b)


def test_refusals_leave_the_open_stream_ticking():
    sv = roomy_pool(6, 8)
    ls = L.LeaseStream(sv, 12, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 2
    run = leased_run(sv, ls, dict(tasks=12, leases=64, renewals=16, frees=16, reports=6, report_ids=64))
    run.tick(requests(ls, 12, 50, 1))
    run.tick(requests(ls, 12, 50, 2))
    ctx = run.ctxs[0]
    blob = ctx.stream_snapshot()
    p = snapshot.parse(blob)
    l_off = snapshot.HEADER.unpack_from(blob)[30]
    srv_off = l_off + 24 * 16  # (ids and expiries, 24 leases of 8 + 8 bytes, then the servants)
    assert len(p["l_id"]) == 24 and int.from_bytes(blob[l_off + 8:l_off + 16], "little") == 1
    swapped = bytearray(blob)
    swapped[l_off:l_off + 8], swapped[l_off + 8:l_off + 16] = blob[l_off + 8:l_off + 16], blob[l_off:l_off + 8]
    swapped[24:32] = snapshot.checksum(bytes(swapped)).to_bytes(8, "little")
    bad = {
        "cut at the header": blob[:100],
        "cut inside a section": blob[:l_off + 40],
        "one byte short": blob[:-1],
        "a flipped byte in the header": corrupt(blob, 40),
        "a flipped byte in L": corrupt(blob, l_off + 3),
        "ids not ascending": bytes(swapped),
        "a servant index >= n_servants": corrupt(blob, srv_off, 6, fix=True),
        "an unknown format version": corrupt(blob, 8, 2, fix=True),
    }
    for name, bytes_ in bad.items():
        with pytest.raises(snapshot.FormatError):
            snapshot.parse(bytes_)
        state = ctx.stream_leases(), ctx.get_running(), ctx.stream_caps()
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_restore(bytes_)
        after = ctx.stream_leases(), ctx.get_running(), ctx.stream_caps()
        assert state[2] == after[2], name
        for x, y in zip(state[0] + (state[1],), after[0] + (after[1],)):
            assert np.array_equal(x, y), "%s: the refused restore changed the stream" % name
    run.tick(requests(ls, 6, 50, 3))
    # More servants than the context was created for.
    tight = binding.Context(device=0, max_servants=5)
    with pytest.raises(binding.YdcError, match=CAPACITY):
        tight.stream_restore(blob)
    tight.close()
    # cap too small: the size needed, nothing written; the second call succeeds.
    cur = ctx.stream_snapshot()
    size = len(cur)
    need = binding.C.c_size_t(0)
    buf = binding.C.create_string_buffer(b"\xAA" * size, size)
    rc = binding.lib().ydc_stream_snapshot(ctx._h, buf, binding.C.c_size_t(size - 1), binding.C.byref(need))
    assert rc == -4 and need.value == size == len(blob) + 6 * 24 and buf.raw == b"\xAA" * size
    rc = binding.lib().ydc_stream_snapshot(ctx._h, buf, binding.C.c_size_t(size), binding.C.byref(need))
    assert rc == 0 and need.value == size and buf.raw == cur and snapshot.parse(cur)["lease_tick"] == 3
    # A pending staging: a snapshot is taken between ticks.
    ctx.stream_book_begin(64)
    ctx.stream_book_stage(np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    with pytest.raises(binding.YdcError, match="staging"):
        ctx.stream_snapshot()
    run.book = BM.Book(64)
    run.tick(requests(ls, 6, 50, 4))  # (consumes the staging)
    assert snapshot.parse(ctx.stream_snapshot())["book"]
    ctx.stream_alive_begin(None, n=6)
    ctx.stream_alive_stage(np.zeros(0, np.int64))
    with pytest.raises(binding.YdcError, match="staging"):
        ctx.stream_snapshot()
    ctx.stream_end()
    # No stream; a plain stream, which goes on afterwards.
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_snapshot()
    ctx.stream_begin(8, 8, 12)
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_snapshot()
    out = ctx.stream_tick(np.empty(0, np.uint32), np.empty(0, binding.ROW_DTYPE), np.empty(0, np.uint32),
                          synth.make_tasks(4, sv, n_envs=1, seed=1, self_frac=0.0))
    assert len(out) == 4
    ctx.stream_end()
    ctx.close()

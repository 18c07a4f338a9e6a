"""Leased streaming ticks at the edges the seeded streams of tests/test_stream_lease_gpu.py only
meet by chance, or never: the hand-written same-tick interactions of tests/stream_lease_cases.py
(pinned against the verbatim reference class by tests/test_stream_lease_model.py), a table filled
to exactly max_leases, max_leases below the table's floor of 1024 slots, and ydc_remove_servants
at that load. Every tick is compared with the model on every output, running_tasks, the tick's
counts and the lease snapshot (check_tick). The last tests take a tick out of the captured step
through the "captured passes ran out" exit, in all three streaming modes."""
import numpy as np
import pytest

from tests import stream_lease_cases as cases
from oracle import oraclebind as O
from tests import cases as pools
from tests import stream_lease_model as M
from tests import stream_wait_model as WM
from tests import test_stream_waiting_gpu as waiting
from tests.test_stream_lease_gpu import begin, check_tick, drop_rows, gpu_tick
from yadcc_amd import binding, pack, streaming, synth

pytestmark = pytest.mark.gpu


class Hand:
    """Hand-written ticks on a leased context, each checked against the model. Every servant may
    report in one tick."""

    def __init__(self, ls, max_leases, tasks):
        self.ls, self.t = ls, 0
        self.ctx = binding.Context(device=0)
        self.ctx.upload_servants(pack.to_abi_columns(ls.es.sv))
        self.ctx.stream_begin_leased(ls.es.hb + 8, 16, tasks, max_leases, 1024, 1024, ls.es.n, 4096)

    def tick(self, ev):
        want = M.model_tick(self.ls, ev)
        check_tick(self.t, self.ctx, self.ls, gpu_tick(self.ctx, self.ls, ev), want)
        self.t += 1
        return want

    def __call__(self, **kw):
        return self.tick(cases.scripted(self.ls, self.ls.next_tick(), **kw))

    def refused(self, n):
        """A tick with n requests too many: refused by the model and by the library; the same
        heartbeats then go out with a tick that asks for nothing."""
        ev = self.ls.next_tick()
        with pytest.raises(OverflowError):
            M.model_tick(self.ls, cases.scripted(self.ls, ev, n=n, lease=[99] * n))
        with pytest.raises(binding.YdcError, match="max_leases"):
            gpu_tick(self.ctx, self.ls, cases.scripted(self.ls, ev, n=n, lease=[99] * n))
        self.tick(cases.scripted(self.ls, ev))

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


@pytest.mark.parametrize("case", cases.CASES, ids=[c.__name__ for c in cases.CASES])
def test_hand_written_same_tick_interactions(case):
    """tests/stream_lease_cases.py on the device: what the kernels settle by launch order and
    atomics (ren_win bids, the CAS on the key, the stamp written before the sweep reads it). Each
    step asserts on the model's record that its situation occurred."""
    ls = cases.small_stream(64)
    h = Hand(ls, 64, cases.MAX_TASKS)
    cases.play(ls, case(), h.tick)
    assert h.t == len(case())
    h.close()


def _fill(h, T, upto, per_tick, lease):
    for _ in range(8):
        n = min(per_tick, upto - len(T))
        if n == 0:
            break
        r = h(n=n, lease=[lease(i) for i in range(n)])
        assert not (r["out"] >= M.IDX_ENV_NOT_FOUND).any(), "the pool is too small for this test"
    assert len(T) == upto


def _look_everything_up(h, T):
    """Every lease by renewal (out of order, with an unknown id between) and by its servant's report."""
    ids = sorted(T.L, key=lambda t: (t * 7919) % 1009)
    r = h(renew=[(t, 5000 + t) for t in ids[:500]] + [(T.next_id + 3, 1)] + [(t, 5000 + t) for t in ids[500:]])
    assert int(r["renewed"].sum()) == len(ids) and r["renew_refused"] == 1
    r = h(reports=cases.every_servant_lists_everything(T))
    assert len(r["report_unknown"]) == len(ids) and not r["report_unknown"].any() and r["swept"] == 0


def test_table_filled_to_exactly_max_leases():
    """max_leases 512: 1024 slots, exactly half of them taken. One more request is refused; every
    other id is freed and the gaps are granted again (new ids, probing past live neighbours at the
    highest load the table allows); every lease is then found by renewal and by report."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=1, seed=5)
    ls = M.LeaseStream(sv, 256, 0, 0, M.LeaseTable(512), n_envs=1)
    T = ls.table
    h = Hand(ls, 512, 256)
    _fill(h, T, 512, 200, lambda i: 5000)
    h.refused(1)
    r = h(free=list(range(0, 512, 2)))
    assert r["freed"] == 256 and r["n_leases"] == 256
    _fill(h, T, 512, 256, lambda i: 5000 + i)
    assert T.next_id == 768 and sorted(T.L)[:2] == [1, 3]
    h.refused(1)
    _look_everything_up(h, T)
    h.close()


@pytest.mark.parametrize("max_leases", [1, 3])
def test_max_leases_below_the_floor_of_the_table(max_leases):
    """The table has 1024 slots whatever is asked; the bound that refuses is max_leases itself."""
    ls = cases.small_stream(max_leases)
    T = ls.table
    h = Hand(ls, max_leases, cases.MAX_TASKS)
    for n in (max_leases - 1, 1):
        if n:
            r = h(n=n, lease=[100] * n)
            assert int((r["out"] < M.IDX_ENV_NOT_FOUND).sum()) == n
    assert len(T) == max_leases
    h.refused(1)
    mid = sorted(T.L)[max_leases // 2]
    r = h(free=[mid])
    assert r["freed"] == 1 and len(T) == max_leases - 1
    h.refused(2)
    r = h(n=1, lease=[100])
    assert list(r["task_id"]) == [max_leases] and len(T) == max_leases
    h.refused(1)
    _look_everything_up(h, T)
    h.close()


def test_remove_servants_at_a_full_table():
    """ydc_remove_servants with the table at exactly max_leases = 512 (1024 slots): the leases of
    three removed rows vanish, the others follow the compaction; the next ticks free, renew and
    report under the new row numbers, sweep the zombies (half the leases expire meanwhile; the
    listed ones one tick later) and grant the table full again."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=1, seed=5)
    ls = M.LeaseStream(sv, 256, 0, 0, M.LeaseTable(512), n_envs=1)
    T = ls.table
    h = Hand(ls, 512, 256)
    _fill(h, T, 512, 200, lambda i: 5 if i % 2 else 5000)
    holders = sorted(cases.held(T))
    assert len(holders) >= 8
    removed = np.array(holders[1:8:3], np.uint32)
    assert sum(1 for e in T.L.values() if e[0] in removed) and sum(1 for e in T.L.values() if e[0] > removed[-1])
    h.ctx.remove_servants(removed)
    drop_rows(ls, removed)
    assert 0 < len(T) < 512
    for name, a, b in zip(("ids", "servants", "expires_at", "zombie"), h.ctx.stream_leases(), T.snapshot()):
        assert np.array_equal(a, b), name
    assert np.array_equal(h.ctx.get_running(), ls.es.running.astype(np.uint32))
    while ls.es.tick_no < 6:
        h()
    of = cases.held(T)
    r = h(free=[ids[0] for ids in of.values()],
          reports=[(s, ids[:1] + ids[1::2]) for s, ids in of.items()])  # (the freed one is listed)
    assert r["expired"] > 100 and r["swept"] > 50 and r["freed"] == len(of) and r["unknown_reported"] > len(of)
    assert r["kept_zombies"] == 0 and any(e[2] for e in T.L.values())  # (the listed zombies stay)
    r = h(reports=[(s, []) for s in cases.held(T)])
    assert r["swept"] > 50 and not any(e[2] for e in T.L.values())
    _fill(h, T, 512, 256, lambda i: 5000)
    h.refused(1)
    _look_everything_up(h, T)
    h.close()


# A fresh context captures max(2, min(round_hint + 1, 12)) = 4 matching passes (round_hint starts
# at 3). A tick that needs more leaves the captured step: the host runs further passes, answers
# from the arena in place, and captures min(rounds + 1, 12) passes for the next tick.
FIRST_CAPTURE = 4


def _huge_servants():
    """Five servants with tens of thousands of slots each, one per class, a tenth of the requests
    from their own hosts: every chunk's start state has holes, about one pass per chunk
    (tests/test_gpu_parity.py: test_tiny_pool_with_huge_servants_and_own_host_traffic)."""
    sv, _ = pools.random_case(seed=2009, n_tasks=150_000, n_servants=5, n_envs=3, self_frac=0.1,
                              unknown_env_frac=0.01, initial_running=True)
    return sv


class Exits:
    """Which ticks left through the exit, from ydc_stats::rounds against the passes captured."""

    def __init__(self):
        self.captured, self.taken, self.rounds = FIRST_CAPTURE, [], []

    def note(self, t, ctx):
        r = ctx.stats()["rounds"]
        self.rounds.append(r)
        if r > self.captured:
            self.taken.append(t)
            self.captured = min(r + 1, 12)


def test_captured_passes_run_out_in_a_plain_tick():
    """The tick's registry deltas are applied by the captured step; the host finishes the passes
    and copies the placement; the next tick runs from a longer captured step."""
    es = streaming.EventStream(_huge_servants(), 150_000, 100_000, n_envs=3)
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(es.sv))
    ctx.stream_begin(es.hb + 8, 100_000, 150_000)
    ex = Exits()
    for t in range(4):
        who, rows, rel, tk = es.next_tick()
        want, _, wrun = O.dispatch(es.registry_snapshot(), tk, "sorted")
        got = ctx.stream_tick(who, rows, rel, tk)
        assert np.array_equal(got, want), t
        es.commit(got)
        assert np.array_equal(ctx.get_running(), wrun), t
        ex.note(t, ctx)
    print("plain: rounds per tick", ex.rounds, "exit taken in ticks", ex.taken)
    assert ex.taken and ex.taken[0] < 3, ex.rounds  # (and at least one tick follows the exit)
    ctx.stream_end()
    ctx.close()


def test_captured_passes_run_out_in_a_waiting_tick():
    """... with a queue: the gated k_wait_compact left W as the gather read it, and the ungated
    one behind the host's passes reads the clock from the arena in place."""
    mw = 300_000
    ws = WM.WaitingStream(_huge_servants(), 150_000, 100_000, mw, n_envs=3)
    q = WM.WaitQueue(mw)
    ctx = waiting.begin(ws.es, mw, 100_000, 150_000)
    ex, queued = Exits(), []
    for t in range(5):
        queued.append(len(q))
        tick = ws.next_tick()
        now, who, rows, rel, tk, dl, tags = tick
        want = q.tick(WM.oracle_place(ws.es), tk, dl, tags, now)
        got = ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, now)
        waiting.check_tick(t, ctx, ws, q, tick, got, want)
        ex.note(t, ctx)
    print("waiting: rounds per tick", ex.rounds, "exit taken in ticks", ex.taken, "|W| before", queued)
    # (with a queue in front of it, and at least one tick behind it)
    assert any(queued[t] > 1000 and t < 4 for t in ex.taken), (ex.rounds, ex.taken, queued)
    ctx.stream_end()
    ctx.close()


def test_captured_passes_run_out_in_a_leased_tick():
    """... with leases: the captured step has applied the tick's renewals, frees by id, report
    stamps and the sweep; its gated k_lease_grant touched neither the ticket nor next_id nor the
    counters; the ungated one behind the host's passes reads expiries and tick number from the
    arena in place and reports the counters of the launches before it."""
    ls = M.LeaseStream(_huge_servants(), 150_000, 100_000, 2000, M.LeaseTable(), n_envs=3, report_frac=0.5)
    ctx = begin(ls, 1 << 20, 150_000, frees=1 << 17, report_ids=1 << 19)
    ex, rec = Exits(), []
    for t in range(5):
        ev = ls.next_tick()
        want = M.model_tick(ls, ev)
        check_tick(t, ctx, ls, gpu_tick(ctx, ls, ev), want)
        ex.note(t, ctx)
        rec.append(dict(want, reported=len(ev["report_ids"])))
    print("leased: rounds per tick", ex.rounds, "exit taken in ticks", ex.taken,
          [(r["freed"], r["swept"], r["expired"]) for r in rec])
    busy = [t for t in ex.taken if rec[t]["freed"] and rec[t]["reported"] and rec[t]["expired"] and rec[t]["renewed"].sum()]
    assert busy and busy[0] < 4, (ex.rounds, ex.taken)  # (and at least one tick follows it)
    ctx.stream_end()
    ctx.close()

"""Leased-mode ticks written by hand: the same-tick interactions that a seeded stream only meets by
chance (one id renewed and freed, freed and reported, overdue in the very tick its servant
reports, ...). One list of cases, played three ways: through the model and through the verbatim
reference class (tests/test_stream_lease_model.py, which compares the two field by field), and on
the GPU against the model (tests/test_stream_lease_edges_gpu.py).

A case is a list of steps on a small pool. A step is (make, expect): make(T, now) -> the tick's
lease traffic, written from the table T as the previous ticks left it (which servant holds which
id is the placement's business, so the ids are looked up, not assumed); expect(r, T) asserts on the
tick's record and the table behind it what the case is about, so a case that no longer meets its
situation fails instead of passing idly. The clock is the tick number; the heartbeats are the
stream's, the requests are drawn here (a LeaseStream drops a tick's requests now and then).
"""
import numpy as np

from tests import stream_lease_model as M
from yadcc_amd import synth

NO_ID = M.NO_ID  # 2^64 - 1: never a task id, and the key of an empty slot of the device's table
MAX_TASKS = 8    # requests per tick at most (what a context is begun with)


def small_stream(max_leases=1 << 30):
    """12 idle servants, one digest; no drawn lease traffic."""
    sv = synth.make_servants(12, n_tasks_hint=600, n_envs=1, seed=17)
    return M.LeaseStream(sv, MAX_TASKS, 0, 0, M.LeaseTable(max_leases), n_envs=1)


def scripted(ls, ev, n=0, lease=(), renew=(), free=(), reports=()):
    """The drawn tick `ev` with its heartbeats kept and everything else written by hand: n requests
    with the expiries `lease`, renew: [(id, expires_at)], free: [id], reports: [(servant, [id])]."""
    assert len(lease) == n
    off = np.cumsum([0] + [len(ids) for _, ids in reports]).astype(np.uint32)
    e = dict(ev)
    e.update(tasks=synth.make_tasks(n, ls.es.sv, n_envs=1, seed=500 + int(ev["now"]), self_frac=0.0),
             release_idx=np.empty(0, np.uint32),
             lease_expires_at=np.array(lease, np.int64),
             renew_ids=np.array([r[0] for r in renew], np.uint64),
             renew_expires_at=np.array([r[1] for r in renew], np.int64),
             free_ids=np.array(free, np.uint64),
             report_servants=np.array([s for s, _ in reports], np.uint32), report_off=off,
             report_ids=np.array([t for _, ids in reports for t in ids], np.uint64))
    return e


def play(ls, steps, tick):
    """tick(ev) -> the tick's record (dict of M.FIELDS); it advances ls.table."""
    for make, expect in steps:
        ev = ls.next_tick()
        r = tick(scripted(ls, ev, **make(ls.table, int(ev["now"]))))
        if expect:
            expect(r, ls.table)


def held(T):
    """servant -> its ids, ascending; the servants in the order of their first id."""
    of = {}
    for t in sorted(T.L):
        of.setdefault(T.L[t][0], []).append(t)
    return of


def idle_servants(T, n=12):
    return [s for s in range(n) if s not in held(T)]


def grant(n, lease):
    """n requests, all granted (the pool is far from full), expiring at `lease` (one value or n)."""
    exp = list(lease) if isinstance(lease, (list, tuple)) else [lease] * n

    def expect(r, T):
        assert int((r["out"] < M.IDX_ENV_NOT_FOUND).sum()) == n, "the pool did not grant all %d" % n
        assert len(held(T)) >= 2, "every lease sits on one servant"
    return (lambda T, now: dict(n=n, lease=exp)), expect


def nothing():
    return (lambda T, now: {}), None


def every_servant_lists_everything(T):
    return [(s, ids) for s, ids in held(T).items()]


def renewed_and_freed():
    """KeepTaskAlive, then FreeTask of the same id in one tick: the renewal succeeds (renewed = 1),
    the free takes the lease and gives the slot back once. The winner's expiry is stored by the
    launch that also erases the lease: nothing of it may survive in the slot's next tenant."""
    def expect(r, T):
        assert list(r["renewed"]) == [1, 1] and r["freed"] == 1 and r["ignored_frees"] == 0
        assert 0 not in T.L and r["n_leases"] == 3 and int(r["running"].sum()) == 3

    def after(r, T):
        assert list(r["renewed"]) == [0] and r["ignored_frees"] == 1
        assert r["n_leases"] == 5 and int(r["running"].sum()) == 5 and T.next_id == 6
    return [grant(4, 100),
            (lambda T, now: dict(renew=[(0, 500), (1, 77)], free=[0]), expect),
            (lambda T, now: dict(n=2, lease=[9, 9], renew=[(0, 600)], free=[0]), after)]


def freed_and_reported():
    """Four leases turn zombie; then, in one tick, lease a is freed by id while its servant's report
    lists it, and lease b of another servant is freed while that servant reports without it: both
    answers say unknown where asked, nothing is swept a second time, each slot comes back once."""
    def make(T, now):
        of = held(T)
        (sa, ia), (sb, ib) = list(of.items())[:2]
        return dict(free=[ia[0], ib[0]], reports=[(sa, [ia[0]]), (sb, [])])

    def expect(r, T):
        assert list(r["report_unknown"]) == [1] and r["freed"] == 2
        # what the report sweeps besides: the other zombies of servant b, never the freed one
        assert r["n_leases"] == 2 - r["swept"] and int(r["running"].sum()) == r["n_leases"]

    def zombies(r, T):
        assert r["expired"] == 4 and r["kept_zombies"] == 4
    return [grant(4, 1), nothing(), ((lambda T, now: {}), zombies), (make, expect)]


def overdue_when_its_servant_reports():
    """Six leases expire at 2. At now == 2 they are not overdue and every servant's report finds
    them known. At now == 3 the first servant reports without listing its leases: expired and swept
    in that one tick. The second lists them: expired, kept, reported unknown. The others do not
    report: kept."""
    def at2(T, now):
        assert now == 2
        return dict(reports=every_servant_lists_everything(T))

    def known(r, T):
        assert r["expired"] == 0 and not r["report_unknown"].any() and len(r["report_unknown"]) == 6

    def at3(T, now):
        (sa, ia), (sb, ib) = list(held(T).items())[:2]
        return dict(reports=[(sa, []), (sb, ib)])

    def expect(r, T):
        assert r["expired"] == 6 and r["swept"] >= 1 and r["report_unknown"].all()
        assert r["n_leases"] == 6 - r["swept"] and int(r["running"].sum()) == r["n_leases"]
        assert all(e[2] for e in T.L.values())
    return [grant(6, 2), nothing(), (at2, known), (at3, expect)]


def overdue_but_renewed_in_time():
    """Leases overdue since the previous tick's clock that no timer has seen yet: the renewal in
    the tick in which lease 0 would expire arrives first, it stays live and its servant's report
    finds it known; the others become zombies."""
    def make(T, now):
        assert now == 3
        return dict(renew=[(0, 10)], reports=[(T.L[0][0], [0])])

    def expect(r, T):
        assert list(r["renewed"]) == [1] and list(r["report_unknown"]) == [0] and r["expired"] == 3
        assert T.L[0][1:] == [10, False] and r["swept"] == 3 - r["kept_zombies"]
    return [grant(4, 2), nothing(), nothing(), (make, expect)]


def expiry_equal_to_now():
    """expires_at == now is not overdue, now - 1 is (both the sweep and the report compare with <);
    the same for a renewal to exactly now, and for one to now - 1."""
    def at2(T, now):
        assert now == 2
        return dict(renew=[(0, 2)], reports=every_servant_lists_everything(T))

    def first(r, T):
        assert r["expired"] == 2 and [T.L[t][2] for t in range(4)] == [False, False, True, True]
        want = {0: 0, 1: 0, 2: 1, 3: 1}
        ids = [t for _, l in every_servant_lists_everything(T) for t in l]
        assert [int(u) for u in r["report_unknown"]] == [want[t] for t in ids]

    def at3(T, now):
        return dict(renew=[(1, 2), (2, 50)], reports=[(T.L[1][0], [t for t in held(T)[T.L[1][0]]])])

    def second(r, T):
        assert list(r["renewed"]) == [1, 0] and r["expired"] == 2 and r["report_unknown"].all()
        assert all(e[2] for e in T.L.values())
    return [grant(4, [2, 2, 1, 1]), nothing(), (at2, first), (at3, second)]


def report_list_oddities():
    """A report naming one id twice, a live lease of another servant, ids the table has not handed
    out, the never-an-id 2^64 - 1; a servant without any lease reporting ids of others; a servant
    without any lease reporting nothing."""
    def make(T, now):
        (sa, ia), (sb, ib) = list(held(T).items())[:2]
        z, w = idle_servants(T)[:2]
        return dict(reports=[(sa, [ia[0], ia[0], ib[0], T.next_id, T.next_id + 5, NO_ID, ia[0]]),
                             (z, [ia[0], T.next_id]), (w, [])])

    def expect(r, T):
        assert list(r["report_unknown"]) == [0, 0, 1, 1, 1, 1, 0, 1, 1]
        assert r["swept"] == 0 and r["n_leases"] == 6 and int(r["running"].sum()) == 6
    return [grant(6, 100), (make, expect)]


def _expiry(p):
    return 1000 + (p * 7919) % 997


def many_renewals_and_frees_of_one_id():
    """900 renewals, 600 of them of lease 0 with different expiries, the others of leases 1 .. 5 and
    of unknown ids in between, so that the bids for one lease come from four workgroups of 256: the
    last in array order wins. Then 600 frees of lease 0 among 300 others: one wins."""
    ids = [0 if p % 3 != 2 else (1 + p % 7) for p in range(900)]  # (6 and 7: unknown)

    def renew(T, now):
        return dict(renew=[(t, _expiry(p)) for p, t in enumerate(ids)])

    def expect(r, T):
        last = {t: p for p, t in enumerate(ids)}
        assert last[0] == 898 and int(r["renewed"].sum()) == sum(t < 6 for t in ids)
        for t in range(6):
            assert T.L[t][1] == _expiry(last[t])
        assert _expiry(last[0]) < max(_expiry(p) for p, t in enumerate(ids) if t == 0)

    def free(T, now):
        return dict(free=[0 if p % 3 != 2 else (1 + (p // 3) % 300) for p in range(900)])

    def freed(r, T):
        # ids 1 .. 5 are named at least once each among the others
        assert r["freed"] == 6 and r["ignored_frees"] == 894 and r["n_leases"] == 0
        assert int(r["running"].sum()) == 0
    return [grant(6, 100), (renew, expect), (free, freed)]


def the_empty_slot_key_as_an_id():
    """2^64 - 1 is no task id (and the device's table keeps it in its empty slots): renewals and
    frees of it are refused and ignored before the table has handed out any id and after; the
    snapshot, n_leases and running_tasks stay."""
    def before(r, T):
        assert list(r["renewed"]) == [0] and r["ignored_frees"] == 1 and list(r["report_unknown"]) == [1]
        assert r["n_leases"] == 0 and T.next_id == 0 and int(r["running"].sum()) == 0

    def after(r, T):
        assert list(r["renewed"]) == [0, 1] and r["ignored_frees"] == 2 and r["freed"] == 0
        assert list(r["report_unknown"]) == [1] and r["n_leases"] == 4 and int(r["running"].sum()) == 4
    return [((lambda T, now: dict(renew=[(NO_ID, 50)], free=[NO_ID], reports=[(0, [NO_ID])])), before),
            grant(4, 100),
            ((lambda T, now: dict(renew=[(NO_ID, 50), (0, 60)], free=[NO_ID, NO_ID],
                                  reports=[(T.L[0][0], [NO_ID])])), after)]


CASES = [renewed_and_freed, freed_and_reported, overdue_when_its_servant_reports, overdue_but_renewed_in_time,
         expiry_equal_to_now, report_list_oddities, many_renewals_and_frees_of_one_id, the_empty_slot_key_as_an_id]

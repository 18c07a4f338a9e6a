"""Waiting + leased ticks written by hand: the same-tick interactions between the queue and the
lease table that a seeded stream only meets by chance. One list of cases, played three ways:
through the model and through the verbatim reference class (tests/test_stream_wait_lease_model.py,
which compares the two field by field), and on the GPU against the model
(tests/test_stream_wait_lease_gpu.py).

A case is a list of steps on a pool of three idle servants with fewer slots than 48 requests ask
for: a tick of 48 fills it and leaves waiters. A step is (make, expect): make(S, now) ->
the tick's traffic, written from the state S (W, L) as the previous ticks left it; expect(r, S)
asserts on the tick's record and the state behind it what the case is about, so a case that no
longer meets its situation fails instead of passing idly. The clock is the tick number; the
heartbeats are the stream's, everything else is written here.
"""
import numpy as np

from tests import stream_wait_lease_model as M
from yadcc_amd import synth

NO_ID = M.NO_ID
MAX_TASKS = 48    # requests per tick at most (what a context is begun with)
MAX_WAITING = 64


def small_stream(max_leases=1 << 30):
    sv = synth.make_servants(3, n_tasks_hint=40, n_envs=1, seed=17)
    # Idle machines with many processors: max_tasks alone bounds a servant, so a slot given back is
    # free in that very tick (a servant bounded by its load has to send a heartbeat first).
    sv["num_processors"][:] = 256
    sv["current_load"][:] = 0
    ws = M.new_stream(sv, MAX_TASKS, 0, 0, MAX_WAITING, n_envs=1, max_leases=max_leases, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n  # every servant sends its heartbeat in every tick
    return ws


def scripted(ws, ev, n=0, lease_for=0, wait=0, renew=(), free=(), reports=()):
    """The drawn tick `ev` with its heartbeats kept and everything else written by hand: n requests
    with the lease duration lease_for and the deadline now + wait (one value or n each), renew:
    [(id, expires_at)], free: [id], reports: [(servant, [id])]."""
    now = int(ev["now"])
    off = np.cumsum([0] + [len(ids) for _, ids in reports]).astype(np.uint32)
    e = dict(ev)
    e.update(tasks=synth.make_tasks(n, ws.es.sv, n_envs=1, seed=500 + now, self_frac=0.0),
             release_idx=np.empty(0, np.uint32),
             lease_for=np.broadcast_to(np.asarray(lease_for, np.int64), (n,)).copy(),
             deadlines=now + np.broadcast_to(np.asarray(wait, np.int64), (n,)),
             tags=np.arange(1000 * now, 1000 * now + n, dtype=np.uint64),
             renew_ids=np.array([r[0] for r in renew], np.uint64),
             renew_expires_at=np.array([r[1] for r in renew], np.int64),
             free_ids=np.array(free, np.uint64),
             report_servants=np.array([s for s, _ in reports], np.uint32), report_off=off,
             report_ids=np.array([t for _, ids in reports for t in ids], np.uint64))
    return e


def play(ws, steps, tick):
    """tick(ev) -> the tick's record (dict of M.FIELDS); it advances ws.state."""
    for make, expect in steps:
        ev = ws.next_tick()
        r = tick(scripted(ws, ev, **make(ws.state, int(ev["now"]))))
        if expect:
            expect(r, ws.state)


def held(S):
    """servant -> its ids, ascending."""
    of = {}
    for t in sorted(S.T.L):
        of.setdefault(S.T.L[t][0], []).append(t)
    return of


def flood(lease_for, wait):
    """48 requests: the pool grants what it has, the others wait."""
    def expect(r, S):
        g = int((r["out"] < M.IDX_WAITING).sum())
        assert g >= 8 and r["n_waiting"] >= 8 and g + r["n_waiting"] == MAX_TASKS, (g, r["n_waiting"])
        assert list(r["task_id"][r["out"] < M.IDX_WAITING]) == list(range(g)) and len(held(S)) >= 2
    return (lambda S, now: dict(n=MAX_TASKS, lease_for=lease_for, wait=wait)), expect


def nothing(expect=None):
    return (lambda S, now: {}), expect


def a_freed_id_lets_a_waiter_in():
    """FreeTask of id 0 and the first waiter's grant in one tick: the waiter gets the very slot, the
    next id, and a lease that runs from this tick (now + 100), not from the tick it was queued in."""
    seen = {}

    def make(S, now):
        seen.update(servant=S.T.L[0][0], next_id=S.T.next_id, first=int(S.q.tag[0]), w=len(S.q), now=now)
        return dict(free=[0])

    def expect(r, S):
        assert r["freed"] == 1 and r["w_granted"] == 1 and r["n_waiting"] == seen["w"] - 1
        assert list(r["res_tags"]) == [seen["first"]] and list(r["res_idx"]) == [seen["servant"]]
        assert list(r["res_ids"]) == [seen["next_id"]] and S.T.next_id == seen["next_id"] + 1
        assert S.T.L[seen["next_id"]] == [seen["servant"], seen["now"] + 100, False] and seen["now"] == 1
    return [flood(100, 40), (make, expect)]


def a_waiter_is_granted_in_the_tick_its_servant_reports():
    """The leases turn zombie at now == 2. At now == 3 one servant reports, naming none of its
    zombies but the id the first waiter is about to get: the zombies are swept, the waiters take
    their slots on that servant in the same tick, and the named id, which becomes a lease of that
    very servant a moment later, is unknown to the report."""
    seen = {}

    def zombies(r, S):
        assert r["expired"] == len(S.T.L) == r["kept_zombies"] and r["w_granted"] == 0

    def make(S, now):
        s, ids = sorted(held(S).items())[0]
        seen.update(servant=s, mine=len(ids), next_id=S.T.next_id, w=len(S.q), now=now)
        return dict(reports=[(s, [S.T.next_id])])

    def expect(r, S):
        k = min(seen["mine"], seen["w"])
        assert r["swept"] == seen["mine"] and r["w_granted"] == k and list(r["report_unknown"]) == [1]
        assert list(r["res_idx"]) == [seen["servant"]] * k
        assert list(r["res_ids"]) == list(range(seen["next_id"], seen["next_id"] + k))
        assert all(S.T.L[t] == [seen["servant"], seen["now"] + 1, False] for t in r["res_ids"].tolist())
    return [flood(1, 40), nothing(), nothing(zombies), (make, expect)]


def a_deadline_and_a_would_be_grant_in_the_same_tick():
    """Every waiter's deadline is 2. At now == 2 three ids are freed, so there would be room: the
    waiters resolve as Timeout without being tried (deadline == now) and consume no id; two new
    requests of that tick take two of the slots and the next two ids."""
    seen = {}

    def still_waiting(r, S):
        assert r["w_expired"] == 0 and r["n_waiting"] == len(S.q) >= 8

    def make(S, now):
        assert now == 2 and (S.q.deadline == 2).all()
        seen.update(next_id=S.T.next_id, w=len(S.q))
        return dict(free=[0, 1, 2], n=2, lease_for=7, wait=0)

    def expect(r, S):
        assert r["freed"] == 3 and r["w_expired"] == seen["w"] and r["w_granted"] == 0 and r["n_waiting"] == 0
        assert (r["res_idx"] == M.IDX_TIMEOUT).all() and (r["res_ids"] == NO_ID).all() and len(r["res_ids"]) == seen["w"]
        assert (r["out"] < M.IDX_WAITING).all() and list(r["task_id"]) == [seen["next_id"], seen["next_id"] + 1]
        assert S.T.next_id == seen["next_id"] + 2 and S.T.L[seen["next_id"]][1] == 9
    return [flood(100, 2), nothing(still_waiting), (make, expect)]


def a_lease_expires_and_is_swept_in_the_tick_a_waiter_takes_its_slot():
    """At now == 2 every lease (expires_at 1) is overdue and every servant reports an empty list:
    expired, swept and the slot granted to a waiter in one tick."""
    seen = {}

    def make(S, now):
        assert now == 2 and not any(e[2] for e in S.T.L.values())
        seen.update(n=len(S.T.L), w=len(S.q), next_id=S.T.next_id)
        return dict(reports=[(s, []) for s in sorted(held(S))])

    def expect(r, S):
        assert r["expired"] == r["swept"] == seen["n"] and r["w_granted"] == seen["w"] and r["n_waiting"] == 0
        assert r["n_leases"] == seen["w"] and int(r["running"].sum()) == seen["w"]
        assert sorted(S.T.L) == list(range(seen["next_id"], seen["next_id"] + seen["w"]))
        assert all(e[1:] == [3, False] for e in S.T.L.values())
    return [flood(1, 40), nothing(), (make, expect)]


def a_lease_for_zero():
    """lease_for == 0: expires_at == now of the grant, overdue from the next clock value on. For a
    waiter that is the tick of its grant (1), not the tick it was queued in (0)."""
    seen = {}

    def make(S, now):
        assert now == 1 and all(e[1:] == [0, False] for e in S.T.L.values()) and (S.lease_for == 0).all()
        seen.update(n=len(S.T.L), w=len(S.q))
        return dict(reports=[(s, []) for s in sorted(held(S))])

    def expect(r, S):
        assert r["expired"] == r["swept"] == seen["n"] and r["w_granted"] == seen["w"]
        assert len(S.T.L) == seen["w"] and all(e[1:] == [1, False] for e in S.T.L.values())

    def overdue(r, S):
        assert r["expired"] == seen["w"] and all(e[2] for e in S.T.L.values())
    return [flood(0, 40), (make, expect), nothing(overdue)]


CASES = [a_freed_id_lets_a_waiter_in, a_waiter_is_granted_in_the_tick_its_servant_reports,
         a_deadline_and_a_would_be_grant_in_the_same_tick,
         a_lease_expires_and_is_swept_in_the_tick_a_waiter_takes_its_slot, a_lease_for_zero]

"""Ticks with aliveness written by hand: the situations of step 5 that a seeded stream only meets by
chance. One list of cases, played three ways: on the model alone, through the verbatim reference
class (tests/test_stream_alive_model.py compares the two field by field) and on the GPU against the
model (tests/test_stream_alive_gpu.py).

A case is a function of a Player. The pool is tests/stream_lease_cases.small_stream: 12 idle
servants, one heartbeat per tick (servant t mod n at tick t), the clock is the tick number. Every
case asserts that its situation is there, so a case that no longer meets it fails instead of passing
idly. A Player runs the model; its subclasses mirror every call on the other side and compare.
"""
import numpy as np

from tests import stream_alive_model as AM
from tests import stream_book_model as BM
from tests import stream_lease_cases as cases
from tests import stream_lease_model as M
from yadcc_amd import synth

FAR = 1000  # an expiry no case reaches
GONE = AM.GONE
FIELDS = M.FIELDS + ("removed", "orphans")


def two_digest_stream():
    """small_stream's pool with a second digest that only servant 5 has, and servant 5 too loaded to
    take anything: requests for digest 1 time out while it lives."""
    sv = synth.make_servants(12, n_tasks_hint=600, n_envs=1, seed=17)
    sv["env_mask"][5] = 3
    sv["current_load"][5] = 4 * sv["num_processors"][5]
    return M.LeaseStream(sv, cases.MAX_TASKS, 0, 0, M.LeaseTable(), n_envs=2)


class Player:
    """The model's side of a case. book: with a running-task book."""

    def __init__(self, make_stream=cases.small_stream, book=False):
        self.make_stream, self.with_book = make_stream, book
        self.ls = make_stream()
        self.book = BM.Book() if book else None
        self.A = AM.attach(self.ls, np.full(self.ls.es.n, FAR, np.int64), self.book)
        self.T = self.ls.table

    def set_expiry(self, row, value):
        """The column replaced (a second ydc_stream_alive_begin) with `row` expiring at `value`."""
        self.A.expires[row] = value
        self.A.bound = int(self.A.expires.min())
        self.on_set_expiry(row, value)

    def next_beater(self):
        """The servant whose heartbeat the next tick carries."""
        return int(self.ls.es.hb_pos % self.ls.es.n)

    def make_ev(self, ls, beat, append, tasks, kw):
        ev = cases.scripted(ls, ls.next_tick(), **kw)
        if tasks is not None:
            ev["tasks"] = {k: np.asarray(v, np.uint32) for k, v in tasks.items()}
        exp = [beat] * len(ev["upd_idx"])
        if append is not None:
            like, ip, e = append
            row, s = AM.append_servant(ls, like, ip)
            ev["upd_idx"] = np.concatenate([ev["upd_idx"], np.array([s], np.uint32)])
            ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
            exp.append(e)
        ev["upd_expires_at"] = np.array(exp, np.int64)
        ev["stid"] = ev["report_ids"] + np.uint64(1000)  # (servant_task_id of every reported id)
        return ev

    def tick(self, beat=FAR, append=None, tasks=None, **kw):
        """One tick: the stream's heartbeat with the expiry `beat`, append: (like, ip, expires_at) adds a
        servant, tasks: the requests' columns (default: kw["n"] requests for digest 0), kw: as
        stream_lease_cases.scripted. -> the model's record."""
        ev = self.make_ev(self.ls, beat, append, tasks, kw)
        if self.book is not None:
            self.book.stage(ev["stid"], np.zeros(len(ev["stid"]), np.uint64))
        r = AM.model_tick(M, self.ls, ev)
        self.on_tick(ev, r, (beat, append, tasks, kw))
        return r

    def on_set_expiry(self, row, value):
        pass

    def on_tick(self, ev, r, how):
        pass

    def close(self):
        pass


def victim(p, n=8, lease=100, file=True, silent_from=5):
    """Tick 0 grants n leases; with a book, tick 1 has every holder report all its grants, so that the
    book has entries on the victim's row and on the survivors'. -> (a servant that holds some, its ids)."""
    r = p.tick(n=n, lease=[lease] * n)
    assert int((r["out"] < M.IDX_ENV_NOT_FOUND).sum()) == n
    if p.book is not None and file:
        r = p.tick(reports=cases.every_servant_lists_everything(p.T))
        assert r["unknown_reported"] == 0 and len(p.book) == n
    # (not one of the next ticks' beaters, rows 1 .. silent_from - 1: a heartbeat would extend its life again)
    holders = sorted((s, i) for s, i in cases.held(p.T).items() if s >= silent_from)
    assert holders, "no lease on a servant that stays silent"
    assert len(cases.held(p.T)) >= 2, "every lease sits on one servant"
    return holders[0]


def clock(p):
    """The next tick's `now`."""
    return int(p.ls.es.tick_no)


def book_lost(p, ids, before):
    """With a book: the victim's entries are gone, every other entry is still there."""
    if p.book is not None:
        assert before > len(ids) and len(p.book) == before - len(ids)
        assert not {e[1] for e in p.book.B} & set(ids)


def renewal_of_a_lease_orphaned_in_the_same_tick(p):
    v, ids = victim(p)
    t, n_book = clock(p), len(p.book or ())
    p.set_expiry(v, t)
    r = p.tick()  # now == t: t < t is false, the servant lives
    assert len(r["removed"]) == 0 and not r["alarm"]
    r = p.tick(renew=[(ids[0], 50), (999, 50)])
    assert list(r["removed"]) == [v] and r["orphans"] == len(ids)
    assert list(r["renewed"]) == [1, 0] and ids[0] not in p.T.L
    assert r["expired"] == 0 and r["swept"] == 0
    book_lost(p, ids, n_book)
    r = p.tick(renew=[(ids[0], 60)])
    assert list(r["renewed"]) == [0] and len(r["removed"]) == 0 and not r["alarm"]


def free_of_a_lease_orphaned_in_the_same_tick(p):
    v, ids = victim(p)
    before, n_book = len(p.T), len(p.book or ())
    p.set_expiry(v, 0)
    r = p.tick(free=[ids[0], ids[0]])
    assert list(r["removed"]) == [v] and r["freed"] == 1 and r["ignored_frees"] == 1
    assert r["orphans"] == len(ids) - 1 and r["n_leases"] == before - len(ids)
    book_lost(p, ids, n_book)


def report_from_a_servant_removed_in_the_same_tick(p):
    """The report of the erased servant lists its own (parked) leases and a survivor's: every id is
    unknown, and with a book nothing is filed for it, while the survivor's report is filed as ever."""
    v, ids = victim(p)
    others = [(s, i) for s, i in cases.held(p.T).items() if s != v]
    assert others
    n_book = len(p.book or ())
    p.set_expiry(v, 0)
    o, o_ids = others[0]
    r = p.tick(reports=[(v, ids + [o_ids[0]]), (o, o_ids)])
    assert list(r["removed"]) == [v]
    assert list(r["report_unknown"]) == [1] * (len(ids) + 1) + [0] * len(o_ids)
    book_lost(p, ids, n_book)
    if p.book is not None:
        o_now = o - (1 if v < o else 0)
        assert [e[1] for e in p.book.B if e[0] == o_now] == o_ids and GONE not in {e[0] for e in p.book.B}
        assert [e[1] for e in p.book.B][-len(o_ids):] == o_ids, "the tick's permitted ids come last"


def removed_servant_with_book_entries(p):
    assert p.book is not None
    v, ids = victim(p, file=False, silent_from=4)
    others = [(s, i) for s, i in cases.held(p.T).items() if s > v]
    assert others, "no lease on a row behind the victim"
    o, o_ids = others[-1]
    r = p.tick(reports=[(v, ids), (o, o_ids)])
    assert r["unknown_reported"] == 0 and len(p.book) == len(ids) + len(o_ids)
    p.set_expiry(v, 1)
    r = p.tick()
    assert list(r["removed"]) == [v] and len(p.book) == len(o_ids)
    assert {e[0] for e in p.book.B} == {o - 1}, "the survivor's entries follow the compaction"


def overdue_orphan(p):
    t0 = 2 if p.book is not None else 1  # (the clock of the first tick behind victim())
    v, ids = victim(p, lease=t0)
    t, n_book = clock(p), len(p.book or ())
    assert t == t0
    p.set_expiry(v, t)
    r = p.tick()
    assert r["expired"] == 0 and len(r["removed"]) == 0
    n_other = len(p.T) - len(ids)
    r = p.tick()  # now == t + 1: the servant and every lease are overdue
    assert list(r["removed"]) == [v] and r["orphans"] == len(ids)
    assert r["expired"] == n_other and r["n_leases"] == n_other, "an orphan is not counted as expired"
    book_lost(p, ids, n_book)


def zombie_orphan(p):
    v, ids = victim(p, lease=1 if p.book is not None else 0)
    n_book = len(p.book or ())
    r = p.tick()  # every lease becomes a zombie
    assert r["expired"] == len(p.T)
    p.set_expiry(v, clock(p) - 1)
    r = p.tick(renew=[(ids[0], 50)], free=[ids[-1]])
    assert list(r["removed"]) == [v] and list(r["renewed"]) == [0] and r["freed"] == 1
    assert r["orphans"] == len(ids) - 1 and r["expired"] == 0
    book_lost(p, ids, n_book)


def heartbeat_saves_the_servant_in_the_tick_it_would_run_out(p):
    p.tick()
    s = p.next_beater()
    now = int(p.ls.es.tick_no)
    p.set_expiry(s, now - 1)
    r = p.tick(beat=FAR)
    assert r["alarm"] and len(r["removed"]) == 0 and p.A.expires[s] == FAR
    assert p.A.empty_alarms == 1
    r = p.tick()
    assert not r["alarm"]


def heartbeat_whose_own_expiry_is_past(p):
    v, ids = victim(p)
    s = p.next_beater()
    now = int(p.ls.es.tick_no)
    r = p.tick(beat=now - 1)
    assert list(r["removed"]) == [s] and r["alarm"]
    assert p.ls.es.n == 11 and len(p.A.expires) == 11


def appended_servant(p):
    p.tick(n=4, lease=[100] * 4)
    now = int(p.ls.es.tick_no)
    r = p.tick(append=(3, (10 << 24) + 200, now - 1), n=4, lease=[100] * 4)  # born overdue: erased at once
    assert list(r["removed"]) == [12] and p.ls.es.n == 12
    r = p.tick(append=(3, (10 << 24) + 201, FAR), n=4, lease=[100] * 4)
    assert len(r["removed"]) == 0 and p.ls.es.n == 13 and p.A.expires[12] == FAR
    p.set_expiry(0, 0)
    r = p.tick(n=4, lease=[100] * 4)
    assert list(r["removed"]) == [0] and p.ls.es.n == 12


def last_servant_of_a_digest_removed(p):
    def ask(n):
        z = np.zeros(n, np.uint32)
        return {"env_id": np.ones(n, np.uint32), "min_version": z, "requestor_ip": z + np.uint32(7)}
    r = p.tick(tasks=ask(3), n=3, lease=[100] * 3)
    assert list(r["out"]) == [M.IDX_TIMEOUT] * 3
    p.set_expiry(5, 0)
    r = p.tick(tasks=ask(3), n=3, lease=[100] * 3)
    assert list(r["removed"]) == [5] and list(r["out"]) == [M.IDX_ENV_NOT_FOUND] * 3


ORPHANS = [renewal_of_a_lease_orphaned_in_the_same_tick, free_of_a_lease_orphaned_in_the_same_tick,
           report_from_a_servant_removed_in_the_same_tick, overdue_orphan, zombie_orphan]
# (case, make_stream, book): the orphan cases without a book and with one that has entries on the
# removed row and on surviving rows
CASES = [(c, cases.small_stream, False) for c in ORPHANS] + [(c, cases.small_stream, True) for c in ORPHANS] + [
    (removed_servant_with_book_entries, cases.small_stream, True),
    (heartbeat_saves_the_servant_in_the_tick_it_would_run_out, cases.small_stream, False),
    (heartbeat_whose_own_expiry_is_past, cases.small_stream, False),
    (appended_servant, cases.small_stream, False),
    (last_servant_of_a_digest_removed, two_digest_stream, False),
]
IDS = [c[0].__name__ + ("_with_a_book" if c[2] and c[0] in ORPHANS else "") for c in CASES]

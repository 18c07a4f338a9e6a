"""The servants' expiry of a leased stream (ydc_stream_alive_begin / _stage / _removed / _get) as a
plain model: the yardstick of tests/test_stream_alive_gpu.py, pinned against the verbatim reference's
KeepServantAlive and OnExpirationTimer by tests/test_stream_alive_model.py.

It sits on top of the lease models (tests/stream_lease_model.py and the two built on it) and edits
none of them. Every one of them runs steps 2 - 7 of a tick in LeaseTable.tick; a stream is given
aliveness by turning ITS table into an AliveTable (attach), whose tick is LeaseTable.tick with step 5
as the whole of OnExpirationTimer (task_dispatcher.cc:498-536):
  1. heartbeat i also sets expires_at[upd_idx[i]] = upd_expires_at[i];
  2. - 4. renewals, frees by id, releases: unchanged, on the numbering the tick came with;
  5. every servant with expires_at < now is erased (the survivors keep their order: drop_rows of
     tests/test_stream_lease_gpu.py, LeaseTable.remove_servants, Book.remove_servants), every lease
     on it goes as an orphan, without the zombie stage and counted neither as expired nor as swept;
     then leases with expires_at < now become zombies;
  6. - 7. on the compacted registry: a report of a servant that was just erased answers 1 for all its
     ids and touches nothing; the requests do not see the servant.
The record gains "removed" (ascending, in the numbering before the removal), "orphans" and "alarm"
(the host's lower bound of the smallest expires_at was below `now`: the device is asked who is due).

AliveGen adds upd_expires_at to a LeaseStream, a waiting-and-leased stream or an rpc stream: most
heartbeats extend the servant's life beyond its next heartbeat, some servants stop beating and run
out, and now and then a heartbeat carries a life that ends before the next one.
"""
import numpy as np

from tests import stream_lease_model as L

NEVER = np.iinfo(np.int64).max
GONE = 0xFFFFFFFF  # a report's or a release's servant that the tick erased


def drop_rows(ls, removed):
    from tests.test_stream_lease_gpu import drop_rows as drop
    drop(ls, removed)


class Alive:
    """The expiry column, the staging, the host's bound and what the last tick erased."""

    def __init__(self, ls, expires_at=None, book=None):
        self.ls, self.book = ls, book
        n = ls.es.n
        self.expires = np.full(n, NEVER, np.int64) if expires_at is None else np.array(expires_at, np.int64)
        assert len(self.expires) == n
        self.stopped = np.zeros(n, bool)  # (the generator's: servants that beat no more)
        self.bound = int(self.expires.min()) if n else NEVER
        self.staged = None
        self.removed_last, self.orphans_last, self.alarm_last = np.empty(0, np.uint32), 0, False
        self.alarms = self.empty_alarms = 0

    def stage(self, upd_expires_at):
        self.staged = np.array(upd_expires_at, np.int64)

    def check(self, ev):
        """The refusals that leave everything untouched, the staging included."""
        n_upd = len(ev["upd_idx"])
        if (0 if self.staged is None else len(self.staged)) != n_upd:
            raise ValueError("staged count differs from the tick's heartbeats")
        if len(set(np.asarray(ev["upd_idx"]).tolist())) != n_upd:
            raise ValueError("a servant beats twice")

    def grow(self, n):
        """Rows the registry gained: "never" until a heartbeat says otherwise."""
        k = n - len(self.expires)
        if k > 0:
            self.expires = np.concatenate([self.expires, np.full(k, NEVER, np.int64)])
            self.stopped = np.concatenate([self.stopped, np.zeros(k, bool)])

    def beat(self, ev):
        """Step 1's expiries; consumes the staging. -> whether the tick asks the device who is due."""
        self.grow(self.ls.es.n)
        exp = self.staged if self.staged is not None else np.empty(0, np.int64)
        self.staged = None
        self.expires[np.asarray(ev["upd_idx"], np.int64)] = exp
        if len(exp):
            self.bound = min(self.bound, int(exp.min()))
        return self.bound < int(ev["now"])

    def remove(self, removed):
        """The rows `removed` (ascending) leave registry, stream, lease table, book and column."""
        drop_rows(self.ls, removed)
        if self.book is not None:
            self.book.remove_servants(removed)
        keep = np.ones(len(self.expires), bool)
        keep[removed] = False
        self.expires, self.stopped = self.expires[keep], self.stopped[keep]

    def renumber(self, idx):
        """Row numbers of the tick's own numbering after its removal; an erased row: GONE."""
        idx = np.asarray(idx, np.int64)
        rm = self.removed_last.astype(np.int64)
        if not len(rm) or not len(idx):
            return idx.astype(np.uint32)
        before = np.searchsorted(rm, idx)
        hit = (before < len(rm)) & (rm[np.minimum(before, len(rm) - 1)] == idx)
        return np.where(hit, GONE, idx - before).astype(np.uint32)

    def renumbered(self, ev):
        return dict(ev, report_servants=self.renumber(ev["report_servants"]))


class AliveTable(L.LeaseTable):
    """LeaseTable whose step 5 is the whole of OnExpirationTimer. `alive`: its Alive."""

    def tick(self, running, ev, place):
        A = self.alive
        now = int(ev["now"])
        n = len(ev["tasks"]["env_id"])
        self.check(n, now)
        if len(set(ev["report_servants"].tolist())) != len(ev["report_servants"]):
            raise ValueError("a servant reports twice")
        self.last_now = now
        alarm = A.beat(ev)
        Lt = self.L
        renewed = np.zeros(len(ev["renew_ids"]), np.uint8)
        for i, (tid, exp) in enumerate(zip(ev["renew_ids"].tolist(), ev["renew_expires_at"].tolist())):
            e = Lt.get(tid)
            if e is not None and not e[2]:
                e[1] = exp
                renewed[i] = 1
        freed = ignored = 0
        for tid in ev["free_ids"].tolist():
            e = Lt.pop(tid, None)
            if e is None:
                ignored += 1
            else:
                running[e[0]] -= 1
                freed += 1
        np.subtract.at(running, ev["release_idx"], 1)
        # Step 5, servants first.
        due = np.nonzero(A.expires < now)[0].astype(np.uint32)
        A.removed_last, A.orphans_last, A.alarm_last = due, 0, alarm
        if alarm:
            A.alarms += 1
            A.empty_alarms += not len(due)
        if len(due):
            assert alarm, "the bound missed a due servant"
            gone = set(due.tolist())
            A.orphans_last = sum(1 for e in Lt.values() if e[0] in gone)
            A.remove(due)  # (LeaseTable.remove_servants makes a new dict, drop_rows a new running column)
            Lt, running = self.L, A.ls.es.running
        if alarm:
            A.bound = int(A.expires.min()) if len(A.expires) else NEVER
        expired = 0
        for e in Lt.values():
            if not e[2] and e[1] < now:
                e[2] = True
                expired += 1
        swept = 0
        unknown = np.ones(len(ev["report_ids"]), np.uint8)
        off = ev["report_off"]
        reporting = set()
        zombies_of = {}
        if len(ev["report_servants"]):
            for tid, e in Lt.items():
                if e[2]:
                    zombies_of.setdefault(e[0], []).append(tid)
        for r, s in enumerate(A.renumber(ev["report_servants"]).tolist()):
            if s == GONE:  # (the servant itself has expired, :240-243)
                continue
            reporting.add(s)
            listed = ev["report_ids"][off[r]:off[r + 1]].tolist()
            named = set(listed)
            for tid in zombies_of.get(s, ()):
                if tid not in named:
                    del Lt[tid]
                    running[s] -= 1
                    swept += 1
            for k, tid in enumerate(listed):
                e = Lt.get(tid)
                if e is not None and e[0] == s and not e[2]:
                    unknown[off[r] + k] = 0
        kept = sum(1 for e in Lt.values() if e[2] and e[0] not in reporting)
        got = np.asarray(place(ev["tasks"]), np.uint32) if n else np.empty(0, np.uint32)
        ids = np.full(n, L.NO_ID, np.uint64)
        for i in np.nonzero(got < L.IDX_ENV_NOT_FOUND)[0].tolist():
            ids[i] = self.next_id
            Lt[self.next_id] = [int(got[i]), int(ev["lease_expires_at"][i]), False]
            self.next_id += 1
        return {"out": got, "task_id": ids, "renewed": renewed, "report_unknown": unknown, "n_leases": len(Lt),
                "expired": expired, "swept": swept, "freed": freed, "renew_refused": int((renewed == 0).sum()),
                "ignored_frees": ignored, "unknown_reported": int(unknown.sum()),
                "timeouts": int((got == L.IDX_TIMEOUT).sum()), "kept_zombies": kept}


def attach(ls, expires_at=None, book=None):
    """Aliveness for the stream `ls` (of any of the three lease models): its table becomes an
    AliveTable in place, so the state objects that hold it see the same one. -> its Alive."""
    T = ls.table
    T.__class__ = AliveTable
    T.alive = Alive(ls, expires_at, book)
    return T.alive


def model_tick(M, ws, ev, place=None):
    """One tick of the lease model M (its model_tick) on a stream with aliveness; ev["upd_expires_at"]
    is staged here. Refusals first, then the tick, then the book from the answers, in the tick's new
    numbering. -> M's record plus "removed", "orphans", "alarm"."""
    A = ws.table.alive
    A.stage(ev["upd_expires_at"])
    A.check(ev)
    if A.book is not None:
        A.book.check(ev)
    r = M.model_tick(ws, ev, place) if place else M.model_tick(ws, ev)
    if A.book is not None:
        A.book.apply(A.renumbered(ev), r["report_unknown"])
    r.update(removed=A.removed_last, orphans=A.orphans_last, alarm=A.alarm_last)
    return r


class AliveGen:
    """upd_expires_at for the ticks of the stream `ws` (attach first). life: what an ordinary heartbeat
    grants, in ticks; a servant beats every 1 / heartbeat_frac ticks, so anything above that keeps it.
    Per tick, with probability p_stop one more servant stops beating for good (its heartbeats are
    dropped from then on) and with probability p_short one heartbeat carries a life of -1 .. 2."""

    def __init__(self, ws, life=14, p_stop=0.35, p_short=0.3, seed=5):
        self.ws, self.A = ws, ws.table.alive
        self.life, self.p_stop, self.p_short = life, p_stop, p_short
        self.rng = np.random.default_rng(seed)

    def next_tick(self):
        ws, A, rng = self.ws, self.A, self.rng
        es = ws.es
        load_before = es.sv["current_load"].copy()
        ev = ws.next_tick()
        now = int(ev["now"])
        if rng.random() < self.p_stop and es.n > 8:
            A.stopped[rng.integers(es.n)] = True
        who = np.asarray(ev["upd_idx"], np.int64)
        beats = ~A.stopped[who]
        # (a heartbeat that is never sent leaves the registry's row as it was)
        es.sv["current_load"][who[~beats]] = load_before[who[~beats]]
        ev["upd_idx"], ev["upd_rows"] = ev["upd_idx"][beats], ev["upd_rows"][beats]
        exp = np.full(int(beats.sum()), now + self.life, np.int64)
        if len(exp) and rng.random() < self.p_short:
            exp[rng.integers(len(exp))] = now + rng.integers(-1, 3)
        ev["upd_expires_at"] = exp
        return ev


def first_expiries(n, life=14, seed=3):
    """What ydc_stream_alive_begin is given: every servant alive until its first heartbeat and beyond."""
    return (life + np.random.default_rng(seed).integers(0, 4, n)).astype(np.int64)


def append_servant(ls, like, ip):
    """A new servant at the end of the stream's registry: a copy of row `like` on another host. -> the
    heartbeat row that adds it (binding.ROW_DTYPE, one entry) and its row number."""
    from yadcc_amd import binding
    es = ls.es
    s = es.n
    es.sv = {k: np.concatenate([v, v[like:like + 1]]) for k, v in es.sv.items()}
    es.sv["ip"][s] = ip
    es.sv["running_tasks"][s] = 0
    es.abi = {k: (np.concatenate([v, v[like:like + 1]]) if isinstance(v, np.ndarray) and len(v) == es.n else v)
              for k, v in es.abi.items()}
    es.abi["ip_id"][s] = ip
    es.abi["running_tasks"][s] = 0
    es.foreign = np.concatenate([es.foreign, es.foreign[like:like + 1]])
    es.running = np.concatenate([es.running, np.zeros(1, np.int64)])
    es.n = s + 1
    row = np.zeros(1, dtype=binding.ROW_DTYPE)
    for k in ("version", "num_processors", "current_load", "max_tasks"):
        row[k] = es.sv[k][s]
    row["flags"], row["ip_id"] = es.abi["flags"][s], ip
    em = es.abi["env_mask"]
    row["env_mask"] = em[s] if em.ndim == 1 else em[s, 0]
    return row, s

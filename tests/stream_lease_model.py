"""The streaming leased mode's semantics as a plain model (the yardstick of the lease tests).

One tick with clock `now` (include/yadcc_dispatch.h, ydc_stream_tick_leased), each step as the
named reference calls made one after another in array order:
  1. heartbeats;
  2. renewals = KeepTaskAlive (task_dispatcher.cc:142-167): unknown id or zombie -> 0, nothing
     changes; otherwise expires_at = the new value -> 1 (overdue but not yet a zombie: renewed);
  3. frees by id = one FreeTask each (:169-188): unknown -> ignored, known (zombie or not) ->
     running_tasks - 1 and the lease erased;
  4. releases by servant index (no lease touched);
  5. expiry = the task loop of OnExpirationTimer (:522-535): expires_at < now -> zombie;
  6. reports = NotifyServantRunningTasks (:225-275, :453-476): zombies of the servant that its list
     does not name are freed; a reported id is unknown unless it is a non-zombie lease of that servant;
  7. the requests as one batch; grants take next_id, next_id + 1, ... in array order.

A leased stream is yadcc_amd.streaming.EventStream (heartbeats and requests; its own frees are
off) plus seeded lease traffic drawn from the table's state: requests with lease_expires_at =
now + {1, 2, 5, 40}; renewals of live, freed, zombie and not-yet-granted ids; frees of live,
zombie, unknown and duplicate ids; reports from a tenth of the servants listing all, some or none
of their grants plus foreign and invented ids; ticks with none of each. The clock is the tick
number.

`place` decides a batch: the plain-C oracle (oracle.oraclebind.dispatch on the stream's registry
snapshot) for the model; ReferenceReplay puts one given tick at a time through the verbatim
reference class (oracle.refbind) and records the reference's own answers (run_reference: the same
seeded stream; tests/stream_lease_cases.py: ticks written by hand).
"""
import numpy as np

from oracle import oraclebind as O
from yadcc_amd import streaming, synth

IDX_TIMEOUT = 0xFFFFFFFF
IDX_ENV_NOT_FOUND = 0xFFFFFFFE
LEASE_STEPS = np.array([1, 2, 5, 40], np.int64)
NO_ID = 0xFFFFFFFFFFFFFFFF
FIELDS = ("out", "task_id", "renewed", "report_unknown", "running", "n_leases", "expired", "swept", "freed",
          "renew_refused", "ignored_frees", "unknown_reported", "timeouts", "kept_zombies")


class LeaseTable:
    """L and next_id; one tick of steps 2-7 (the heartbeats are the stream's)."""

    def __init__(self, max_leases=1 << 30):
        self.max_leases = max_leases
        self.L = {}  # task id -> [servant index, expires_at, zombie]
        self.next_id = 0
        self.last_now = None

    def __len__(self):
        return len(self.L)

    def check(self, n_tasks, now):
        """The refusals that leave everything untouched."""
        if len(self.L) + n_tasks > self.max_leases:
            raise OverflowError("capacity")
        if self.last_now is not None and now < self.last_now:
            raise ValueError("now goes backwards")

    def tick(self, running, ev, place):
        """running: the registry's running_tasks (int64, changed in place); ev: the tick's lease
        columns (dict, see LeaseStream.next_tick); place(tasks) -> servant index per request, called
        after steps 2-6 have given their slots back. -> dict of FIELDS (without "running")."""
        now = int(ev["now"])
        n = len(ev["tasks"]["env_id"])
        self.check(n, now)
        if len(set(ev["report_servants"].tolist())) != len(ev["report_servants"]):
            raise ValueError("a servant reports twice")
        self.last_now = now
        L = self.L
        renewed = np.zeros(len(ev["renew_ids"]), np.uint8)
        for i, (tid, exp) in enumerate(zip(ev["renew_ids"].tolist(), ev["renew_expires_at"].tolist())):
            e = L.get(tid)
            if e is not None and not e[2]:
                e[1] = exp
                renewed[i] = 1
        freed = ignored = 0
        for tid in ev["free_ids"].tolist():
            e = L.pop(tid, None)
            if e is None:
                ignored += 1
            else:
                running[e[0]] -= 1
                freed += 1
        np.subtract.at(running, ev["release_idx"], 1)
        expired = 0
        for e in L.values():
            if not e[2] and e[1] < now:
                e[2] = True
                expired += 1
        swept = 0
        unknown = np.ones(len(ev["report_ids"]), np.uint8)
        off = ev["report_off"]
        reporting = set()
        zombies_of = {}
        if len(ev["report_servants"]):
            for tid, e in L.items():
                if e[2]:
                    zombies_of.setdefault(e[0], []).append(tid)
        for r, s in enumerate(ev["report_servants"].tolist()):
            reporting.add(s)
            listed = ev["report_ids"][off[r]:off[r + 1]].tolist()
            named = set(listed)
            for tid in zombies_of.get(s, ()):
                if tid not in named:
                    del L[tid]
                    running[s] -= 1
                    swept += 1
            for k, tid in enumerate(listed):
                e = L.get(tid)
                if e is not None and e[0] == s and not e[2]:
                    unknown[off[r] + k] = 0
        kept = sum(1 for e in L.values() if e[2] and e[0] not in reporting)
        got = np.asarray(place(ev["tasks"]), np.uint32) if n else np.empty(0, np.uint32)
        ids = np.full(n, NO_ID, np.uint64)
        for i in np.nonzero(got < IDX_ENV_NOT_FOUND)[0].tolist():
            ids[i] = self.next_id
            L[self.next_id] = [int(got[i]), int(ev["lease_expires_at"][i]), False]
            self.next_id += 1
        return {"out": got, "task_id": ids, "renewed": renewed, "report_unknown": unknown, "n_leases": len(L),
                "expired": expired, "swept": swept, "freed": freed, "renew_refused": int((renewed == 0).sum()),
                "ignored_frees": ignored, "unknown_reported": int(unknown.sum()),
                "timeouts": int((got == IDX_TIMEOUT).sum()), "kept_zombies": kept}

    def remove_servants(self, removed):
        """ydc_remove_servants: leases of removed rows vanish, the others follow the compaction."""
        removed = np.asarray(removed, np.int64)
        gone = set(removed.tolist())
        self.L = {t: [e[0] - int(np.searchsorted(removed, e[0])), e[1], e[2]]
                  for t, e in self.L.items() if e[0] not in gone}

    def snapshot(self):
        """(task ids, servant, expires_at, zombie) in id order, as ydc_stream_leases_get."""
        ids = sorted(self.L)
        return (np.array(ids, np.uint64), np.array([self.L[t][0] for t in ids], np.uint32),
                np.array([self.L[t][1] for t in ids], np.int64), np.array([self.L[t][2] for t in ids], np.uint8))


class LeaseStream:
    """EventStream plus seeded lease traffic drawn from a LeaseTable's state (`table`: the one the
    caller advances with every tick's answers)."""

    def __init__(self, sv, tasks_per_tick, frees_per_tick, renewals_per_tick, table, n_envs=1, seed=83,
                 report_frac=0.10):
        self.es = streaming.EventStream(sv, tasks_per_tick, 0, n_envs=n_envs)
        self.table = table
        self.rng = np.random.default_rng(seed)
        self.frees, self.renewals = frees_per_tick, renewals_per_tick
        self.n_rep = max(1, int(self.es.n * report_frac))
        self.rep_pos = 0
        self.gone = []  # ids freed or swept lately (unknown by now)

    def _mix(self, pools, weights, n):
        """n ids drawn from the non-empty pools with the given weights."""
        pools = [(np.asarray(p, np.uint64), w) for p, w in zip(pools, weights) if len(p)]
        if not pools or n == 0:
            return np.empty(0, np.uint64)
        w = np.array([w for _, w in pools], float)
        which = self.rng.choice(len(pools), n, p=w / w.sum())
        return np.array([pools[k][0][self.rng.integers(len(pools[k][0]))] for k in which], np.uint64)

    def next_tick(self):
        rng, T = self.rng, self.table
        now = self.es.tick_no
        who, rows, rel, tk = self.es.next_tick()
        live = [t for t, e in T.L.items() if not e[2]]
        zomb = [t for t, e in T.L.items() if e[2]]
        ahead = T.next_id + rng.integers(0, 1000, 16)
        quiet = rng.random(4) < 0.12  # renewals, frees, reports, requests: none this tick
        if quiet[3]:
            tk = {k: v[:0] for k, v in tk.items()}
        n = len(tk["env_id"])
        ren = np.empty(0, np.uint64) if quiet[0] else self._mix([live, self.gone, zomb, ahead], [7, 1, 1, 1],
                                                                self.renewals)
        fr = np.empty(0, np.uint64)
        if not quiet[1]:
            k = min(self.frees, len(live))
            a = rng.choice(np.asarray(live, np.uint64), int(k * 0.85), replace=False) if k else fr
            b = self._mix([zomb, self.gone, ahead], [3, 2, 1], max(1, self.frees // 12))
            fr = np.concatenate([a, b])
            if len(fr):
                fr = np.concatenate([fr, rng.choice(fr, max(1, len(fr) // 20))])  # duplicates
            rng.shuffle(fr)
        rs, off, rid = np.empty(0, np.uint32), np.zeros(1, np.uint32), []
        if not quiet[2]:
            rs = ((self.rep_pos + np.arange(self.n_rep)) % self.es.n).astype(np.uint32)
            self.rep_pos = (self.rep_pos + self.n_rep) % self.es.n
            of = {}
            for t, e in T.L.items():
                of.setdefault(e[0], []).append(t)
            everything = list(T.L)
            off = [0]
            for s in rs.tolist():
                mine = of.get(s, [])
                mode = rng.integers(3)  # all, some, none of its grants
                lst = mine if mode == 0 else [t for t in mine if rng.random() < 0.5] if mode == 1 else []
                if rng.random() < 0.3 and everything:  # foreign and invented ids
                    lst = lst + [everything[rng.integers(len(everything))], int(ahead[0])]
                    if self.gone:
                        lst.append(self.gone[rng.integers(len(self.gone))])
                rid += lst
                off.append(len(rid))
            off = np.array(off, np.uint32)
        return {"now": now, "upd_idx": who, "upd_rows": rows, "release_idx": rel.astype(np.uint32), "tasks": tk,
                "lease_expires_at": (now + rng.choice(LEASE_STEPS, n)).astype(np.int64),
                "renew_ids": ren, "renew_expires_at": (now + rng.choice(LEASE_STEPS, len(ren))).astype(np.int64),
                "free_ids": fr, "report_servants": rs, "report_off": off, "report_ids": np.array(rid, np.uint64)}

    def commit(self, before, out):
        """After the tick: which ids left the table (they are unknown from now on). The grants are in
        es.running already (the table's tick counted the frees, this adds the grants)."""
        self.es.commit(np.asarray(out, np.uint32))
        left = [t for t in before if t not in self.table.L]
        self.gone = (self.gone + left)[-400:]


def oracle_place(es):
    """The model's placement: the plain-C oracle on the stream's registry as it is now."""
    return lambda batch: O.dispatch(es.registry_snapshot(), batch, "sorted", want_util=False)[0]


def model_tick(ls, ev, place=None):
    """One tick of the model on the stream's table; feeds the answers back. -> dict of FIELDS."""
    before = set(ls.table.L)
    r = ls.table.tick(ls.es.running, ev, place or oracle_place(ls.es))
    ls.commit(before, r["out"])
    r["running"] = ls.es.running.astype(np.uint32)
    return r


def run_model(sv, tasks, frees, renewals, ticks, n_envs=1, seed=83, max_leases=1 << 30):
    ls = LeaseStream(sv, tasks, frees, renewals, LeaseTable(max_leases), n_envs=n_envs, seed=seed)
    return [model_tick(ls, ls.next_tick()) for _ in range(ticks)]


def hash_u64(a):
    return synth.placement_hash(np.ascontiguousarray(a, dtype=np.uint64).view(np.uint32))


def digests(rec):
    """Per-tick digests and counts of a record (the fixture's columns)."""
    d = {
        "digest": np.array([synth.placement_hash(r["out"]) for r in rec], np.uint64),
        "id_digest": np.array([hash_u64(r["task_id"][r["out"] < IDX_ENV_NOT_FOUND]) for r in rec], np.uint64),
        "renewed_digest": np.array([synth.placement_hash(r["renewed"]) for r in rec], np.uint64),
        "unknown_digest": np.array([synth.placement_hash(r["report_unknown"]) for r in rec], np.uint64),
        "run_digest": np.array([synth.placement_hash(r["running"]) for r in rec], np.uint64),
    }
    for k in FIELDS[5:]:
        d[k] = np.array([r[k] for r in rec], np.uint32)
    return d


def check_conditions(d):
    """What a lease stream must contain to prove anything (asserted by the fixture's generator and
    by the test that loads it)."""
    for k in ("expired", "swept", "renew_refused", "unknown_reported", "ignored_frees", "timeouts"):
        assert int(d[k].sum()) > 0, "the stream has no %s" % k
    assert int(d["kept_zombies"].max()) > 0, "no zombie ever survives because its servant did not report"


def location(sv, s):
    ip, port = int(sv["ip"][s]), int(sv["port"][s])
    return "%u.%u.%u.%u:%u" % (ip >> 24, (ip >> 16) & 255, (ip >> 8) & 255, ip & 255, port)


class ReferenceReplay:
    """One GIVEN tick at a time through the VERBATIM reference class (oracle/_ref), one clock unit =
    1 ms: clock to `now`, heartbeats as KeepServantAlive, renewals as KeepTaskAlive, frees as
    FreeTask, fire_timers (OnExpirationTimer), reports as NotifyServantRunningTasks, the batch as
    sequential WaitForStartingNewTask calls. Servants live 30 s there and a run's clock stays far
    below 30000, so the timer removes none. refbind's batch call grants with a fixed lease; each
    grant's own expiry is set right behind it with KeepTaskAlive. `ls`: the stream the ticks come
    from (drawn by it or written by hand on top of its heartbeats and requests); its table is the
    shadow that follows the reference's placement. Every recorded field is the reference's own
    answer (running_tasks from DumpInternals); the counts it does not report are the shadow's."""

    def __init__(self, ls):
        from oracle import refbind as R
        self.R, self.ls = R, ls
        sv = ls.es.sv
        self.ref = R.RefDispatcher()
        self.ref.load_servants(sv)
        self.base = int(np.asarray(sv["running_tasks"], np.int64).sum())  # ids the priming grants took
        self.loc = [location(sv, s) for s in range(ls.es.n)]
        self.row_of = {l: s for s, l in enumerate(self.loc)}
        self.clock = None

    def close(self):
        self.ref.close()

    def _id(self, t):
        """A task id of the stream as the reference numbers it (ids are 64 bit there too)."""
        return (int(t) + self.base) & NO_ID

    def tick(self, ev):
        """-> dict of FIELDS, as model_tick."""
        ref, ls, es = self.ref, self.ls, self.ls.es
        now = int(ev["now"])
        if self.clock is not None and now > self.clock:
            self.R.clock_advance_ms(now - self.clock)
        self.clock = now
        hb = {k: v[ev["upd_idx"]] for k, v in es.sv.items()}
        hb["running_tasks"] = np.zeros(len(ev["upd_idx"]), np.uint32)  # (kept by a renewal anyway)
        ref.load_servants(hb)
        renewed = np.array([ref.keep_task_alive(self._id(t), int(e) - now)
                            for t, e in zip(ev["renew_ids"], ev["renew_expires_at"])], np.uint8)
        for t in ev["free_ids"].tolist():
            ref.free_task(self._id(t))
        self.R.fire_timers()
        unknown = np.zeros(len(ev["report_ids"]), np.uint8)
        off = ev["report_off"]
        for r, s in enumerate(ev["report_servants"].tolist()):
            listed = ev["report_ids"][off[r]:off[r + 1]].tolist()
            unk = set(ref.notify_servant_running_tasks(
                self.loc[s], np.array([self._id(t) for t in listed], np.uint64)))
            unknown[off[r]:off[r + 1]] = [self._id(t) in unk for t in listed]
        got = {}

        def place(batch):
            ridx, rids, _, _ = ref.dispatch_batch(batch)
            got["ids"] = rids
            return ridx

        before = set(ls.table.L)
        r = ls.table.tick(es.running, ev, place)
        ls.commit(before, r["out"])
        granted = r["out"] < IDX_ENV_NOT_FOUND
        ids = np.full(len(granted), NO_ID, np.uint64)
        if granted.any():
            ids[granted] = got["ids"][granted] - np.uint64(self.base)
            for t, e in zip(got["ids"][granted].tolist(), ev["lease_expires_at"][granted].tolist()):
                assert ref.keep_task_alive(t, e - now)
        dump = ref.dump_internals()
        running = np.zeros(es.n, np.uint32)
        for s in dump["servants"]:
            running[self.row_of[s["location"]]] = s["running_tasks"]
        r.update(task_id=ids, renewed=renewed, report_unknown=unknown, running=running,
                 renew_refused=int((renewed == 0).sum()), unknown_reported=int(unknown.sum()))
        return r


def run_reference(sv, tasks, frees, renewals, ticks, n_envs=1, seed=83):
    """The seeded stream of run_model through ReferenceReplay: the traffic is drawn from the shadow
    table. Same record as run_model."""
    ls = LeaseStream(sv, tasks, frees, renewals, LeaseTable(), n_envs=n_envs, seed=seed)
    ref = ReferenceReplay(ls)
    try:
        return [ref.tick(ls.next_tick()) for _ in range(ticks)]
    finally:
        ref.close()

"""Waiting queue and lease table in one streaming context, as a plain model (the yardstick of the
waiting + leased tests). It COMPOSES tests/stream_wait_model.WaitQueue and
tests/stream_lease_model.LeaseTable, neither of which is edited.

One tick with clock `now` (include/yadcc_dispatch.h, ydc_stream_tick_waiting_leased):
  1. - 6. steps 1 - 6 of a leased tick (heartbeats, renewals, frees by id, releases, expiry, reports);
  7. every entry of W with deadline <= now resolves as Timeout without being tried;
  8. the rest of W in queue order, then the new requests, are placed as ONE batch of sequential
     WaitForStartingNewTask calls; a Timeout with a deadline ahead stays in / joins W;
  9. every grant of the batch, the queue's first, takes next_id++ and its lease runs from the
     grant: expires_at = now + lease_for of that request (W carries the duration).

A stream is LeaseStream (heartbeats, requests, seeded lease traffic; lease_for = its drawn expiry -
now, one of LEASE_STEPS) plus the deadlines and tags of a WaitingStream, and a request rate that
alternates so that the pool is saturated part of the time and roomy part of the time.

`place` decides a batch: the plain-C oracle for the model; ReferenceReplay puts one given tick at
a time through the verbatim reference class (oracle.refbind): the batch as sequential
WaitForStartingNewTask calls, each grant's expiry set right behind it with
keep_task_alive(id, lease_for) at clock `now`.
"""
import numpy as np

from tests import stream_lease_model as L
from tests import stream_wait_model as W
from yadcc_amd import synth

IDX_TIMEOUT, IDX_ENV_NOT_FOUND, IDX_WAITING = W.IDX_TIMEOUT, W.IDX_ENV_NOT_FOUND, W.IDX_WAITING
NO_ID = L.NO_ID
# Per tick, beside stream_lease_model.FIELDS: the resolved list, |W|, and what the tick proves.
FIELDS = L.FIELDS + ("res_tags", "res_idx", "res_ids", "n_waiting", "w_granted", "w_expired", "joined",
                     "new_granted", "w_zombies")
COUNTS = L.FIELDS[5:] + FIELDS[len(L.FIELDS) + 3:]


class WaitLeaseState:
    """W (with its lease_for column), L and next_id; one tick of steps 2 - 9."""

    def __init__(self, max_waiting, max_leases=1 << 30):
        self.max_waiting, self.max_leases = max_waiting, max_leases
        self.q = W.WaitQueue(max_waiting)
        self.lease_for = np.empty(0, np.int64)  # W's sixth column
        self.T = L.LeaseTable(max_leases)
        self.from_w = set()  # ids granted to queue entries (for w_zombies)

    def check(self, n_tasks, now):
        """The refusals that leave everything untouched."""
        if len(self.q) + n_tasks > self.max_waiting:
            raise OverflowError("max_waiting")
        if len(self.T) + len(self.q) + n_tasks > self.max_leases:
            raise OverflowError("max_leases")  # (every waiting entry may be granted in this tick)
        self.T.check(0, now)

    def tick(self, running, ev, place):
        """ev: a leased tick's columns with lease_for, deadlines and tags in place of
        lease_expires_at. place(batch) -> servant index per request of the batch (live queue ++ new).
        -> dict of FIELDS (without "running"), plus "got": the batch's placement."""
        now = int(ev["now"])
        new = {k: np.asarray(v, np.uint32) for k, v in ev["tasks"].items()}
        n = len(new["env_id"])
        self.check(n, now)
        q, T = self.q, self.T
        live = q.deadline > now
        n_live, n_before = int(live.sum()), len(q)
        lease_for = np.asarray(ev["lease_for"], np.int64)
        batch_for = np.concatenate([self.lease_for[live], lease_for])
        zombie_before = {t for t, e in T.L.items() if e[2]}
        box = {}

        def place_batch(_):
            def guarded(batch):
                return place(batch) if len(batch["env_id"]) else np.empty(0, np.uint32)
            box["q"] = q.tick(guarded, new, ev["deadlines"], ev["tags"], now)
            return box["q"][4]

        # The lease table sees the whole batch as its tick's requests, each with the expiry its
        # grant would get NOW; the queue's tick runs where the table places them (after steps 2 - 6).
        z = np.zeros(n_live + n, np.uint32)
        ev2 = dict(ev, tasks={"env_id": z, "min_version": z, "requestor_ip": z}, lease_expires_at=now + batch_for)
        r = T.tick(running, ev2, place_batch)
        if "q" not in box:  # (an empty batch: the table asked for no placement; W's expiries remain)
            place_batch(None)
        out, res_tags, res_idx, n_waiting, got = box["q"]
        ids = r["task_id"]
        # The queue's answers and ids at their queue positions, as WaitQueue.tick resolves them.
        wans = np.full(n_before, IDX_TIMEOUT, np.uint32)
        wans[live] = got[:n_live]
        wids = np.full(n_before, NO_ID, np.uint64)
        wids[live] = ids[:n_live]
        resolved = ~live | (wans != IDX_TIMEOUT)
        assert np.array_equal(wans[resolved], res_idx)
        join = (got[n_live:] == IDX_TIMEOUT) & (np.asarray(ev["deadlines"], np.int64) > now)
        self.lease_for = np.concatenate([self.lease_for[~resolved], lease_for[join]])
        assert len(self.lease_for) == len(q) == n_waiting
        w_granted = wids[resolved][res_idx < IDX_ENV_NOT_FOUND]
        self.from_w.update(w_granted.tolist())
        self.from_w &= set(T.L)
        r.update(out=out, task_id=ids[n_live:], got=got, res_tags=res_tags, res_idx=res_idx, res_ids=wids[resolved],
                 n_waiting=n_waiting, w_granted=len(w_granted), w_expired=int((~live).sum()), joined=int(join.sum()),
                 new_granted=int((out < IDX_WAITING).sum()),
                 w_zombies=sum(1 for t in self.from_w if T.L[t][2] and t not in zombie_before))
        return r

    def take(self):
        self.lease_for = self.lease_for[:0]
        return self.q.take()


def saturate_then_relax(now):
    """Share of the drawn requests a tick keeps: 24 full ticks, 12 ticks at an eighth, and so on."""
    return 1.0 if now % 36 < 24 else 0.125


class WaitLeaseStream(L.LeaseStream):
    """LeaseStream whose requests carry lease_for, deadlines and tags; `state`: the WaitLeaseState the
    caller advances with every tick's answers (its table is where the lease traffic is drawn from)."""

    def __init__(self, sv, tasks_per_tick, frees_per_tick, renewals_per_tick, state, n_envs=1, seed=83, wait_seed=71,
                 rate=saturate_then_relax, report_frac=0.10):
        super().__init__(sv, tasks_per_tick, frees_per_tick, renewals_per_tick, state.T, n_envs=n_envs, seed=seed,
                         report_frac=report_frac)
        self.state, self.rate = state, rate
        self.wrng = np.random.default_rng(wait_seed)
        self.next_tag = 1

    def next_tick(self):
        ev = super().next_tick()
        now = int(ev["now"])
        n = int(len(ev["tasks"]["env_id"]) * self.rate(now))
        n = min(n, self.state.max_waiting - len(self.state.q))  # (a host keeps |W| + n <= max_waiting)
        ev["tasks"] = {k: v[:n] for k, v in ev["tasks"].items()}
        ev["lease_for"] = (ev.pop("lease_expires_at")[:n] - now).astype(np.int64)
        ev["deadlines"] = (now + self.wrng.choice(W.DEADLINE_STEPS, n)).astype(np.int64)
        ev["tags"] = np.arange(self.next_tag, self.next_tag + n, dtype=np.uint64)
        self.next_tag += n
        return ev


def new_stream(sv, tasks, frees, renewals, max_waiting, n_envs=1, max_leases=1 << 30, **kw):
    return WaitLeaseStream(sv, tasks, frees, renewals, WaitLeaseState(max_waiting, max_leases), n_envs=n_envs, **kw)


def model_tick(ws, ev, place=None):
    """One tick of the model on the stream's state; feeds the answers back. -> dict of FIELDS."""
    before = set(ws.table.L)
    r = ws.state.tick(ws.es.running, ev, place or L.oracle_place(ws.es))
    ws.commit(before, r.pop("got"))
    r["running"] = ws.es.running.astype(np.uint32)
    return r


def run_model(sv, tasks, frees, renewals, ticks, max_waiting, n_envs=1):
    ws = new_stream(sv, tasks, frees, renewals, max_waiting, n_envs=n_envs)
    return [model_tick(ws, ws.next_tick()) for _ in range(ticks)]


def digests(rec):
    """Per-tick digests and counts of a record (the fixture's columns)."""
    h, h64 = synth.placement_hash, L.hash_u64
    d = {
        "digest": np.array([h(r["out"]) for r in rec], np.uint64),
        "id_digest": np.array([h64(r["task_id"][r["out"] < IDX_WAITING]) for r in rec], np.uint64),
        "res_tag_digest": np.array([h64(r["res_tags"]) for r in rec], np.uint64),
        "res_idx_digest": np.array([h(r["res_idx"]) for r in rec], np.uint64),
        "res_id_digest": np.array([h64(r["res_ids"][r["res_idx"] < IDX_ENV_NOT_FOUND]) for r in rec], np.uint64),
        "renewed_digest": np.array([h(r["renewed"]) for r in rec], np.uint64),
        "unknown_digest": np.array([h(r["report_unknown"]) for r in rec], np.uint64),
        "run_digest": np.array([h(r["running"]) for r in rec], np.uint64),
        "n_resolved": np.array([len(r["res_tags"]) for r in rec], np.uint32),
    }
    for k in COUNTS:
        d[k] = np.array([r[k] for r in rec], np.uint32)
    return d


def check_conditions(d):
    """What a stream must contain to prove anything (asserted by the fixture's generator and by
    every test that loads it), each total > 0 over the run."""
    for k in ("w_granted", "w_expired", "joined", "expired", "swept", "freed", "renew_refused", "w_zombies"):
        assert int(np.asarray(d[k]).sum()) > 0, "the stream has no %s" % k
    both = (np.asarray(d["w_granted"]) > 0) & (np.asarray(d["new_granted"]) > 0)
    assert both.any(), "no tick grants in both regions of the batch"
    nw = np.asarray(d["n_waiting"])
    assert (nw > 0).any() and (nw == 0).any(), "the pool is never saturated, or never roomy"


class ReferenceReplay(L.ReferenceReplay):
    """stream_lease_model.ReferenceReplay with a tick of this mode: steps 1 - 6 as there; the batch
    (live queue ++ new requests, kept from the reference's own answers) as sequential
    WaitForStartingNewTask calls; each grant's expiry set right behind it with
    keep_task_alive(id, lease_for) at clock `now`. `ws`: the WaitLeaseStream; its state is the
    shadow that follows the reference's placement."""

    def tick(self, ev):
        ref, ws, es = self.ref, self.ls, self.ls.es
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
        live = ws.state.q.deadline > now
        batch_for = np.concatenate([ws.state.lease_for[live], np.asarray(ev["lease_for"], np.int64)])
        seen = {}

        def place(batch):
            ridx, rids, _, _ = ref.dispatch_batch(batch)
            g = ridx < IDX_ENV_NOT_FOUND
            for t, d in zip(rids[g].tolist(), batch_for[g].tolist()):
                assert ref.keep_task_alive(t, d)
            seen["ids"], seen["granted"] = rids, g
            return ridx

        before = set(ws.table.L)
        r = ws.state.tick(es.running, ev, place)
        got = r.pop("got")
        ws.commit(before, got)
        if "ids" in seen:  # the reference's own ids in place of the shadow's
            ids = np.full(len(got), NO_ID, np.uint64)
            ids[seen["granted"]] = seen["ids"][seen["granted"]] - np.uint64(self.base)
            n_live = int(live.sum())
            wids = np.full(len(live), NO_ID, np.uint64)
            wids[live] = ids[:n_live]
            wans = np.full(len(live), IDX_TIMEOUT, np.uint32)
            wans[live] = got[:n_live]
            r.update(task_id=ids[n_live:], res_ids=wids[~live | (wans != IDX_TIMEOUT)])
        dump = ref.dump_internals()
        running = np.zeros(es.n, np.uint32)
        for s in dump["servants"]:
            running[self.row_of[s["location"]]] = s["running_tasks"]
        r.update(renewed=renewed, report_unknown=unknown, running=running,
                 renew_refused=int((renewed == 0).sum()), unknown_reported=int(unknown.sum()))
        return r


def run_reference(sv, tasks, frees, renewals, ticks, max_waiting, n_envs=1):
    """The seeded stream of run_model through ReferenceReplay. Same record as run_model."""
    ws = new_stream(sv, tasks, frees, renewals, max_waiting, n_envs=n_envs)
    ref = ReferenceReplay(ws)
    try:
        return [ref.tick(ws.next_tick()) for _ in range(ticks)]
    finally:
        ref.close()

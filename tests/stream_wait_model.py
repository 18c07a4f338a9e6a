"""The streaming waiting mode's semantics as a plain model (the yardstick of the waiting tests).

A waiting stream is yadcc_amd.streaming.EventStream plus, per request, a deadline and a tag: the
clock is the tick number, a request's deadline is now + one of DEADLINE_STEPS (seeded), its tag a
running counter. A host never sends more new requests than the queue has room for
(|W| + n <= max_waiting): it keeps the first max_waiting - |W| of the tick's requests.

One tick (include/yadcc_dispatch.h, ydc_stream_tick_waiting): heartbeats, frees; every waiting
entry whose deadline has passed (deadline <= now) resolves as Timeout; the rest of the queue in
order, then the new requests, are placed as ONE batch of sequential WaitForStartingNewTask calls
(timeout == now). Waiting entries granted or EnvironmentNotFound resolve, their Timeouts stay; new
requests answer as in a plain tick except that a Timeout with a deadline ahead is IDX_WAITING and
joins the queue.

`place` is what decides a batch: the plain-C oracle (oracle.oraclebind.dispatch, on the stream's
registry snapshot) for the model, the verbatim reference class (oracle.refbind) for the replay in
tests/golden/make_stream_wait_golden.py. Both feed the stream their own answers.
"""
import numpy as np

from oracle import oraclebind as O
from yadcc_amd import streaming, synth

IDX_TIMEOUT = 0xFFFFFFFF
IDX_ENV_NOT_FOUND = 0xFFFFFFFE
IDX_WAITING = 0xFFFFFFFD
DEADLINE_STEPS = np.array([0, 1, 2, 5, 40], np.int64)


class WaitingStream:
    """EventStream with deadlines and tags; the clock is the tick number."""

    def __init__(self, sv, tasks_per_tick, frees_per_tick, max_waiting, n_envs=1, seed=71):
        self.es = streaming.EventStream(sv, tasks_per_tick, frees_per_tick, n_envs=n_envs)
        self.max_waiting = max_waiting
        self.rng = np.random.default_rng(seed)
        self.next_tag = 1
        self.n_waiting = 0  # |W| as the last tick left it (the host's bookkeeping)

    def next_tick(self):
        """-> (now, upd_idx, upd_rows, release_idx, tasks, deadlines, tags)."""
        now = self.es.tick_no
        who, rows, rel, tk = self.es.next_tick()
        n = min(len(tk["env_id"]), self.max_waiting - self.n_waiting)
        tk = {k: v[:n] for k, v in tk.items()}
        deadlines = now + self.rng.choice(DEADLINE_STEPS, n)
        tags = np.arange(self.next_tag, self.next_tag + n, dtype=np.uint64)
        self.next_tag += n
        return now, who, rows, rel, tk, deadlines.astype(np.int64), tags

    def commit(self, out, resolved_idx, n_waiting):
        """Feeds a tick's answers back: the grants of the queue (queue order), then the new ones."""
        v = np.concatenate([np.asarray(resolved_idx, np.uint32), np.asarray(out, np.uint32)])
        self.es.commit(v[v < IDX_WAITING])
        self.n_waiting = n_waiting


class WaitQueue:
    """W and one tick of the semantics; `place(batch) -> servant index per request` decides."""

    def __init__(self, max_waiting):
        self.max_waiting = max_waiting
        self.cols = {k: np.empty(0, np.uint32) for k in ("env_id", "min_version", "requestor_ip")}
        self.deadline = np.empty(0, np.int64)
        self.tag = np.empty(0, np.uint64)
        self.last_now = None

    def __len__(self):
        return len(self.tag)

    def tick(self, place, tasks, deadlines, tags, now):
        """-> (out, resolved_tags, resolved_idx, n_waiting, batch_placement)."""
        n = len(tasks["env_id"])
        if len(self) + n > self.max_waiting:
            raise OverflowError("capacity")
        if self.last_now is not None and now < self.last_now:
            raise ValueError("now goes backwards")
        self.last_now = now
        live = self.deadline > now
        batch = {k: np.concatenate([self.cols[k][live], np.asarray(tasks[k], np.uint32)]) for k in self.cols}
        got = np.asarray(place(batch), np.uint32)
        n_live = int(live.sum())
        gw, gn = got[:n_live], got[n_live:]
        # The queue's answers at their queue positions (expired: Timeout without a try).
        wans = np.full(len(self), IDX_TIMEOUT, np.uint32)
        wans[live] = gw
        resolved = ~live | (wans != IDX_TIMEOUT)
        stay = ~resolved
        deadlines = np.asarray(deadlines, np.int64)
        join = (gn == IDX_TIMEOUT) & (deadlines > now)
        out = np.where(join, np.uint32(IDX_WAITING), gn).astype(np.uint32)
        res_tags, res_idx = self.tag[resolved], wans[resolved]
        for k in self.cols:
            self.cols[k] = np.concatenate([self.cols[k][stay], np.asarray(tasks[k], np.uint32)[join]])
        self.deadline = np.concatenate([self.deadline[stay], deadlines[join]])
        self.tag = np.concatenate([self.tag[stay], np.asarray(tags, np.uint64)[join]])
        return out, res_tags, res_idx, len(self), got

    def take(self):
        t = self.tag.copy()
        for k in self.cols:
            self.cols[k] = self.cols[k][:0]
        self.deadline, self.tag = self.deadline[:0], self.tag[:0]
        return t


def oracle_place(es):
    """The model's placement: the plain-C oracle on the stream's registry as it is now."""
    return lambda batch: O.dispatch(es.registry_snapshot(), batch, "sorted", want_util=False)[0]


def hash_u64(a):
    return synth.placement_hash(np.ascontiguousarray(a, dtype=np.uint64).view(np.uint32))


def run_model(sv, tasks_per_tick, frees_per_tick, ticks, max_waiting, n_envs=1, seed=71):
    """The model over a whole waiting stream: per tick (out, resolved_tags, resolved_idx,
    n_waiting, running after the tick)."""
    ws = WaitingStream(sv, tasks_per_tick, frees_per_tick, max_waiting, n_envs=n_envs, seed=seed)
    q = WaitQueue(max_waiting)
    rec = []
    for _ in range(ticks):
        now, who, rows, rel, tk, dl, tags = ws.next_tick()
        out, rt, ri, nw, _ = q.tick(oracle_place(ws.es), tk, dl, tags, now)
        ws.commit(out, ri, nw)
        rec.append((out, rt, ri, nw, ws.es.running.astype(np.uint32)))
    return rec


def digests(rec):
    """Per-tick digests of run_model's record (the fixture's columns)."""
    return {
        "digest": np.array([synth.placement_hash(r[0]) for r in rec], np.uint64),
        "res_tag_digest": np.array([hash_u64(r[1]) for r in rec], np.uint64),
        "res_idx_digest": np.array([synth.placement_hash(r[2]) for r in rec], np.uint64),
        "n_resolved": np.array([len(r[1]) for r in rec], np.uint32),
        "n_waiting": np.array([r[3] for r in rec], np.uint32),
        "run_digest": np.array([synth.placement_hash(r[4]) for r in rec], np.uint64),
    }


def run_reference(sv, tasks_per_tick, frees_per_tick, ticks, max_waiting, n_envs=1, seed=71):
    """The same stream through the VERBATIM reference class (oracle/_ref): heartbeats as
    KeepServantAlive, frees by grant id, every batch (live queue ++ new requests) as sequential
    WaitForStartingNewTask calls; the queue kept from the reference's own answers. Same record
    as run_model."""
    from oracle import refbind as R
    ws = WaitingStream(sv, tasks_per_tick, frees_per_tick, max_waiting, n_envs=n_envs, seed=seed)
    es = ws.es
    q = WaitQueue(max_waiting)
    ref = R.RefDispatcher()
    ref.load_servants(sv)
    ref_ids = np.empty(0, np.uint64)  # grant id of every live grant, in es.live's order
    rec = []
    try:
        for _ in range(ticks):
            now, who, rows, rel, tk, dl, tags = ws.next_tick()
            hb = {k: v[who] for k, v in es.sv.items()}
            hb["running_tasks"] = np.zeros(len(who), np.uint32)  # (kept by a renewal anyway)
            ref.load_servants(hb)
            ref.free_tasks(ref_ids[es.last_freed])
            ref_ids = ref_ids[es.last_kept]
            ids = []

            def place(batch):
                ridx, rids, _, _ = ref.dispatch_batch(batch)
                ids.append(rids)
                return ridx

            out, rt, ri, nw, got = q.tick(place, tk, dl, tags, now)
            ref_ids = np.concatenate([ref_ids, ids[0][got < IDX_ENV_NOT_FOUND]])
            ws.commit(out, ri, nw)
            rec.append((out, rt, ri, nw, es.running.astype(np.uint32)))
    finally:
        ref.close()
    return rec

"""One request row per WaitForStartingTask RPC, as a plain model (the yardstick of the rpc stream
tests). It COMPOSES tests/stream_wait_lease_model.WaitLeaseState (its lease table and next_id; its
streams) and a `place` function; neither is edited.

A request is (env_id, min_version, requestor_ip, n_immediate, n_prefetch, lease_for, deadline, tag);
rows = n_immediate + n_prefetch, rows == 0 is refused. One tick with clock `now`
(include/yadcc_dispatch.h, ydc_stream_tick_rpc):
  1. - 6. steps 1 - 6 of a leased tick;
  7. every entry of W with deadline <= now resolves as Timeout, untried, with 0 grants;
  8. the rest of W in queue order, then the new requests, each expand into `rows` identical batch
     rows; the expansion is placed as ONE batch. Nothing frees between identical consecutive rows,
     so a request's granted rows are a prefix of its rows (asserted here);
  9. granted rows in batch order take next_id++, expires_at = now + lease_for.
A request with g granted rows: g > 0 granted; g == 0 and EnvironmentNotFound: ENV_NOT_FOUND if
n_immediate > 0 else TIMEOUT; g == 0, Timeout: WAITING as ONE entry of W while deadline > now, else
TIMEOUT.

ReferenceReplay puts a tick through the verbatim reference class: steps 1 - 6 as
stream_lease_model.ReferenceReplay, then per RPC the handler's two loops
(scheduler_service_impl.cc:233-264) literally: the breaks, the `i == 0 ? max_wait : 0` deadline and
the `grants().empty()` deadline of the prefetch loop, on the fake clock (a wait that would block is
an immediate timeout there).
"""
import numpy as np

from tests import stream_lease_model as L
from tests import stream_wait_lease_model as WL
from yadcc_amd import synth

IDX_TIMEOUT, IDX_ENV_NOT_FOUND, IDX_WAITING = WL.IDX_TIMEOUT, WL.IDX_ENV_NOT_FOUND, WL.IDX_WAITING
NO_ID = L.NO_ID
COLS = ("env_id", "min_version", "requestor_ip")
# Per tick. servants / task_ids: the granted rows of the new requests, request by request (packed);
# res_servants / res_task_ids: those of the resolved entries of W, entry by entry.
LISTS = ("status", "n_granted", "servants", "task_ids", "renewed", "report_unknown", "running", "res_tags",
         "res_status", "res_n_granted", "res_first", "res_servants", "res_task_ids")
COUNTS = ("n_leases", "expired", "swept", "freed", "renew_refused", "n_waiting", "n_waiting_rows", "partial",
          "w_granted", "w_expired", "joined", "env_failed", "no_quota_unknown")
FIELDS = LISTS + COUNTS
NIMM = np.array([0, 1, 1, 1, 2, 3], np.uint32)
NPRE = np.array([0, 0, 1, 2, 4], np.uint32)


class RpcQueue:
    """W: one entry per blocked RPC."""

    def __init__(self):
        self.cols = {k: np.empty(0, np.uint32) for k in COLS + ("n_imm", "n_pre")}
        self.lease_for = np.empty(0, np.int64)
        self.deadline = np.empty(0, np.int64)
        self.tag = np.empty(0, np.uint64)

    def __len__(self):
        return len(self.tag)

    def rows(self):
        return int(self.cols["n_imm"].sum()) + int(self.cols["n_pre"].sum())


class RpcState:
    """W, L and next_id; one tick of steps 2 - 9."""

    def __init__(self, max_waiting, max_rows, max_leases=1 << 30):
        self.max_waiting, self.max_rows, self.max_leases = max_waiting, max_rows, max_leases
        self.S = WL.WaitLeaseState(max_waiting, max_leases)  # (its queue stays empty: W holds RPCs here)
        self.T = self.S.T
        self.q = RpcQueue()

    def check(self, n_imm, n_pre, now):
        """The refusals that leave everything untouched."""
        rows = n_imm.astype(np.int64) + n_pre
        if len(self.q) + len(rows) > self.max_waiting:
            raise OverflowError("max_waiting")
        if (rows == 0).any():
            raise ValueError("rows == 0")
        if self.q.rows() + int(rows.sum()) > self.max_rows:
            raise OverflowError("max_rows")
        if len(self.T) + self.q.rows() + int(rows.sum()) > self.max_leases:
            raise OverflowError("max_leases")
        self.T.check(0, now)

    def tick(self, running, ev, place):
        """ev: a waiting + leased tick's columns (tasks: one row per RPC) plus n_immediate and
        n_prefetch. place(batch) -> servant index per row of the expanded batch.
        -> dict of FIELDS (without "running"), plus "got": the batch's placement."""
        now = int(ev["now"])
        q, T = self.q, self.T
        new = {k: np.asarray(ev["tasks"][k], np.uint32) for k in COLS}
        new["n_imm"], new["n_pre"] = np.asarray(ev["n_immediate"], np.uint32), np.asarray(ev["n_prefetch"], np.uint32)
        n = len(new["env_id"])
        self.check(new["n_imm"], new["n_pre"], now)
        live = q.deadline > now
        n_live, n_before = int(live.sum()), len(q)
        pos = {k: np.concatenate([q.cols[k][live], new[k]]) for k in new}
        pos_for = np.concatenate([q.lease_for[live], np.asarray(ev["lease_for"], np.int64)])
        pos_dl = np.concatenate([q.deadline[live], np.asarray(ev["deadlines"], np.int64)])
        pos_tag = np.concatenate([q.tag[live], np.asarray(ev["tags"], np.uint64)])
        rows = (pos["n_imm"].astype(np.int64) + pos["n_pre"])
        start = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        batch = {k: np.repeat(pos[k], rows) for k in COLS}
        ev2 = dict(ev, tasks=batch, lease_expires_at=now + np.repeat(pos_for, rows))
        r = T.tick(running, ev2, place)
        got, ids = r["out"], r["task_id"]
        granted = got < IDX_ENV_NOT_FOUND
        rank = np.concatenate([[0], np.cumsum(granted)]).astype(np.int64)
        g = rank[start[1:]] - rank[start[:-1]]
        for a, k in zip(start[:-1].tolist(), g.tolist()):  # the handler's break changes nothing
            assert granted[a:a + k].all(), "a request's granted rows are not a prefix of its rows"
        first = got[start[:-1]]  # (every position has rows: rows == 0 is refused)
        status = np.where(g > 0, 0, np.where(first == IDX_ENV_NOT_FOUND,
                                             np.where(pos["n_imm"] > 0, IDX_ENV_NOT_FOUND, IDX_TIMEOUT),
                                             np.where(pos_dl > now, IDX_WAITING, IDX_TIMEOUT))).astype(np.uint32)
        stay = status == IDX_WAITING
        # W's entries at their queue positions (expired: Timeout, untried).
        wst = np.full(n_before, IDX_TIMEOUT, np.uint32)
        wst[live] = status[:n_live]
        wg, wfirst = np.zeros(n_before, np.uint32), np.zeros(n_before, np.uint32)
        wg[live] = g[:n_live]
        wfirst[live] = rank[start[:n_live]]
        # (an expired entry's `first` is the grant rank at its place in the queue)
        wfirst[~live] = rank[start[np.searchsorted(np.nonzero(live)[0], np.nonzero(~live)[0])]]
        resolved = wst != IDX_WAITING
        w_rows_gr = rank[start[n_live]]

        def packed(a, lo, hi):
            return np.concatenate([a[start[i]:start[i] + g[i]] for i in range(lo, hi)] or [a[:0]])
        rec = {"status": status[n_live:], "n_granted": g[n_live:].astype(np.uint32),
               "servants": packed(got, n_live, n_live + n), "task_ids": packed(ids, n_live, n_live + n),
               "res_tags": q.tag[resolved], "res_status": wst[resolved], "res_n_granted": wg[resolved],
               "res_first": wfirst[resolved], "res_servants": got[:start[n_live]][granted[:start[n_live]]],
               "res_task_ids": ids[:start[n_live]][granted[:start[n_live]]]}
        assert len(rec["res_servants"]) == w_rows_gr
        keep = np.zeros(n_before, bool)
        keep[live] = stay[:n_live]
        join = stay[n_live:]
        for k in q.cols:
            q.cols[k] = np.concatenate([q.cols[k][keep], new[k][join]])
        q.lease_for = np.concatenate([q.lease_for[keep], np.asarray(ev["lease_for"], np.int64)[join]])
        q.deadline = np.concatenate([q.deadline[keep], np.asarray(ev["deadlines"], np.int64)[join]])
        q.tag = np.concatenate([q.tag[keep], np.asarray(ev["tags"], np.uint64)[join]])
        enf = (g == 0) & (first == IDX_ENV_NOT_FOUND) & (rows > 0)
        r.update(rec, got=got, n_waiting=len(q), n_waiting_rows=q.rows(),
                 partial=int(((g > 0) & (g < rows)).sum()), w_granted=int((wg > 0).sum()),
                 w_expired=int((~live).sum()), joined=int(join.sum()),
                 env_failed=int((enf & (pos["n_imm"] > 0)).sum()), no_quota_unknown=int((enf & (pos["n_imm"] == 0)).sum()))
        del r["out"], r["task_id"]
        return r

    def take(self):
        t = self.q.tag.copy()
        self.q = RpcQueue()
        return t


class RpcStream(WL.WaitLeaseStream):
    """WaitLeaseStream whose requests are RPCs: seeded counts beside every request, a few of them for
    a digest nobody has, and no more rows than max_rows has room for."""

    def __init__(self, sv, rpcs_per_tick, frees_per_tick, renewals_per_tick, state, rpc_seed=19, unknown_frac=0.03,
                 imm=NIMM, pre=NPRE, **kw):
        super().__init__(sv, rpcs_per_tick, frees_per_tick, renewals_per_tick, state, **kw)
        self.rrng = np.random.default_rng(rpc_seed)
        self.unknown_frac, self.imm, self.pre = unknown_frac, np.asarray(imm, np.uint32), np.asarray(pre, np.uint32)

    def next_tick(self):
        ev = super().next_tick()
        n = len(ev["tags"])
        ni, npf = self.rrng.choice(self.imm, n), self.rrng.choice(self.pre, n)
        npf = np.where(ni + npf == 0, 1, npf).astype(np.uint32)
        unknown = self.rrng.random(n) < self.unknown_frac
        room = self.state.max_rows - self.state.q.rows()  # (a host keeps rows(W) + rows(new) <= max_rows)
        k = int(np.searchsorted(np.cumsum(ni.astype(np.int64) + npf), room, side="right"))
        ev["tasks"] = {c: v[:k].copy() for c, v in ev["tasks"].items()}
        ev["tasks"]["env_id"][unknown[:k]] = 0xFFFF
        for c in ("lease_for", "deadlines", "tags"):
            ev[c] = ev[c][:k]
        ev["n_immediate"], ev["n_prefetch"] = ni[:k], npf[:k]
        return ev


def new_stream(sv, rpcs, frees, renewals, max_waiting, max_rows, n_envs=1, max_leases=1 << 30, **kw):
    return RpcStream(sv, rpcs, frees, renewals, RpcState(max_waiting, max_rows, max_leases), n_envs=n_envs, **kw)


def model_tick(ws, ev, place=None):
    """One tick of the model on the stream's state; feeds the answers back. -> dict of FIELDS."""
    before = set(ws.table.L)
    r = ws.state.tick(ws.es.running, ev, place or L.oracle_place(ws.es))
    ws.commit(before, r.pop("got"))
    r["running"] = ws.es.running.astype(np.uint32)
    return r


def run_model(sv, rpcs, frees, renewals, ticks, max_waiting, max_rows, n_envs=1, **kw):
    ws = new_stream(sv, rpcs, frees, renewals, max_waiting, max_rows, n_envs=n_envs, **kw)
    return [model_tick(ws, ws.next_tick()) for _ in range(ticks)]


def digests(rec):
    """Per-tick digests and counts of a record (the fixture's columns)."""
    h, h64 = synth.placement_hash, L.hash_u64
    d = {k + "_digest": np.array([(h64 if rec[0][k].dtype.itemsize == 8 else h)(r[k]) for r in rec], np.uint64)
         for k in LISTS}
    d["n_resolved"] = np.array([len(r["res_tags"]) for r in rec], np.uint32)
    d["n_requests"] = np.array([len(r["status"]) for r in rec], np.uint32)
    d["timed_out"] = np.array([int((r["res_status"] == IDX_TIMEOUT).sum()) for r in rec], np.uint32)
    for k in COUNTS:
        d[k] = np.array([r[k] for r in rec], np.uint32)
    return d


def shares(d):
    """Of all RPCs of a run: granted partially; waited and later granted; waited and timed out."""
    n = max(int(np.asarray(d["n_requests"]).sum()), 1)
    return (int(np.asarray(d["partial"]).sum()) / n, int(np.asarray(d["w_granted"]).sum()) / n,
            int(np.asarray(d["timed_out"]).sum()) / n)


def check_conditions(d):
    """What a stream must contain to prove anything (asserted on the reference's own record by the
    fixture's generator and by every test that replays one): at least 10 % of the RPCs each are
    granted partially, wait and are granted later, wait and time out."""
    s = shares(d)
    assert min(s) >= 0.10, "shares (partial, waited then granted, waited then timed out): %s" % (s,)
    for k in ("expired", "swept", "freed", "renew_refused", "joined", "env_failed", "no_quota_unknown"):
        assert int(np.asarray(d[k]).sum()) > 0, "the stream has no %s" % k


def cfg5_one_slot():
    """cfg5's 2000 servants with one slot each: a handful of large RPCs per tick saturates the pool,
    so that the shares of check_conditions are met (the full pool has 164 427 slots)."""
    sv, _ = synth.make_config("cfg5")
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 1)
    return sv


def ip_string(ip):
    ip = int(ip)
    return "%u.%u.%u.%u" % (ip >> 24, (ip >> 16) & 255, (ip >> 8) & 255, ip & 255)


class ReferenceReplay(L.ReferenceReplay):
    """stream_lease_model.ReferenceReplay with a tick of this mode. `ws`: the RpcStream; its state is
    the shadow that follows the reference's own answers."""

    def handler(self, ev_now, env, minv, ip, n_imm, n_pre, lease_for, deadline, rows_out, ids_out):
        """scheduler_service_impl.cc:233-264 for one RPC at clock ev_now. Appends one answer per row
        of the RPC (rows the loops never reach: the answer that ended them). -> the RPC's status
        as the handler sets it: "grants", "env_not_available" or "no_quota"; "blocked" where the
        RPC's first call timed out with its deadline ahead: the real call would still be waiting."""
        ref, R = self.ref, self.R
        digest = R.digest_name(env) if env < self.env_bits else "unknown-digest"
        max_wait = deadline - ev_now
        grants, fail, failed_rpc, calls = [], None, None, []
        for i in range(n_imm):
            st, tid, loc = ref.wait_for_starting_new_task(ip_string(ip), digest, minv, expires_in_ms=lease_for,
                                                          timeout_in_ms=max_wait if i == 0 else 0, prefetching=False)
            calls.append((st, max_wait if i == 0 else 0))
            if st != R.OK:
                fail = st
                if st == R.ENV_NOT_FOUND:
                    failed_rpc = "env_not_available"
                break
            grants.append((self.row_of[loc], tid))
        if failed_rpc is None:
            for i in range(n_pre):
                st, tid, loc = ref.wait_for_starting_new_task(ip_string(ip), digest, minv, expires_in_ms=lease_for,
                                                              timeout_in_ms=max_wait if not grants else 0,
                                                              prefetching=True)
                calls.append((st, max_wait if not grants else 0))
                if st != R.OK:
                    fail = st
                    break
                grants.append((self.row_of[loc], tid))
        ans = IDX_ENV_NOT_FOUND if fail == R.ENV_NOT_FOUND else IDX_TIMEOUT
        rows_out += [s for s, _ in grants] + [ans] * (n_imm + n_pre - len(grants))
        ids_out += [t for _, t in grants] + [self.base] * (n_imm + n_pre - len(grants))  # (no id: never read)
        blocked = calls[0][0] == R.TIMEOUT and calls[0][1] > 0
        return failed_rpc or ("grants" if grants else "blocked" if blocked else "no_quota")

    def tick(self, ev):
        ref, ws, es = self.ref, self.ls, self.ls.es
        now = int(ev["now"])
        if self.clock is not None and now > self.clock:
            self.R.clock_advance_ms(now - self.clock)
        self.clock = now
        hb = {k: v[ev["upd_idx"]] for k, v in es.sv.items()}
        hb["running_tasks"] = np.zeros(len(ev["upd_idx"]), np.uint32)  # (kept by a renewal anyway)
        ref.load_servants(hb)
        em = es.sv["env_mask"]
        self.env_bits = 64 * (em.shape[1] if em.ndim == 2 else 1)
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
        q = ws.state.q
        live = q.deadline > now
        new = ev["tasks"]
        pos = [(int(q.cols["env_id"][j]), int(q.cols["min_version"][j]), int(q.cols["requestor_ip"][j]),
                int(q.cols["n_imm"][j]), int(q.cols["n_pre"][j]), int(q.lease_for[j]), int(q.deadline[j]))
               for j in np.nonzero(live)[0].tolist()]
        pos += [(int(new["env_id"][i]), int(new["min_version"][i]), int(new["requestor_ip"][i]),
                 int(ev["n_immediate"][i]), int(ev["n_prefetch"][i]), int(ev["lease_for"][i]), int(ev["deadlines"][i]))
                for i in range(len(ev["tags"]))]
        seen = {}

        def place(batch):
            rows, ids = [], []
            seen["rpc"] = [self.handler(now, *p, rows, ids) for p in pos]
            assert len(rows) == len(batch["env_id"])
            seen["ids"] = np.array(ids, np.uint64) - np.uint64(self.base)
            return np.array(rows, np.uint32)

        before = set(ws.table.L)
        r = ws.state.tick(es.running, ev, place)
        got = r.pop("got")
        ws.commit(before, got)
        if "ids" in seen:  # the reference's own ids and RPC outcomes in place of the shadow's
            n_live = int(live.sum())
            ids, g = seen["ids"], got < IDX_ENV_NOT_FOUND
            rows = np.array([p[3] + p[4] for p in pos], np.int64)
            start = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
            w_end = start[n_live]
            r.update(res_task_ids=ids[:w_end][g[:w_end]], task_ids=ids[w_end:][g[w_end:]])
            mine = np.array([{"grants": 0, "env_not_available": IDX_ENV_NOT_FOUND}.get(s, IDX_TIMEOUT)
                             for s in seen["rpc"]], np.uint32)
            mine[np.array([s == "blocked" for s in seen["rpc"]], bool)] = IDX_WAITING
            wst = np.full(len(live), IDX_TIMEOUT, np.uint32)
            wst[live] = mine[:n_live]
            r.update(status=mine[n_live:], res_status=wst[wst != IDX_WAITING])
        dump = ref.dump_internals()
        running = np.zeros(es.n, np.uint32)
        for s in dump["servants"]:
            running[self.row_of[s["location"]]] = s["running_tasks"]
        r.update(renewed=renewed, report_unknown=unknown, running=running,
                 renew_refused=int((renewed == 0).sum()))
        return r


def run_reference(sv, rpcs, frees, renewals, ticks, max_waiting, max_rows, n_envs=1, **kw):
    """The seeded stream of run_model through ReferenceReplay. Same record as run_model."""
    ws = new_stream(sv, rpcs, frees, renewals, max_waiting, max_rows, n_envs=n_envs, **kw)
    ref = ReferenceReplay(ws)
    try:
        return [ref.tick(ws.next_tick()) for _ in range(ticks)]
    finally:
        ref.close()

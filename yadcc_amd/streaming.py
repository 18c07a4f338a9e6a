"""Synthetic event stream of BASELINE.json configs[4] (SURVEY.md §8d "Streaming"): per tick
10 % of the servants (round robin) re-heartbeat with current_load := foreign load + running
(what the daemon would report), a number of live grants are freed, then a fresh batch of
requests is dispatched. Shared by bench.py (cfg5) and the streaming parity test, which
replays the same stream through the oracle."""
import numpy as np

from . import binding, pack, synth


class EventStream:
    def __init__(self, sv, tasks_per_tick, frees_per_tick, heartbeat_frac=0.10, n_envs=1, seed=44):
        self.sv = {k: v.copy() for k, v in sv.items()}
        self.n = len(sv["version"])
        self.rng = np.random.default_rng(seed)
        self.tasks_per_tick = tasks_per_tick
        self.frees_per_tick = frees_per_tick
        self.hb = max(1, int(self.n * heartbeat_frac))
        self.hb_pos = 0
        self.n_envs = n_envs
        self.foreign = self.sv["current_load"].astype(np.int64)  # load of other jobs on the node
        self.running = self.sv["running_tasks"].astype(np.int64).copy()
        self.live = np.empty(0, np.uint32)  # servant index of every live grant
        self.tick_no = 0
        self.abi = pack.to_abi_columns(self.sv)

    def next_tick(self):
        """-> (upd_idx, upd_rows, release_idx, tasks); applies the heartbeat / free part to the
        stream's own view of the registry (self.sv, self.running)."""
        who = (self.hb_pos + np.arange(self.hb)) % self.n
        self.hb_pos = (self.hb_pos + self.hb) % self.n
        who = np.unique(who).astype(np.uint32)
        self.sv["current_load"][who] = np.minimum(self.foreign[who] + self.running[who],
                                                  0xFFFFFFFF).astype(np.uint32)
        rows = np.zeros(len(who), dtype=binding.ROW_DTYPE)
        for k in ("version", "num_processors", "current_load", "max_tasks"):
            rows[k] = self.sv[k][who]
        rows["flags"] = self.abi["flags"][who]
        rows["ip_id"] = self.abi["ip_id"][who]
        em = self.abi["env_mask"]
        rows["env_mask"] = em[who] if em.ndim == 1 else em[who, 0]  # (wide masks travel beside the rows)
        n_free = min(self.frees_per_tick, len(self.live))
        pick = self.rng.choice(len(self.live), n_free, replace=False) if n_free else np.empty(0, np.int64)
        rel = self.live[pick]
        keep = np.ones(len(self.live), bool)
        keep[pick] = False
        # Which of the live grants (in the order commit() appended them) this tick frees: lets a
        # caller that tracks grant ids beside the stream (the reference replay) free the same ones.
        self.last_freed, self.last_kept = pick, keep
        self.live = self.live[keep]
        np.subtract.at(self.running, rel, 1)
        tk = synth.make_tasks(self.tasks_per_tick, self.sv, n_envs=self.n_envs,
                              seed=1000 + self.tick_no)
        self.tick_no += 1
        return who, rows, rel, tk

    def commit(self, servant_idx):
        """Feeds the placement of the tick's requests back (grants become live)."""
        # (below every sentinel: IDX_OVER_QUOTA, the lowest, is never a servant)
        granted = servant_idx[servant_idx < binding.IDX_OVER_QUOTA]
        np.add.at(self.running, granted, 1)
        self.live = np.concatenate([self.live, granted.astype(np.uint32)])

    def registry_snapshot(self):
        """Servant columns as the scheduler sees them right now (for the oracle)."""
        sv = {k: v.copy() for k, v in self.sv.items()}
        sv["running_tasks"] = self.running.astype(np.uint32)
        return sv


def rpc_grants(result, i):
    """Views of a stream_tick_rpc result (binding.Context.stream_tick_rpc): the (servants, task ids)
    granted to new request i: the first n_granted[i] rows at its offset in the expanded layout."""
    a = int(result["row_off"][i])
    b = a + int(result["n_granted"][i])
    return result["servants"][a:b], result["task_ids"][a:b]


def rpc_admitted(result, adm_immediate, adm_prefetch):
    """A stream_tick_rpc result of a stream with a quota (binding.Context.stream_quota_begin), unpacked
    by ADMITTED rows: the tick laid its expanded outputs out as if every request had asked for what
    it was admitted (binding.Context.stream_quota_result), so request i's rows begin at the sum of
    adm_immediate + adm_prefetch over the requests in front of it and a request answered
    IDX_OVER_QUOTA has none. -> the result with row_off, servants and task_ids by that layout;
    rpc_grants then reads it as usual."""
    rows = np.asarray(adm_immediate, np.int64) + np.asarray(adm_prefetch, np.int64)
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    out = dict(result)
    out["row_off"] = row_off
    out["servants"] = result["servants"][:int(row_off[-1])]
    out["task_ids"] = result["task_ids"][:int(row_off[-1])]
    return out


def rpc_resolved_grants(result, j):
    """... and of the j-th waiting RPC answered in that tick (packed behind res_first[j])."""
    a = int(result["res_first"][j])
    b = a + int(result["res_n_granted"][j])
    return result["res_servants"][a:b], result["res_task_ids"][a:b]


PRIORITY_NAMES = {0: "SERVANT_PRIORITY_UNKNOWN", 1: "SERVANT_PRIORITY_DEDICATED", 2: "SERVANT_PRIORITY_USER"}
REASON_NAMES = {0: "NOT_ACCEPTING_TASK_REASON_UNKNOWN", 1: "NOT_ACCEPTING_TASK_REASON_USER_INSTRUCTED",
                2: "NOT_ACCEPTING_TASK_REASON_POOR_MACHINE", 3: "NOT_ACCEPTING_TASK_REASON_CGROUPS_PRESENT",
                4: "NOT_ACCEPTING_TASK_REASON_BEHIND_NAT", 100: "NOT_ACCEPTING_TASK_REASON_NOT_VERIFIED"}


def format_time(t, unit_s=1e-3):
    """A clock reading of the ticks (`unit_s` seconds per unit) as the reference's FormatTime prints it."""
    import time
    return time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime(int(t) * unit_s))


def dump_internals(servants, tasks, sv, locations, digest_names, host_names, expires_at=None, fmt=format_time):
    """The reference's DumpInternals (task_dispatcher.cc:538-614) as a dict of the JSON's shape, from
    what an open stream with inspection answers and the tables a scheduler owns anyway. No compute:
    every number is one of the two get calls' (binding.Context.stream_inspect_servants / _tasks).

    servants, tasks: the two dicts. sv: the registry's columns as the scheduler keeps them (version,
    num_processors, current_load, max_tasks, priority, total_memory, memory_available, env_mask;
    optionally not_accepting_task_reason). locations: per servant row its observed location, or
    (observed, reported). digest_names: env_id -> compiler digest; host_names: requestor_ip id -> the
    requestor's address (a lease granted while inspection was off has neither: None). expires_at: the
    servants' expiry column where aliveness keeps one (ydc_stream_alive_get). Times go through fmt."""
    out = {}
    em = sv["env_mask"]
    reason = sv.get("not_accepting_task_reason")
    for s in range(len(servants["running_tasks"])):
        item = {"version": int(sv["version"][s])}
        loc = locations[s]
        observed, reported = (loc, loc) if isinstance(loc, str) else loc
        if observed != reported:
            item["observed_location"], item["reported_location"] = observed, reported
        else:
            item["location"] = observed
        item["discovered_at"] = fmt(servants["discovered_at"][s])
        item["expires_at"] = fmt(expires_at[s]) if expires_at is not None else None
        words = [int(em[s])] if em.ndim == 1 else [int(w) for w in em[s]]
        envs = [digest_names[64 * k + b] for k, w in enumerate(words) for b in range(64) if w >> b & 1]
        if envs:
            item["environments"] = envs
        item["priority"] = PRIORITY_NAMES[int(sv["priority"][s])]
        if int(sv["max_tasks"][s]):
            item["max_tasks"] = int(sv["max_tasks"][s])
        else:
            item["not_accepting_task_reason"] = REASON_NAMES[int(reason[s]) if reason is not None else 0]
        item["num_processors"] = int(sv["num_processors"][s])
        item["current_load"] = int(sv["current_load"][s])
        item["capacity_available"] = int(servants["capacity_available"][s])
        item["total_memory_mb"] = int(sv["total_memory"][s]) >> 20
        item["memory_available_mb"] = int(sv["memory_available"][s]) >> 20
        item["running_tasks"] = int(servants["running_tasks"][s])
        item["ever_assigned_tasks"] = int(servants["ever_assigned"][s])
        out.setdefault("servants", []).append(item)
    for k in range(len(tasks["task_id"])):
        tid, env, ip = int(tasks["task_id"][k]), int(tasks["env_id"][k]), int(tasks["requestor_ip"][k])
        loc = locations[int(tasks["servant_idx"][k])]
        known = env != binding.INSPECT_NO_ID
        out.setdefault("tasks", {})[str(tid)] = {
            "task_id": tid,
            "requestor_ip": host_names[ip] if known else None,
            "compiler_digest": digest_names[env] if known else None,
            "started_at": fmt(tasks["started_at"][k]) if known else None,
            "expires_at": fmt(tasks["expires_at"][k]),
            "prefetched_task": bool(tasks["prefetch"][k]),
            "servant_location": loc if isinstance(loc, str) else loc[0],
            "zombie": bool(tasks["zombie"][k]),
        }
    tot = servants["totals"]
    for k in ("servants_up", "running_tasks", "capacity", "capacity_available", "capacity_unavailable"):
        out[k] = int(tot[k])
    return out


OUTLOOK_COLUMNS = ("eligible", "free_servants", "grants_available", "running_tasks", "max_tasks",
                   "capacity_available", "waiting", "waiting_rows", "leases", "zombies")


def outlook_table(outlook, digest_names, env_id=None, min_version=None):
    """The per-digest table /inspect gains: one line per row of a binding.Context.stream_outlook result,
    named by compiler digest. No compute: every number is the call's. digest_names: env_id -> digest,
    indexed by env_id[i] (without env_id: by the row number); an id without a name prints as "#id";
    a column that is OUTLOOK_UNKNOWN (leases / zombies while inspection is off) prints as "-"."""
    n = len(outlook["eligible"])
    ids = list(range(n)) if env_id is None else [int(e) for e in env_id]
    names = []
    for i, e in enumerate(ids):
        name = digest_names[e] if e < len(digest_names) and digest_names[e] is not None else "#%d" % e
        names.append(name if min_version is None else "%s >= %d" % (name, int(min_version[i])))
    rows = [("digest",) + OUTLOOK_COLUMNS]
    for i in range(n):
        cells = []
        for k in OUTLOOK_COLUMNS:
            v = int(outlook[k][i])
            cells.append("-" if k in ("leases", "zombies") and v == binding.OUTLOOK_UNKNOWN else str(v))
        rows.append((names[i],) + tuple(cells))
    width = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    return "\n".join("  ".join(cell.ljust(width[c]) if c == 0 else cell.rjust(width[c])
                               for c, cell in enumerate(r)).rstrip() for r in rows)


def find_running(ctx, row_to_location, keys):
    """The daemon's TryFindTask (running_task_keeper.cc:67-75) for a batch of digests, asked of an
    open stream's book (binding.Context.stream_book_find) instead of a copy of the whole list: per
    key (location, servant_task_id) of the servant that already compiles it — the last entry of the
    book with that digest_key, as after a Refresh —, or None. row_to_location: per servant row its
    location, as the scheduler keeps it. No compute: every number is the call's."""
    hits, _ = ctx.stream_book_find(keys)
    return [None if int(h["pos"]) == binding.BOOK_NOT_FOUND
            else (row_to_location[int(h["servant_idx"])], int(h["servant_task_id"])) for h in hits]


def iter_tasks(ctx, page, **filter):
    """The leases that satisfy a filter, a page at a time (binding.Context.stream_inspect_select with the
    cursor): yields dicts of the columns stream_inspect_tasks returns, at most `page` rows each, in
    ascending id order; the pages, concatenated, are the filtered lease table. filter: the keywords of
    stream_inspect_select; an after_id given is where the first page starts. Between two pages the
    stream may tick: a page shows the table as it is when it is asked for. No compute: every number is
    the call's."""
    page = int(page)
    if page < 1:
        raise ValueError("iter_tasks: a page of %d rows" % page)
    while True:
        cols, matches = ctx.stream_inspect_select(page, **filter)
        n = len(cols["task_id"])
        if n:
            yield cols
        if matches <= n:
            return
        filter["after_id"] = int(cols["task_id"][-1])


REQUESTOR_COLUMNS = ("leases", "zombies", "prefetch_leases", "waiting", "waiting_rows")


def requestor_table(load, host_names):
    """The per-requestor table of /inspect, next to outlook_table: one line per row of a
    binding.Context.stream_requestors / stream_requestor_find result, named by the requestor's
    address. No compute: every number is the call's. host_names: requestor_ip id -> address (a dict
    or a list); an id without a name prints as "#id"; a column that is REQUESTOR_UNKNOWN (the lease
    columns while inspection is off or on a stream without leases) prints as "-"."""
    def name(ip):
        got = host_names.get(ip) if isinstance(host_names, dict) else (host_names[ip] if ip < len(host_names) else None)
        return got if got is not None else "#%d" % ip
    rows = [("requestor",) + REQUESTOR_COLUMNS]
    for r in load:
        cells = []
        for k in REQUESTOR_COLUMNS:
            v = int(r[k])
            cells.append("-" if k in REQUESTOR_COLUMNS[:3] and v == binding.REQUESTOR_UNKNOWN else str(v))
        rows.append((name(int(r["requestor_ip"])),) + tuple(cells))
    width = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    return "\n".join("  ".join(cell.ljust(width[c]) if c == 0 else cell.rjust(width[c])
                               for c, cell in enumerate(r)).rstrip() for r in rows)


def admit(ctx, requests, n_immediate, n_prefetch, cap):
    """A fair share at the door: the tick's requests (dict with a requestor_ip column, arrival order)
    clipped so that no requestor has more than `cap` grants outstanding — leases, zombies included,
    plus the rows it waits for — once they are all admitted. One ctx.stream_requestor_find for the
    requestors of the tick, then binding.admit_clip. n_prefetch: None outside rpc mode.
    -> (n_immediate, n_prefetch, keep): the two clipped columns (prefetch is clipped first) and the
    mask of the rows that are admitted any grant; a scheduler answers the others
    STATUS_NO_QUOTA_AVAILABLE and sends the kept rows with their clipped counts."""
    ips = np.ascontiguousarray(requests["requestor_ip"], dtype=np.uint32)
    load, _ = ctx.stream_requestor_find(ips)
    imm, pre = binding.admit_clip(ips, n_immediate, n_prefetch, load, cap)
    return imm, pre, (imm.astype(np.uint64) + pre) > 0


def fair_share(ctx, percent=100, floor=1):
    """The common setting of the fair-share level (binding.Context.stream_quota_fair) for a stream with
    the quota on: the pool is `percent` of what the registry can run, as every tick's heartbeats leave
    it, and nobody without an override is capped below `floor`. The static default_cap stays an upper
    bound, the overrides stay exceptions. -> the function to call after a tick for that tick's level
    (binding.Context.stream_quota_fair_result). No compute: every number is the call's."""
    ctx.stream_quota_fair(binding.FAIR_REGISTRY, percent, floor)
    return ctx.stream_quota_fair_result


DEPART_COLUMNS = ("requestor_ip", "leases", "zombies", "waiting", "waiting_rows")


def dismiss(ctx, requestors):
    """A departed requestor (connection closed, daemon restarted, host gone): its leases and waiting
    calls leave inside the NEXT accepted tick (binding.Context.stream_depart_stage), with no list of
    its grants or tags kept on the host. Stages `requestors` (requestor_ip ids, any order, repeats
    allowed) and returns the function to call after that tick: -> a dict of columns, one row per staged
    requestor in the staged order (DEPART_COLUMNS), plus "leases_freed" and "n_withdrawn", the totals
    with every lease and entry counted once. No compute: every number is the call's."""
    ctx.stream_depart_stage(requestors)

    def result():
        rows, leases, waiting = ctx.stream_depart_result()
        out = {k: rows[k].copy() for k in DEPART_COLUMNS}
        out["leases_freed"], out["n_withdrawn"] = leases, waiting
        return out
    return result


def usage(ctx, reset=False):
    """Who has used the cluster since the accounting began or was last reset
    (binding.Context.stream_usage_get): -> (rows of binding.USAGE_DTYPE sorted by requestor_ip, the totals
    as a dict: unattributed_time, quanta, ticks, n_keys, slots). Times are in quanta of the clock unit
    given to stream_usage_begin. reset: the periodic export of a long-running scheduler, which empties
    the table behind the copy. No compute beyond the sort: every number is the call's."""
    rows, totals = ctx.stream_usage_get(reset=reset)
    return rows[np.argsort(rows["requestor_ip"], kind="stable")], totals


def standby_base(primary):
    """What a standby of the stream on `primary` (inspection on) starts from: -> (base, sidecar), the bytes
    of binding.Context.stream_delta_base and the full inspection sidecar beside them
    (binding.Context.stream_delta_inspect). No compute: both are the calls'."""
    return primary.stream_delta_base(), primary.stream_delta_inspect()


def standby_restore(standby, base, sidecar):
    """The standby's side of standby_base: ydc_stream_restore, then ydc_stream_inspect_restore. Afterwards
    `standby` answers the snapshot and the inspection calls as the primary did when it took the base."""
    caps = standby.stream_restore(base)
    standby.stream_inspect_restore(sidecar)
    return caps


def standby_step(primary, standby=None):
    """One step of the chain, between two ticks of the primary: -> (delta, sidecar), applied to `standby`
    where one is given (binding.Context.stream_delta, stream_delta_inspect, stream_delta_apply_inspected).
    At promotion the standby's host sets quota, withdrawal and departure settings again: they are not
    state of the stream's."""
    delta = primary.stream_delta()
    sidecar = primary.stream_delta_inspect(delta)
    if standby is not None:
        standby.stream_delta_apply_inspected(delta, sidecar)
    return delta, sidecar

"""Inspection's model (tests/stream_inspect_model.py) and yadcc_amd.streaming.dump_internals against
the verbatim reference class: the yardstick of tests/test_stream_inspect_gpu.py pinned on the CPU.

An rpc stream (one WaitForStartingNewTask per row, prefetching as the handler's two loops set it:
stream_rpc_model.ReferenceReplay) runs through the reference; after every tick the dump built from
the model's state equals TaskDispatcher::DumpInternals key for key (td_scenarios.assert_same_dump:
everything but the formatted times). started_at and discovered_at are pinned against the rule
(task_dispatcher.cc:133, :208) on the model itself."""
import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_alive_model as AM
from tests import stream_inspect_model as IM
from tests import stream_lease_model as L
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WM
from tests.td_scenarios import assert_same_dump
from tests.test_stream_alive_model import AliveReplay
from yadcc_amd import binding, pack, streaming, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")


class Hosts:
    """requestor_ip id -> dotted address (the streams' ids are the addresses themselves)."""

    def __getitem__(self, ip):
        return RM.ip_string(ip)


class Digests:
    def __getitem__(self, env):
        return R.digest_name(int(env))


def pathological(sv):
    """The rows the totals have to get right, in a registry whose running_tasks start at 0 (the
    reference reaches them by grants): row 0 stops accepting (max_tasks == 0), row 1 is busy with
    other work (load >= nproc whatever it runs). Two more rows change later: mutate()."""
    sv = {k: v.copy() for k, v in sv.items()}
    sv["running_tasks"][:] = 0
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 4)  # (a pool a few RPCs saturate: some wait)
    sv["max_tasks"][0] = 0
    sv["current_load"][1] = sv["num_processors"][1] + 3
    return sv


def mutate(ws, ev, s, **cols):
    """The daemon on row s reports something new, in a heartbeat of the tick `ev` (added to it where
    the round robin did not send one: the registry learns of a change by a heartbeat only)."""
    es = ws.es
    for k, v in cols.items():
        es.sv[k][s] = v
    es.abi["flags"] = pack.to_abi_columns(es.sv)["flags"]
    es.sv["current_load"][s] = min(int(es.foreign[s] + es.running[s]), 0xFFFFFFFF)
    row = np.zeros(1, dtype=binding.ROW_DTYPE)
    for k in ("version", "num_processors", "current_load", "max_tasks"):
        row[k] = es.sv[k][s]
    row["flags"], row["ip_id"] = es.abi["flags"][s], es.abi["ip_id"][s]
    em = es.abi["env_mask"]
    row["env_mask"] = em[s] if em.ndim == 1 else em[s, 0]
    at = np.nonzero(ev["upd_idx"] == s)[0]
    if len(at):
        ev["upd_rows"][at[0]] = row[0]
    else:
        ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s]]).astype(np.uint32)
        ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])


def our_dump(ws, I):
    es = ws.es
    locs = [L.location(es.sv, s) for s in range(es.n)]
    return streaming.dump_internals(I.servants(), I.tasks(), es.sv, locs, Digests(), Hosts())


def pinned_rule(I, before, now):
    """Every lease the tick added started at the tick's clock, whatever tick submitted its request."""
    for t, d in I.details.items():
        if t not in before:
            assert d[0] == now, (t, d, now)


@needs_ref
def test_dump_equals_the_reference_on_an_rpc_stream():
    sv = pathological(synth.make_servants(14, n_tasks_hint=240, n_envs=3, seed=5))
    ws = RM.new_stream(sv, 8, 10, 12, 120, 2400, n_envs=3, rate=lambda now: 1.0 if now % 12 < 8 else 0.125,
                       report_frac=0.3)
    ws.es.hb = 5  # (every servant beats every third tick)
    I = IM.attach(ws)
    ref = RM.ReferenceReplay(ws)
    mutated = False
    seen = dict(prefetch=0, immediate=0, w_granted=0, zombies=0, swept=0, freed=0, wrap=0, below=0, grants=0)
    try:
        for t in range(40):
            ev = ws.next_tick()
            busiest = np.argsort(-ws.es.running, kind="stable")[:2].tolist()
            if t >= 6 and not mutated and ws.es.running[busiest[1]] >= 2:
                # The two busiest rows. One runs out of memory with tasks on it and lowers max_tasks below
                # them: the term max_tasks - capacity_available wraps. The other's capacity drops below
                # its running tasks.
                a, b = busiest
                mutated = True
                mutate(ws, ev, a, memory_available=1 << 20, total_memory=64 << 30, max_tasks=1)
                mutate(ws, ev, b, max_tasks=1)
            before = set(ws.table.L)
            I.stage(ev)
            r = ref.tick(ev)
            now = int(ev["now"])
            pinned_rule(I, before, now)
            theirs = ref.ref.dump_internals()
            assert_same_dump(our_dump(ws, I), theirs)
            sv_now, run = ws.es.sv, ws.es.running
            tasks = I.tasks()
            seen["prefetch"] += int(tasks["prefetch"].sum())
            seen["immediate"] += int((tasks["prefetch"] == 0).sum())
            seen["zombies"] += int(tasks["zombie"].sum())
            seen["w_granted"] += r["w_granted"]
            seen["swept"] += r["swept"]
            seen["freed"] += r["freed"]
            seen["grants"] += len(set(ws.table.L) - before)
            low = (np.asarray(ws.es.abi["flags"]) & IM.LOW_MEMORY) != 0
            seen["wrap"] += int((low & (run > sv_now["max_tasks"])).any())
            seen["below"] += int((~low & (run > sv_now["max_tasks"]) & (sv_now["max_tasks"] > 0)).any())
    finally:
        ref.close()
    # (a vacuous stream fails: every kind of row and task the dump has to get right was there)
    assert all(v > 0 for v in seen.values()), seen
    assert 100 <= seen["grants"] <= 2000, seen


class ReturnReplay(AliveReplay):
    """AliveReplay that knows a returning address: refbind numbers a location by its first sight, so
    the new row of a servant that comes back is listed without a second entry in `loc`."""

    def beat(self, s, expires_in):
        loc = L.location(self.ls.es.sv, s)
        if s == len(self.rows) and loc in self.loc:
            self.rows.append(loc)
        super().beat(s, expires_in)


@needs_ref
def test_dump_equals_the_reference_when_a_servant_expires_and_returns():
    """Row 5's last heartbeat carries a life of one tick; the timer erases it with the leases on it
    (orphans lose their details), and its daemon is back a few ticks later under its old address: a
    new row at the end, discovered then, assigned nothing."""
    sv = pathological(synth.make_servants(12, n_tasks_hint=200, n_envs=2, seed=9))
    ws = L.LeaseStream(sv, 12, 6, 4, L.LeaseTable(), n_envs=2, report_frac=0.3)
    ws.es.hb = 4
    LIFE = 30000
    first = np.full(12, LIFE, np.int64)
    A = AM.attach(ws, first)
    I = IM.attach(ws)
    ref = ReturnReplay(ws, first)
    gone_loc, returned, removed_at, orphans = L.location(ws.es.sv, 5), None, None, 0
    try:
        for t in range(16):
            ev = ws.next_tick()
            now = int(ev["now"])
            short = None
            if t == 4:
                mutate(ws, ev, 5)  # (a heartbeat of row 5 in this tick, whatever the round robin says)
                short = 5
            elif returned is None and removed_at is None and t > 4:  # (it beats no more)
                keep = ev["upd_idx"] != 5
                ev["upd_idx"], ev["upd_rows"] = ev["upd_idx"][keep], ev["upd_rows"][keep]
            if t == 9:  # the daemon is back under its old address
                row, s_new = AM.append_servant(ws, 0, int(sv["ip"][5]))
                ws.es.sv["port"][s_new] = sv["port"][5]
                ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
                ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
                returned = s_new
                assert L.location(ws.es.sv, s_new) == gone_loc
            ev["upd_expires_at"] = np.where(ev["upd_idx"] == short, now + 1, now + LIFE).astype(np.int64) \
                if short is not None else np.full(len(ev["upd_idx"]), now + LIFE, np.int64)
            before = set(ws.table.L)
            I.stage(ev)
            r = ref.tick(ev)
            if len(r["removed"]):
                assert r["removed"].tolist() == [5] and removed_at is None
                removed_at, orphans = t, r["orphans"]
            pinned_rule(I, before, now)
            assert_same_dump(our_dump(ws, I), ref.ref.dump_internals())
            if t == 9:  # (discovered now; what it has been assigned since, it was assigned in this tick)
                assert I.disc[returned] == now and I.ever[returned] == sum(1 for e in ws.table.L.values() if e[0] == returned)
        assert removed_at == 6 and orphans > 0 and returned == 11 and len(I.disc) == ws.es.n == 12
        assert (I.disc[:11] == 0).all() and I.disc[11] == 9
    finally:
        ref.close()


def test_totals_by_hand():
    """Four servants, every branch of :283-313, summed as :541-612 does.

      row  nproc load max_tasks running low_memory   capacity_available (:283-313)
      0      8     2     4         1       no        foreign = max(2 - 1, 0) = 1; min(4, max(8 - 1, 0)) = 4
      1      8    11     4         0       no        foreign = 11; max(8 - 11, 0) = 0; min(4, 0) = 0
      2     16     5     2         5       yes       low memory: running = 5
      3      8     6     1         3       no        foreign = max(6 - 3, 0) = 3; min(1, max(8 - 3, 0)) = 1
      4      8     0     0         0       no        min(0, 8) = 0

    capacity = 4 + 4 + 2 + 1 + 0 = 11; running_tasks = 1 + 0 + 5 + 3 + 0 = 9;
    capacity_unavailable = (4 - 4) + (4 - 0) + (2 - 5 mod 2^64) + (1 - 1) + (0 - 0) = 4 + (2^64 - 3) = 2^64 + 1 = 1 (mod 2^64);
    capacity_available = max((int64)(11 - 9 - 1), 0) = 1."""
    nproc, load, maxt, run = [8, 8, 16, 8, 8], [2, 11, 5, 6, 0], [4, 4, 2, 1, 0], [1, 0, 5, 3, 0]
    low = [False, False, True, False, False]
    avail = [IM.capacity(*x) for x in zip(nproc, load, maxt, run, low)]
    assert avail == [4, 0, 5, 1, 0]
    assert IM.totals(maxt, run, avail) == {"servants_up": 5, "running_tasks": 9, "capacity": 11,
                                           "capacity_available": 1, "capacity_unavailable": 1}
    # ... and where the difference is negative (:607-611): one servant, capacity 1, running 3.
    assert IM.totals([1], [3], [IM.capacity(8, 3, 1, 3, False)])["capacity_available"] == 0
    # ... and a wrapped term that stays wrapped: capacity_unavailable prints as 2^64 - 3.
    t = IM.totals([2], [5], [IM.capacity(16, 5, 2, 5, True)])
    assert t == {"servants_up": 1, "running_tasks": 5, "capacity": 2, "capacity_available": 0,
                 "capacity_unavailable": (1 << 64) - 3}


def test_dump_shape_without_the_reference():
    """Keys exactly those of :546-612: location against observed / reported, max_tasks against the
    reason, no "environments" for a servant that has none."""
    servants = {"discovered_at": np.array([5, 7], np.int64), "ever_assigned": np.array([3, 0], np.uint64),
                "running_tasks": np.array([1, 0], np.uint32), "capacity_available": np.array([2, 0], np.uint32),
                "totals": {"servants_up": 2, "running_tasks": 1, "capacity": 2, "capacity_available": 1,
                           "capacity_unavailable": 0}}
    tasks = {"task_id": np.array([9], np.uint64), "servant_idx": np.array([0], np.uint32),
             "expires_at": np.array([40], np.int64), "zombie": np.array([0], np.uint8),
             "started_at": np.array([6], np.int64), "env_id": np.array([1], np.uint32),
             "requestor_ip": np.array([0x0A000007], np.uint32), "prefetch": np.array([1], np.uint8)}
    sv = {"version": np.array([8, 8]), "num_processors": np.array([8, 4]), "current_load": np.array([1, 0]),
          "max_tasks": np.array([2, 0]), "priority": np.array([1, 2]), "total_memory": np.array([64 << 30, 0], np.uint64),
          "memory_available": np.array([32 << 30, 0], np.uint64), "env_mask": np.array([3, 0], np.uint64),
          "not_accepting_task_reason": np.array([0, 1])}
    d = streaming.dump_internals(servants, tasks, sv, ["10.0.0.1:8334", ("10.0.0.2:8334", "192.168.0.2:8334")],
                                 ["d0", "d1"], Hosts())
    a, b = d["servants"]
    assert a["location"] == "10.0.0.1:8334" and a["environments"] == ["d0", "d1"] and a["max_tasks"] == 2
    assert a["priority"] == "SERVANT_PRIORITY_DEDICATED" and a["ever_assigned_tasks"] == 3 and a["total_memory_mb"] == 65536
    assert "not_accepting_task_reason" not in a and "observed_location" not in a
    assert (b["observed_location"], b["reported_location"]) == ("10.0.0.2:8334", "192.168.0.2:8334")
    assert b["not_accepting_task_reason"] == "NOT_ACCEPTING_TASK_REASON_USER_INSTRUCTED"
    assert "location" not in b and "max_tasks" not in b and "environments" not in b
    assert d["tasks"]["9"] == {"task_id": 9, "requestor_ip": "10.0.0.7", "compiler_digest": "d1",
                               "started_at": streaming.format_time(6), "expires_at": streaming.format_time(40),
                               "prefetched_task": True, "servant_location": "10.0.0.1:8334", "zombie": False}
    assert (d["servants_up"], d["running_tasks"], d["capacity"], d["capacity_available"], d["capacity_unavailable"]) == (
        2, 1, 2, 1, 0)


def test_model_on_each_mode_without_the_reference():
    """The three modes' ticks with inspection attached: details exist for exactly the leases granted
    since, ever_assigned counts the grants, started_at is the granting tick's clock."""
    sv = synth.make_servants(40, n_tasks_hint=900, n_envs=2, seed=4)
    streams = [(L, L.LeaseStream(sv, 120, 60, 20, L.LeaseTable(), n_envs=2)),
               (WM, WM.new_stream(sv, 160, 60, 20, 800, n_envs=2, rate=lambda now: 1.0 if now % 8 < 5 else 0.125)),
               (RM, RM.new_stream(sv, 12, 60, 20, 200, 4000, n_envs=2, rate=lambda now: 1.0 if now % 8 < 5 else 0.125))]
    for M, ws in streams:
        for _ in range(3):  # (inspection begins late: these leases have no details)
            M.model_tick(ws, ws.next_tick())
        early = set(ws.table.L)
        I = IM.attach(ws)
        grants = 0
        for _ in range(16):
            ev = ws.next_tick()
            before = set(ws.table.L)
            IM.model_tick(M, ws, ev)
            pinned_rule(I, before, int(ev["now"]))
            grants += len(set(ws.table.L) - before)
        tk = I.tasks()
        late = np.array([int(t) not in early for t in tk["task_id"]], bool)
        assert (tk["env_id"][~late] == IM.NO_ID).all() and (tk["started_at"][~late] == IM.NO_TIME).all()
        assert (tk["env_id"][late] != IM.NO_ID).all() and late.any()
        assert int(I.ever.sum()) >= grants > 0
        if M is RM:
            assert tk["prefetch"].any() and (tk["prefetch"][late] == 0).any()
        else:
            assert not tk["prefetch"].any()

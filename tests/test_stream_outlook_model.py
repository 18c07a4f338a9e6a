"""The outlook's model (tests/stream_outlook_model.py) against the verbatim reference class: the
yardstick of tests/test_stream_outlook_gpu.py pinned on the CPU, three ways.

  - against the dump: after every tick of a seeded rpc stream replayed through the reference
    (stream_rpc_model.ReferenceReplay), every supply column and the lease counts are computed again
    from TaskDispatcher::DumpInternals' own JSON and must equal the model's;
  - against the reference's own answer: grants_available + 1 sequential WaitForStartingNewTask calls
    with the deadline at now are granted exactly grants_available times, and the first call's status
    tells eligible == 0 (EnvironmentNotFound) from free_servants == 0 (Timeout);
  - two registries written by hand, the deriving lines of task_dispatcher.cc beside them."""
import itertools

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_inspect_model as IM
from tests import stream_lease_model as L
from tests import stream_outlook_model as OM
from tests import stream_rpc_model as RM
from tests.test_stream_inspect_model import pathological
from yadcc_amd import binding, pack, streaming, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
SUPPLY = OM.COLUMNS[:6]


def from_dump(dump, digest, min_version):
    """One outlook row from the reference's dump alone: eligibility by the servant's own
    `environments`, `version` and max_tasks (printed only while the servant accepts tasks), the rest
    from its capacity_available and running_tasks. A servant the dump shows free is not short of
    memory (:291 would print capacity_available == running_tasks), so its further grants follow
    :308-312 from its num_processors and current_load."""
    row = dict.fromkeys(SUPPLY, 0)
    for s in dump.get("servants", []):
        if digest not in s.get("environments", []) or not s.get("max_tasks") or s["version"] < min_version:
            continue
        run, cap = s["running_tasks"], s["capacity_available"]
        row["eligible"] += 1
        row["free_servants"] += run < cap
        if run < cap:
            row["grants_available"] += OM.grants_by_rule(s["num_processors"], s["current_load"], s["max_tasks"], run, False)
        row["running_tasks"] += run
        row["max_tasks"] += s["max_tasks"]
        row["capacity_available"] += cap
    tasks = [t for t in dump.get("tasks", {}).values() if t["compiler_digest"] == digest]
    row["leases"], row["zombies"] = len(tasks), sum(1 for t in tasks if t["zombie"])
    return row


@needs_ref
def test_supply_and_leases_equal_the_reference_dump_after_every_tick():
    sv = pathological(synth.make_servants(14, n_tasks_hint=240, n_envs=3, seed=5))  # row 0 accepts nothing, row 1: load >= nproc
    sv["total_memory"][2], sv["memory_available"][2] = 64 << 30, 1 << 20             # row 2 is short of memory
    sv["version"][:] = 20
    sv["version"][[3, 7]] = 19
    assert (pack.to_abi_columns(sv)["flags"][2] & IM.LOW_MEMORY) and sv["max_tasks"][0] == 0
    assert sv["current_load"][1] >= sv["num_processors"][1]
    ws = RM.new_stream(sv, 8, 10, 12, 120, 2400, n_envs=3, rate=lambda now: 1.0 if now % 12 < 8 else 0.125,
                       report_frac=0.3)
    ws.es.hb = 5
    I = IM.attach(ws)
    ref = RM.ReferenceReplay(ws)
    env = np.repeat(np.arange(3, dtype=np.uint32), 3)
    minv = np.tile(np.array([0, 20, 21], np.uint32), 3)
    seen = dict(zombies=0, leases=0, waiting=0, not_free=0, grew=0, differs=0)
    try:
        for t in range(30):
            ev = ws.next_tick()
            I.stage(ev)
            ref.tick(ev)
            dump = ref.ref.dump_internals()
            ours = OM.stream_outlook(ws, env, minv, inspect=I)
            for q in range(len(env)):
                theirs = from_dump(dump, R.digest_name(int(env[q])), int(minv[q]))
                for k in SUPPLY + (("leases", "zombies") if minv[q] == 0 else ()):
                    assert int(ours[k][q]) == theirs[k], (t, q, k, int(ours[k][q]), theirs[k])
            # (demand by digest alone: the same for every min_version)
            for k in ("waiting", "waiting_rows", "leases", "zombies"):
                assert (ours[k].reshape(3, 3) == ours[k].reshape(3, 3)[:, :1]).all(), k
            assert int(ours["waiting"][::3].sum()) == len(ws.state.q) - int((ws.state.q.cols["env_id"] >= 3).sum())
            assert int(ours["waiting_rows"][::3].sum()) == ws.state.q.rows()  # (a digest nobody has never waits)
            seen["zombies"] += int(ours["zombies"][::3].sum())
            seen["leases"] += int(ours["leases"][::3].sum())
            seen["waiting"] += int(ours["waiting"][::3].sum())
            seen["not_free"] += int((ours["free_servants"] < ours["eligible"]).any())
            seen["grew"] += int((ours["grants_available"] > ours["capacity_available"] - np.minimum(
                ours["capacity_available"], ours["running_tasks"])).any())
            seen["differs"] += int((ours["eligible"][0::3] != ours["eligible"][1::3]).any())
            assert (ours["eligible"][2::3] == 0).all()  # (nobody is at version 21)
    finally:
        ref.close()
    assert all(v > 0 for v in seen.values()), seen


def registry(rows, n_envs=2):
    """rows: (version, environments, nproc, load, max_tasks, running, low_memory, ip). -> sv with the
    columns the reference's loader and the models read."""
    n = len(rows)
    sv = synth.make_servants(n, n_envs=n_envs, seed=1)
    for s, (ver, envs, nproc, load, maxt, run, low, ip) in enumerate(rows):
        sv["version"][s], sv["num_processors"][s], sv["current_load"][s] = ver, nproc, load
        sv["max_tasks"][s], sv["running_tasks"][s], sv["ip"][s] = maxt, run, ip
        sv["env_mask"][s] = sum(1 << e for e in envs)
        sv["total_memory"][s] = 64 << 30
        sv["memory_available"][s] = (1 << 20) if low else (32 << 30)
    return sv


def model_row(sv, env, minv):
    o = OM.outlook(sv, pack.to_abi_columns(sv)["flags"], sv["running_tasks"], [env], [minv])
    return {k: int(o[k][0]) for k in SUPPLY}


OUTSIDER = (172 << 24) + (16 << 16) + 9  # a host that owns no servant
HOST = lambda k: (10 << 24) + 1 + k


def foreign_load_pool():
    """Capacity grows with running_tasks while current_load covers them (first
    quirk): row 0 shows capacity_available 3 at running_tasks 0 and still takes 6 grants."""
    rows = [(20, [0], 8, 5, 6, 0, False, HOST(0)), (20, [0], 4, 3, 8, 2, False, HOST(1)),
            (20, [0, 1], 16, 9, 12, 4, False, HOST(2)), (19, [0], 8, 7, 8, 1, False, HOST(3)),
            (20, [1], 8, 0, 3, 0, False, HOST(4)), (20, [0], 8, 9, 4, 0, False, HOST(5)),
            (20, [0], 8, 0, 0, 0, False, HOST(6)), (20, [0], 16, 5, 2, 5, True, HOST(7))]
    rows += [(20, [s % 2], 6 + s % 5, s % 4, 2 + s % 3, s % 2, False, HOST(8 + s)) for s in range(40)]
    return registry(rows), OUTSIDER


def own_servant_is_the_last_resort_pool():
    """Every servant but the requestor's own is taken; the grant call still succeeds (:392-396), so
    the slots of a requestor's own servant count."""
    rows = [(20, [0], 8, 0, 3, 0, False, HOST(0))]
    rows += [(20, [0], 4, 0, 2, 2, False, HOST(1 + s)) for s in range(20)]
    return registry(rows), HOST(0)


def saturated_pool():
    rows = [(20, [0, 1], 4, 0, 2, 2, False, HOST(s)) for s in range(30)]
    rows += [(20, [0], 8, 12, 4, 0, False, HOST(30)), (20, [1], 8, 0, 4, 1, True, HOST(31))]
    return registry(rows), OUTSIDER


@needs_ref
@pytest.mark.parametrize("pool", [foreign_load_pool, own_servant_is_the_last_resort_pool, saturated_pool])
def test_the_reference_grants_exactly_grants_available(pool):
    sv, requestor = pool()
    assert len(sv["version"]) <= 64
    ip = RM.ip_string(requestor)
    kinds = set()
    for env, minv in itertools.product((0, 1, 5), (0, 20, 21)):
        want = model_row(sv, env, minv)
        ref = R.RefDispatcher()
        try:
            ref.load_servants(sv)
            answers = [ref.wait_for_starting_new_task(ip, R.digest_name(env), minv, expires_in_ms=1000, timeout_in_ms=0)[0]
                       for _ in range(want["grants_available"] + 1)]
        finally:
            ref.close()
        granted = sum(1 for a in answers if a == R.OK)
        assert granted == want["grants_available"] and answers[-1] != R.OK, (env, minv, want, answers[-3:])
        assert answers[:granted] == [R.OK] * granted  # (nothing frees in between: a prefix)
        assert (want["eligible"] == 0) == (answers[0] == R.ENV_NOT_FOUND), (env, minv, want, answers[0])
        assert (want["free_servants"] == 0 and want["eligible"] > 0) == (answers[0] == R.TIMEOUT), (env, minv, want)
        kinds.add(answers[0])
    assert R.ENV_NOT_FOUND in kinds
    if pool is foreign_load_pool:
        sv0 = model_row(sv, 0, 0)
        assert sv0["grants_available"] > sv0["capacity_available"] - sv0["running_tasks"] > 0  # (the quirk shows)
    if pool is own_servant_is_the_last_resort_pool:
        assert model_row(sv, 0, 0)["free_servants"] == 1 and model_row(sv, 0, 0)["grants_available"] == 3
    if pool is saturated_pool:
        assert kinds == {R.ENV_NOT_FOUND, R.TIMEOUT}


def test_closed_form_of_the_grants_equals_the_rule():
    """grants() (servant_slot_count) against :354 / :123 applied one grant at a time, over every
    small servant."""
    for nproc, load, maxt, run, low in itertools.product(range(7), range(9), range(7), range(8), (False, True)):
        assert OM.grants(nproc, load, maxt, run, low) == OM.grants_by_rule(nproc, load, maxt, run, low), (
            nproc, load, maxt, run, low)


def test_hand_written_registries():
    A, B = 0, 1
    #        version envs   nproc load max_tasks running low_memory
    rows = [(20, [A, B], 8, 2, 4, 1, False, HOST(0)),   # :308 foreign = 2 - 1 = 1; :311 8 - 1 = 7; :312 min(4, 7) = 4; :354 1 < 4: free;
                                                        #   grants at running 1, 2, 3 (capacity stays 4): 3
            (19, [A], 8, 11, 4, 0, False, HOST(1)),     # :308 foreign 11; :311 max(8 - 11, 0) = 0; :312 0; :354 0 >= 0: not free
            (20, [B], 16, 5, 2, 5, True, HOST(2)),      # :291 low memory: capacity = running = 5; :354 5 >= 5: not free
            (20, [A], 8, 0, 0, 0, False, HOST(3))]      # :330 max_tasks == 0: never eligible
    sv = registry(rows)
    flags = pack.to_abi_columns(sv)["flags"]
    assert [bool(f & IM.LOW_MEMORY) for f in flags] == [False, False, True, False]
    env = [A, A, B, B, 2, 64]
    minv = [0, 20, 20, 21, 0, 0]
    queue = (np.array([A, A, B, 7, 0xFFFF]), np.array([3, 1, 2, 9, 4]))
    leases = (np.array([A, OM.NO_ID, B, A, 9], np.uint32), np.array([0, 1, 1, 1, 1], np.uint8))
    o = OM.outlook(sv, flags, sv["running_tasks"], env, minv, queue, leases)
    want = {"eligible": [2, 1, 2, 0, 0, 0],             # :333 version 19 < 20 drops row 1
            "free_servants": [1, 1, 1, 0, 0, 0],
            "grants_available": [3, 3, 3, 0, 0, 0],
            "running_tasks": [1, 1, 6, 0, 0, 0],
            "max_tasks": [8, 4, 6, 0, 0, 0],
            "capacity_available": [4, 4, 9, 0, 0, 0],   # (B, 20): rows 0 and 2: 4 + 5
            "waiting": [2, 2, 1, 1, 0, 0],              # by digest alone; env 7 / 0xFFFF are nobody's query
            "waiting_rows": [4, 4, 2, 2, 0, 0],
            "leases": [2, 2, 1, 1, 0, 0],               # the lease without a record counts for no digest
            "zombies": [1, 1, 1, 1, 0, 0]}
    for k in OM.COLUMNS:
        assert o[k].dtype == OM.DTYPES[k] and o[k].tolist() == want[k], (k, o[k].tolist(), want[k])
    off = OM.outlook(sv, flags, sv["running_tasks"], env, minv, None, None)
    assert (off["leases"] == OM.UNKNOWN).all() and (off["zombies"] == OM.UNKNOWN).all() and not off["waiting"].any()
    # The quirk by hand, and 64-bit sums.
    rows = [(20, [A], 8, 5, 6, 0, False, HOST(0)),      # capacity: foreign 5, 8 - 5 = 3, min(6, 3) = 3. Grants: at running r the
                                                        #   foreign load is 5 - r: capacity 3, 4, 5, 6, 6, 6 at r = 0 .. 5, r = 6: 6 >= 6. 6 grants
            (20, [A], 4, 3, 8, 2, False, HOST(1))]      # capacity: foreign 1, 4 - 1 = 3, min(8, 3) = 3. r = 2: 2 < 3; r = 3: foreign 0,
                                                        #   capacity 4: 3 < 4; r = 4: 4 >= 4. 2 grants
    sv = registry(rows)
    o = OM.outlook(sv, pack.to_abi_columns(sv)["flags"], sv["running_tasks"], [A], [0])
    assert [int(o[k][0]) for k in OM.COLUMNS[:6]] == [2, 2, 8, 2, 14, 6]
    big = registry([(20, [A], 0xFFFFFFFF, 0, 0xFFFFFFFF, 0, False, HOST(0)), (20, [A], 0xFFFFFFFF, 0, 0xFFFFFFFF, 1, False, HOST(1))])
    o = OM.outlook(big, pack.to_abi_columns(big)["flags"], big["running_tasks"], [A], [0])
    assert int(o["max_tasks"][0]) == 2 * 0xFFFFFFFF and int(o["grants_available"][0]) == 2 * 0xFFFFFFFF - 1
    assert int(o["capacity_available"][0]) == 2 * 0xFFFFFFFF


def test_waiting_view_of_each_queue_model_and_the_table_helper():
    from tests import stream_wait_model as WM
    q = WM.WaitQueue(8)
    q.cols = {"env_id": np.array([1, 0], np.uint32), "min_version": np.array([20, 0], np.uint32),
              "requestor_ip": np.array([7, 8], np.uint32)}
    q.deadline, q.tag = np.array([5, 9], np.int64), np.array([11, 12], np.uint64)
    w = OM.waiting(q)
    assert set(w) == set(OM.WAITING_COLUMNS) and w["n_immediate"].tolist() == [1, 1] and not w["n_prefetch"].any()
    assert not w["lease_for"].any() and w["tag"].tolist() == [11, 12] and w["env_id"].tolist() == [1, 0]
    assert OM.waiting(q, np.array([40, 50]))["lease_for"].tolist() == [40, 50]
    r = RM.RpcQueue()
    r.cols = dict(q.cols, n_imm=np.array([2, 0], np.uint32), n_pre=np.array([1, 4], np.uint32))
    r.lease_for, r.deadline, r.tag = np.array([3, 4], np.int64), q.deadline, q.tag
    w = OM.waiting(r)
    assert w["n_immediate"].tolist() == [2, 0] and w["n_prefetch"].tolist() == [1, 4] and w["lease_for"].tolist() == [3, 4]
    assert all(len(v) == 0 for v in OM.waiting(None).values())
    o = OM.outlook(registry([(20, [0], 8, 0, 4, 1, False, HOST(0))]), [0], [1], [0, 1], [0, 0])
    text = streaming.outlook_table(o, ["gcc-12", None], env_id=[0, 1], min_version=[0, 0])
    lines = text.splitlines()
    assert len(lines) == 3 and lines[0].split()[:3] == ["digest", "eligible", "free_servants"]
    assert lines[1].split()[0] == "gcc-12" and lines[2].split()[0] == "#1" and lines[1].split()[-1] == "-"
    assert binding.OUTLOOK_UNKNOWN == OM.UNKNOWN and binding.OUTLOOK_DTYPE.itemsize == 56

"""RPC ticks written by hand: what the handler's two loops (scheduler_service_impl.cc:233-264) do
that a seeded stream only meets by chance. One list of cases, played three ways: through the model
and through the verbatim reference class (tests/test_stream_rpc_model.py, field by field), and on
the GPU against the model (tests/test_stream_rpc_gpu.py).

The pool is stream_wait_lease_cases.small_stream's three idle servants. A step is (make, expect):
make(S, now) -> the tick's traffic written from the state S (W, L) as the previous ticks left it;
expect(r, S) asserts what the case is about, so a case that no longer meets its situation fails
instead of passing idly. An RPC is (n_immediate, n_prefetch, lease_for, wait[, env_id]).
"""
import numpy as np

from tests import stream_rpc_model as M
from tests import stream_wait_lease_cases as WC
from yadcc_amd import synth

MAX_REQUESTS = 8
MAX_ROWS = 509  # (not a multiple of 4)
MAX_WAITING = 16
HUGE = 300      # more rows than the pool has slots


def small_stream(max_leases=1 << 30, max_rows=MAX_ROWS, max_waiting=MAX_WAITING):
    sv = WC.small_stream().es.sv
    ws = M.new_stream(sv, MAX_REQUESTS, 0, 0, max_waiting, max_rows, n_envs=1, max_leases=max_leases,
                      rate=lambda now: 1.0)
    ws.es.hb = ws.es.n  # every servant sends its heartbeat in every tick
    return ws


def scripted(ws, ev, rpcs=(), renew=(), free=(), reports=()):
    """The drawn tick `ev` with its heartbeats kept and everything else written by hand."""
    now, n = int(ev["now"]), len(rpcs)
    off = np.cumsum([0] + [len(ids) for _, ids in reports]).astype(np.uint32)
    tk = synth.make_tasks(n, ws.es.sv, n_envs=1, seed=500 + now, self_frac=0.0)
    for i, r in enumerate(rpcs):
        if len(r) > 4:
            tk["env_id"][i] = r[4]
    e = dict(ev)
    e.update(tasks=tk, release_idx=np.empty(0, np.uint32),
             n_immediate=np.array([r[0] for r in rpcs], np.uint32), n_prefetch=np.array([r[1] for r in rpcs], np.uint32),
             lease_for=np.array([r[2] for r in rpcs], np.int64), deadlines=now + np.array([r[3] for r in rpcs], np.int64),
             tags=np.arange(1000 * now, 1000 * now + n, dtype=np.uint64),
             renew_ids=np.array([r[0] for r in renew], np.uint64),
             renew_expires_at=np.array([r[1] for r in renew], np.int64), free_ids=np.array(free, np.uint64),
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


def an_unknown_digest_fails_the_rpc_only_in_the_immediate_loop():
    """n_immediate == 0 on a digest nobody has: the prefetch loop breaks, NO_QUOTA (TIMEOUT although
    the deadline is ahead: nothing waits). n_immediate == 1: ENV_NOT_FOUND."""
    def expect(r, S):
        assert list(r["status"]) == [M.IDX_TIMEOUT, M.IDX_ENV_NOT_FOUND] and list(r["n_granted"]) == [0, 0]
        assert r["n_waiting"] == 0 and r["no_quota_unknown"] == 1 and r["env_failed"] == 1 and S.T.next_id == 0
    return [(lambda S, now: dict(rpcs=[(0, 2, 9, 5, 0xFFFF), (1, 2, 9, 5, 0xFFFF)]), expect)]


def a_waiting_rpc_of_3_plus_2_is_granted_4_in_a_later_tick():
    seen = {}

    def waits(r, S):
        assert list(r["status"]) == [0, M.IDX_WAITING] and r["n_waiting"] == 1 and r["n_waiting_rows"] == 5
        seen.update(next_id=S.T.next_id)

    def expect(r, S):
        assert r["freed"] == 4 and list(r["res_status"]) == [0] and list(r["res_n_granted"]) == [4]
        assert list(r["res_first"]) == [0] and list(r["res_tags"]) == [1]
        assert list(r["res_task_ids"]) == list(range(seen["next_id"], seen["next_id"] + 4))
        # (the fifth row is dropped, never queued; the leases run from THIS tick)
        assert r["n_waiting"] == 0 and r["n_waiting_rows"] == 0 and r["partial"] == 1
        assert all(S.T.L[t][1] == 1 + 7 for t in r["res_task_ids"].tolist())
    return [(lambda S, now: dict(rpcs=[(HUGE - 1, 1, 100, 0), (3, 2, 7, 40)]), waits),
            (lambda S, now: dict(free=[0, 1, 2, 3]), expect)]


def a_waiting_rpc_whose_deadline_is_now():
    """Its deadline is 2. At now == 2 three ids are freed: it resolves as TIMEOUT, untried, with 0
    grants, and a new RPC of that tick takes the slots and the next ids."""
    seen = {}

    def still(r, S):
        assert r["n_waiting"] == 1 and r["w_expired"] == 0 and len(r["res_tags"]) == 0
        seen.update(next_id=S.T.next_id)

    def expect(r, S):
        assert list(r["res_status"]) == [M.IDX_TIMEOUT] and list(r["res_n_granted"]) == [0] and r["w_expired"] == 1
        assert list(r["status"]) == [0] and list(r["n_granted"]) == [3] and r["n_waiting"] == 0
        assert list(r["task_ids"]) == list(range(seen["next_id"], seen["next_id"] + 3))
    return [(lambda S, now: dict(rpcs=[(HUGE - 1, 1, 100, 0), (2, 2, 7, 2)]), None),
            (lambda S, now: {}, still),
            (lambda S, now: dict(free=[0, 1, 2], rpcs=[(1, 3, 5, 0)]), expect)]


def an_id_is_freed_in_the_tick_its_rpc_sibling_is_renewed():
    """Ids 0, 1, 2 are one RPC's grants: 1 is freed, 0 renewed, 2 left alone, in one tick."""
    def granted(r, S):
        assert list(r["n_granted"]) == [3] and sorted(S.T.L) == [0, 1, 2]

    def expect(r, S):
        assert r["freed"] == 1 and list(r["renewed"]) == [1] and sorted(S.T.L) == [0, 2]
        assert S.T.L[0][1] == 77 and S.T.L[2][1] == 0 + 9
    return [(lambda S, now: dict(rpcs=[(2, 1, 9, 0)]), granted),
            (lambda S, now: dict(free=[1], renew=[(0, 77)]), expect)]


CASES = [an_unknown_digest_fails_the_rpc_only_in_the_immediate_loop,
         a_waiting_rpc_of_3_plus_2_is_granted_4_in_a_later_tick, a_waiting_rpc_whose_deadline_is_now,
         an_id_is_freed_in_the_tick_its_rpc_sibling_is_renewed]


def refusals(tick, refused):
    """rows == 0 and each capacity refusal at exactly the bound (accepted) and one above (refused),
    with the state unchanged afterwards. tick(ws, ev) plays a tick and returns its record;
    refused(ws, ev, what) asserts that the tick is refused for `what` and that nothing was applied."""
    # max_rows: rows(W) + rows(new) == max_rows is taken, one more row is not.
    ws = small_stream(max_rows=HUGE + 5)
    r = tick(ws, scripted(ws, ws.next_tick(), rpcs=[(HUGE - 1, 1, 100, 0), (3, 2, 7, 40)]))
    assert r["n_waiting_rows"] == 5
    refused(ws, scripted(ws, ws.next_tick(), rpcs=[(HUGE, 1, 7, 40)]), "max_rows")
    refused(ws, scripted(ws, ws.next_tick(), rpcs=[(1, 0, 7, 40), (0, 0, 7, 40)]), "rows == 0")
    r = tick(ws, scripted(ws, ws.next_tick(), rpcs=[(HUGE, 0, 7, 40)]))
    assert r["n_waiting"] == 2 and r["n_waiting_rows"] == HUGE + 5
    # max_waiting: |W| + n_req == max_waiting is taken, one more request is not.
    ws = small_stream(max_waiting=3)
    r = tick(ws, scripted(ws, ws.next_tick(), rpcs=[(HUGE - 1, 1, 100, 0), (1, 0, 7, 40)]))
    assert r["n_waiting"] == 1
    refused(ws, scripted(ws, ws.next_tick(), rpcs=[(1, 0, 7, 40)] * 3), "max_waiting")
    r = tick(ws, scripted(ws, ws.next_tick(), rpcs=[(1, 0, 7, 40)] * 2))
    assert r["n_waiting"] == 3
    # max_leases: |L| + rows(W) + rows(new) == max_leases is taken, one more row is not.
    ws = small_stream()
    r = tick(ws, scripted(ws, ws.next_tick(), rpcs=[(HUGE - 1, 1, 100, 0), (3, 2, 7, 40)]))
    held = int(r["n_granted"][0])
    ws = small_stream(max_leases=held + 5 + 4)
    tick(ws, scripted(ws, ws.next_tick(), rpcs=[(held, 0, 100, 0), (3, 2, 7, 40)]))
    refused(ws, scripted(ws, ws.next_tick(), rpcs=[(2, 3, 7, 40)]), "max_leases")
    r = tick(ws, scripted(ws, ws.next_tick(), rpcs=[(2, 2, 7, 40)]))
    assert r["n_leases"] == held and r["n_waiting_rows"] == 9

"""The waiting + leased model (tests/stream_wait_lease_model.py, a composition of the waiting
queue's and the lease table's models) against the verbatim reference class: the yardstick of
tests/test_stream_wait_lease_gpu.py pinned on the CPU. Tick by tick and field by field the model and
the reference replay agree on small seeded streams; the model reproduces the committed cfg5
fixture; a hand case with literal values pins what is new in this mode (a lease runs from its
grant; the queue's grants take their ids first); the hand-written ticks of
tests/stream_wait_lease_cases.py go through the verbatim class tick by tick; the ABI carries the
feature without a new version."""
import os
import re

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_wait_lease_cases as cases
from tests import stream_wait_lease_model as M
from tests.conftest import ROOT
from yadcc_amd import binding, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ref_stream_wait_lease_cfg5_ticks.npz")


def same_records(got, want):
    assert len(got) == len(want)
    for t, (x, y) in enumerate(zip(got, want)):
        for k in M.FIELDS:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), "tick %d: %s differs" % (t, k)


@needs_ref
@pytest.mark.parametrize("shape", [
    # servants, requests / tick, frees / tick, renewals / tick, ticks, digests, servant seed, max_waiting
    (60, 300, 200, 60, 80, 2, 3, 1500),
    (150, 600, 400, 100, 80, 2, 42, 3000),
    (90, 400, 250, 80, 80, 3, 8, 2000),
])
def test_model_agrees_with_the_reference_replay(shape):
    n_sv, tasks, frees, renewals, ticks, n_envs, seed, mw = shape
    sv = synth.make_servants(n_sv, n_tasks_hint=tasks * 6, n_envs=n_envs, seed=seed)
    got = M.run_model(sv, tasks, frees, renewals, ticks, mw, n_envs=n_envs)
    want = M.run_reference(sv, tasks, frees, renewals, ticks, mw, n_envs=n_envs)
    same_records(got, want)
    M.check_conditions(M.digests(got))


def test_model_reproduces_the_fixture():
    fx = np.load(FIXTURE)
    M.check_conditions(fx)
    assert int(fx["ticks"]) >= 60 and int(fx["tasks"]) >= 2000
    sv, _ = synth.make_config("cfg5")
    assert len(sv["version"]) == 2000
    rec = M.run_model(sv, int(fx["tasks"]), int(fx["frees"]), int(fx["renewals"]), int(fx["ticks"]),
                      int(fx["max_waiting"]))
    for k, v in M.digests(rec).items():
        bad = np.nonzero(v != fx[k])[0]
        assert bad.size == 0, "%s differs from tick %d on" % (k, bad[0])


def _ev(now, n=0, lease_for=(), deadlines=(), tags=(), free=()):
    z = np.zeros(n, np.uint32)
    return {"now": now, "release_idx": np.empty(0, np.uint32), "tasks": {"env_id": z, "min_version": z, "requestor_ip": z},
            "lease_for": np.array(lease_for, np.int64), "deadlines": np.array(deadlines, np.int64),
            "tags": np.array(tags, np.uint64), "renew_ids": np.empty(0, np.uint64),
            "renew_expires_at": np.empty(0, np.int64), "free_ids": np.array(free, np.uint64),
            "report_servants": np.empty(0, np.uint32), "report_off": np.zeros(1, np.uint32),
            "report_ids": np.empty(0, np.uint64)}


def test_model_semantics_by_hand():
    """Two servants, one slot each; every placement is scripted (a request gets the first servant
    with running_tasks == 0, in batch order)."""
    S = M.WaitLeaseState(max_waiting=4, max_leases=5)
    run = np.zeros(2, np.int64)

    def place(batch):
        out = []
        for _ in range(len(batch["env_id"])):
            free = np.nonzero(run == 0)[0]
            out.append(int(free[0]) if len(free) else M.IDX_TIMEOUT)
            if len(free):
                run[free[0]] += 1
        return np.array(out, np.uint32)

    # tick 0: three requests, two slots. The third waits with lease_for = 5.
    r = S.tick(run, _ev(0, 3, lease_for=[100, 100, 5], deadlines=[9, 9, 9], tags=[7, 8, 9]), place)
    assert list(r["out"]) == [0, 1, M.IDX_WAITING] and list(r["task_id"]) == [0, 1, M.NO_ID]
    assert r["n_waiting"] == 1 and list(S.lease_for) == [5] and S.T.next_id == 2
    # ticks 1, 2: no room, it stays (no id is consumed by a try).
    for now in (1, 2):
        r = S.tick(run, _ev(now), place)
        assert r["n_waiting"] == 1 and len(r["res_tags"]) == 0 and S.T.next_id == 2
    # tick 3: lease 1 is freed; the waiter and a new request are one batch, the waiter first. It gets
    # servant 1 and id 2; its lease runs from THIS tick: 3 + 5 == 8, not 0 + 5. The new request finds
    # nothing and waits. task_dispatcher.cc:127-135: next_task_id++ at the moment of the grant.
    r = S.tick(run, _ev(3, 1, lease_for=[6], deadlines=[9], tags=[10], free=[1]), place)
    assert list(r["res_tags"]) == [9] and list(r["res_idx"]) == [1] and list(r["res_ids"]) == [2]
    assert S.T.L[2] == [1, 8, False] and S.T.L[2][1] != 5
    assert list(r["out"]) == [M.IDX_WAITING] and r["n_waiting"] == 1 and list(S.lease_for) == [6]
    # tick 4: lease 0 is freed; the waiter (id 3) and a new request whose grant comes from the slot
    # that lease 2 gives back in the same tick (id 4): the queue's grant has the smaller id.
    r = S.tick(run, _ev(4, 1, lease_for=[1], deadlines=[4], tags=[11], free=[0, 2]), place)
    assert list(r["res_ids"]) == [3] and list(r["task_id"]) == [4] and r["res_ids"][0] < r["task_id"][0]
    assert r["w_granted"] == 1 and r["new_granted"] == 1
    assert S.T.L[3][1] == 4 + 6 and S.T.L[4][1] == 4 + 1 and r["n_leases"] == 2
    # a waiter whose deadline is now resolves as Timeout and consumes no id.
    r = S.tick(run, _ev(5, 1, lease_for=[1], deadlines=[6], tags=[12]), place)
    assert list(r["out"]) == [M.IDX_WAITING]
    r = S.tick(run, _ev(6, 0, free=[3]), place)
    assert list(r["res_tags"]) == [12] and list(r["res_idx"]) == [M.IDX_TIMEOUT] and list(r["res_ids"]) == [M.NO_ID]
    assert S.T.next_id == 5 and r["w_expired"] == 1 and r["n_waiting"] == 0
    # refusals leave everything untouched: |W| + n > max_waiting; |L| + |W| + n > max_leases; the clock.
    with pytest.raises(OverflowError, match="max_waiting"):
        S.tick(run, _ev(6, 5, lease_for=[1] * 5, deadlines=[9] * 5, tags=[0] * 5), place)
    r = S.tick(run, _ev(6, 4, lease_for=[1] * 4, deadlines=[9] * 4, tags=[1, 2, 3, 4]), place)
    assert r["n_waiting"] == 3 and r["n_leases"] == 2
    with pytest.raises(OverflowError, match="max_leases"):  # 2 + 3 + 1 > 5 although |L| + n is not
        S.tick(run, _ev(6, 1, lease_for=[1], deadlines=[9], tags=[0]), place)
    with pytest.raises(ValueError):
        S.tick(run, _ev(5), place)
    assert S.T.next_id == 6 and len(S.q) == 3 and list(run) == [1, 1]
    assert list(S.take()) == [2, 3, 4] and len(S.lease_for) == 0


def _play(case, tick_of):
    ws = cases.small_stream()
    rec = []
    tick = tick_of(ws)
    cases.play(ws, case(), lambda ev: rec.append(tick(ev)) or rec[-1])
    return ws, rec


@needs_ref
@pytest.mark.parametrize("case", cases.CASES, ids=[c.__name__ for c in cases.CASES])
def test_hand_written_ticks_model_against_the_reference_replay(case):
    """Every tick through the model and through the verbatim class, field by field; each step's own
    expectations are asserted on both records."""
    ws, got = _play(case, lambda ws: lambda ev: M.model_tick(ws, ev))
    snap = ws.table.snapshot()
    refs = []

    def with_ref(ws):
        refs.append(M.ReferenceReplay(ws))
        return refs[-1].tick
    try:
        ws, want = _play(case, with_ref)
    finally:
        refs[-1].close()
    assert len(got) == len(case())
    same_records(got, want)
    for a, b in zip(snap, ws.table.snapshot()):
        assert np.array_equal(a, b)


def test_hand_written_ticks_on_the_model_alone():
    """Without oracle/_ref the cases still hold their own expectations on the model."""
    for case in cases.CASES:
        _play(case, lambda ws: lambda ev: M.model_tick(ws, ev))


def test_abi_carries_the_waiting_leased_stream():
    assert binding.ABI_VERSION == 8
    src = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define YDC_ABI_VERSION 8u", src)
    for name in ("ydc_stream_begin_waiting_leased", "ydc_stream_tick_waiting_leased"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.ABI_SYMBOLS
        assert hasattr(binding.Context, name[4:])
    assert "out_resolved_task_id" in src and "lease_for" in src

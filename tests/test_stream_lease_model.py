"""The leased-mode model (tests/stream_lease_model.py) against the verbatim reference class: the
yardstick of tests/test_stream_lease_gpu.py pinned on the CPU. Tick by tick and field by field the
model (plain-C oracle placement, plain dict for the lease table) and the reference replay
(KeepTaskAlive, FreeTask, OnExpirationTimer, NotifyServantRunningTasks, WaitForStartingNewTask of
oracle/_ref) agree on small seeded streams; the model reproduces the committed cfg5 fixture; hand
cases with literal values pin the semantics to the reference lines; the hand-written ticks of
tests/stream_lease_cases.py (same-tick interactions) go through the verbatim class tick by tick; the ABI carries the feature."""
import os
import re

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_lease_cases as cases
from tests import stream_lease_model as M
from tests.conftest import ROOT
from yadcc_amd import binding, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ref_stream_lease_cfg5_ticks.npz")


@needs_ref
@pytest.mark.parametrize("shape", [
    # servants, requests / tick, frees / tick, renewals / tick, ticks, digests, servant seed
    (60, 300, 200, 60, 40, 2, 3),
    (150, 600, 400, 100, 40, 2, 42),
    (90, 400, 250, 80, 40, 3, 8),
])
def test_model_agrees_with_the_reference_replay(shape):
    n_sv, tasks, frees, renewals, ticks, n_envs, seed = shape
    sv = synth.make_servants(n_sv, n_tasks_hint=tasks * 6, n_envs=n_envs, seed=seed)
    got = M.run_model(sv, tasks, frees, renewals, ticks, n_envs=n_envs)
    want = M.run_reference(sv, tasks, frees, renewals, ticks, n_envs=n_envs)
    assert len(got) == len(want)
    for t, (x, y) in enumerate(zip(got, want)):
        for k in M.FIELDS:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), "tick %d: %s differs" % (t, k)
    M.check_conditions(M.digests(got))


def test_model_reproduces_the_fixture():
    fx = np.load(FIXTURE)
    M.check_conditions(fx)
    assert int(fx["ticks"]) >= 60 and int(fx["tasks"]) >= 2000
    sv, _ = synth.make_config("cfg5")
    assert len(sv["version"]) == 2000
    rec = M.run_model(sv, int(fx["tasks"]), int(fx["frees"]), int(fx["renewals"]), int(fx["ticks"]))
    for k, v in M.digests(rec).items():
        bad = np.nonzero(v != fx[k])[0]
        assert bad.size == 0, "%s differs from tick %d on" % (k, bad[0])


def _ev(now, tasks=0, lease=(), renew=(), free=(), reports=()):
    """A tick's lease columns; reports: [(servant, [ids])]."""
    off = np.cumsum([0] + [len(ids) for _, ids in reports]).astype(np.uint32)
    z = np.zeros(tasks, np.uint32)
    return {"now": now, "release_idx": np.empty(0, np.uint32),
            "tasks": {"env_id": z, "min_version": z, "requestor_ip": z},
            "lease_expires_at": np.array(lease, np.int64),
            "renew_ids": np.array([r[0] for r in renew], np.uint64),
            "renew_expires_at": np.array([r[1] for r in renew], np.int64),
            "free_ids": np.array(free, np.uint64),
            "report_servants": np.array([s for s, _ in reports], np.uint32), "report_off": off,
            "report_ids": np.array([t for _, ids in reports for t in ids], np.uint64)}


def test_model_semantics_by_hand():
    """Two servants; every placement is scripted."""
    T = M.LeaseTable(max_leases=8)
    run = np.zeros(2, np.int64)

    def placing(answers):
        def place(_):
            a = np.array(answers, np.uint32)
            np.add.at(run, a[a < M.IDX_ENV_NOT_FOUND], 1)
            return a
        return place

    # task_dispatcher.cc:127-135: the first id is next_task_id{} == 0; only grants take ids.
    r = T.tick(run, _ev(0, 5, lease=[3, 3, 3, 3, 10]), placing([0, M.IDX_TIMEOUT, 1, M.IDX_ENV_NOT_FOUND, 0]))
    assert list(r["task_id"]) == [0, M.NO_ID, 1, M.NO_ID, 2] and T.next_id == 3 and r["n_leases"] == 3
    assert list(run) == [2, 1]
    # :142-167 with :522-535: at now == 4 lease 0 (expires_at 3) is overdue, but the timer has not
    # fired since: the renewal in the same tick arrives first and succeeds; lease 1 becomes a zombie.
    r = T.tick(run, _ev(4, renew=[(0, 9), (7, 9)]), None)
    assert list(r["renewed"]) == [1, 0] and r["expired"] == 1 and r["renew_refused"] == 1
    assert [list(c) for c in T.snapshot()] == [[0, 1, 2], [0, 1, 0], [9, 3, 10], [0, 1, 0]]
    assert list(run) == [2, 1]  # a zombie keeps its slot
    # :156-165 a zombie cannot be renewed; :453-476 a report that lists it keeps it, :264-275 and the
    # id comes back as unknown (a zombie is not "permitted"); a live lease of the servant is known; a
    # live lease of another servant is unknown.
    r = T.tick(run, _ev(5, renew=[(1, 50)], reports=[(1, [1, 0])]), None)
    assert list(r["renewed"]) == [0] and list(r["report_unknown"]) == [1, 1] and r["swept"] == 0
    assert r["n_leases"] == 3 and r["kept_zombies"] == 0
    # servant 0 reports, servant 1 does not: its zombie survives.
    r = T.tick(run, _ev(5, reports=[(0, [0, 2, 99])]), None)
    assert list(r["report_unknown"]) == [0, 0, 1] and r["swept"] == 0 and r["kept_zombies"] == 1
    # a report without the id sweeps the zombie: running_tasks - 1, lease erased.
    r = T.tick(run, _ev(6, reports=[(1, [])]), None)
    assert r["swept"] == 1 and list(run) == [2, 0] and r["n_leases"] == 2
    # :169-188 freeing a zombie returns the slot; the same id again and an unknown id are ignored.
    r = T.tick(run, _ev(11, free=[], renew=[]), None)  # lease 0 (9) and lease 2 (10) expire
    assert r["expired"] == 2
    r = T.tick(run, _ev(11, free=[0, 0, 42]), None)
    assert r["freed"] == 1 and r["ignored_frees"] == 2 and list(run) == [1, 0]
    # ids go on from next_id whatever was freed.
    r = T.tick(run, _ev(12, 2, lease=[20, 20]), placing([M.IDX_TIMEOUT, 1]))
    assert list(r["task_id"]) == [M.NO_ID, 3] and [list(c) for c in T.snapshot()][0] == [2, 3]
    # refusals leave everything untouched.
    with pytest.raises(ValueError):
        T.tick(run, _ev(11), None)
    with pytest.raises(OverflowError):
        T.tick(run, _ev(12, 7, lease=[20] * 7), placing([0] * 7))
    with pytest.raises(ValueError):
        T.tick(run, _ev(12, reports=[(0, []), (0, [])]), None)
    assert T.next_id == 4 and len(T) == 2 and list(run) == [1, 1]
    # ydc_remove_servants: the leases of the removed row vanish, the others' rows move up.
    T.remove_servants([0])
    assert [list(c) for c in T.snapshot()][:2] == [[3], [0]]


@needs_ref
@pytest.mark.parametrize("case", cases.CASES, ids=[c.__name__ for c in cases.CASES])
def test_hand_written_ticks_model_against_the_reference_replay(case):
    """The same-tick interactions of tests/stream_lease_cases.py: every tick through the model and
    through the verbatim class, field by field; each step's own expectations are asserted on both
    records."""
    got, want = [], []
    ls = cases.small_stream()
    cases.play(ls, case(), lambda ev: got.append(M.model_tick(ls, ev)) or got[-1])
    snap = ls.table.snapshot()
    ls = cases.small_stream()
    ref = M.ReferenceReplay(ls)
    try:
        cases.play(ls, case(), lambda ev: want.append(ref.tick(ev)) or want[-1])
    finally:
        ref.close()
    assert len(got) == len(want) == len(case())
    for t, (x, y) in enumerate(zip(got, want)):
        for k in M.FIELDS:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), "tick %d: %s differs" % (t, k)
    for a, b in zip(snap, ls.table.snapshot()):
        assert np.array_equal(a, b)


def test_hand_written_ticks_on_the_model_alone():
    """Without oracle/_ref the cases still hold their own expectations on the model."""
    for case in cases.CASES:
        ls = cases.small_stream()
        cases.play(ls, case(), lambda ev: M.model_tick(ls, ev))


def test_abi_carries_the_leased_stream():
    assert binding.ABI_VERSION == 8
    src = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define YDC_ABI_VERSION 8u", src)
    for name in ("ydc_stream_begin_leased", "ydc_stream_tick_leased", "ydc_stream_leases_get"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.ABI_SYMBOLS
    for k in ("leases_expired", "leases_swept", "leases_freed", "renewals_refused"):
        assert k in src and k in dict(binding.Stats._fields_)
    assert [k for k, _ in binding.Stats._fields_][-5] == "stage_ms"  # appended behind the old fields

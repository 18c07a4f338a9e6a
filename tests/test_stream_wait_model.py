"""The waiting-mode model (tests/stream_wait_model.py) against the verbatim reference class: the
yardstick of tests/test_stream_waiting_gpu.py pinned on the CPU. Tick by tick, on small saturated
streams, the model (plain-C oracle placement) and the reference replay (sequential
WaitForStartingNewTask calls of oracle/_ref) give the same answers, resolved lists, queue sizes
and running_tasks; and the model reproduces the committed fixture."""
import os

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_wait_model as M
from yadcc_amd import synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ref_stream_wait_cfg5_60_ticks.npz")


def same_records(a, b):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k, name in enumerate(("out", "resolved_tags", "resolved_idx", "n_waiting", "running")):
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), "tick %d: %s differs" % (t, name)


@needs_ref
@pytest.mark.parametrize("shape", [
    # servants, requests / tick, frees / tick, ticks, max_waiting, digests, servant seed
    (60, 900, 120, 25, 3000, 2, 3),
    (150, 1500, 200, 30, 4000, 2, 42),
    (90, 700, 150, 30, 2500, 3, 8),
])
def test_model_agrees_with_the_reference_replay(shape):
    n_sv, tasks, frees, ticks, mw, n_envs, seed = shape
    sv = synth.make_servants(n_sv, n_tasks_hint=tasks * 6, n_envs=n_envs, seed=seed)
    got = M.run_model(sv, tasks, frees, ticks, mw, n_envs=n_envs)
    want = M.run_reference(sv, tasks, frees, ticks, mw, n_envs=n_envs)
    same_records(got, want)
    # the streams are saturated: requests wait, waiters get served, some expire, the queue is
    # near its bound (new requests are cut to the room left)
    waited = sum(int((r[0] == M.IDX_WAITING).sum()) for r in got)
    served = sum(int((r[2] < M.IDX_WAITING).sum()) for r in got)
    expired = sum(int((r[2] == M.IDX_TIMEOUT).sum()) for r in got)
    assert waited > 0 and served > 0 and expired > 0, (waited, served, expired)


def test_model_reproduces_the_fixture():
    fx = np.load(FIXTURE)
    sv, _ = synth.make_config("cfg5")
    rec = M.run_model(sv, int(fx["tasks"]), int(fx["frees"]), int(fx["ticks"]), int(fx["max_waiting"]))
    d = M.digests(rec)
    for k, v in d.items():
        bad = np.nonzero(v != fx[k])[0]
        assert bad.size == 0, "%s differs from tick %d on" % (k, bad[0])
    assert fx["n_waiting"].max() > 5000 and fx["n_resolved"].sum() > 0


def test_model_semantics_by_hand():
    """One servant with two slots: the queue goes first, expiry precedes placement, a new request
    whose deadline has passed is Timeout and never queued, the queue keeps arrival order."""
    q = M.WaitQueue(8)
    free = [2]

    def place(batch):  # every request asks for the same digest; `free` slots left
        out = []
        for e in batch["env_id"]:
            if e == 9:
                out.append(M.IDX_ENV_NOT_FOUND)
            elif free[0]:
                free[0] -= 1
                out.append(0)
            else:
                out.append(M.IDX_TIMEOUT)
        return np.array(out, np.uint32)

    tk = lambda envs: {"env_id": np.array(envs, np.uint32), "min_version": np.zeros(len(envs), np.uint32),
                       "requestor_ip": np.zeros(len(envs), np.uint32)}
    out, rt, ri, nw, _ = q.tick(place, tk([1, 1, 1, 1, 1]), [0, 5, 3, 9, 0], [10, 11, 12, 13, 14], now=0)
    assert list(out) == [0, 0, M.IDX_WAITING, M.IDX_WAITING, M.IDX_TIMEOUT] and len(rt) == 0 and nw == 2
    free[0] = 1
    out, rt, ri, nw, _ = q.tick(place, tk([1, 9]), [9, 9], [20, 21], now=3)
    # tag 12 expired (deadline 3 <= 3) untried; tag 13 takes the slot ahead of the new request
    assert list(rt) == [12, 13] and list(ri) == [M.IDX_TIMEOUT, 0]
    assert list(out) == [M.IDX_WAITING, M.IDX_ENV_NOT_FOUND] and nw == 1
    with pytest.raises(ValueError):
        q.tick(place, tk([]), [], [], now=2)
    with pytest.raises(OverflowError):
        q.tick(place, tk([1] * 8), [9] * 8, list(range(8)), now=4)
    assert list(q.take()) == [20] and len(q) == 0

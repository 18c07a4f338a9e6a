"""The rpc stream's model (tests/stream_rpc_model.py) against the verbatim reference class: the
yardstick of tests/test_stream_rpc_gpu.py pinned on the CPU. The replay runs the handler's two loops
(scheduler_service_impl.cc:233-264) literally per RPC; model and replay agree tick by tick and field
by field on seeded saturate-then-relax streams, on the committed cfg5 fixture and on the
hand-written ticks of tests/stream_rpc_cases.py. The shares that make a stream prove something are
checked on the reference's own record."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_rpc_cases as cases
from tests import stream_rpc_model as M
from tests.conftest import ROOT
from yadcc_amd import binding, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ref_stream_rpc_cfg5_ticks.npz")
BIG = dict(imm=[0, 1, 2, 8, 32, 64], pre=[0, 2, 8, 24, 100])  # (few large RPCs: many are granted partially)


def same_records(got, want):
    assert len(got) == len(want)
    for t, (x, y) in enumerate(zip(got, want)):
        for k in M.FIELDS:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), "tick %d: %s differs" % (t, k)


@needs_ref
@pytest.mark.parametrize("shape", [
    # servants, RPCs / tick, frees / tick, renewals / tick, ticks, digests, servant seed, max_waiting
    (60, 8, 150, 60, 80, 2, 3, 200),
    (150, 10, 300, 100, 80, 2, 42, 300),
    (90, 10, 150, 80, 80, 3, 8, 300),
])
def test_model_agrees_with_the_reference_replay(shape):
    n_sv, rpcs, frees, renewals, ticks, n_envs, seed, mw = shape
    sv = synth.make_servants(n_sv, n_tasks_hint=rpcs * 60, n_envs=n_envs, seed=seed)
    got = M.run_model(sv, rpcs, frees, renewals, ticks, mw, mw * 20, n_envs=n_envs, **BIG)
    want = M.run_reference(sv, rpcs, frees, renewals, ticks, mw, mw * 20, n_envs=n_envs, **BIG)
    M.check_conditions(M.digests(want))  # (on the reference's own record: a vacuous stream fails)
    same_records(got, want)


def test_model_reproduces_the_fixture():
    fx = np.load(FIXTURE)
    M.check_conditions(fx)
    sv = M.cfg5_one_slot()
    assert len(sv["version"]) == 2000 and int(fx["ticks"]) >= 60
    rec = M.run_model(sv, int(fx["rpcs"]), int(fx["frees"]), int(fx["renewals"]), int(fx["ticks"]),
                      int(fx["max_waiting"]), int(fx["max_rows"]), **BIG)
    for k, v in M.digests(rec).items():
        bad = np.nonzero(v != fx[k])[0]
        assert bad.size == 0, "%s differs from tick %d on" % (k, bad[0])


def _play(case, tick_of):
    ws = cases.small_stream()
    rec = []
    tick = tick_of(ws)
    cases.play(ws, case(), lambda ev: rec.append(tick(ev)) or rec[-1])
    return ws, rec


@needs_ref
@pytest.mark.parametrize("case", cases.CASES, ids=[c.__name__ for c in cases.CASES])
def test_hand_written_ticks_model_against_the_reference_replay(case):
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


def test_refusals_on_the_model():
    def refused(ws, ev, what):
        S = ws.state
        before = (len(S.q), S.q.rows(), len(S.T), S.T.next_id, ws.es.running.copy())
        with pytest.raises((OverflowError, ValueError), match=what):
            S.tick(ws.es.running, ev, lambda batch: pytest.fail("a refused tick places nothing"))
        assert before[:4] == (len(S.q), S.q.rows(), len(S.T), S.T.next_id) and np.array_equal(before[4], ws.es.running)
    cases.refusals(lambda ws, ev: M.model_tick(ws, ev), refused)


def test_abi_carries_the_rpc_stream():
    """The two symbols are declared, listed and exported; the version stays 8 (no struct changed)."""
    assert binding.ABI_VERSION == 8
    src = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define YDC_ABI_VERSION 8u", src)
    so = os.path.join(ROOT, "yadcc_amd", "libydc.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("ydc_stream_begin_rpc", "ydc_stream_tick_rpc"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.ABI_SYMBOLS
        assert re.search(r"\b%s$" % name, exported, re.M), "%s is not exported by libydc.so" % name
        assert hasattr(binding.Context, name[4:])
    for word in ("n_immediate", "n_prefetch", "out_n_waiting_rows", "out_resolved_first"):
        assert word in src, word

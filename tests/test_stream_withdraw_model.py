"""The withdrawal model (tests/stream_withdraw_model.py) on the CPU: the yardstick of
tests/test_stream_withdraw_gpu.py.

The defining property, in all three modes, on seeded streams over a saturated small pool: apart from
the label IDX_WITHDRAWN every tick equals the tick of the BASE model (pinned to the verbatim
reference by the existing model tests) on the same stream in which the withdrawn requests had been
submitted with a deadline equal to the withdrawing tick's now; where oracle/_ref is built the
comparison run also goes through the verbatim class (the existing ReferenceReplay classes). Hand
cases with literal vectors, and the staging conventions as far as they are host logic."""
import os
import re

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WL
from tests import stream_wait_model as W
from tests import stream_withdraw_model as X
from tests.conftest import ROOT
from yadcc_amd import binding, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
WD, TO, WAITING, ENF = X.IDX_WITHDRAWN, W.IDX_TIMEOUT, W.IDX_WAITING, W.IDX_ENV_NOT_FOUND
WITHDRAW_AT = (3, 4, 9, 15, 16, 22)  # the ticks that stage something


def small_pool(n=12, seed=5, n_envs=1):
    """A pool one tick of requests saturates: one or two slots per servant, idle machines."""
    sv = synth.make_servants(n, n_tasks_hint=400, n_envs=n_envs, seed=seed)
    sv["max_tasks"] = (1 + np.arange(n) % 2).astype(np.uint32)
    sv["num_processors"][:], sv["current_load"][:] = 256, 0
    return sv


def pick(rng, q_tags, now):
    """The tags a withdrawing tick stages: a seeded third of W, unsorted, and two nobody has."""
    if now not in WITHDRAW_AT or not len(q_tags):
        return np.empty(0, np.uint64)
    some = rng.choice(q_tags, max(1, len(q_tags) // 3), replace=False)
    return np.concatenate([some, np.array([1 << 40, (1 << 64) - 1], np.uint64)]).astype(np.uint64)


def swapped(ev_tags, ev_deadlines, swap):
    """The deadlines of a comparison run: a request that the first run withdrew at `now` is submitted
    with that deadline."""
    dl = np.asarray(ev_deadlines, np.int64).copy()
    for i, t in enumerate(np.asarray(ev_tags).tolist()):
        if t in swap:
            dl[i] = swap[t]
    return dl


# ---- the defining property -----------------------------------------------------------------------

def _waiting_run(swap=None, ticks=28):
    ws = W.WaitingStream(small_pool(), 40, 6, 1500, seed=71)
    q = W.WaitQueue(1500)
    w = X.waiting(q, 4096)
    rng, rec, gone = np.random.default_rng(3), [], {}
    for _ in range(ticks):
        now, who, rows, rel, tk, dl, tags = ws.next_tick()
        if swap is None:
            staged = pick(rng, q.tag, now)
            w.stage(staged)
            before = q.tag.copy()
            out, rt, ri, nw, _ = w.run(W.oracle_place(ws.es), tk, dl, tags, now)
            gone.update({int(t): now for t in before[np.isin(before, staged)]})
            assert w.result[1] == int((ri == WD).sum()) and set(rt[ri == WD].tolist()) <= set(staged.tolist())
        else:
            out, rt, ri, nw, _ = q.tick(W.oracle_place(ws.es), tk, swapped(tags, dl, swap), tags, now)
        ws.commit(out, X.unlabelled(ri), nw)
        rec.append((out, rt, ri, nw, ws.es.running.astype(np.uint32)))
    return rec, gone


def test_defining_property_waiting():
    got, gone = _waiting_run()
    want, _ = _waiting_run(swap=gone)
    assert len(gone) > 30 and sum(int((r[2] == WD).sum()) for r in got) == len(gone)
    assert max(r[3] for r in got) > 100, "W is never deep"
    for t, (a, b) in enumerate(zip(got, want)):
        assert not (b[2] == WD).any()
        for k in (0, 1, 3, 4):
            assert np.array_equal(a[k], b[k]), (t, k)
        assert np.array_equal(X.unlabelled(a[2]), b[2]), t


def _leased_run(mode, swap=None, ticks=28, replay=False):
    M = WL if mode == "wl" else RM
    if mode == "wl":
        ws = WL.new_stream(small_pool(), 40, 6, 4, 1500)
        w = X.wait_lease(ws, 4096)
    else:
        ws = RM.new_stream(small_pool(), 40, 6, 4, 1500, 6000)
        w = X.rpc(ws, 4096)
    label = "res_idx" if mode == "wl" else "res_status"
    ref = M.ReferenceReplay(ws) if replay else None
    rng, rec, gone = np.random.default_rng(3), [], {}
    try:
        for _ in range(ticks):
            ev = ws.next_tick()
            now, q = int(ev["now"]), ws.state.q
            if swap is None:
                staged = pick(rng, q.tag, now)
                w.stage(staged)
                before = q.tag.copy()
                r = w.run(ev)
                gone.update({int(t): now for t in before[np.isin(before, staged)]})
                assert w.result[1] == int((r[label] == WD).sum())
            else:
                ev["deadlines"] = swapped(ev["tags"], ev["deadlines"], swap)
                r = ref.tick(ev) if replay else M.model_tick(ws, ev)
            r["next_id"], r["rows_w"] = ws.table.next_id, (q.rows() if mode == "rpc" else len(ws.state.q))
            rec.append(r)
    finally:
        if ref:
            ref.close()
    return rec, gone


def _same_but_for_the_label(mode, got, want, gone):
    M = WL if mode == "wl" else RM
    label = "res_idx" if mode == "wl" else "res_status"
    assert len(gone) > 20 and sum(int((r[label] == WD).sum()) for r in got) == len(gone)
    assert max(r["n_waiting"] for r in got) > 60, "W is never deep"
    for t, (a, b) in enumerate(zip(got, want)):
        assert not (b[label] == WD).any()
        for k in M.FIELDS + ("next_id", "rows_w"):
            x = X.unlabelled(a[k]) if k == label else np.asarray(a[k])
            assert np.array_equal(x, np.asarray(b[k])), "tick %d: %s differs" % (t, k)


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_defining_property_leased_modes(mode):
    got, gone = _leased_run(mode)
    want, _ = _leased_run(mode, swap=gone)
    _same_but_for_the_label(mode, got, want, gone)


@needs_ref
@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_defining_property_against_the_reference_replay(mode):
    """The comparison run through the verbatim class: a withdrawn call is a call whose max_wait ended in
    the withdrawing tick."""
    got, gone = _leased_run(mode)
    want, _ = _leased_run(mode, swap=gone, replay=True)
    _same_but_for_the_label(mode, got, want, gone)


# ---- hand cases, literal ---------------------------------------------------------------------------

def _ev(now, n=0, lease_for=(), deadlines=(), tags=(), free=(), imm=None, pre=None):
    z = np.zeros(n, np.uint32)
    ev = {"now": now, "release_idx": np.empty(0, np.uint32), "tasks": {"env_id": z, "min_version": z, "requestor_ip": z},
          "lease_for": np.array(lease_for, np.int64), "deadlines": np.array(deadlines, np.int64),
          "tags": np.array(tags, np.uint64), "renew_ids": np.empty(0, np.uint64),
          "renew_expires_at": np.empty(0, np.int64), "free_ids": np.array(free, np.uint64),
          "report_servants": np.empty(0, np.uint32), "report_off": np.zeros(1, np.uint32),
          "report_ids": np.empty(0, np.uint64)}
    if imm is not None:
        ev["n_immediate"], ev["n_prefetch"] = np.array(imm, np.uint32), np.array(pre, np.uint32)
    return ev


def _first_free(run):
    """A scripted placement: a request gets the first servant with running_tasks == 0, in batch order."""
    def place(batch):
        out = []
        for _ in range(len(batch["env_id"])):
            free = np.nonzero(run == 0)[0]
            out.append(int(free[0]) if len(free) else TO)
            if len(free):
                run[free[0]] += 1
        return np.array(out, np.uint32)
    return place


def _wl_state(slots=1, max_waiting=8):
    S = WL.WaitLeaseState(max_waiting=max_waiting, max_leases=64)
    run = np.zeros(slots, np.int64)
    w = X.Withdrawal(lambda: S.q, 8)
    tick = lambda ev: w.tick(lambda: S.tick(run, ev, _first_free(run)), "res_idx")  # noqa: E731
    return S, run, w, tick


def test_withdrawn_before_the_retry():
    """W = [A, B], the only slot is freed in the tick that withdraws A: B is granted, A consumed nothing."""
    S, run, w, tick = _wl_state()
    r = tick(_ev(0, 3, lease_for=[50, 50, 50], deadlines=[40, 40, 40], tags=[7, 100, 200]))
    assert list(r["out"]) == [0, WAITING, WAITING] and list(S.q.tag) == [100, 200] and S.T.next_id == 1
    w.stage([100])
    r = tick(_ev(1, free=[0]))
    assert list(r["res_tags"]) == [100, 200] and list(r["res_idx"]) == [WD, 0]
    assert list(r["res_ids"]) == [WL.NO_ID, 1] and S.T.next_id == 2 and r["n_waiting"] == 0
    assert sorted(S.T.L) == [1] and S.T.L[1] == [0, 51, False] and list(run) == [1]
    assert list(w.result[0]) == [1] and w.result[1] == 1 and w.staged is None


def test_tags_by_hand():
    S, run, w, tick = _wl_state()
    r = tick(_ev(0, 6, lease_for=[9] * 6, deadlines=[40, 40, 40, 40, 2, 40], tags=[1, 5, 6, 5, 8, 5]))
    assert list(S.q.tag) == [5, 6, 5, 8, 5]
    # An unknown tag; one tag of three entries, staged twice; the tag of a NEW request of this tick.
    w.stage([77, 5, 5, 9])
    r = tick(_ev(1, 1, lease_for=[9], deadlines=[40], tags=[9]))
    assert list(r["res_tags"]) == [5, 5, 5] and list(r["res_idx"]) == [WD, WD, WD]
    assert list(r["out"]) == [WAITING] and list(S.q.tag) == [6, 8, 9]
    assert list(w.result[0]) == [0, 3, 3, 0] and w.result[1] == 3
    # The next tick (now == 2): 9 can be withdrawn now; 8 expires naturally and is staged as well, so
    # it is WITHDRAWN; 5 was resolved in the previous tick: count 0. Unsorted, as the caller likes.
    w.stage([9, 5, 8])
    r = tick(_ev(2))
    assert list(r["res_tags"]) == [8, 9] and list(r["res_idx"]) == [WD, WD] and list(S.q.tag) == [6]
    assert list(w.result[0]) == [1, 0, 1] and w.result[1] == 2
    # Nothing staged: a natural expiry stays a Timeout, and the result says nothing was staged.
    r = tick(_ev(40))
    assert list(r["res_tags"]) == [6] and list(r["res_idx"]) == [TO] and len(w.result[0]) == 0 and w.result[1] == 0
    assert S.T.next_id == 1, "a withdrawn entry took an id"


def test_neighbouring_and_extreme_tags():
    S, run, w, tick = _wl_state(max_waiting=16)
    big = [0, 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1, 10, 11, 12]
    tick(_ev(0, 9, lease_for=[9] * 9, deadlines=[40] * 9, tags=[3] + big))
    w.stage([11, (1 << 64) - 1, 0])
    r = tick(_ev(1))
    assert list(r["res_tags"]) == [0, (1 << 64) - 1, 11] and list(r["res_idx"]) == [WD] * 3
    assert list(S.q.tag) == [1, 1 << 63, (1 << 64) - 2, 10, 12] and list(w.result[0]) == [1, 1, 1]
    w.stage([1, 1 << 63, (1 << 64) - 2])
    r = tick(_ev(2))
    assert list(r["res_tags"]) == [1, 1 << 63, (1 << 64) - 2] and list(S.q.tag) == [10, 12]


def test_a_blocked_rpc_of_five_rows_is_withdrawn():
    """One slot. W = [an RPC of 2 + 3 rows, an RPC of 1 row]; the slot is freed in the tick that
    withdraws the first: the RPC behind it takes the row."""
    S = RM.RpcState(max_waiting=8, max_rows=32, max_leases=64)
    run = np.zeros(1, np.int64)
    w = X.Withdrawal(lambda: S.q, 8)
    tick = lambda ev: w.tick(lambda: S.tick(run, ev, _first_free(run)), "res_status")  # noqa: E731
    r = tick(_ev(0, 3, lease_for=[50] * 3, deadlines=[40] * 3, tags=[1, 2, 3], imm=[1, 2, 1], pre=[0, 3, 0]))
    assert list(r["status"]) == [0, WAITING, WAITING] and r["n_waiting_rows"] == 6
    w.stage([2])
    r = tick(_ev(1, free=[0], imm=[], pre=[]))
    assert list(r["res_tags"]) == [2, 3] and list(r["res_status"]) == [WD, 0]
    assert list(r["res_n_granted"]) == [0, 1] and list(r["res_first"]) == [0, 0]
    assert list(r["res_servants"]) == [0] and list(r["res_task_ids"]) == [1]
    assert r["n_waiting"] == 0 and r["n_waiting_rows"] == 0 and S.T.next_id == 2
    assert list(w.result[0]) == [1] and w.result[1] == 1


# ---- staging conventions ---------------------------------------------------------------------------

def test_staging_conventions():
    S, run, w, tick = _wl_state()
    tick(_ev(0, 4, lease_for=[9] * 4, deadlines=[40] * 4, tags=[1, 2, 3, 4]))
    with pytest.raises(OverflowError):
        w.stage(np.arange(9))
    w.stage([2])
    w.stage([3])  # replaces
    with pytest.raises(OverflowError, match="max_waiting"):  # a refused tick keeps the stage and W
        tick(_ev(1, 9, lease_for=[9] * 9, deadlines=[40] * 9, tags=[0] * 9))
    assert list(w.staged) == [3] and list(S.q.deadline) == [40, 40, 40]
    r = tick(_ev(1))
    assert list(r["res_tags"]) == [3] and list(S.q.tag) == [2, 4] and w.staged is None
    w.stage([2])
    w.stage([])  # clears
    r = tick(_ev(2))
    assert len(r["res_tags"]) == 0 and list(S.q.tag) == [2, 4] and len(w.result[0]) == 0
    w.begin(16)
    w.begin(4)
    assert w.max_withdraw == 16
    for bad in (0, (1 << 30) + 1):
        with pytest.raises(ValueError):
            w.begin(bad)


def test_abi_carries_withdrawal():
    assert binding.ABI_VERSION == 8 and binding.IDX_WITHDRAWN == WD == 0xFFFFFFFC
    src = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define YDC_ABI_VERSION 8u", src) and re.search(r"#define YDC_IDX_WITHDRAWN 0xFFFFFFFCu", src)
    for name in ("ydc_stream_withdraw_begin", "ydc_stream_withdraw_stage", "ydc_stream_withdraw_result"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.ABI_SYMBOLS and hasattr(binding.Context, name[4:])

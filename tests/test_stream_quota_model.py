"""The quota model (tests/stream_quota_model.py) on the CPU: the yardstick of
tests/test_stream_quota_gpu.py.

The defining property, in both modes, on seeded streams over a saturated 12-servant pool: apart from the
label IDX_OVER_QUOTA every tick equals the tick of the BASE model (pinned to the verbatim reference by
the existing model tests) on the same stream given the clipped requests, where the clip is the LITERAL
loop (one row at a time while held < cap, prefetch rows after immediate rows); where oracle/_ref is
built that comparison run goes through the verbatim class (the existing ReferenceReplay classes). The
invariant after every tick; all caps unlimited equals the base model; hand cases with literal vectors;
the constants against the header."""
import os
import re
import types

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_inspect_model as IM
from tests import stream_requestor_model as QM
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WL
from tests import stream_withdraw_model as X
from tests import stream_quota_model as Q
from tests.conftest import ROOT
from yadcc_amd import binding, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
OQ, TO, WAITING, ENF, WD = Q.IDX_OVER_QUOTA, WL.IDX_TIMEOUT, WL.IDX_WAITING, WL.IDX_ENV_NOT_FOUND, X.IDX_WITHDRAWN
UNL = Q.UNLIMITED
MODS = {"wl": WL, "rpc": RM}


def small_pool(n=12, seed=5):
    """A pool one tick of requests saturates: one or two slots per servant, idle machines."""
    sv = synth.make_servants(n, n_tasks_hint=400, n_envs=1, seed=seed)
    sv["max_tasks"] = (1 + np.arange(n) % 2).astype(np.uint32)
    sv["num_processors"][:], sv["current_load"][:] = 256, 0
    return sv


def few_requestors(ev, rng, k=5):
    """The tick's requests come from k requestors, the first of them from most."""
    n = len(ev["tags"])
    ips = np.where(rng.random(n) < 0.5, 0x0A000001, 0x0A000001 + rng.integers(0, k, n)).astype(np.uint32)
    ev["tasks"] = dict(ev["tasks"], requestor_ip=ips)
    return ev


def new_stream(mode):
    ws = WL.new_stream(small_pool(), 40, 6, 4, 1500) if mode == "wl" else RM.new_stream(small_pool(), 40, 6, 4, 1500, 6000)
    IM.attach(ws)
    return ws


CAPS = (5, {0x0A000001: 9, 0x0A000003: 2})  # a default, one override above it and one below


def load_now(ws, ip):
    rows, _ = QM.stream_fold(ws, ws.table.inspect)
    f = QM.find(rows, [ip])
    return int(f["leases"][0]) + int(f["waiting_rows"][0])


def _run(mode, caps=CAPS, clips=None, replay=False, ticks=28, base_only=False):
    """clips None: the quota model, -> (labelled records, base records, the clip per tick). Otherwise
    the comparison run: a stream of its own given the clipped requests, through the base model or the
    verbatim reference class."""
    M = MODS[mode]
    ws = new_stream(mode)
    q = Q.Quota(M, ws)
    q.begin(4)
    q.set(*caps)
    ref = M.ReferenceReplay(ws) if replay else None
    rng, rec, base, out = np.random.default_rng(7), [], [], []
    try:
        for t in range(ticks):
            ev = few_requestors(ws.next_tick(), rng)
            if clips is None and not base_only:
                ips = np.unique(ev["tasks"]["requestor_ip"]).tolist()
                before = {ip: load_now(ws, ip) for ip in ips}
                r = q.tick(ev)
                # the clip is the literal loop on the loads of the clip point
                lit = Q.literal(*q.requests(ev), q.held, q.cap_of)
                assert np.array_equal(lit[0], q.result[0]) and np.array_equal(lit[1], q.result[1]), t
                # the invariant: after the tick nobody is above max(cap, where it was)
                for ip in ips:
                    assert load_now(ws, ip) <= max(q.cap_of(ip), before[ip]), (t, hex(ip), load_now(ws, ip), before[ip])
                out.append(q.result)
                b = q.base
            else:
                if clips is not None:
                    ev, _ = q.clipped(ev, clips[t][0], clips[t][1])
                if replay:
                    ws.table.inspect.stage(ev)
                    r = ref.tick(ev)
                else:
                    r = IM.model_tick(M, ws, ev)
                b = r
            for x in (r, b):
                x["next_id"] = ws.table.next_id
                x["rows_w"] = ws.state.q.rows() if mode == "rpc" else len(ws.state.q)
            rec.append(r)
            base.append(b)
    finally:
        if ref:
            ref.close()
    return rec, base, out


def _same(mode, a, b, what):
    M = MODS[mode]
    for t, (x, y) in enumerate(zip(a, b)):
        for k in M.FIELDS + ("next_id", "rows_w"):
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), "%s: tick %d: %s differs" % (what, t, k)


def _clips_something(mode, rec, clips):
    label = "out" if mode == "wl" else "status"
    refused = sum(c[3] for c in clips)
    assert refused > 40 and sum(int((r[label] == OQ).sum()) for r in rec) == refused
    assert sum(c[2] for c in clips) > refused or mode == "wl"  # (rpc: partial clips as well)
    # (the caps bound what can be outstanding: 9 + 2 + 3 x 5 = 26 against the pool's 18 slots)
    assert max(r["n_waiting"] for r in rec) > 4, "the pool is never saturated"
    assert any(0 < int((r[label] == OQ).sum()) < len(r[label]) for r in rec)


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_defining_property(mode):
    rec, base, clips = _run(mode)
    _clips_something(mode, rec, clips)
    want, _, _ = _run(mode, clips=clips)
    _same(mode, base, want, "the base model on the clipped requests")
    label = "out" if mode == "wl" else "status"
    for t, (r, b, c) in enumerate(zip(rec, base, clips)):  # the label, apart
        keep = (c[0].astype(np.int64) + c[1]) > 0
        assert (r[label][~keep] == OQ).all() and np.array_equal(r[label][keep], b[label]), t
        assert not (b[label] == OQ).any()
        if mode == "rpc":
            assert not r["n_granted"][~keep].any()
            assert int(r["n_granted"].sum()) == len(r["servants"]) and (r["n_granted"] <= c[0] + c[1]).all()


@needs_ref
@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_defining_property_against_the_reference_replay(mode):
    rec, base, clips = _run(mode)
    want, _, _ = _run(mode, clips=clips, replay=True)
    _same(mode, base, want, "the verbatim class on the clipped requests")


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_every_cap_unlimited_is_the_base_model(mode):
    rec, _, clips = _run(mode, caps=(UNL, {}))
    want, _, _ = _run(mode, base_only=True)
    _same(mode, rec, want, "all unlimited")
    assert all(c[2] == 0 and c[3] == 0 for c in clips)


# ---- hand cases, literal ---------------------------------------------------------------------------

A, B, C_ = 0x0A000001, 0x0A000002, 0x0A000003


class Hand:
    """A stream by hand: `slots` servants of one slot each, placed first free first."""

    def __init__(self, mode, slots, inspect=True):
        self.mode = mode
        self.state = (WL.WaitLeaseState(64, 256) if mode == "wl" else RM.RpcState(64, 256, 256))
        self.table = self.state.T
        self.es = types.SimpleNamespace(n=slots, running=np.zeros(slots, np.int64))
        self.tag = 0
        if inspect:
            IM.attach(self)

    def commit(self, before, got):
        pass

    def place(self):
        run = self.es.running

        def place(batch):
            out = []
            for e in batch["env_id"].tolist():
                free = np.nonzero(run == 0)[0]
                ok = e == 0 and len(free)
                out.append(int(free[0]) if ok else ENF if e else TO)
                if ok:
                    run[free[0]] += 1
            return np.array(out, np.uint32)
        return place

    def ev(self, now, reqs=(), free=(), wait=40):
        """reqs: (requestor, n_immediate, n_prefetch[, env_id[, deadline]]) per request."""
        n = len(reqs)
        z = np.zeros(n, np.uint32)
        ev = {"now": now, "release_idx": np.empty(0, np.uint32), "upd_idx": np.empty(0, np.uint32),
              "tasks": {"env_id": np.array([r[3] if len(r) > 3 else 0 for r in reqs], np.uint32), "min_version": z,
                        "requestor_ip": np.array([r[0] for r in reqs], np.uint32)},
              "lease_for": np.full(n, 100, np.int64),
              "deadlines": np.array([r[4] if len(r) > 4 else now + wait for r in reqs], np.int64),
              "tags": np.arange(self.tag, self.tag + n, dtype=np.uint64), "renew_ids": np.empty(0, np.uint64),
              "renew_expires_at": np.empty(0, np.int64), "free_ids": np.array(free, np.uint64),
              "report_servants": np.empty(0, np.uint32), "report_off": np.zeros(1, np.uint32),
              "report_ids": np.empty(0, np.uint64)}
        self.tag += n
        if self.mode == "rpc":
            ev["n_immediate"] = np.array([r[1] for r in reqs], np.uint32)
            ev["n_prefetch"] = np.array([r[2] for r in reqs], np.uint32)
        return ev


def hand(mode, slots, default=UNL, over=()):
    h = Hand(mode, slots)
    q = Q.Quota(MODS[mode], h)
    q.begin(8)
    q.set(default, over)
    return h, q, lambda *a, **k: q.tick(h.ev(*a, **k), h.place())


def test_free_then_ask_in_one_tick_is_admitted():
    h, q, tick = hand("wl", 8, default=3)
    r = tick(0, [(A, 1, 0)] * 3)
    assert list(r["out"]) == [0, 1, 2] and list(r["task_id"]) == [0, 1, 2]
    r = tick(1, [(A, 1, 0)] * 3, free=[0, 2])  # A holds 1 at the clip point: room 2
    assert list(q.result[0]) == [1, 1, 0] and q.result[2:] == (1, 1) and q.held == {A: 1}
    assert list(r["out"]) == [0, 2, OQ] and list(r["task_id"]) == [3, 4, WL.NO_ID]
    r = tick(2, [(A, 1, 0), (B, 1, 0)])  # room 0
    assert list(r["out"]) == [OQ, 3] and q.held == {A: 3, B: 0} and h.table.next_id == 6


def test_a_cap_reached_inside_one_rpc():
    h, q, tick = hand("rpc", 16, default=4, over={B: 1})
    r = tick(0, [(A, 2, 3), (A, 2, 1), (B, 2, 3), (C_, 0, 5)])
    assert list(q.result[0]) == [2, 0, 1, 0] and list(q.result[1]) == [2, 0, 0, 4] and q.result[2:] == (1 + 3 + 4 + 1, 1)
    assert list(r["status"]) == [0, OQ, 0, 0] and list(r["n_granted"]) == [4, 0, 1, 4]
    assert list(r["servants"]) == list(range(9)) and list(r["task_ids"]) == list(range(9))
    tk = h.table.inspect.tasks()  # the prefetch flag follows the ADMITTED n_immediate
    assert list(tk["prefetch"]) == [0, 0, 1, 1, 0, 1, 1, 1, 1]


def test_cap_zero_and_overrides_around_the_default():
    h, q, tick = hand("wl", 32, default=2, over={A: 0, B: 4, 0xFFFFFFFF: 1})
    r = tick(0, [(A, 1, 0), (B, 1, 0), (C_, 1, 0)] * 5 + [(0xFFFFFFFF, 1, 0)] * 2)
    want = [OQ, 0, 1, OQ, 2, 3, OQ, 4, OQ, OQ, 5, OQ, OQ, OQ, OQ, 6, OQ]
    assert list(r["out"]) == want and q.result[3] == want.count(OQ)
    rows, _ = QM.stream_fold(h, h.table.inspect)
    assert {int(x["requestor_ip"]): int(x["leases"]) for x in rows} == {B: 4, C_: 2, 0xFFFFFFFF: 1}


@pytest.mark.parametrize("how", ["expires", "withdrawn"])
def test_an_entry_of_w_that_leaves_in_this_tick_gives_its_rows_back(how):
    h, q, _ = hand("rpc", 2, default=3)
    w = X.Withdrawal(lambda: h.state.q, 8)
    tick = lambda *a, **k: w.tick(lambda: q.tick(h.ev(*a, **k), h.place()), "res_status")  # noqa: E731
    r = tick(0, [(B, 2, 0), (A, 2, 1, 0, 1 if how == "expires" else 40)])
    assert list(r["status"]) == [0, WAITING] and r["n_waiting_rows"] == 3
    if how == "withdrawn":
        w.stage([1])
    r = tick(1, [(A, 1, 1), (A, 1, 1)])  # A's three waiting rows no longer count
    assert q.held == {A: 0} and list(q.result[0]) == [1, 1] and list(q.result[1]) == [1, 0]
    assert list(r["res_status"]) == [TO if how == "expires" else WD] and list(r["status"]) == [WAITING, WAITING]
    assert r["n_waiting_rows"] == 3
    r = tick(2, [(A, 1, 0)])  # ... and the rows it waits for now do
    assert q.held == {A: 3} and list(r["status"]) == [OQ]


def test_an_unattributed_lease_counts_for_nobody_and_an_unknown_digest_takes_room():
    h = Hand("wl", 8, inspect=False)
    r = WL.model_tick(h, h.ev(0, [(A, 1, 0)] * 3), h.place())  # granted before inspection: nobody's
    assert list(r["out"]) == [0, 1, 2]
    IM.attach(h)
    q = Q.Quota(WL, h)
    q.begin(0)
    q.set(2)
    r = q.tick(h.ev(1, [(A, 1, 0, 0xFFFF), (A, 1, 0), (A, 1, 0)]), h.place())
    assert q.held == {A: 0} and list(r["out"]) == [ENF, 3, OQ] and h.table.next_id == 4


def test_settings_conventions():
    h, q, tick = hand("wl", 4)
    with pytest.raises(OverflowError):
        q.set(1, [(i, 1) for i in range(9)])
    with pytest.raises(ValueError):
        q.set(1, [(A, 1), (A, 2)])
    with pytest.raises(ValueError):
        q.begin((1 << 24) + 1)
    assert q.default == UNL and q.over == {}  # (a refused set leaves the settings)
    r = tick(0, [(A, 1, 0)] * 3)
    assert list(r["out"]) == [0, 1, 2] and q.result[2:] == (0, 0)


def test_abi_carries_the_quota():
    assert binding.ABI_VERSION == 8 and binding.IDX_OVER_QUOTA == OQ == 0xFFFFFFFB
    assert binding.QUOTA_UNLIMITED == UNL == 0xFFFFFFFF
    src = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define YDC_ABI_VERSION 8u", src) and re.search(r"#define YDC_IDX_OVER_QUOTA 0xFFFFFFFBu", src)
    assert re.search(r"#define YDC_QUOTA_UNLIMITED 0xFFFFFFFFu", src)
    for name in ("ydc_stream_quota_begin", "ydc_stream_quota_set", "ydc_stream_quota_result"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.ABI_SYMBOLS and hasattr(binding.Context, name[4:])

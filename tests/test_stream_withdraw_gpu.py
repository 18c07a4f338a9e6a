"""Withdrawal by tag on the device (ydc_stream_withdraw_begin / _stage / _result; k_withdraw_load,
k_withdraw_mark, k_withdraw_label): every tick of a waiting, waiting-and-leased or rpc stream with the
capability on is compared with the model (tests/stream_withdraw_model.py, pinned on the CPU by
tests/test_stream_withdraw_model.py) on every output, through the modes' own gpu_tick / check_tick,
and on ydc_stream_withdraw_result. The pools are small (a handful of slots), so one tick of
far-deadline requests fills W."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_rpc_cases as RC
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_cases as WC
from tests import stream_wait_lease_model as WL
from tests import stream_wait_model as W
from tests import stream_withdraw_model as X
from tests import test_stream_alive_gpu as alive
from tests import test_stream_rpc_gpu as TR
from tests import test_stream_wait_lease_gpu as TWL
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu
MODES = ("waiting", "wl", "rpc")
WD, TO, WAITING, ENF = X.IDX_WITHDRAWN, W.IDX_TIMEOUT, W.IDX_WAITING, W.IDX_ENV_NOT_FOUND
INVALID, CAPACITY = "invalid argument", "capacity of the context exceeded"
GPU = True  # (False: the scenarios on the model alone, to rehearse them where there is no device)


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def tiny_pool(n=1, slots=1):
    """n idle servants of one kind with `slots` slots each: max_tasks alone bounds them."""
    sv = synth.make_servants(n, n_tasks_hint=40, n_envs=1, seed=17)
    sv["max_tasks"][:], sv["num_processors"][:], sv["current_load"][:] = slots, 256, 0
    sv["version"][:], sv["memory_available"][:] = 30, 64 << 30  # (none is short of memory)
    return sv


def crowded_pool(n=200, seed=42, n_envs=2):
    sv = synth.make_servants(n, n_tasks_hint=2000, n_envs=n_envs, seed=seed)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    return sv


class Rig:
    """A stream of `mode` with the capability, on the device and in the model. Scripted (every
    servant beats in every tick, the traffic is written by event()) or seeded (next())."""

    def __init__(self, mode, sv, mw, per_tick, max_withdraw=64, max_rows=None, frees=0, renewals=0, n_envs=1,
                 scripted=True, withdraw=True, masks=False, rpc_mix=None, max_leases=1 << 15):
        self.mode, self.masks, self.t, self.on = mode, masks, 0, withdraw
        rate = (lambda now: 1.0) if scripted else (lambda now: 1.0 if now % 12 < 9 else 0.125)
        if mode == "waiting":
            self.ws = W.WaitingStream(sv, per_tick, frees, mw, n_envs=n_envs)
            self.q = W.WaitQueue(mw)
            self.w = X.waiting(self.q, max_withdraw)
        elif mode == "wl":
            self.ws = WL.new_stream(sv, per_tick, frees, renewals, mw, n_envs=n_envs, rate=rate)
            self.w = X.wait_lease(self.ws, max_withdraw)
        else:
            max_rows = max_rows or 4 * (mw + per_tick)
            self.ws = RM.new_stream(sv, per_tick, frees, renewals, mw, max_rows, n_envs=n_envs, rate=rate,
                                    **(rpc_mix or {}))
            self.w = X.rpc(self.ws, max_withdraw)
        es = self.ws.es
        if scripted:
            es.hb = es.n
        self.ctx = None
        if GPU:
            if mode == "waiting":
                self.ctx = binding.Context(device=0)
                self.ctx.upload_servants(pack.to_abi_columns(es.sv))
                self.ctx.stream_begin(es.hb + 8, max(frees, 16), per_tick, max_waiting=mw)
            else:
                # (a scripted stream brings a few frees and no reports; a seeded one the modes' own bounds)
                caps = dict(renewals=16, frees=64, report_ids=64, reports=es.n) if scripted else {}
                if mode == "wl":
                    self.ctx = TWL.begin(self.ws, max_leases, per_tick, **caps)
                else:
                    self.ctx = TR.begin(self.ws, per_tick, max_leases=max_leases, **caps)
            if withdraw:
                self.ctx.stream_withdraw_begin(max_withdraw)

    def W(self):
        return self.q if self.mode == "waiting" else self.ws.state.q

    def held(self):
        return sorted(self.ws.table.L)

    def event(self, n=0, wait=1000, tags=None, free=0, rows=(1, 0)):
        """A scripted tick: n requests any servant may take, deadline now + wait (one value or n), the
        given tags; `free`: how many grants are given back (by id where the mode has ids)."""
        wait = np.broadcast_to(np.asarray(wait, np.int64), (n,))
        if self.mode == "waiting":
            es = self.ws.es
            es.tasks_per_tick, es.frees_per_tick = n, free
            now, who, hb, rel, tk, dl, tg = self.ws.next_tick()
            assert len(dl) == n
            ev = [now, who, hb, rel, tk, (now + wait).astype(np.int64), tg]
        elif self.mode == "wl":
            ev = WC.scripted(self.ws, self.ws.next_tick(), n=n, lease_for=100, wait=wait, free=self.held()[:free])
        else:
            rows = [rows] * n if isinstance(rows, tuple) else rows
            ev = RC.scripted(self.ws, self.ws.next_tick(), rpcs=[(rows[i][0], rows[i][1], 100, int(wait[i])) for i in range(n)],
                             free=self.held()[:free])
        tk = ev[4] if self.mode == "waiting" else ev["tasks"]
        tk["min_version"][:] = 0
        if tags is not None:
            tags = np.asarray(tags, np.uint64)
            assert len(tags) == n
            if self.mode == "waiting":
                ev[6] = tags
            else:
                ev["tags"] = tags
        return ev

    def next(self, dup_every=0):
        """The seeded stream's next tick; dup_every: every that-many-th request repeats its neighbour's tag."""
        ev = list(self.ws.next_tick()) if self.mode == "waiting" else self.ws.next_tick()
        if dup_every:
            tags = (ev[6] if self.mode == "waiting" else ev["tags"]).copy()
            tags[dup_every::dup_every] = tags[dup_every - 1:-1:dup_every]
            if self.mode == "waiting":
                ev[6] = tags
            else:
                ev["tags"] = tags
        return ev

    def now_of(self, ev):
        return int(ev[0] if self.mode == "waiting" else ev["now"])

    def stage(self, tags):
        self.w.stage(tags)
        if self.ctx:
            self.ctx.stream_withdraw_stage(tags)

    def gpu_tick(self, ev):
        if self.mode == "waiting":
            now, who, hb, rel, tk, dl, tg = ev
            em = self.ws.es.abi["env_mask"][who] if self.masks else None
            return self.ctx.stream_tick_waiting(who, hb, rel, tk, dl, tg, now, env_masks=em)
        return (TWL if self.mode == "wl" else TR).gpu_tick(self.ctx, self.ws, ev, self.masks)

    def tick(self, ev, stage=None, snapshot=True, model=None):
        """One tick on both sides, compared on every output. model: how the base model's tick is run
        (default: the mode's model_tick). -> the model's record, with "res": the resolved answers."""
        if stage is not None:
            self.stage(stage)
        ctx, ws, t = self.ctx, self.ws, self.t
        if self.mode == "waiting":
            now, who, hb, rel, tk, dl, tg = ev
            out, rt, ri, nw, batch = self.w.run(W.oracle_place(ws.es), tk, dl, tg, now)
            if ctx:
                g_out, g_rt, g_ri, g_nw = self.gpu_tick(ev)
                assert np.array_equal(g_out, out), "tick %d: the new requests' answers differ" % t
                assert np.array_equal(g_rt, rt), "tick %d: resolved tags differ (%d vs %d)" % (t, len(g_rt), len(rt))
                assert np.array_equal(g_ri, ri), "tick %d: resolved answers differ" % t
                assert g_nw == nw, (t, g_nw, nw)
            ws.commit(out, X.unlabelled(ri), nw)  # (a withdrawn entry is no grant)
            if ctx:
                assert np.array_equal(ctx.get_running(), ws.es.running.astype(np.uint32)), "tick %d: running differs" % t
                assert ctx.stats()["granted"] == int((batch < ENF).sum()), t
            r = dict(out=out, res_tags=rt, res=ri, n_waiting=nw)
        elif self.mode == "wl":
            got = self.gpu_tick(ev) if ctx else None
            r = self.w.tick(model or (lambda: WL.model_tick(ws, ev)), "res_idx")
            if ctx:
                # (the mode's own check reads res_idx < ENV_NOT_FOUND as a grant: the label apart)
                plain = got[:6] + (X.unlabelled(got[6]),) + got[7:]
                TWL.check_tick(t, ctx, ws, plain, dict(r, res_idx=X.unlabelled(r["res_idx"])), snapshot=snapshot)
                assert np.array_equal(got[6], r["res_idx"]), "tick %d: the withdrawn entries differ" % t
            r = dict(r, res=r["res_idx"])
        else:
            got = self.gpu_tick(ev) if ctx else None
            r = self.w.tick(model or (lambda: RM.model_tick(ws, ev)), "res_status")
            if ctx:
                TR.check_tick(t, ctx, ws, got, r, snapshot=snapshot)
            r = dict(r, res=r["res_status"], out=r["status"])
        if ctx and self.on:
            counts, total = ctx.stream_withdraw_result()
            assert np.array_equal(counts, self.w.result[0]), (t, counts, self.w.result[0])
            assert total == self.w.result[1] == int((r["res"] == WD).sum()), (t, total, self.w.result[1])
        r["now"] = self.now_of(ev)
        self.t += 1
        return r

    def close(self):
        if self.ctx:
            self.ctx.stream_end()
            self.ctx.close()


# ---- tile boundaries -------------------------------------------------------------------------------

PATTERNS = ("none", "head", "tail", "middle", "every other", "all")


@pytest.mark.parametrize("size", [1, 2, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("mode", MODES)
def test_tile_boundaries(mode, size):
    """|W| == size when the withdrawing tick finds it (kWaitTile = kRpcTile = 1024), for every pattern in
    turn: W is topped up to `size` with requests of which every fifth expires naturally in the next
    tick, and that tick withdraws the pattern plus one of the expiring entries."""
    rig = Rig(mode, tiny_pool(2, 1), size + 7, size + 3, max_withdraw=size + 2)
    r = rig.tick(rig.event(n=2))
    assert r["n_waiting"] == 0
    next_tag, seen_both = 10, False
    for pat in PATTERNS:
        need = size - len(rig.W())
        wait = np.where(np.arange(need) % 5 == 2, 1, 1000)
        rows = [((1, 0), (1, 1), (2, 1))[i % 3] for i in range(need)]
        r = rig.tick(rig.event(n=need, wait=wait, tags=np.arange(next_tag, next_tag + need), rows=rows))
        next_tag += need
        tags = rig.W().tag.copy()
        assert r["n_waiting"] == size == len(tags) and not len(r["res_tags"])
        expiring = tags[rig.W().deadline <= r["now"] + 1]
        staged = {"none": tags[:0], "head": tags[:1], "tail": tags[-1:], "middle": tags[size // 2:size // 2 + 1],
                  "every other": tags[::2], "all": tags}[pat]
        if pat != "none":
            staged = np.concatenate([staged, expiring[:1]])
        r = rig.tick(rig.event(), stage=staged[::-1])
        gone = np.isin(tags, staged)
        assert np.array_equal(r["res_tags"][r["res"] == WD], tags[gone])
        assert np.array_equal(r["res_tags"][r["res"] == TO], tags[~gone & np.isin(tags, expiring)])
        assert r["n_waiting"] == size - len(r["res_tags"])
        seen_both |= bool((r["res"] == WD).any() and (r["res"] == TO).any())
        if pat == "all":
            assert r["n_waiting"] == 0 and len(r["res_tags"]) == size
    assert seen_both or size < 8
    rig.close()


# ---- before the retry ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,inspect", [("waiting", False), ("wl", False), ("wl", True), ("rpc", False), ("rpc", True)])
def test_withdrawn_before_the_retry(mode, inspect):
    """W = [A, B], the pool's one slot is given back in the tick that withdraws A: B is granted, and A
    left no trace: no id, no lease, no running task, no detail record, no ever_assigned count."""
    rig = Rig(mode, tiny_pool(1, 1), 8, 8)
    ctx = rig.ctx
    if inspect and ctx:
        ctx.stream_inspect_begin()
    r = rig.tick(rig.event(n=3, tags=[7, 100, 200]))
    assert list(r["out"]) == [0, WAITING, WAITING] and list(rig.W().tag) == [100, 200]
    next_id = rig.ws.table.next_id if mode != "waiting" else None
    ever = int(ctx.stream_inspect_servants()["ever_assigned"].sum()) if inspect and ctx else 0
    r = rig.tick(rig.event(free=1), stage=[100])
    assert list(r["res_tags"]) == [100, 200] and list(r["res"]) == [WD, 0] and r["n_waiting"] == 0
    assert list(rig.ws.es.running) == [1]  # (compared with ydc_get_running by the tick)
    if mode != "waiting":
        assert rig.ws.table.next_id == next_id + 1 and rig.held() == [next_id]  # (the lease snapshot was compared)
    if inspect and ctx:
        assert int(ctx.stream_inspect_servants()["ever_assigned"].sum()) == ever + 1
        assert list(ctx.stream_inspect_tasks()["task_id"]) == [next_id]
    rig.close()


# ---- tags ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_tags(mode):
    top = (1 << 64) - 1
    rig = Rig(mode, tiny_pool(1, 1), 32, 16, max_withdraw=8)
    w = rig.w
    rig.tick(rig.event(n=6, wait=[40, 40, 40, 40, 2, 40], tags=[1, 5, 6, 5, 8, 5]))
    assert list(rig.W().tag) == [5, 6, 5, 8, 5]
    # An unknown tag; one tag of three entries, staged twice; the tag of a NEW request of this tick.
    r = rig.tick(rig.event(n=1, wait=40, tags=[9]), stage=[77, 5, 5, 9])
    assert list(r["res_tags"]) == [5, 5, 5] and list(r["res"]) == [WD] * 3
    assert list(r["out"]) == [WAITING] and list(rig.W().tag) == [6, 8, 9]
    assert list(w.result[0]) == [0, 3, 3, 0] and w.result[1] == 3
    # now == 2: 9 can be withdrawn now; 8 expires naturally and is staged: WITHDRAWN; 5 went a tick ago.
    r = rig.tick(rig.event(), stage=[9, 5, 8])
    assert list(r["res_tags"]) == [8, 9] and list(r["res"]) == [WD, WD] and list(rig.W().tag) == [6]
    assert list(w.result[0]) == [1, 0, 1] and w.result[1] == 2
    # Tags at both ends of the range, and neighbours k, k + 1, k + 2 of which only k + 1 is staged.
    big = [0, 1, 1 << 63, top - 1, top, 10, 11, 12]
    rig.tick(rig.event(n=8, tags=big))
    r = rig.tick(rig.event(), stage=[11, top, 0])
    assert list(r["res_tags"]) == [0, top, 11] and list(r["res"]) == [WD] * 3
    assert list(rig.W().tag) == [6, 1, 1 << 63, top - 1, 10, 12] and list(w.result[0]) == [1, 1, 1]
    r = rig.tick(rig.event(), stage=[top - 1, 1])  # two tags, unsorted
    assert list(r["res_tags"]) == [1, top - 1] and list(rig.W().tag) == [6, 1 << 63, 10, 12]
    # max_withdraw tags, unsorted, most of them unknown; max_withdraw + 1 is refused and changes nothing.
    full = [top, 500, 12, 400, 1 << 63, 300, 2, 0]
    if rig.ctx:
        with pytest.raises(binding.YdcError, match=CAPACITY):
            rig.ctx.stream_withdraw_stage(np.array(full + [10], np.uint64))
    r = rig.tick(rig.event(), stage=full)
    assert list(r["res_tags"]) == [1 << 63, 12] and list(rig.W().tag) == [6, 10]
    assert list(w.result[0]) == [0, 0, 1, 0, 1, 0, 0, 0] and w.result[1] == 2
    # Nothing staged: a natural expiry stays a Timeout.
    rig.tick(rig.event())
    assert len(w.result[0]) == 0
    rig.close()


# ---- rpc -------------------------------------------------------------------------------------------

def test_a_blocked_rpc_of_five_rows_is_withdrawn():
    rig = Rig("rpc", tiny_pool(1, 1), 8, 8)
    r = rig.tick(rig.event(n=3, tags=[1, 2, 3], rows=[(1, 0), (2, 3), (1, 0)]))
    assert list(r["status"]) == [0, WAITING, WAITING] and r["n_waiting_rows"] == 6
    r = rig.tick(rig.event(free=1), stage=[2])
    assert list(r["res_tags"]) == [2, 3] and list(r["res_status"]) == [WD, 0]
    assert list(r["res_n_granted"]) == [0, 1] and list(r["res_first"]) == [0, 0]
    assert list(r["res_servants"]) == [0] and list(r["res_task_ids"]) == [1]
    assert r["n_waiting"] == 0 and r["n_waiting_rows"] == 0
    # Two RPCs queue behind a withdrawn one of 5 rows: rows(W) drops by exactly 5.
    r = rig.tick(rig.event(n=3, tags=[4, 5, 6], rows=[(2, 3), (1, 1), (3, 0)]))
    assert r["n_waiting_rows"] == 10
    r = rig.tick(rig.event(), stage=[4])
    assert list(r["res_tags"]) == [4] and list(r["res_status"]) == [WD] and r["n_waiting_rows"] == 5
    rig.close()


# ---- routes ----------------------------------------------------------------------------------------

def _third_of_w(rig, rng, unknown=3):
    tags = rig.W().tag
    some = rng.choice(tags, (len(tags) + 2) // 3, replace=False) if len(tags) else tags
    return np.concatenate([some, rng.integers(1 << 40, 1 << 41, unknown).astype(np.uint64)]).astype(np.uint64)


@pytest.mark.parametrize("stream_graph", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_randomised_differential(mode, stream_graph, monkeypatch):
    """200 servants with at most two slots, 300 requests a tick, 40 ticks: every tick stages a seeded
    third of W's tags plus some nobody has; a few tags of the stream occur twice. With the captured
    step and with the step enqueued kernel by kernel (stream_graph=0)."""
    _graph(monkeypatch, stream_graph)
    rig = Rig(mode, crowded_pool(), 6000, 300, max_withdraw=4096, frees=60, renewals=20, n_envs=2, scripted=False,
              max_rows=1 << 14)
    rng = np.random.default_rng(11)
    n_wd = n_to = n_twice = 0
    for t in range(40):
        staged = _third_of_w(rig, rng) if t % 5 else np.empty(0, np.uint64)  # (every fifth tick: nothing staged)
        r = rig.tick(rig.next(dup_every=17), stage=staged, snapshot=t % 8 == 0)
        n_wd += int((r["res"] == WD).sum())
        n_to += int((r["res"] == TO).sum())
        n_twice += int((rig.w.result[0] > 1).sum())
    assert n_wd > 500 and n_to > 20 and n_twice > 0, (n_wd, n_to, n_twice)
    assert len(rig.W()) > 100
    rig.close()


def _eager_rig(mode, withdraw=True):
    """The shape of the modes' test_more_than_256_classes_runs_eagerly: ~600 servant classes."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    if mode == "rpc":
        sv["max_tasks"] = np.minimum(sv["max_tasks"], 1)
        return Rig(mode, sv, 1000, 60, max_withdraw=512, frees=300, renewals=100, n_envs=n_envs, scripted=False,
                   withdraw=withdraw, masks=True, rpc_mix=BIG, max_rows=1 << 14, max_leases=1 << 16)
    return Rig(mode, sv, 8000, 3000, max_withdraw=4096, frees=1500, renewals=300, n_envs=n_envs, scripted=False,
               withdraw=withdraw, masks=True, max_leases=1 << 16)


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_more_than_256_classes_runs_eagerly(mode):
    """eager_only: every tick is enqueued, the three launches with it."""
    rig = _eager_rig(mode)
    rng = np.random.default_rng(5)
    rig.ctx.set_profiling(True)
    n_wd = 0
    for t in range(6):
        r = rig.tick(rig.next(), stage=_third_of_w(rig, rng))
        n_wd += int((r["res"] == WD).sum())
        assert "k_withdraw_label" in rig.ctx.kernel_profile()
    assert n_wd > 10
    rig.close()


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_feature_off_means_untouched(mode):
    """A stream that never calls ydc_stream_withdraw_begin launches no kernel of the feature (the eager
    route names its launches); with the capability on and nothing staged every tick is the base model's."""
    rig = _eager_rig(mode, withdraw=False)
    rig.ctx.set_profiling(True)
    for t in range(3):
        rig.tick(rig.next())
        prof = rig.ctx.kernel_profile()
        assert prof and not [k for k in prof if k.startswith("k_withdraw")], sorted(prof)
        assert ("k_rpc_settle" if mode == "rpc" else "k_wait_lease_commit") in prof, sorted(prof)
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_nothing_staged_is_the_base_model(mode):
    rig = Rig(mode, crowded_pool(60, seed=7), 2000, 150, frees=30, renewals=10, n_envs=2, scripted=False)
    for t in range(12):
        r = rig.tick(rig.next())
        assert not (r["res"] == WD).any() and len(rig.w.result[0]) == 0
    assert len(rig.W()) > 50
    rig.close()


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_a_structural_heartbeat_in_the_withdrawing_tick(mode):
    """The tick that withdraws also appends a servant: its heartbeats take the eager path, the tables
    are rebuilt and the step is captured again, the staging applies all the same."""
    rig = Rig(mode, tiny_pool(2, 1), 16, 8)
    rig.tick(rig.event(n=6, tags=[1, 2, 3, 4, 5, 6]))
    assert list(rig.W().tag) == [3, 4, 5, 6]
    ev = rig.event()
    row, s_new = AM.append_servant(rig.ws, 0, 0x0A636363)
    ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
    ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
    r = rig.tick(ev, stage=[3, 5])
    granted = 0 if mode == "rpc" else s_new  # (rpc: the status; the servant is in the packed grants)
    assert list(r["res_tags"]) == [3, 4, 5] and list(r["res"]) == [WD, granted, WD] and list(rig.W().tag) == [6]
    if mode == "rpc":
        assert list(r["res_servants"]) == [s_new]
    r = rig.tick(rig.event(), stage=[6])
    assert list(r["res"]) == [WD] and r["n_waiting"] == 0
    rig.close()


@pytest.mark.parametrize("mode", ["wait_leased", "rpc"])
def test_aliveness_on_and_a_servant_expiring_in_the_withdrawing_tick(mode):
    """The removal route (servant_alive.h) runs in front of the step; every tick withdraws a third of W."""
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    ws, ctx = alive.begun(mode, sv)
    x = alive.Lively(mode, ws, ctx, AM.first_expiries(70, life=alive.LIFE))
    gen = AM.AliveGen(ws, life=alive.LIFE, p_stop=0.3, p_short=0.3, seed=3)
    ctx.stream_withdraw_begin(1024)
    w = X.Withdrawal(lambda: ws.state.q, 1024)
    M, G = alive.MODS[mode]
    label = "res_status" if mode == "rpc" else "res_idx"
    rng, both = np.random.default_rng(9), 0
    for t in range(12):
        ev = gen.next_tick()
        tags = ws.state.q.tag
        staged = rng.choice(tags, len(tags) // 3, replace=False) if len(tags) else tags
        ctx.stream_withdraw_stage(staged)
        w.stage(staged)
        ctx.stream_alive_stage(ev["upd_expires_at"])
        got = G.gpu_tick(ctx, ws, ev, False)
        want = w.tick(lambda: AM.model_tick(M, ws, ev), label)
        if mode == "rpc":
            G.check_tick(t, ctx, ws, got, want)
        else:
            plain = got[:6] + (X.unlabelled(got[6]),) + got[7:]
            G.check_tick(t, ctx, ws, plain, dict(want, res_idx=X.unlabelled(want["res_idx"])))
            assert np.array_equal(got[6], want["res_idx"]), t
        x.t = t
        x.check_alive(want)
        counts, total = ctx.stream_withdraw_result()
        assert np.array_equal(counts, w.result[0]) and total == w.result[1] == len(staged)
        both += bool(len(want["removed"]) and total)
    assert both, "no tick both erased a servant and withdrew"
    x.close()


# ---- conventions -----------------------------------------------------------------------------------

def test_conventions():
    rig = Rig("wl", tiny_pool(1, 1), 8, 8, max_withdraw=4)
    ctx, ws = rig.ctx, rig.ws
    rig.tick(rig.event(n=5, tags=[1, 2, 3, 4, 5]))
    assert list(rig.W().tag) == [2, 3, 4, 5]
    # Stage twice replaces. A tick refused with YDC_ERR_CAPACITY keeps the stage; after ydc_stream_reserve
    # (which keeps the capability) the same tick applies it.
    ctx.stream_withdraw_stage([2])
    rig.stage([3])
    ev = rig.event(n=5, tags=[6, 7, 8, 9, 10])
    before = ctx.stream_waiting()["tag"]
    with pytest.raises(binding.YdcError, match=CAPACITY):
        rig.gpu_tick(ev)
    with pytest.raises(binding.YdcError, match=INVALID):  # (the stage is still pending)
        ctx.stream_snapshot()
    assert np.array_equal(ctx.stream_waiting()["tag"], before) and len(ctx.stream_withdraw_result()[0]) == 0
    ctx.stream_reserve(max_waiting=16)
    ws.state.max_waiting = ws.state.q.max_waiting = 16
    r = rig.tick(ev)
    assert list(r["res_tags"]) == [3] and list(r["res"]) == [WD] and list(rig.W().tag) == [2, 4, 5, 6, 7, 8, 9, 10]
    # The view and the outlook see an entry before the tick that withdraws it and not after.
    assert 4 in ctx.stream_waiting()["tag"] and ctx.stream_outlook([0], [0])["waiting"][0] == 8
    rig.tick(rig.event(), stage=[4])
    assert 4 not in ctx.stream_waiting()["tag"] and ctx.stream_outlook([0], [0])["waiting"][0] == 7
    # n == 0 clears; a snapshot is refused while a stage is pending and works once it is consumed or cleared.
    rig.stage([5])
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_snapshot()
    rig.stage([])
    blob = ctx.stream_snapshot()
    r = rig.tick(rig.event())
    assert not len(r["res_tags"]) and 5 in rig.W().tag
    # ydc_stream_withdraw_result with too little room: the count, nothing written.
    rig.tick(rig.event(), stage=[5, 77])
    n, room = C.c_uint32(0), np.full(2, 99, np.uint32)
    assert binding.lib().ydc_stream_withdraw_result(ctx._h, room.ctypes.data, 1, C.byref(n), None) == -4
    assert n.value == 2 and list(room) == [99, 99]
    assert [list(a) if hasattr(a, "__len__") else a for a in ctx.stream_withdraw_result()] == [[1, 0], 1]
    # ydc_stream_withdraw_begin grows and keeps W and a pending stage; smaller or equal does nothing.
    rig.stage([6])
    before = ctx.stream_waiting()["tag"]
    with pytest.raises(binding.YdcError, match=CAPACITY):
        ctx.stream_withdraw_stage(np.arange(5, dtype=np.uint64))
    ctx.stream_withdraw_begin(64)
    ctx.stream_withdraw_begin(4)
    rig.w.begin(64)
    assert np.array_equal(ctx.stream_waiting()["tag"], before)
    r = rig.tick(rig.event())
    assert list(r["res_tags"]) == [6] and list(r["res"]) == [WD]
    rig.tick(rig.event(), stage=np.arange(100, 164))
    for bad in (0, (1 << 30) + 1):
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_withdraw_begin(bad)
    # After ydc_stream_restore the capability is off until ydc_stream_withdraw_begin is called.
    b = binding.Context(device=0)
    b.stream_restore(blob)
    with pytest.raises(binding.YdcError, match=INVALID):
        b.stream_withdraw_stage([5])
    with pytest.raises(binding.YdcError, match=INVALID):
        b.stream_withdraw_result()
    b.stream_withdraw_begin(4)
    b.stream_withdraw_stage([5])
    assert len(b.stream_withdraw_result()[0]) == 0
    b.stream_end()
    b.close()
    # ydc_stream_end switches it off; a plain and a leased-only stream cannot have it.
    ctx.stream_end()
    for begin in (None, lambda: ctx.stream_begin(8, 8, 8), lambda: ctx.stream_begin_leased(8, 8, 8, 64, 8, 8, 8, 8)):
        if begin:
            begin()
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_withdraw_begin(4)
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_withdraw_stage([1])
    ctx.stream_begin(8, 8, 8, max_waiting=8)
    ctx.stream_withdraw_begin(4)
    ctx.stream_withdraw_stage([1])
    ctx.stream_begin(8, 8, 8, max_waiting=8)  # (the next begin call switches it off)
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_withdraw_stage([1])
    ctx.stream_end()
    ctx.close()


def test_waiting_take_leaves_a_pending_stage_alone():
    rig = Rig("rpc", tiny_pool(1, 1), 8, 8)
    rig.tick(rig.event(n=4, tags=[1, 2, 3, 4]))
    rig.stage([3])
    assert list(rig.ctx.stream_waiting_take()) == [2, 3, 4] == list(rig.ws.state.take())
    r = rig.tick(rig.event(n=2, tags=[3, 5]))  # (the stage finds nothing in W; the new 3 is not withdrawn)
    assert not len(r["res_tags"]) and list(rig.W().tag) == [3, 5] and list(rig.w.result[0]) == [0]
    rig.close()

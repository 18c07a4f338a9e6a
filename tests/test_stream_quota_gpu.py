"""The cap per requestor inside the tick on the device (ydc_stream_quota_begin / _set / _result;
stream_quota.h: k_quota_claim, k_quota_loads, k_quota_clip, k_quota_label): every tick of a
waiting-and-leased or rpc stream with the capability on is compared with the model
(tests/stream_quota_model.py, pinned on the CPU by tests/test_stream_quota_model.py):

  - the admitted counts and totals of ydc_stream_quota_result, integer for integer;
  - the label YDC_IDX_OVER_QUOTA, apart: exactly the requests that were admitted nothing carry it;
  - everything else through the modes' own check_tick and the inspection check, with the label taken
    back as INTEGRATION 5 describes (the refused requests dropped, an rpc tick's expanded outputs read
    by admitted rows), against the BASE model's record of the stream that was given the clipped requests;
  - the invariant on the device's own state: ydc_stream_requestor_find before and after the tick.
"""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_quota_model as Q
from tests import stream_rpc_cases as RC
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_cases as WC
from tests import stream_wait_lease_model as WL
from tests import stream_withdraw_model as X
from tests import test_stream_inspect_gpu as ist
from tests import test_stream_rpc_gpu as TR
from tests import test_stream_wait_lease_gpu as TWL
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, pack, streaming, synth

pytestmark = pytest.mark.gpu
MODES = ("wl", "rpc")
OQ, WD, TO, WAITING, ENF = Q.IDX_OVER_QUOTA, X.IDX_WITHDRAWN, WL.IDX_TIMEOUT, WL.IDX_WAITING, WL.IDX_ENV_NOT_FOUND
UNL = Q.UNLIMITED
INVALID, CAPACITY = "invalid argument", "capacity of the context exceeded"
A, B = 0x0A000001, 0x0A000002
BOUND = 1 << 20  # ydc_create's max_servants: no servant index is ever a sentinel


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def tiny_pool(n=1, slots=1):
    """n idle servants of one kind with `slots` slots each: max_tasks alone bounds them."""
    sv = synth.make_servants(n, n_tasks_hint=40, n_envs=1, seed=17)
    sv["max_tasks"][:], sv["num_processors"][:], sv["current_load"][:] = slots, 1 << 20, 0
    sv["version"][:], sv["memory_available"][:] = 30, 64 << 30  # (none is short of memory)
    return sv


def crowded_pool(n=200, seed=42, n_envs=2):
    sv = synth.make_servants(n, n_tasks_hint=2000, n_envs=n_envs, seed=seed)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    return sv


def uploaded(sv):
    ctx = binding.Context(device=0, max_servants=BOUND)
    ctx.upload_servants(pack.to_abi_columns(sv))
    return ctx


class Rig:
    """A stream of `mode` with inspection and the capability, on the device and in the model. Scripted
    (every servant beats in every tick, the traffic is written by event()) or seeded (next())."""

    def __init__(self, mode, sv, mw, per_tick, max_overrides=8, max_rows=None, frees=0, renewals=0, n_envs=1,
                 scripted=True, quota=True, withdraw=0, masks=False, rpc_mix=None, max_leases=1 << 15, alive=None,
                 requestors=None):
        self.mode, self.masks, self.t, self.rpc = mode, masks, 0, mode == "rpc"
        self.M, self.G = (RM, TR) if self.rpc else (WL, TWL)
        rate = (lambda now: 1.0) if scripted else (lambda now: 1.0 if now % 12 < 9 else 0.125)
        if self.rpc:
            max_rows = max_rows or 4 * (mw + per_tick)
            self.ws = RM.new_stream(sv, per_tick, frees, renewals, mw, max_rows, n_envs=n_envs, rate=rate, **(rpc_mix or {}))
        else:
            self.ws = WL.new_stream(sv, per_tick, frees, renewals, mw, n_envs=n_envs, rate=rate)
        es = self.ws.es
        if scripted:
            es.hb = es.n
        caps = dict(renewals=16, frees=8192, report_ids=64, reports=es.n) if scripted else {}
        ctx = uploaded(es.sv)
        self.ctx = TR.begin(self.ws, per_tick, max_leases=max_leases, ctx=ctx, **caps) if self.rpc else TWL.begin(
            self.ws, max_leases, per_tick, ctx=ctx, **caps)
        if alive is not None:
            AM.attach(self.ws, alive)
            ctx.stream_alive_begin(alive)
        self.x = ist.Inspected("rpc" if self.rpc else "wait_leased", self.ws, ctx, alive=alive is not None)
        self.q = Q.Quota(self.M, self.ws, alive=alive is not None)
        self.on = quota
        if quota:
            self.begin(max_overrides)
        self.w = None
        if withdraw:
            ctx.stream_withdraw_begin(withdraw)
            self.w = X.Withdrawal(lambda: self.ws.state.q, withdraw)
        self.requestors, self.rng = requestors, np.random.default_rng(7)

    def begin(self, max_overrides):
        self.ctx.stream_quota_begin(max_overrides)
        self.q.begin(max_overrides)

    def set(self, default, over=()):
        self.ctx.stream_quota_set(default, over)
        self.q.set(default, over)

    def held(self):
        return sorted(self.ws.table.L)

    def event(self, reqs=(), wait=1000, free=()):
        """A scripted tick. reqs: (requestor, n_immediate, n_prefetch[, env_id]) per request, deadline
        now + wait (one value or one each); free: the ids given back."""
        n = len(reqs)
        wait = np.broadcast_to(np.asarray(wait, np.int64), (n,))
        if self.rpc:
            ev = RC.scripted(self.ws, self.ws.next_tick(), rpcs=[(reqs[i][1], reqs[i][2], 100, int(wait[i])) for i in range(n)],
                             free=list(free))
        else:
            assert all(r[1] == 1 and r[2] == 0 for r in reqs)
            ev = WC.scripted(self.ws, self.ws.next_tick(), n=n, lease_for=100, wait=wait, free=list(free))
        tk = ev["tasks"]
        tk["min_version"][:] = 0
        tk["requestor_ip"] = np.array([r[0] for r in reqs], np.uint32)
        for i, r in enumerate(reqs):
            if len(r) > 3:
                tk["env_id"][i] = r[3]
        return ev

    def next(self):
        """The seeded stream's next tick, its requests spread over self.requestors (the first has half)."""
        ev = self.ws.next_tick()
        if self.requestors is not None:
            n, k = len(ev["tags"]), len(self.requestors)
            pick = np.where(self.rng.random(n) < 0.5, 0, self.rng.integers(0, k, n))
            ev["tasks"] = dict(ev["tasks"], requestor_ip=np.asarray(self.requestors, np.uint32)[pick])
        return ev

    def load(self, ips):
        f, _ = self.ctx.stream_requestor_find(np.asarray(ips, np.uint32))
        return {int(r["requestor_ip"]): int(r["leases"]) + int(r["waiting_rows"]) for r in f}

    def tick(self, ev, stage=None, snapshot=True):
        """One tick on both sides. -> the model's labelled record; "label": the new requests' answers."""
        ctx, ws, t, rpc = self.ctx, self.ws, self.t, self.rpc
        ips = np.unique(np.asarray(ev["tasks"]["requestor_ip"], np.uint32))
        before = self.load(ips)
        if stage is not None:
            self.w.stage(stage)
            ctx.stream_withdraw_stage(stage)
        if self.x.alive:
            ctx.stream_alive_stage(ev["upd_expires_at"])
        # (the GPU first: gpu_tick reads the heartbeats' masks by the numbering the tick came with)
        got = self.G.gpu_tick(ctx, ws, ev, self.masks)
        res = "res_status" if rpc else "res_idx"
        want = self.w.tick(lambda: self.q.tick(ev), res) if self.w else self.q.tick(ev)
        m_imm, m_pre, m_clipped, m_refused = self.q.result
        if self.on:
            a_imm, a_pre, clipped, refused = ctx.stream_quota_result()
            assert np.array_equal(a_imm, m_imm), "tick %d: admitted immediate gpu %s model %s" % (t, a_imm, m_imm)
            assert np.array_equal(a_pre, m_pre), "tick %d: admitted prefetch gpu %s model %s" % (t, a_pre, m_pre)
            assert (clipped, refused) == (m_clipped, m_refused), (t, clipped, refused, m_clipped, m_refused)
        else:
            assert m_clipped == 0
        # the label, apart
        status, label = (got["status"], want["status"]) if rpc else (got[0], want["out"])
        assert np.array_equal(status, label), "tick %d: the new requests' answers gpu %s model %s" % (t, status, label)
        assert np.array_equal(status == OQ, (m_imm.astype(np.int64) + m_pre) == 0), t
        if rpc:
            assert not got["n_granted"][status == OQ].any(), t
        g_res = got["res_status"] if rpc else got[6]
        assert np.array_equal(g_res, want[res]), "tick %d: the resolved answers differ" % t
        # ... and everything else, with both labels taken back, as the stream that was given the clipped requests
        plain = Q.unlabelled(rpc, got, m_imm, m_pre)
        if rpc:
            plain["res_status"] = X.unlabelled(g_res)
        else:
            plain = plain[:6] + (X.unlabelled(g_res),) + plain[7:]
        self.G.check_tick(t, ctx, ws, plain, self.q.base, snapshot=snapshot)
        self.x.t = t
        self.x.check()
        # the invariant, on the device's own state
        after = self.load(ips)
        for ip in ips.tolist():
            assert after[ip] <= max(self.q.cap_of(ip), before[ip]), "tick %d: requestor %#x holds %d (cap %d, before %d)" % (
                t, ip, after[ip], self.q.cap_of(ip), before[ip])
        self.t += 1
        return dict(want, label=label)

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


REQUESTORS = [A, B, 0x0A000003, 0x0A000004, 0xFFFFFFFF, 0]
# The default, a CI host, a laptop, a banned one: 300 + 3 x 80 + 10 > the crowded pool's slots (at most 400), so it saturates.
THREE_CLASSES = (80, {A: 300, 0x0A000003: 10, 0xFFFFFFFF: 0})


# ---- both modes, every route ------------------------------------------------------------------------

@pytest.mark.parametrize("stream_graph", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_randomised_differential(mode, stream_graph, monkeypatch):
    """200 servants with at most two slots, 300 requests a tick, 40 ticks, six requestors in three cap
    classes; the settings change twice on the way. With the captured step and with the step enqueued
    kernel by kernel (stream_graph=0)."""
    _graph(monkeypatch, stream_graph)
    rig = Rig(mode, crowded_pool(), 6000, 300, frees=60, renewals=20, n_envs=2, scripted=False, max_rows=1 << 14,
              requestors=REQUESTORS)
    rig.set(*THREE_CLASSES)
    refused = partial = waited = 0
    for t in range(40):
        if t == 20:
            rig.set(60, {A: 200, B: 5})
        if t == 30:
            rig.set(*THREE_CLASSES)
        r = rig.tick(rig.next(), snapshot=t % 8 == 0)
        refused += rig.q.result[3]
        partial += rig.q.result[2]
        waited += r["n_waiting"]
    assert refused > 300 and waited > 100 and (partial > refused or mode == "wl"), (refused, partial, waited)
    rig.close()


def _eager_rig(mode, quota=True):
    """The shape of the modes' test_more_than_256_classes_runs_eagerly: ~600 servant classes."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    if mode == "rpc":
        sv["max_tasks"] = np.minimum(sv["max_tasks"], 1)
        return Rig(mode, sv, 1000, 60, frees=300, renewals=100, n_envs=n_envs, scripted=False, quota=quota, masks=True,
                   rpc_mix=BIG, max_rows=1 << 14, max_leases=1 << 16, requestors=REQUESTORS)
    return Rig(mode, sv, 8000, 3000, frees=1500, renewals=300, n_envs=n_envs, scripted=False, quota=quota, masks=True,
               max_leases=1 << 16, requestors=REQUESTORS)


@pytest.mark.parametrize("mode", MODES)
def test_more_than_256_classes_runs_eagerly(mode):
    """eager_only: every tick is enqueued, the four launches with it, once."""
    rig = _eager_rig(mode)
    rig.set(30 if mode == "rpc" else 200, {A: 400, 0xFFFFFFFF: 0})
    rig.ctx.set_profiling(True)
    refused = 0
    for t in range(4):
        rig.tick(rig.next(), snapshot=t == 3)
        refused += rig.q.result[3]
        prof = rig.ctx.kernel_profile()
        assert "k_quota_label" in prof
    assert refused > 10
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_feature_off_means_untouched(mode):
    """A stream that never calls ydc_stream_quota_begin launches no kernel of the feature (the eager
    route names its launches)."""
    rig = _eager_rig(mode, quota=False)
    rig.ctx.set_profiling(True)
    for t in range(2):
        rig.tick(rig.next(), snapshot=False)
        prof = rig.ctx.kernel_profile()
        assert prof and not [k for k in prof if k.startswith("k_quota")], sorted(prof)
        assert ("k_rpc_settle" if mode == "rpc" else "k_wait_lease_commit_inspect") in prof, sorted(prof)
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_twin_with_every_cap_unlimited(mode):
    """Begin alone, and a set of nothing but unlimited caps, change no answer: identical answers, lease
    snapshot, running_tasks and snapshot bytes to a stream that never called begin."""
    rig = Rig(mode, crowded_pool(60, seed=7), 2000, 150, frees=30, renewals=10, n_envs=2, scripted=False,
              requestors=REQUESTORS)
    twin = uploaded(rig.ws.es.sv)
    twin = TR.begin(rig.ws, 150, max_leases=1 << 15, ctx=twin) if mode == "rpc" else TWL.begin(rig.ws, 1 << 15, 150, ctx=twin)
    twin.stream_inspect_begin()
    for t in range(10):
        if t == 4:
            rig.set(UNL, {A: UNL})
        ev = rig.next()
        other = rig.G.gpu_tick(twin, rig.ws, ev)
        r = rig.tick(ev, snapshot=False)
        mine = other["status"] if mode == "rpc" else other[0]
        assert np.array_equal(mine, r["label"]) and not (mine == OQ).any(), t
        for a, b in zip(rig.ctx.stream_leases(), twin.stream_leases()):
            assert np.array_equal(a, b), t
        assert np.array_equal(rig.ctx.get_running(), twin.get_running()), t
    assert rig.ws.state.q.tag.size > 20
    assert rig.ctx.stream_snapshot() == twin.stream_snapshot(), "the capability left a trace in the snapshot"
    twin.stream_end()
    twin.close()
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_structural_heartbeat_in_a_clipping_tick(mode):
    """The tick that clips also appends a servant: its heartbeats take the eager path, the tables are
    rebuilt and the step is captured again, the clip applies all the same."""
    rig = Rig(mode, tiny_pool(2, 1), 16, 8)
    rig.set(3)
    r = rig.tick(rig.event([(A, 1, 0)] * 4))
    assert (r["label"][:2] < WAITING).all() and list(r["label"][2:]) == [WAITING, OQ]  # (two slots, room for three)
    ev = rig.event([(A, 1, 0), (B, 1, 0)])
    row, s_new = AM.append_servant(rig.ws, 0, 0x0A636363)
    ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
    ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
    r = rig.tick(ev)
    assert list(r["label"]) == [OQ, WAITING] and r["n_waiting"] == 1  # (A's waiting entry took the new slot)
    rig.close()


@pytest.mark.parametrize("short", MODES)
def test_aliveness_on_and_a_servant_expiring_in_a_clipping_tick(short):
    """The removal route (servant_alive.h) runs in front of the step: the leases of a servant that
    expires in this tick no longer count for their requestors."""
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    first = AM.first_expiries(70, life=4)
    rig = Rig(short, sv, 1100 if short == "wl" else 400, 400 if short == "wl" else 40, frees=30, renewals=10, n_envs=2,
              scripted=False, alive=first, requestors=REQUESTORS, rpc_mix=BIG if short == "rpc" else None, max_rows=1536)
    rig.set(12, {A: 60, B: 3})
    gen = AM.AliveGen(rig.ws, life=4, p_stop=0.3, p_short=0.3, seed=3)
    both = 0
    for t in range(12):
        ev = gen.next_tick()
        n, k = len(ev["tags"]), len(REQUESTORS)
        pick = np.where(rig.rng.random(n) < 0.5, 0, rig.rng.integers(0, k, n))
        ev["tasks"] = dict(ev["tasks"], requestor_ip=np.asarray(REQUESTORS, np.uint32)[pick])
        rig.tick(ev)
        both += bool(len(rig.q.base["removed"]) and rig.q.result[3])
    assert both, "no tick both erased a servant and refused a request"
    rig.close()


# ---- arrival order at its boundaries --------------------------------------------------------------

def _patterns(n, k):
    """Requestor columns of n requests, each with the caps that make the room run out where it matters."""
    i = np.arange(n)
    one = np.full(n, A, np.uint32)
    yield "one requestor owns every request", one, (n // 2 + 1, {})
    yield "the room ends with the last request", one, (n, {})
    yield "64 distinct requestors in every wave", (0x0B000000 + i % 64).astype(np.uint32), (max(1, n // 128), {})
    yield "a, b, a, b", np.where(i % 2 == 0, A, B).astype(np.uint32), (n // 4 + 1, {B: 3})
    # one requestor whose requests straddle lanes 63 / 64, the workgroup's and the tile's boundary (256)
    at = [p for p in (62, 63, 64, 65, 254, 255, 256, 257, 510, 511, 512, 513, 1023, 1024, 2047, 2048) if p < n]
    if at:
        col = (0x0C000000 + i).astype(np.uint32)
        col[at] = A
        for cut in sorted({1, sum(p < 64 for p in at), sum(p < 256 for p in at), sum(p < 256 for p in at) + 1, len(at)}):
            if cut:  # the room runs out at the last request of a wave / tile, and at the first of the next
                yield "straddling, room %d" % cut, col, (UNL, {A: cut * k})


@pytest.mark.parametrize("sizes", [(1, 63, 64, 65), (255, 256, 257), (1023, 1024, 1025), (2049,)])
@pytest.mark.parametrize("mode", MODES)
def test_arrival_order_at_the_wave_and_tile_boundaries(mode, sizes):
    """n new requests for every n at which the clip pass takes another shape (a wave is 64 requests, a
    tile 256). Every tick gives back all that is held, so held is 0 and pre_i alone decides."""
    rows = (2, 1) if mode == "rpc" else (1, 0)
    rig = Rig(mode, tiny_pool(8, 1200), max(sizes) + 64, max(sizes), max_rows=8192, max_leases=1 << 14)
    seen = set()
    for n in sizes:
        for what, col, caps in _patterns(n, sum(rows)):
            rig.set(*caps)
            r = rig.tick(rig.event([(int(ip), rows[0], rows[1]) for ip in col], wait=0, free=rig.held()), snapshot=False)
            seen.add(int((r["label"] == OQ).sum()) > 0)
            assert len(rig.ws.state.q) == 0, what
    assert seen == {True, False} or max(sizes) == 1
    rig.close()


# ---- the loads -------------------------------------------------------------------------------------

def test_a_large_lease_table_with_a_hot_requestor_and_erased_leases():
    """|L| = 4 097 with one requestor holding 90 %; then 200 of its leases are freed (their records
    stay behind in the slots) in the tick that asks again."""
    rig = Rig("wl", tiny_pool(8, 600), 2112, 2049, max_leases=1 << 14)
    n = 4097
    ips = np.where(np.arange(n) % 10 == 9, B, A).astype(np.uint32)
    for lo in (0, 2049):
        rig.tick(rig.event([(int(ip), 1, 0) for ip in ips[lo:lo + 2049][:n - lo]]), snapshot=False)
    hot = int((ips == A).sum())
    assert len(rig.held()) == n and rig.load([A, B]) == {A: hot, B: n - hot}
    rig.set(hot - 100, {B: n - hot + 2})
    mine = [t for t in rig.held() if rig.x.I.details[t][2] == A][:200]
    r = rig.tick(rig.event([(A, 1, 0)] * 150 + [(B, 1, 0)] * 5, free=mine))
    assert rig.q.held == {A: hot - 200, B: n - hot}
    assert int((r["label"][:150] == OQ).sum()) == 50 and list(r["label"][150:] == OQ) == [False, False, True, True, True]
    rig.close()


@pytest.mark.parametrize("size", [0, 1, 1023, 1024, 1025])
@pytest.mark.parametrize("mode", MODES)
def test_waiting_entries_count_while_they_live(mode, size):
    """|W| == size when the clipping tick finds it, a saturated pool: a third of the clipped requestor's
    entries expire in that tick and another third is withdrawn; what is left counts."""
    rows = (1, 1) if mode == "rpc" else (1, 0)
    rig = Rig(mode, tiny_pool(1, 1), 2100, 1100, withdraw=2048, max_rows=8192)
    rig.tick(rig.event([(B, 1, 0)]))  # (the only slot is taken)
    i = np.arange(size)
    wait = np.where(i % 3 == 0, 1, 1000)
    ev = rig.event([(A if k % 5 else B, rows[0], rows[1]) for k in range(size)], wait=wait)
    rig.tick(ev, snapshot=False)
    assert len(rig.ws.state.q) == size
    gone = ev["tags"][i % 3 == 1]
    live_a = int(((i % 3 == 2) & (i % 5 != 0)).sum()) * sum(rows)
    rig.set(live_a + 3 * sum(rows), {B: 0})
    r = rig.tick(rig.event([(A, rows[0], rows[1])] * 5 + [(B, rows[0], rows[1])]), stage=gone)
    assert rig.q.held == {A: live_a, B: 1 + int(((i % 3 == 2) & (i % 5 == 0)).sum()) * sum(rows)}
    assert list(r["label"]) == [WAITING] * 3 + [OQ] * 3
    assert int((r["res_status" if mode == "rpc" else "res_idx"] == WD).sum()) == len(gone)
    rig.close()


def test_after_remove_servants_reserve_and_restore():
    """The capability is carried over ydc_stream_reserve (settings included), follows ydc_remove_servants'
    renumbering, and is off after ydc_stream_restore until begin is called again."""
    rig = Rig("wl", tiny_pool(6, 2), 64, 32)
    ctx = rig.ctx
    rig.set(4, {B: 2})
    r = rig.tick(rig.event([(A, 1, 0)] * 5 + [(B, 1, 0)] * 3))
    assert list(r["label"] == OQ) == [False] * 4 + [True] + [False] * 2 + [True]
    ctx.stream_reserve(max_tasks=64, max_leases=1 << 16)
    r = rig.tick(rig.event([(A, 1, 0), (B, 1, 0)] * 20, free=rig.held()[:2]))
    assert int((r["label"] == OQ).sum()) == 38 and len(r["label"]) == 40
    removed = np.array([0, 3], np.uint32)
    ctx.remove_servants(removed)
    ist.lease.drop_rows(rig.ws, removed)
    rig.x.check()
    r = rig.tick(rig.event([(A, 1, 0), (B, 1, 0)] * 3))
    assert len(r["label"]) == 6
    blob, sv_cols, tk_cols = ctx.stream_snapshot(), ctx.stream_inspect_servants(), ctx.stream_inspect_tasks()
    b = binding.Context(device=0, max_servants=BOUND)
    b.stream_restore(blob)
    with pytest.raises(binding.YdcError, match=INVALID):
        b.stream_quota_set(1)
    with pytest.raises(binding.YdcError, match=INVALID):  # (inspection is off after a restore)
        b.stream_quota_begin(4)
    b.stream_inspect_begin(sv_cols["discovered_at"], sv_cols["ever_assigned"])
    b.stream_inspect_load(**tk_cols)
    b.stream_quota_begin(4)
    b.stream_quota_set(4, {B: 2})
    ev = rig.event([(A, 1, 0), (B, 1, 0)] * 4, free=rig.held()[:1])
    got_b = TWL.gpu_tick(b, rig.ws, ev)
    r = rig.tick(ev)
    assert np.array_equal(got_b[0], r["label"]) and (r["label"] == OQ).any()
    assert [list(x) if hasattr(x, "__len__") else x for x in b.stream_quota_result()] == [
        list(x) if hasattr(x, "__len__") else x for x in ctx.stream_quota_result()]
    b.stream_end()
    b.close()
    rig.close()


# ---- rpc: the layout by admitted rows --------------------------------------------------------------

def test_rpc_partial_clips_and_the_layout_by_admitted_rows():
    """Partial clips inside an RPC (prefetch first), a refused RPC between two admitted ones, the 5-row
    RPC, and W holding the ADMITTED counts."""
    rig = Rig("rpc", tiny_pool(1, 6), 16, 8, max_rows=256)
    rig.set(4, {B: 1})
    ev = rig.event([(A, 2, 3), (B, 0, 2), (A, 1, 0), (B, 2, 2), (0x0A000003, 2, 3)])
    r = rig.tick(ev)
    a_imm, a_pre, clipped, refused = rig.ctx.stream_quota_result()
    assert list(a_imm) == [2, 0, 0, 0, 2] and list(a_pre) == [2, 1, 0, 0, 2] and (clipped, refused) == (1 + 1 + 1 + 4 + 1, 2)
    assert list(r["label"]) == [0, 0, OQ, OQ, 0] and list(r["n_granted"]) == [4, 1, 0, 0, 1]
    # (the pool had 6 slots: the last RPC got one grant of its 4 admitted rows and does not wait for the rest)
    w = rig.ctx.stream_waiting()
    assert len(w["tag"]) == 0
    tk = rig.ctx.stream_inspect_tasks()
    assert list(tk["prefetch"]) == [0, 0, 1, 1, 1, 0] and list(tk["requestor_ip"]) == [A] * 4 + [B, 0x0A000003]
    # a saturated pool: the RPCs wait with their admitted counts
    rig.set(3)
    ev = rig.event([(0x0A000004, 2, 3), (0x0A000005, 0, 4), (0x0A000004, 1, 1)])
    r = rig.tick(ev)
    assert list(r["label"]) == [WAITING, WAITING, OQ] and r["n_waiting_rows"] == 6
    w = rig.ctx.stream_waiting()
    assert list(w["n_immediate"]) == [2, 0] and list(w["n_prefetch"]) == [1, 3]
    rig.close()


def test_rpc_admitted_unpacks_the_device_outputs():
    """streaming.rpc_admitted on a tick's raw answer: request i's grants at the admitted offsets."""
    rig = Rig("rpc", tiny_pool(2, 8), 16, 8, max_rows=256)
    rig.set(3, {B: 0})
    ev = rig.event([(A, 1, 1), (B, 2, 2), (0x0A000003, 2, 2), (A, 2, 0)])
    raw = TR.gpu_tick(rig.ctx, rig.ws, ev)
    want = rig.q.tick(ev)
    a_imm, a_pre, _, _ = rig.ctx.stream_quota_result()
    assert list(a_imm) == [1, 0, 2, 1] and list(a_pre) == [1, 0, 1, 0]
    res = streaming.rpc_admitted(raw, a_imm, a_pre)
    assert list(res["row_off"]) == [0, 2, 2, 5, 6] and list(raw["status"]) == [0, OQ, 0, 0]
    parts = [streaming.rpc_grants(res, i) for i in range(4)]
    assert [len(p[0]) for p in parts] == [2, 0, 3, 1]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), want["servants"])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want["task_ids"])
    rig.close()


# ---- conventions -----------------------------------------------------------------------------------

def test_conventions_and_refusals():
    rig = Rig("wl", tiny_pool(1, 2), 8, 8, max_overrides=2)
    ctx = rig.ctx
    # max_overrides and max_overrides + 1; a duplicate; a refused set leaves the settings
    rig.set(1, {A: 2, B: 0})
    with pytest.raises(binding.YdcError, match=CAPACITY):
        ctx.stream_quota_set(5, {A: 1, B: 1, 3: 1})
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_quota_set(5, [(A, 1), (A, 2)])
    r = rig.tick(rig.event([(A, 1, 0)] * 3 + [(B, 1, 0), (7, 1, 0), (7, 1, 0)], wait=0))
    assert list(r["label"]) == [0, 0, OQ, OQ, TO, OQ]
    # a refused tick leaves the settings and the last result
    before = ctx.stream_quota_result()
    with pytest.raises(binding.YdcError, match=CAPACITY):
        rig.G.gpu_tick(ctx, rig.ws, rig.event([(A, 1, 0)] * 9))
    assert all(np.array_equal(x, y) for x, y in zip(ctx.stream_quota_result(), before))
    # too little room for the result: the count, nothing written
    n, room = C.c_uint32(0), np.full(6, 99, np.uint32)
    assert binding.lib().ydc_stream_quota_result(ctx._h, room.ctypes.data, None, 5, C.byref(n), None, None) == -4
    assert n.value == 6 and list(room) == [99] * 6
    # begin grows and keeps the settings; smaller or equal does nothing; out of range is refused
    ctx.stream_quota_begin(16)
    ctx.stream_quota_begin(1)
    rig.q.begin(16)
    r = rig.tick(rig.event([(A, 1, 0), (B, 1, 0)], wait=0, free=rig.held()))
    assert list(r["label"]) == [0, OQ]
    rig.set(1, {i: i for i in range(16)})
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_quota_begin((1 << 24) + 1)
    # the capability is carried by book_begin and withdraw_begin
    ctx.stream_book_begin(64)
    ctx.stream_withdraw_begin(8)
    r = rig.tick(rig.event([(1, 1, 0), (1, 1, 0), (0, 1, 0)], wait=0, free=rig.held()))
    assert list(r["label"]) == [0, OQ, OQ]
    # end switches it off; a plain, a waiting-only and a leased-only stream cannot have it; nor can a
    # stream without inspection, nor a context without a bound of servants
    ctx.stream_end()
    begins = (None, lambda: ctx.stream_begin(8, 8, 8), lambda: ctx.stream_begin(8, 8, 8, max_waiting=8),
              lambda: ctx.stream_begin_leased(8, 8, 8, 64, 8, 8, 8, 8),
              lambda: ctx.stream_begin_waiting_leased(8, 8, 8, 8, 64, 8, 8, 8, 8))
    for begin in begins:
        if begin:
            begin()
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_quota_begin(4)
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_quota_set(1)
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_quota_result()
    ctx.stream_inspect_begin()
    ctx.stream_quota_begin(4)
    ctx.stream_quota_set(1)
    ctx.stream_begin_waiting_leased(8, 8, 8, 8, 64, 8, 8, 8, 8)  # (the next begin call switches it off)
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_quota_set(1)
    ctx.stream_end()
    ctx.close()
    free = binding.Context(device=0)  # (max_servants == 0: index 0xFFFFFFFB is possible)
    free.upload_servants(pack.to_abi_columns(tiny_pool(1, 2)))
    free.stream_begin_waiting_leased(8, 8, 8, 8, 64, 8, 8, 8, 8)
    free.stream_inspect_begin()
    with pytest.raises(binding.YdcError, match=INVALID):
        free.stream_quota_begin(4)
    free.stream_end()
    free.close()

"""Departure of requestors on the device (ydc_stream_depart_begin / _stage / _result; stream_depart.h:
k_depart_load, k_depart_leases, k_depart_mark, k_depart_done): every tick of a leased, waiting-and-leased
or rpc stream with the capability on is compared with the model (tests/stream_depart_model.py, pinned on
the CPU by tests/test_stream_depart_model.py), record for record through the modes' own check_tick and
the inspection check, and the counts of ydc_stream_depart_result integer for integer. Rig.final compares
what the device keeps: ydc_stream_leases_get, ydc_stream_inspect_tasks, ydc_stream_inspect_waiting,
ydc_get_running and ydc_stream_requestor_find.

Rig(device=False) runs the model's side alone: the streams' own conditions (a tick that both erases a
servant and frees a departed lease on it, and the like) can be rehearsed without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_depart_model as D
from tests import stream_inspect_model as IM
from tests import stream_lease_cases as LC
from tests import stream_lease_model as L
from tests import stream_outlook_model as OM
from tests import stream_quota_model as Q
from tests import stream_requestor_model as QM
from tests import stream_rpc_cases as RC
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_cases as WC
from tests import stream_wait_lease_model as WL
from tests import stream_withdraw_model as X
from tests import test_stream_inspect_gpu as ist
from tests import test_stream_lease_gpu as TL
from tests import test_stream_rpc_gpu as TR
from tests import test_stream_wait_lease_gpu as TWL
from tests.test_stream_depart_model import A, B, C as CC, NOBODY, REQUESTORS, tiny_pool
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, pack, streaming, synth

pytestmark = pytest.mark.gpu
MODES = ("leased", "wl", "rpc")
IMODE = {"leased": "leased", "wl": "wait_leased", "rpc": "rpc"}
OQ, WD, TO, WAITING, ENF = Q.IDX_OVER_QUOTA, X.IDX_WITHDRAWN, WL.IDX_TIMEOUT, WL.IDX_WAITING, WL.IDX_ENV_NOT_FOUND
INVALID, CAPACITY = "invalid argument", "capacity of the context exceeded"
BOUND = 1 << 20  # ydc_create's max_servants: no servant index is ever a sentinel (the quota asks for it)


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def crowded_pool(n=120, seed=42, n_envs=2):
    sv = synth.make_servants(n, n_tasks_hint=2000, n_envs=n_envs, seed=seed)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    return sv


def begin_stream(ctx, mode, ws, per_tick, max_leases, **caps):
    """The stream of `mode` on ctx, with the bounds the modes' own begin helpers use."""
    if mode == "rpc":
        return TR.begin(ws, per_tick, max_leases=max_leases, ctx=ctx, **caps)
    if mode == "wl":
        return TWL.begin(ws, max_leases, per_tick, ctx=ctx, **caps)
    ctx.stream_begin_leased(ws.es.hb + 8, 16, max(per_tick, 1), max_leases, caps.get("renewals", 4096),
                            caps.get("frees", 8192), caps.get("reports", ws.n_rep), caps.get("report_ids", 1 << 17))
    return ctx


class Rig:
    """A stream of `mode` with inspection and the capability, on the device and in the model. Scripted
    (every servant beats in every tick, the traffic is written by event()) or seeded (next())."""

    def __init__(self, mode, sv, per_tick, mw=64, max_rows=None, max_leases=1 << 12, max_depart=8, frees=0, renewals=0,
                 n_envs=1, scripted=True, depart=True, withdraw=0, quota=False, alive=None, inspect=True, book=0,
                 masks=False, rpc_mix=None, requestors=None, device=True):
        self.mode, self.masks, self.t, self.rpc = mode, masks, 0, mode == "rpc"
        self.M, self.G = {"leased": (L, TL), "wl": (WL, TWL), "rpc": (RM, TR)}[mode]
        self.caps = (per_tick, max_leases, dict(renewals=16, frees=8192, report_ids=64) if scripted else {})
        rate = (lambda now: 1.0) if scripted else (lambda now: 1.0 if now % 12 < 9 else 0.125)
        if self.rpc:
            max_rows = max_rows or 5 * (mw + per_tick)
            self.ws = RM.new_stream(sv, per_tick, frees, renewals, mw, max_rows, n_envs=n_envs, rate=rate, **(rpc_mix or {}))
        elif mode == "wl":
            self.ws = WL.new_stream(sv, per_tick, frees, renewals, mw, n_envs=n_envs, rate=rate)
        else:
            self.ws = L.LeaseStream(sv, per_tick, frees, renewals, L.LeaseTable(), n_envs=n_envs)
        es = self.ws.es
        if scripted:
            es.hb = es.n
            self.caps[2]["reports"] = es.n
        self.ctx = None
        if device:
            self.ctx = self.new_context()
        self.alive = alive is not None
        if self.alive:
            AM.attach(self.ws, alive)
            if device:
                self.ctx.stream_alive_begin(alive)
        self.x = self.d = self.q = self.w = None
        self.max_depart, self.on = max_depart, depart
        if inspect:
            self.inspect()
        if quota:
            self.q = Q.Quota(self.M, self.ws, alive=self.alive)
            self.q.begin(8)
            if device:
                self.ctx.stream_quota_begin(8)
        if withdraw:
            self.w = X.Withdrawal(lambda: self.ws.state.q, withdraw)
            if device:
                self.ctx.stream_withdraw_begin(withdraw)
        if book and device:
            self.ctx.stream_book_begin(book)
        self.requestors, self.rng = requestors, np.random.default_rng(7)

    def new_context(self):
        """A context with this stream's registry and a stream of its bounds (the rig's own, or a twin)."""
        ctx = binding.Context(device=0, max_servants=BOUND)
        ctx.upload_servants(pack.to_abi_columns(self.ws.es.sv))
        per_tick, max_leases, caps = self.caps
        return begin_stream(ctx, self.mode, self.ws, per_tick, max_leases, **caps)

    def inspect(self):
        """Inspection on (late, where the test wants leases that belong to nobody), then the capability."""
        if self.ctx:
            self.x = ist.Inspected(IMODE[self.mode], self.ws, self.ctx, alive=self.alive)
        else:
            IM.attach(self.ws)
        if self.on:
            self.d = D.Departure(self.ws, self.max_depart)
            if self.ctx:
                self.ctx.stream_depart_begin(self.max_depart)

    @property
    def I(self):
        return self.ws.table.inspect

    def begin(self, max_depart):
        self.d.begin(max_depart)
        self.ctx.stream_depart_begin(max_depart)

    def held(self):
        return sorted(self.ws.table.L)

    def event(self, reqs=(), wait=1000, lease_for=100, **kw):
        """A scripted tick. reqs: per request (requestor, n_immediate, n_prefetch); deadline now + wait (one
        value or one each); kw: renew / free / reports as the modes' scripted()."""
        ws, n = self.ws, len(reqs)
        drawn = ws.next_tick()
        wait = np.broadcast_to(np.asarray(wait, np.int64), (n,))
        if self.rpc:
            ev = RC.scripted(ws, drawn, rpcs=[(reqs[i][1], reqs[i][2], lease_for, int(wait[i])) for i in range(n)], **kw)
        elif self.mode == "wl":
            ev = WC.scripted(ws, drawn, n=n, lease_for=lease_for, wait=wait, **kw)
        else:
            ev = LC.scripted(ws, drawn, n=n, lease=[int(drawn["now"]) + lease_for] * n, **kw)
        ev["tasks"]["min_version"][:] = 0
        ev["tasks"]["requestor_ip"] = np.array([r[0] for r in reqs], np.uint32)
        return ev

    def next(self):
        """The seeded stream's next tick, its requests spread over self.requestors (the first has half)."""
        ev = self.ws.next_tick()
        return self.spread(ev)

    def spread(self, ev):
        n, k = len(ev["tasks"]["env_id"]), len(self.requestors)
        pick = np.where(self.rng.random(n) < 0.5, 0, self.rng.integers(0, k, n))
        ev["tasks"] = dict(ev["tasks"], requestor_ip=np.asarray(self.requestors, np.uint32)[pick])
        return ev

    def tick(self, ev, stage=None, wstage=None, snapshot=True):
        """One tick on both sides. -> the model's record; "label": the new requests' answers."""
        ctx, ws, t, rpc = self.ctx, self.ws, self.t, self.rpc
        if stage is not None:
            self.d.stage(stage)
            if ctx:
                ctx.stream_depart_stage(stage)
        if wstage is not None:
            self.w.stage(wstage)
            if ctx:
                ctx.stream_withdraw_stage(wstage)
        if self.alive and ctx:
            ctx.stream_alive_stage(ev["upd_expires_at"])
        # (the GPU first: gpu_tick reads the heartbeats' masks by the numbering the tick came with)
        got = self.G.gpu_tick(ctx, ws, ev, self.masks) if ctx else None
        res = "res_status" if rpc else "res_idx"
        if self.q:
            base = lambda e: self.q.tick(e)  # noqa: E731
        elif getattr(ws.table, "inspect", None) is None:  # (inspection begins late)
            base = lambda e: AM.model_tick(self.M, ws, e) if self.alive else self.M.model_tick(ws, e)  # noqa: E731
        else:
            base = lambda e: IM.model_tick(self.M, ws, e, alive=self.alive)  # noqa: E731
        run = (lambda: self.d.tick(ev, base)) if self.d else (lambda: base(ev))
        want = self.w.tick(run, res) if self.w else run()
        self.t += 1
        label = want["status"] if rpc else want["out"]
        if not ctx:
            return dict(want, label=label)
        if self.d:
            rows, n_l, n_w = self.d.result
            g_rows, g_l, g_w = ctx.stream_depart_result()
            for k in D.COLUMNS:
                assert np.array_equal(g_rows[k], rows[k]), "tick %d: depart %s gpu %s model %s" % (t, k, g_rows[k], rows[k])
            assert (g_l, g_w) == (n_l, n_w), "tick %d: totals gpu %s model %s" % (t, (g_l, g_w), (n_l, n_w))
        # the labels of the other capabilities, apart; then everything else with them taken back
        plain, base_want = got, dict(want)
        if self.q:
            m_imm, m_pre = self.q.result[:2]
            assert np.array_equal(got["status"] if rpc else got[0], label), "tick %d: the new requests' answers" % t
            plain, base_want = Q.unlabelled(rpc, got, m_imm, m_pre), dict(self.q.base)
        if self.w:
            g_res = got["res_status"] if rpc else got[6]
            assert np.array_equal(g_res, want[res]), "tick %d: the resolved answers differ" % t
            base_want[res] = X.unlabelled(want[res])
            if rpc:
                plain = dict(plain, res_status=X.unlabelled(g_res))
            else:
                plain = plain[:6] + (X.unlabelled(g_res),) + plain[7:]
        self.G.check_tick(t, ctx, ws, plain, base_want, snapshot=snapshot)
        if self.x:
            self.x.t = t
            self.x.check()
        return dict(want, label=label)

    def final(self):
        """What the device keeps, against the model: L, the detail records, W, running_tasks, the loads."""
        ctx, ws = self.ctx, self.ws
        if not ctx:
            return
        for name, a, b in zip(("ids", "servants", "expires_at", "zombie"), ctx.stream_leases(), ws.table.snapshot()):
            assert np.array_equal(a, b), "lease snapshot %s differs" % name
        self.x.check()
        assert np.array_equal(ctx.get_running(), ws.es.running.astype(np.uint32))
        if self.mode != "leased":
            got, want = ctx.stream_waiting(), OM.stream_waiting(ws)
            for k in want:
                assert np.array_equal(got[k], want[k]), "W's %s differs" % k
        ips = np.concatenate([REQUESTORS, [NOBODY]]).astype(np.uint32)
        found, un = ctx.stream_requestor_find(ips)
        rows, m_un = QM.stream_fold(ws, ws.table.inspect)
        model = QM.find(rows, ips)
        for k in QM.DTYPE.names:
            assert np.array_equal(found[k], model[k]), "requestor_find %s: gpu %s model %s" % (k, found[k], model[k])
        assert un == m_un

    def close(self):
        self.final()
        if self.ctx:
            self.ctx.stream_end()
            self.ctx.close()


def rows_of(rig):
    rows, n_l, n_w = rig.d.result
    return [tuple(int(rows[k][i]) for k in D.COLUMNS) for i in range(len(rows["requestor_ip"]))], n_l, n_w


def one(ip, k=1):
    return [(int(ip), 1, 0)] * k


# ---- the lease table's pass ------------------------------------------------------------------------

def _fill(rig, ips, per_tick):
    for lo in range(0, len(ips), per_tick):
        r = rig.tick(rig.event([(int(ip), 1, 0) for ip in ips[lo:lo + per_tick]]), snapshot=False)
        assert (r["label"] < ENF).all()


@pytest.mark.parametrize("pattern", ["one holds everything", "every lease its own requestor", "half belong to nobody"])
@pytest.mark.parametrize("max_leases,fills", [(512, (0, 1, 511)), (2048, (1500, 2048))])
def test_lease_table_sizes(max_leases, fills, pattern, device=True):
    """1 024 and 4 096 slots: one workgroup of the pass over L and four. |L| as the departing tick finds it,
    up to a table filled to exactly max_leases; a staged list in LDS (<= 2 048 requestors) and, with every
    lease its own requestor at |L| = 2 048, a longer one that is searched in HBM."""
    per_tick = min(max_leases, 1024)
    late = pattern.startswith("half")
    rig = Rig("leased", tiny_pool(8, 600), per_tick, max_leases=max_leases, max_depart=4096, inspect=not late, device=device)
    for fill in fills:
        if pattern.startswith("one"):
            ips = np.where(np.arange(fill) % 10 == 9, B, A).astype(np.uint32)
            staged = np.array([A], np.uint32)
        else:
            ips = (0x0C000000 + np.arange(fill)).astype(np.uint32)
            staged = np.random.default_rng(fill).permutation(np.concatenate([ips, ips[:3], 0x0D000000 + np.arange(100)]))
            staged = staged.astype(np.uint32)
        if late and rig.d is None:
            _fill(rig, ips[:fill // 2], per_tick)
            rig.inspect()
            _fill(rig, ips[fill // 2:], per_tick)
            nobody = fill // 2
        else:
            _fill(rig, ips, per_tick)
            nobody = 0
        held_before = len(rig.held())
        assert held_before == fill
        r = rig.tick(rig.event(), stage=staged)
        rows, n_l, n_w = rows_of(rig)
        gone = int(np.isin(ips[nobody:], staged).sum())
        assert n_l == gone and r["freed"] == gone and r["n_leases"] == held_before - gone and n_w == 0
        assert [x[0] for x in rows] == staged.tolist()
        for x in rows:  # (a requestor staged twice reports the same row twice)
            assert x[1] == int((ips[nobody:] == x[0]).sum()) and x[2:] == (0, 0, 0)
        r = rig.tick(rig.event(free=rig.held()), snapshot=False)  # (an empty table again)
        assert r["n_leases"] == 0
    rig.close()


def test_a_hot_requestor_with_zombies_and_erased_slots(device=True):
    """One requestor holds 90 % of 1 500 leases, a third of them zombies by now; 200 of its leases are freed
    by the caller in the departing tick (their records stay behind in the slots) and are the caller's."""
    rig = Rig("leased", tiny_pool(8, 600), 1024, max_leases=2048, device=device)
    n = 1500
    ips = np.where(np.arange(n) % 10 == 9, B, A).astype(np.uint32)
    r = rig.tick(rig.event([(int(ip), 1, 0) for ip in ips[:500]], lease_for=1), snapshot=False)
    r = rig.tick(rig.event([(int(ip), 1, 0) for ip in ips[500:]], lease_for=100), snapshot=False)
    r = rig.tick(rig.event(), snapshot=False)
    r = rig.tick(rig.event(), snapshot=False)
    assert sum(e[2] for e in rig.ws.table.L.values()) == 500  # (the first 500: 450 of A, 50 of B)
    mine = [t for t in rig.held() if rig.I.details[t][2] == A][:200]
    r = rig.tick(rig.event(one(A, 3), free=mine), stage=[A, B, A])
    hot = int((ips == A).sum())
    assert rows_of(rig) == ([(A, hot - 200, 250, 0, 0), (B, n - hot, 50, 0, 0), (A, hot - 200, 250, 0, 0)], n - 200, 0)
    assert r["freed"] == n and r["n_leases"] == 3 and (r["label"] < ENF).all()
    rig.close()


# ---- W ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(0, 1, 255), (256, 257), (1024, 1025)])
@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_waiting_queue_sizes(mode, sizes, device=True):
    """|W| == size when the departing tick finds it (a workgroup of the mark pass is 256 positions), a
    saturated pool; in rpc mode the entries have 1 ... 5 rows. The departed requestor asks again in the
    same tick: that request queues."""
    rig = Rig(mode, tiny_pool(1, 1), 1100, mw=1100, max_rows=8192, max_leases=1 << 14, device=device)
    rig.tick(rig.event(one(B)))  # (the only slot is taken)
    for size in sizes:
        k = np.arange(size)
        reqs = [(A if i % 3 else CC, 1 + (i % 5) // 2, (i % 5) - (i % 5) // 2) if mode == "rpc" else (A if i % 3 else CC, 1, 0)
                for i in range(size)]
        rig.tick(rig.event(reqs), snapshot=False)
        assert len(rig.ws.state.q) == size
        r = rig.tick(rig.event(one(A)), stage=[A])
        rows, n_l, n_w = rows_of(rig)
        mine = k % 3 != 0
        want_rows = int((1 + k % 5)[mine].sum()) if mode == "rpc" else int(mine.sum())
        assert rows == [(A, 0, 0, int(mine.sum()), want_rows)] and (n_l, n_w) == (0, int(mine.sum()))
        assert r["n_waiting"] == size - int(mine.sum()) + 1 and list(r["label"]) == [WAITING]
        r = rig.tick(rig.event(), stage=[CC, A, CC], snapshot=False)
        assert r["n_waiting"] == 0 and rows_of(rig)[2] == size - int(mine.sum()) + 1
    rig.close()


@pytest.mark.parametrize("d", [1, 4, 5, 64])
@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_one_wave_of_waiting_entries_of_d_requestors(mode, d, device=True):
    """|W| == 64, one wave of the mark pass, its entries dealt round to d requestors that all depart: one
    key, as many as a wave combines (4), one more (the lanes of the fifth add for themselves), and a key
    for every lane. In rpc mode the entries have 1 ... 5 rows, so the two sums differ."""
    rig = Rig(mode, tiny_pool(1, 1), 80, mw=80, max_leases=1 << 10, max_depart=64, device=device)
    rig.tick(rig.event(one(B)))  # (the only slot is taken)
    k = np.arange(64)
    ips = (0x0C000000 + k % d).astype(np.uint32)
    reqs = [(int(ips[i]), 1 + (i % 5) // 2, (i % 5) - (i % 5) // 2) if mode == "rpc" else (int(ips[i]), 1, 0) for i in range(64)]
    rig.tick(rig.event(reqs), snapshot=False)
    assert len(rig.ws.state.q) == 64
    staged = np.unique(ips)[::-1].copy()
    r = rig.tick(rig.event(), stage=staged)
    rows, n_l, n_w = rows_of(rig)
    per_row = 1 + k % 5 if mode == "rpc" else np.ones(64, np.int64)
    assert rows == [(int(ip), 0, 0, int((ips == ip).sum()), int(per_row[ips == ip].sum())) for ip in staged]
    assert (n_l, n_w) == (0, 64) and r["n_waiting"] == 0
    rig.close()


# ---- the staged list -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["wl", "leased"])
def test_staged_list_sizes(mode, device=True):
    """Lists of 0, 1, 2, 63, 64, 65 and max_depart requestors (a wave is 64 lanes), unsorted, with a repeat
    and a requestor that holds nothing; max_depart + 1 is refused."""
    MX = 130
    rig = Rig(mode, tiny_pool(2, 600), MX, mw=256, max_leases=1 << 11, max_depart=MX, device=device)
    everybody = (0x0C000000 + 7 * np.arange(MX)).astype(np.uint32)
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 63, 64, 65, MX):
        rig.tick(rig.event([(int(ip), 1, 0) for ip in everybody]), snapshot=False)
        staged = rng.permutation(everybody)[:n].copy()
        if n >= 2:
            staged[-1] = staged[0]  # a repeat
        if n >= 63:
            staged[1] = NOBODY
        held_before = len(rig.held())
        r = rig.tick(rig.event(), stage=staged)
        rows, n_l, n_w = rows_of(rig)
        assert [x[0] for x in rows] == staged.tolist() and all(x[1] >= 1 for x in rows if x[0] != NOBODY)
        assert n_l == held_before - r["n_leases"] and (n_l > 0) == (n > 0)
        if n >= 2:
            assert rows[0] == rows[-1]
    if device:
        with pytest.raises(binding.YdcError, match=CAPACITY):
            rig.ctx.stream_depart_stage(np.arange(MX + 1))
        r = rig.tick(rig.event())  # (the refused staging staged nothing)
        assert rows_of(rig) == ([], 0, 0)
    rig.close()


# ---- the three modes, every route -----------------------------------------------------------------

def _stagings(rng, t):
    """A seeded staging for tick t: most ticks none; otherwise one to three requestors, one of them twice,
    and now and then one that holds nothing or everybody."""
    if rng.random() < 0.6:
        return None
    some = rng.choice(REQUESTORS, int(rng.integers(1, 4)), replace=False)
    extra = [NOBODY] if rng.random() < 0.3 else []
    if rng.random() < 0.1:
        some = REQUESTORS
    return np.concatenate([some, extra, some[:1]]).astype(np.uint32)


def _differential(mode, ticks, device=True, **kw):
    mw = 3000
    rig = Rig(mode, crowded_pool(), 150, mw=mw, frees=40, renewals=15, n_envs=2, scripted=False, max_rows=1 << 14,
              max_leases=1 << 14, max_depart=16, requestors=REQUESTORS, device=device, **kw)
    rng = np.random.default_rng(13)
    freed = dismissed = zombies = staged_ticks = 0
    for t in range(ticks):
        stage = _stagings(rng, t)
        rig.tick(rig.next(), stage=stage, snapshot=t % 8 == 0)
        rows, n_l, n_w = rig.d.result
        freed, dismissed, zombies = freed + n_l, dismissed + n_w, zombies + int(rows["zombies"].sum())
        staged_ticks += stage is not None
    rig.close()
    return freed, dismissed, zombies, staged_ticks


@pytest.mark.parametrize("stream_graph,ticks", [("1", 60), ("0", 24)])
@pytest.mark.parametrize("mode", MODES)
def test_randomised_differential(mode, stream_graph, ticks, monkeypatch):
    """120 servants with at most two slots, 150 requests a tick, six requestors, random stagings; with the
    captured step and with the step enqueued kernel by kernel (stream_graph=0)."""
    _graph(monkeypatch, stream_graph)
    freed, dismissed, zombies, staged_ticks = _differential(mode, ticks)
    assert freed > 100 and staged_ticks > 5 and (mode == "leased" or dismissed > 100), (freed, dismissed, zombies)


def _eager_rig(mode, depart=True, device=True):
    """The shape of the modes' test_more_than_256_classes_runs_eagerly: ~600 servant classes."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    kw = dict(n_envs=n_envs, scripted=False, depart=depart, masks=True, max_leases=1 << 16, requestors=REQUESTORS,
              device=device)
    if mode == "rpc":
        sv["max_tasks"] = np.minimum(sv["max_tasks"], 1)
        return Rig(mode, sv, 60, mw=1000, frees=300, renewals=100, rpc_mix=BIG, max_rows=1 << 14, **kw)
    return Rig(mode, sv, 3000, mw=8000, frees=1500, renewals=300, **kw)


@pytest.mark.parametrize("mode", MODES)
def test_more_than_256_classes_runs_eagerly(mode):
    """eager_only: every tick is enqueued, the capability's launches with it, once."""
    rig = _eager_rig(mode)
    rig.ctx.set_profiling(True)
    freed = 0
    for t in range(4):
        rig.tick(rig.next(), stage=[REQUESTORS[t % 2], NOBODY] if t else None, snapshot=t == 3)
        freed += rig.d.result[1]
        prof = rig.ctx.kernel_profile()
        # (the profile names the launches from the batch's front on: of the capability's, the one behind it;
        # that the ones in front of it ran is what the comparison with the model shows)
        assert "k_depart_done" in prof and prof["k_depart_done"][0] == 1, sorted(prof)
    assert freed > 50
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_feature_off_means_untouched(mode):
    """A stream that never calls ydc_stream_depart_begin launches no kernel of the feature (the eager
    route names its launches)."""
    rig = _eager_rig(mode, depart=False)
    rig.ctx.set_profiling(True)
    for t in range(2):
        rig.tick(rig.next(), snapshot=False)
        prof = rig.ctx.kernel_profile()
        assert prof and not [k for k in prof if k.startswith("k_depart")], sorted(prof)
        behind = {"leased": "k_lease_grant_inspect", "wl": "k_wait_lease_commit_inspect", "rpc": "k_rpc_settle"}[mode]
        assert behind in prof, sorted(prof)
    rig.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_twin_that_never_stages(mode):
    """The capability on and nothing ever staged: identical ticks, lease snapshot, running_tasks and snapshot
    bytes to a stream that never called begin."""
    rig = Rig(mode, crowded_pool(60, seed=7), 150, mw=2000, frees=30, renewals=10, n_envs=2, scripted=False,
              max_leases=1 << 14, requestors=REQUESTORS)
    twin = rig.new_context()
    twin.stream_inspect_begin()
    for t in range(10):
        ev = rig.next()
        other = rig.G.gpu_tick(twin, rig.ws, ev)
        r = rig.tick(ev, snapshot=False)
        assert np.array_equal(other["status"] if mode == "rpc" else other[0], r["label"]), t
        for a, b in zip(rig.ctx.stream_leases(), twin.stream_leases()):
            assert np.array_equal(a, b), t
        assert np.array_equal(rig.ctx.get_running(), twin.get_running()), t
        assert rows_of(rig) == ([], 0, 0)
    assert len(rig.held()) > 20
    assert rig.ctx.stream_snapshot() == twin.stream_snapshot(), "the capability left a trace in the snapshot"
    twin.stream_end()
    twin.close()
    rig.close()


# ---- special ticks ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_a_structural_heartbeat_in_the_departing_tick(mode, device=True):
    """The departing tick also appends a servant: its heartbeats take the eager path, the tables are rebuilt
    and the step is captured again; the departure applies all the same, and a waiting request takes the
    new servant's slot."""
    rig = Rig(mode, tiny_pool(2, 1), 8, mw=16, device=device)
    r = rig.tick(rig.event(one(A, 2) + one(B, 2)))
    assert (r["label"][:2] < ENF).all()
    ev = rig.event(one(CC))
    row, s_new = AM.append_servant(rig.ws, 0, 0x0A636363)
    ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
    ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
    r = rig.tick(ev, stage=[A])
    assert rows_of(rig)[1] == 2 and r["n_leases"] == (1 if mode == "leased" else 3)
    assert len(r["running"]) == 3 and int(r["running"].sum()) == r["n_leases"]
    rig.close()


def _alive_run(mode, device=True):
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    first = AM.first_expiries(70, life=4)
    per_tick, mw = {"leased": (120, 64), "wl": (400, 1100), "rpc": (40, 400)}[mode]
    rig = Rig(mode, sv, per_tick, mw=mw, frees=30, renewals=10, n_envs=2, scripted=False, alive=first, requestors=REQUESTORS,
              rpc_mix=BIG if mode == "rpc" else None, max_rows=1536, max_leases=1 << 14, device=device)
    gen = AM.AliveGen(rig.ws, life=4, p_stop=0.3, p_short=0.3, seed=3)
    both = 0
    for t in range(12):
        ev = rig.spread(gen.next_tick())
        on = {tid: e[0] for tid, e in rig.ws.table.L.items()}
        r = rig.tick(ev, stage=[A, REQUESTORS[1 + t % 5]] if t % 2 else [REQUESTORS[t % 6]])
        gone = set(np.asarray(r["removed"]).tolist())
        both += any(on[int(tid)] in gone for tid in rig.d.freed_ids)
    rig.close()
    return both


@pytest.mark.parametrize("mode", MODES)
def test_a_servant_expires_in_the_departing_tick_with_leases_of_the_departed(mode):
    """The removal route (servant_alive.h) runs in front of the step and parks the expired servant's leases:
    a parked lease of a departed requestor is freed by the departure (counted there, no row touched), not as
    an orphan."""
    assert _alive_run(mode), "no tick both erased a servant and freed a departed lease on it"


def test_remove_servants_between_staging_and_tick():
    rig = Rig("wl", tiny_pool(4, 2), 16, mw=16)
    rig.tick(rig.event(one(A, 5) + one(B, 5)))
    assert rig.ws.state.q.tag.size == 2
    rig.d.stage([A])
    rig.ctx.stream_depart_stage([A])
    removed = np.array([1], np.uint32)
    on_it = [t for t, e in rig.ws.table.L.items() if e[0] == 1 and rig.I.details[t][2] == A]
    rig.ctx.remove_servants(removed)
    ist.lease.drop_rows(rig.ws, removed)
    rig.x.check()
    r = rig.tick(rig.event())
    held_a = 5 - len(on_it)  # (the leases on the removed row went with it)
    assert rows_of(rig)[0][0][:2] == (A, held_a) and r["freed"] == held_a
    rig.close()


# ---- composition -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_with_withdrawal_the_same_entry_in_both(mode, device=True):
    rig = Rig(mode, tiny_pool(1, 1), 8, mw=16, withdraw=8, device=device)
    ev = rig.event(one(B) + one(A, 3) + one(CC))
    r = rig.tick(ev)
    assert list(r["label"]) == [0] + [WAITING] * 4
    tags = ev["tags"]
    r = rig.tick(rig.event(), stage=[A], wstage=[tags[2], tags[4]])
    res = r["res_status" if mode == "rpc" else "res_idx"]
    assert list(r["res_tags"]) == list(tags[1:]) and list(res) == [TO, WD, TO, WD]
    assert rows_of(rig) == ([(A, 0, 0, 2, 2)], 0, 2)
    assert list(rig.w.result[0]) == [1, 1] and rig.w.result[1] == 2
    if device:
        counts, total = rig.ctx.stream_withdraw_result()
        assert list(counts) == [1, 1] and total == 2
    rig.close()


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_with_a_quota_a_requestor_at_its_cap_departs_and_asks_again(mode, device=True):
    rig = Rig(mode, tiny_pool(1, 6), 8, mw=16, quota=True, device=device)
    rig.q.set(2)
    if device:
        rig.ctx.stream_quota_set(2)
    r = rig.tick(rig.event(one(A, 3)))
    assert list(r["label"]) == [0, 0, OQ]
    r = rig.tick(rig.event(one(A), wait=0))
    assert list(r["label"]) == [OQ]
    r = rig.tick(rig.event(one(A, 3)), stage=[A])
    assert list(r["label"]) == [0, 0, OQ] and rig.q.held == {A: 0} and rows_of(rig) == ([(A, 2, 0, 0, 0)], 2, 0)
    rig.close()


def test_with_the_book_on(device=True):
    rig = Rig("wl", tiny_pool(2, 3), 8, mw=16, book=64, device=device)
    r = rig.tick(rig.event(one(A, 3) + one(B, 3) + one(A, 2)))
    mine = [t for t in rig.held() if rig.I.details[t][2] == A]
    on0 = [t for t in rig.held() if rig.ws.table.L[t][0] == 0]
    r = rig.tick(rig.event(reports=[(0, on0)]), stage=[A])
    # (a departed lease is unknown to the report that lists it, so the book files nothing for it)
    assert list(r["report_unknown"]) == [int(t in mine) for t in on0] and rows_of(rig) == ([(A, 3, 0, 2, 2)], 3, 2)
    if device:
        assert sorted(rig.ctx.stream_book()[1].tolist()) == sorted(t for t in on0 if t not in mine)
    rig.close()


# ---- conventions -----------------------------------------------------------------------------------

def test_growth_keeps_the_staging_and_the_state(device=True):
    """depart_begin, reserve, book_begin, withdraw_begin and quota_begin all go through stream_regrow: the
    pending staging, the last result, L, W and the records are carried over."""
    rig = Rig("wl", tiny_pool(2, 3), 16, mw=32, max_depart=2, device=device)
    ctx = rig.ctx
    rig.tick(rig.event(one(A, 4) + one(B, 4) + one(CC, 4)))
    growths = [lambda: None] * 5 if not device else [lambda: rig.begin(64), lambda: ctx.stream_reserve(max_tasks=32, max_leases=1 << 13),
               lambda: ctx.stream_book_begin(32), lambda: ctx.stream_withdraw_begin(8), lambda: ctx.stream_quota_begin(4)]
    stagings = [[A], [B, NOBODY], [CC], [A, B], [CC, CC]]
    for grow, staged in zip(growths, stagings):
        rig.d.stage(staged)
        if device:
            before = ctx.stream_depart_result()
            ctx.stream_depart_stage(staged)
            grow()
            after = ctx.stream_depart_result()
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
            rig.x.check()
        r = rig.tick(rig.event(one(int(staged[0]), 2)))
        assert rows_of(rig)[1] + rows_of(rig)[2] > 0
    if device:
        ctx.stream_depart_begin(1)  # (smaller: nothing happens)
        ctx.stream_depart_stage(np.arange(64))
        ctx.stream_depart_stage([])
    rig.close()


def test_snapshot_waits_for_the_staging_and_restore_leaves_it_off():
    rig = Rig("wl", tiny_pool(2, 3), 16, mw=32)
    ctx = rig.ctx
    rig.tick(rig.event(one(A, 4) + one(B, 4)))
    ctx.stream_depart_stage([A])
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_snapshot()
    ctx.stream_depart_stage([])  # (cleared: nothing is pending)
    assert len(ctx.stream_snapshot()) > 0
    r = rig.tick(rig.event(), stage=[A])
    assert rows_of(rig) == ([(A, 4, 0, 0, 0)], 4, 0)
    blob, sv_cols, tk_cols = ctx.stream_snapshot(), ctx.stream_inspect_servants(), ctx.stream_inspect_tasks()
    b = binding.Context(device=0, max_servants=BOUND)
    b.stream_restore(blob)
    for call in (lambda: b.stream_depart_stage([A]), b.stream_depart_result, lambda: b.stream_depart_begin(4)):
        with pytest.raises(binding.YdcError, match=INVALID):  # (off, and inspection is off after a restore)
            call()
    b.stream_inspect_begin(sv_cols["discovered_at"], sv_cols["ever_assigned"])
    b.stream_inspect_load(**{k: tk_cols[k] for k in ("task_id", "started_at", "env_id", "requestor_ip", "prefetch")})
    b.stream_depart_begin(4)
    b.stream_depart_stage([B])
    ev = rig.event(one(A, 2))
    got_b = TWL.gpu_tick(b, rig.ws, ev)
    r = rig.tick(ev, stage=[B])
    assert np.array_equal(got_b[0], r["label"])
    mine, theirs = ctx.stream_depart_result(), b.stream_depart_result()
    # (B's two waiting requests took A's slots in the tick A departed: four leases, nothing waiting)
    assert np.array_equal(mine[0], theirs[0]) and mine[1:] == theirs[1:] == (4, 0)
    b.stream_end()
    b.close()
    rig.close()


def test_conventions_and_refusals():
    rig = Rig("wl", tiny_pool(1, 2), 8, mw=8, max_depart=2)
    ctx, lib = rig.ctx, binding.lib()
    rig.tick(rig.event(one(A, 2) + one(B, 2)))
    # staging again replaces; a refused tick keeps the staging and the last result
    ctx.stream_depart_stage([B])
    ctx.stream_depart_stage([A, A])
    rig.d.stage([A, A])
    before = ctx.stream_depart_result()
    with pytest.raises(binding.YdcError, match=CAPACITY):
        rig.G.gpu_tick(ctx, rig.ws, rig.event(one(A, 9)))
    rig.ws.es.tick_no -= 1
    after = ctx.stream_depart_result()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    r = rig.tick(rig.event())
    assert rows_of(rig) == ([(A, 2, 0, 0, 0)] * 2, 2, 0)
    # too little room for the result: the count, nothing written; the totals are nullable
    n, room = C.c_uint32(0), np.full(2, 99, binding.DEPART_DTYPE)
    p = room.ctypes.data_as(C.POINTER(binding.DepartCount))
    assert lib.ydc_stream_depart_result(ctx._h, p, 1, C.byref(n), None, None) == -4
    assert n.value == 2 and list(room["leases"]) == [99, 99]
    assert lib.ydc_stream_depart_result(ctx._h, p, 2, C.byref(n), None, None) == 0 and list(room["leases"]) == [2, 2]
    assert lib.ydc_stream_depart_result(ctx._h, p, 2, None, None, None) == -1
    assert lib.ydc_stream_depart_stage(ctx._h, None, 1) == -1
    # n > max_depart; out of range begins
    with pytest.raises(binding.YdcError, match=CAPACITY):
        ctx.stream_depart_stage([1, 2, 3])
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_depart_begin(bad)
    # the helper of yadcc_amd.streaming: stage, tick, the result as columns
    result = streaming.dismiss(ctx, [B, NOBODY])
    rig.d.stage([B, NOBODY])
    rig.tick(rig.event())
    cols = result()
    # (B's two waiting requests took A's slots in the tick A departed)
    assert list(cols["requestor_ip"]) == [B, NOBODY] and list(cols["leases"]) == [2, 0] and list(cols["waiting"]) == [0, 0]
    assert (cols["leases_freed"], cols["n_withdrawn"]) == (2, 0) and sorted(cols) == sorted(
        streaming.DEPART_COLUMNS + ("leases_freed", "n_withdrawn"))
    # end switches it off; a plain and a waiting-only stream cannot have it; nor can a stream without inspection
    ctx.stream_end()
    begins = (None, lambda: ctx.stream_begin(8, 8, 8), lambda: ctx.stream_begin(8, 8, 8, max_waiting=8),
              lambda: ctx.stream_begin_leased(8, 8, 8, 64, 8, 8, 8, 8),
              lambda: ctx.stream_begin_waiting_leased(8, 8, 8, 8, 64, 8, 8, 8, 8),
              lambda: ctx.stream_begin_rpc(8, 8, 8, 64, 8, 64, 8, 8, 8, 8))
    for begin in begins:
        if begin:
            begin()
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_depart_begin(4)
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_depart_stage([1])
        with pytest.raises(binding.YdcError, match=INVALID):
            ctx.stream_depart_result()
    ctx.stream_inspect_begin()
    ctx.stream_depart_begin(4)
    ctx.stream_depart_stage([1])
    ctx.stream_begin_leased(8, 8, 8, 64, 8, 8, 8, 8)  # (the next begin call switches it off)
    with pytest.raises(binding.YdcError, match=INVALID):
        ctx.stream_depart_stage([1])
    ctx.stream_inspect_begin()
    ctx.stream_depart_begin(4)  # (a leased stream with inspection can have it)
    ctx.stream_end()
    ctx.close()
    rig.ctx = None

"""ydc_stream_delta_inspect / ydc_stream_inspect_restore / ydc_stream_delta_apply_inspected: a standby
whose inspection records follow the primary delta by delta.

Twins as in tests/test_stream_delta_gpu.py: the primary P ticks against the mode's model with inspection on
(tests/stream_inspect_model.py on top of the lease models). The standby S is restored once from
ydc_stream_delta_base's bytes, gets ydc_stream_inspect_restore with the full sidecar, and then only
applies. After every step: (a) S's snapshot is P's, byte for byte; (b) S's ydc_stream_inspect_tasks and
ydc_stream_inspect_servants equal P's and the model's in every column; (c) the sidecar's bytes are
snapshot.build_inspect_delta of the model's records. At the end both get the same further ticks and agree
with each other and with the model. The promotion test is the one that shows why: quota, departure and
the load per requestor work on S for leases it never granted itself.
Every test fails without the feature: the entry points are missing."""
import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_book_model as BM
from tests import stream_inspect_model as IM
from tests import stream_lease_model as L
from tests import stream_quota_model as Q
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_cases as wcases
from tests import stream_wait_lease_model as WM
from tests import test_stream_alive_gpu as alive
from tests import test_stream_quota_gpu as quota
from tests import test_stream_reserve_gpu as reserve
from tests import test_stream_rpc_gpu as rpc
from tests.test_stream_inspect_gpu import SERVANT_COLS, TASK_COLS
from tests.test_stream_reserve_gpu import all_granted, requests, roomy_pool
from tests.test_stream_snapshot_gpu import Run, leased_run, wait_leased_run
from yadcc_amd import binding, snapshot, synth

pytestmark = pytest.mark.gpu
INVALID = "invalid argument"
FAR = 1 << 40
C = binding.C


class Staged:
    """The lease model M for a stream with the inspection model attached: the tick's batch is staged first
    (stream_inspect_model.model_tick's order), whoever calls model_tick."""

    def __init__(self, M):
        self.M = M

    def model_tick(self, ws, ev, *place):
        ws.table.inspect.stage(ev)
        return self.M.model_tick(ws, ev, *place)


def inspect_begin(run):
    """Inspection on for the Run's stream, on its context and in its model. -> the model's Inspect."""
    I = IM.attach(run.ws)
    run.ctxs[0].stream_inspect_begin()
    run.M = Staged(run.M)
    return I


def inspection_of(ctx):
    return ctx.stream_inspect_tasks(), ctx.stream_inspect_servants()


def same_inspection(what, I, *ctxs):
    """(b): every context answers the two inspection calls as the model does, in every column."""
    want_t, want_s = I.tasks(), I.servants()
    for who, ctx in zip("PS", ctxs):
        got_t, got_s = inspection_of(ctx)
        assert len(got_t["task_id"]) == len(want_t["task_id"]), "%s: |L| on %s is %d, the model's %d" % (
            what, who, len(got_t["task_id"]), len(want_t["task_id"]))
        for k in TASK_COLS:
            bad = np.nonzero(got_t[k] != want_t[k])[0]
            assert bad.size == 0, "%s: tasks %s on %s: lease %d is %s, the model's %s (%d differ)" % (
                what, k, who, got_t["task_id"][bad[0]], got_t[k][bad[0]], want_t[k][bad[0]], bad.size)
        for k in SERVANT_COLS:
            assert got_s[k].dtype == want_s[k].dtype and np.array_equal(got_s[k], want_s[k]), "%s: servants %s on %s" % (what, k, who)
        assert got_s["totals"] == want_s["totals"], (what, who)


class Pair:
    """P with a base taken now, and S restored from the base's bytes and the full sidecar. I: the model's
    Inspect of P's stream; epoch: how often P's records were rewritten (one inspect_begin: 1)."""

    def __init__(self, p, I, epoch=1, run=None, s=None):
        self.p, self.I, self.epoch, self.run, self.steps = p, I, epoch, run, 0
        self.s = s or binding.Context(device=0)
        self.rebase()

    def model_state(self, full):
        return snapshot.inspect_state(full, self.I.tasks(), self.I.servants(), self.epoch)

    def rebase(self):
        base = self.p.stream_delta_base()
        side = self.p.stream_delta_inspect()
        self.prev = snapshot.parse(base)
        assert side == snapshot.build_inspect_delta(self.model_state(self.prev), None, snapshot.INSPECT_FULL), \
            "the full sidecar is not the model's records"
        self.s.stream_restore(base)
        with pytest.raises(binding.YdcError):  # (the blob says nothing about inspection: off after a restore)
            self.s.stream_inspect_tasks()
        self.s.stream_inspect_restore(side)
        assert self.s.stream_snapshot() == base
        same_inspection("after the restore", self.I, self.p, self.s)
        return base, side

    def take(self):
        """One delta with its sidecar taken on P, with (c). -> (delta, sidecar, P's snapshot)."""
        delta = self.p.stream_delta()
        side = self.p.stream_delta_inspect(delta)
        full = self.p.stream_snapshot()
        now = snapshot.parse(full)
        assert delta == snapshot.build_delta(self.prev, now), "step %d: the delta is not f(before, after)" % self.steps
        d = snapshot.parse_delta(delta)
        assert side == snapshot.build_inspect_delta(self.model_state(now), d["ins_id"], snapshot.INSPECT_DELTA), \
            "step %d: the sidecar is not the model's records of the inserted leases" % self.steps
        assert len(side) == 120 + 24 * d["n_ins"] + snapshot._pad8(d["n_ins"]) + 16 * d["n_servants"]
        self.prev = now
        return delta, side, full

    def step(self, **want):
        """One delta taken on P and applied on S, with (a), (b) and (c). want: header fields to assert."""
        delta, side, full = self.take()
        self.s.stream_delta_apply_inspected(delta, side)
        assert self.s.stream_snapshot() == full, "step %d: the standby's snapshot is not the primary's" % self.steps
        same_inspection("step %d" % self.steps, self.I, self.p, self.s)
        self.steps += 1
        d = snapshot.parse_delta(delta)
        for k, v in want.items():
            assert d[k] == v, "step %d: %s is %d, expected %d" % (self.steps, k, d[k], v)
        return d, snapshot.parse_inspect_delta(side)

    def finish(self, events):
        """The same further ticks on both (a step captured on S now runs on the buffers the applies wrote),
        each against the model and against the other."""
        run = self.run
        run.ctxs = [self.p, self.s]
        for ev in events:
            run.tick(ev() if callable(ev) else ev)
            same_inspection("further tick %d" % run.t, self.I, self.p, self.s)
        assert self.p.stream_snapshot() == self.s.stream_snapshot()
        self.p.stream_delta_stop()
        run.end()


def held(ls):
    return np.array(sorted(ls.table.L), np.uint64)


def grant(run, ls, n, seed):
    while n:
        k = min(n, 1000)
        assert all_granted(run.tick(requests(ls, k, FAR, seed)))
        n, seed = n - k, seed + 1


@pytest.mark.parametrize("max_leases", [512, 1024])
def test_insert_lists_of_every_length_and_slots_used_again(max_leases):
    """Tables of 1024 and 2048 slots (one and two workgroups of kLeaseTile). Deltas of 0, 1, 63, 64, 65 and,
    in the larger table, 1000 inserted leases: the gather's and the insert's last wave empty, one lane,
    one short of full, full, one over, and four workgroups. Then every lease erased and as many granted in
    one delta: the new leases take slots whose stale records must not show."""
    sv = roomy_pool(40, 64)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 4
    run = leased_run(sv, ls, dict(tasks=1100, leases=max_leases, renewals=2048, frees=2048, reports=40, report_ids=2048))
    I = inspect_begin(run)
    grant(run, ls, 100, 100)
    pair = Pair(run.ctxs[0], I, run=run)
    seed = 200
    for k in [0, 1, 63, 64, 65] + ([1000] if max_leases == 1024 else []):
        ids = held(ls)
        f = min(k, len(ids))
        start = (len(ids) - f) // 2  # (out of the middle of the id range)
        want = run.tick(requests(ls, 0, 0, seed, free_ids=ids[start:start + f]))
        assert want["freed"] == f
        _, side = pair.step(n_ins=0, n_era=f, n_upd=0)
        assert side["n"] == 0 and side["n_leases"] == len(ids) - f
        g = min(k, max_leases - len(ls.table))
        assert g == k
        assert all_granted(run.tick(requests(ls, g, FAR, seed + 1)))
        _, side = pair.step(n_ins=g, n_era=0, n_upd=0)
        assert side["n"] == g and (side["started_at"] == run.t - 1).all() and (side["env_id"] != binding.INSPECT_NO_ID).all()
        seed += 2
    # Every lease erased, as many granted, one delta: other requestors, another clock.
    ids = held(ls)
    before = inspection_of(pair.s)[0]
    want = run.tick(requests(ls, 0, 0, seed, free_ids=ids))
    assert want["freed"] == len(ids) and want["n_leases"] == 0
    grant(run, ls, len(ids), seed + 1)
    d, side = pair.step(n_ins=len(ids), n_era=len(ids), n_upd=0, n_leases=len(ids))
    after = inspection_of(pair.s)[0]
    assert len(after["task_id"]) == len(before["task_id"]) and (after["started_at"] > before["started_at"].max()).all()
    assert not np.isin(after["task_id"], before["task_id"]).any()

    def further(i):
        def ev():
            ids = held(ls)
            return requests(ls, min(20, max_leases - len(ids)), FAR, 900 + i, free_ids=ids[i::7][:30])
        return ev
    pair.finish([further(i) for i in range(5)])


def test_leases_granted_before_inspection_carry_the_sentinels():
    """80 leases granted while inspection was off: the full sidecar carries the sentinels for them, S shows
    them as P does, and the leases a later delta inserts have their details."""
    sv = roomy_pool(40, 40)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 4
    run = leased_run(sv, ls, dict(tasks=300, leases=512, renewals=512, frees=512, reports=40, report_ids=512))
    grant(run, ls, 80, 1)
    early = held(ls)
    I = inspect_begin(run)
    pair = Pair(run.ctxs[0], I, run=run)
    tk = inspection_of(pair.s)[0]
    assert (tk["env_id"] == binding.INSPECT_NO_ID).all() and (tk["requestor_ip"] == binding.INSPECT_NO_ID).all()
    assert (tk["started_at"] == binding.INSPECT_NO_TIME).all() and not tk["prefetch"].any()
    assert all_granted(run.tick(requests(ls, 30, FAR, 2, free_ids=early[:10])))
    _, side = pair.step(n_ins=30, n_era=10)
    assert (side["env_id"] != binding.INSPECT_NO_ID).all()
    tk = inspection_of(pair.s)[0]
    old = np.isin(tk["task_id"], early)
    assert old.sum() == 70 and (~old).sum() == 30
    assert (tk["env_id"][old] == binding.INSPECT_NO_ID).all() and (tk["env_id"][~old] != binding.INSPECT_NO_ID).all()
    assert (tk["started_at"][old] == binding.INSPECT_NO_TIME).all() and (tk["started_at"][~old] >= 0).all()
    assert pair.p.stream_requestors()[1] == pair.s.stream_requestors()[1] == 70  # (unattributed on both)
    pair.finish([lambda: requests(ls, 5, FAR, 3, free_ids=held(ls)[::9])] * 2)


def test_a_chain_of_20_deltas_and_a_delta_over_20_ticks():
    """The lease model's own traffic (grants, frees, renewals, reports, expiry): a delta with its sidecar
    after each of 20 ticks, then one pair over 20 ticks, whose inserted leases are those of 20 ticks that
    are still there."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=5)
    ls = L.LeaseStream(sv, 40, 30, 10, L.LeaseTable(), n_envs=2)
    run = leased_run(sv, ls, dict(tasks=40, leases=1024, renewals=1024, frees=2048, reports=ls.n_rep, report_ids=1 << 13))
    I = inspect_begin(run)
    run.drive(3)
    pair = Pair(run.ctxs[0], I, run=run)
    seen = dict(n_ins=0, n_era=0, n_upd=0)
    for _ in range(20):
        run.drive(1)
        d, _ = pair.step()
        for k in seen:
            seen[k] += d[k]
    assert min(seen.values()) > 0, seen
    run.drive(20)
    d, side = pair.step()
    assert d["lease_tick"] - d["base_lease_tick"] == 20 and d["n_ins"] > 40 and d["n_era"] > 0
    assert len(set(side["started_at"].tolist())) > 5  # (granted in many different ticks)
    pair.finish([ls.next_tick] * 5)


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_and_leased(stream_graph, monkeypatch):
    """Requests that wait and are granted ticks later start in the tick that grants them; with the captured
    step and with the step enqueued kernel by kernel."""
    reserve._graph(monkeypatch, stream_graph)
    sv = wcases.small_stream().es.sv
    ws = WM.new_stream(sv, 48, 0, 0, 64, n_envs=1, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    run = wait_leased_run(ws, 48, 64, 256)
    I = inspect_begin(run)
    k = np.arange(48)
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=48, lease_for=20 + 3 * k, wait=2 + k % 5))   # now 0
    assert want["n_waiting"] >= 8
    pair = Pair(run.ctxs[0], I, run=run)
    run.tick(wcases.scripted(ws, ws.next_tick(), n=10, lease_for=7 + np.arange(10), wait=3))           # now 1
    pair.step()
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=5, lease_for=9, wait=2, free=sorted(ws.state.T.L)[:6]))  # now 2
    assert want["w_granted"] == 6
    _, side = pair.step(n_era=6)
    assert side["n"] >= 6 and (side["started_at"] == 2).all()  # (asked in tick 0 or 1, started in tick 2)
    for _ in range(2):
        run.tick(wcases.scripted(ws, ws.next_tick(), n=0))
    pair.step()
    pair.finish([lambda: wcases.scripted(ws, ws.next_tick(), n=3, lease_for=5, wait=2, free=sorted(ws.state.T.L)[:2])] * 5)


def test_rpc_with_prefetch_rows_the_book_and_aliveness():
    """An rpc stream over 70 digests with the running-task book and the servants' expiry column: the
    sidecars carry prefetched and immediate grants, env ids beyond one mask word, and ever_assigned as
    the grants of every tick moved it."""
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=70, seed=3)
    ws = RM.new_stream(sv, 40, 300, 100, 1000, 1 << 12, n_envs=70, report_frac=0.3, **alive.BIG)
    ws.es.hb = alive.HB
    ctx = rpc.begin(ws, 40)
    ctx.stream_book_begin(6000)
    book = BM.Book(6000)
    expires = np.full(70, alive.FAR, np.int64)
    A = AM.attach(ws, expires, book)
    ctx.stream_alive_begin(expires)
    run = Run("rpc", ws, ctx, masks=True, A=A, book=book)
    I = inspect_begin(run)
    gen = AM.AliveGen(ws, life=alive.FAR, p_stop=0, p_short=0)
    run.drive(4, gen)
    pair = Pair(ctx, I, run=run)
    flags, envs, ever = set(), set(), I.ever.copy()
    for _ in range(6):
        run.drive(1, gen)
        d, side = pair.step()
        flags |= set(side["prefetch"].tolist())
        envs |= set(side["env_id"].tolist())
        assert len(side["ever_assigned"]) == 70
    assert flags == {0, 1} and max(envs) >= 64 and (I.ever > ever).any()
    run.drive(3, gen)
    pair.step()
    assert ws.es.n == 70
    pair.finish([gen.next_tick] * 5)


class Tee:
    """A mode's GPU test module that remembers the outputs of its last tick."""

    def __init__(self, G):
        self.G, self.last = G, None

    def gpu_tick(self, *a):
        self.last = self.G.gpu_tick(*a)
        return self.last

    def __getattr__(self, k):
        return getattr(self.G, k)


def test_promotion_quota_departure_and_load_on_inherited_leases():
    """After a chain P and S both get ydc_stream_quota_begin with the same settings and five identical ticks.
    Requestor A is at its cap through leases S never granted itself: on both every request of A's is
    answered YDC_IDX_OVER_QUOTA, as the model says. Without the records S would see no holdings and admit
    A in full. Then a departure of C, which holds only inherited leases, frees the same leases on both, and
    ydc_stream_requestor_get is equal."""
    A, B, CC, D = quota.A, quota.B, 0x0A000003, 0x0A000004
    rig = quota.Rig("wl", quota.tiny_pool(8, 16), 64, 32, quota=False, max_leases=512)
    rig.G = tee = Tee(rig.G)
    p, ws, I = rig.ctx, rig.ws, rig.x.I
    rig.tick(rig.event([(A, 1, 0)] * 20 + [(B, 1, 0)] * 5))
    pair = Pair(p, I, s=binding.Context(device=0, max_servants=quota.BOUND))  # (as P's: no index is ever a sentinel)
    s = pair.s
    rig.tick(rig.event([(A, 1, 0)] * 10 + [(CC, 1, 0)] * 6, free=rig.held()[:2]))
    pair.step(n_ins=16, n_era=2)
    rig.tick(rig.event([(A, 1, 0)] * 2))
    pair.step(n_ins=2)
    rig.tick(rig.event())
    pair.step(n_ins=0, n_era=0)
    load = rig.load([A, B, CC])
    assert load == {A: 30, B: 5, CC: 6}
    # Promotion: the host sets the settings again, on both.
    rig.begin(8)
    rig.on = True
    s.stream_quota_begin(8)
    rig.set(30, {B: 6})
    s.stream_quota_set(30, {B: 6})
    refused_a = 0
    for i in range(5):
        ev = rig.event([(A, 1, 0)] * 3 + [(B, 1, 0)] * 2 + [(D, 1, 0)])
        got_s = tee.G.gpu_tick(s, ws, ev)  # (the GPU first: the model's tick moves the registry's numbering)
        want = rig.tick(ev)
        got_p = tee.last
        assert np.array_equal(got_s[0], got_p[0]) and np.array_equal(got_s[0], want["label"]), "tick %d: the answers differ" % i
        assert (want["label"][:3] == quota.OQ).all(), "A was admitted"
        refused_a += int((got_s[0][:3] == quota.OQ).sum())
        g = got_p[0] < quota.OQ
        assert np.array_equal(got_s[1][g], got_p[1][g]), "tick %d: the grant ids differ" % i
        for x, y in zip(got_s[2:], got_p[2:]):
            assert np.array_equal(x, y), "tick %d: outputs differ between the twins" % i
        rp, rs = p.stream_quota_result(), s.stream_quota_result()
        assert all(np.array_equal(x, y) for x, y in zip(rp, rs)), (i, rp, rs)
        assert p.stream_snapshot() == s.stream_snapshot(), "tick %d: the snapshots differ" % i
        same_inspection("promoted tick %d" % i, I, p, s)
    assert refused_a == 15 and rig.load([A, B, D]) == {A: 30, B: 6, D: 5}
    for x, y in zip(p.stream_requestors(), s.stream_requestors()):
        assert np.array_equal(x, y), "ydc_stream_requestor_get differs"
    # C departs: it asked for nothing after the base, so every lease of its is an inherited one on S.
    c_ids = I.tasks()["task_id"][I.tasks()["requestor_ip"] == CC]
    assert len(c_ids) == 6
    ev = rig.event()
    got = []
    for ctx in (p, s):
        ctx.stream_depart_begin(4)
        ctx.stream_depart_stage([CC])
        got.append(tee.G.gpu_tick(ctx, ws, ev))
    for x, y in zip(*got):
        assert np.array_equal(x, y), "the departure tick's outputs differ"
    (rows_p, leases_p, waiting_p), (rows_s, leases_s, waiting_s) = p.stream_depart_result(), s.stream_depart_result()
    assert np.array_equal(rows_p, rows_s) and (leases_p, waiting_p) == (leases_s, waiting_s) == (6, 0)
    assert int(rows_s["leases"][0]) == 6
    assert p.stream_snapshot() == s.stream_snapshot()
    tp, ts = inspection_of(p)[0], inspection_of(s)[0]
    for k in TASK_COLS:
        assert np.array_equal(tp[k], ts[k]), k
    assert not np.isin(c_ids, ts["task_id"]).any() and not (ts["requestor_ip"] == CC).any()
    for x, y in zip(p.stream_requestors(), s.stream_requestors()):
        assert np.array_equal(x, y), "ydc_stream_requestor_get differs after the departure"
    p.stream_delta_stop()
    s.stream_end()
    s.close()
    rig.close()


def unchanged(ctx, what):
    """Context manager: the refused call inside leaves ctx's snapshot bytes and inspection columns as they
    were, with inspection off if it was off."""
    def look():
        try:
            t, sv = inspection_of(ctx)
        except binding.YdcError:
            return ctx.stream_snapshot(), None
        return ctx.stream_snapshot(), {k: t[k] for k in TASK_COLS}, {k: sv[k] for k in SERVANT_COLS}

    class Guard:
        def __enter__(self):
            self.before = look()

        def __exit__(self, *exc):
            if exc[0] is None:
                after = look()
                assert after[0] == self.before[0], "%s changed the stream" % what
                assert (after[1] is None) == (self.before[1] is None), "%s switched inspection" % what
                for x, y in zip(after[1:], self.before[1:]):
                    if x is not None:
                        assert all(np.array_equal(x[k], y[k]) for k in x), "%s changed the inspection columns" % what
    return Guard()


def refused(ctx, what, call):
    with unchanged(ctx, what):
        with pytest.raises(binding.YdcError, match=INVALID):
            call()
            pytest.fail("%s was accepted" % what)


def resealed(blob):
    b = bytearray(blob)
    b[24:32] = snapshot.checksum(bytes(b)).to_bytes(8, "little")
    return bytes(b)


def test_refusals_leave_the_standby_as_it_was():
    sv = roomy_pool(6, 16)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 2
    run = leased_run(sv, ls, dict(tasks=24, leases=512, renewals=16, frees=16, reports=6, report_ids=64))
    p = run.ctxs[0]
    I = inspect_begin(run)
    run.tick(requests(ls, 12, FAR, 1))                                              # ids 0 .. 11
    pair = Pair(p, I, run=run)
    s = pair.s
    base, full_side = p.stream_snapshot(), p.stream_delta_inspect()
    off = binding.Context(device=0)  # a standby without inspection
    off.stream_restore(base)
    run.tick(requests(ls, 4, FAR, 2, free_ids=np.array([3, 7], np.uint64)))          # ids 12 .. 15
    d1, s1, snap1 = pair.take()
    run.tick(requests(ls, 3, FAR, 3, free_ids=np.array([8], np.uint64)))             # ids 16 .. 18
    d2, s2, snap2 = pair.take()
    h1 = snapshot.parse_inspect_delta(s1)
    assert list(h1["task_id"]) == [12, 13, 14, 15] and h1["epoch"] == 1
    one_id = bytearray(s1)
    one_id[120:128] = (11).to_bytes(8, "little")  # ([11, 13, 14, 15]: ascending, below next_id, not the delta's list)
    one_id = resealed(one_id)
    snapshot.parse_inspect_delta(one_id)  # (well-formed: only the pair can tell)
    forged = s1[:24] + bytes([s1[24] ^ 1]) + s1[25:]
    bad = {
        "a sidecar of another delta": (d1, s2),
        "a delta with the sidecar of the one before": (d2, s1),
        "an id column that differs in one id": (d1, one_id),
        "a full sidecar given to apply": (d1, full_side),
        "a forged checksum in the sidecar": (d1, forged),
        "a forged checksum in the delta": (d1[:24] + bytes([d1[24] ^ 1]) + d1[25:], s1),
        "a sidecar cut short": (d1, s1[:-8]),
        "a delta out of order": (d2, s2),
    }
    for name, (delta, side) in bad.items():
        refused(s, name, lambda: s.stream_delta_apply_inspected(delta, side))
    refused(s, "a delta's sidecar given to ydc_stream_inspect_restore", lambda: s.stream_inspect_restore(s1))
    refused(off, "a delta's sidecar given to ydc_stream_inspect_restore, inspection off", lambda: off.stream_inspect_restore(s1))
    refused(off, "a forged full sidecar", lambda: off.stream_inspect_restore(full_side[:24] + bytes([full_side[24] ^ 1]) + full_side[25:]))
    refused(off, "ydc_stream_delta_apply_inspected with inspection off", lambda: off.stream_delta_apply_inspected(d1, s1))
    refused(s, "ydc_stream_delta_apply while inspection is on", lambda: s.stream_delta_apply(d1))  # (the existing refusal)
    off.stream_delta_apply(d1)  # (the plain apply is the call for a standby without inspection)
    assert off.stream_snapshot() == snap1
    refused(off, "a full sidecar of an earlier state", lambda: off.stream_inspect_restore(full_side))
    s.stream_delta_apply_inspected(d1, s1)
    assert s.stream_snapshot() == snap1
    refused(s, "the same pair twice", lambda: s.stream_delta_apply_inspected(d1, s1))
    s.stream_delta_apply_inspected(d2, s2)
    assert s.stream_snapshot() == snap2
    same_inspection("after both pairs", I, p, s)
    # cap one byte short: the size needed, nothing written, nothing changed; then the same bytes.
    run.tick(requests(ls, 2, FAR, 4, free_ids=np.array([12], np.uint64)))
    d3 = p.stream_delta()
    need = C.c_size_t(0)
    buf = C.create_string_buffer(b"\xAA" * 1024, 1024)
    size = 120 + 24 * 2 + 8 + 16 * 6
    with unchanged(p, "a ydc_stream_delta_inspect whose cap is too small"):
        rc = binding.lib().ydc_stream_delta_inspect(p._h, d3, C.c_size_t(len(d3)), buf, C.c_size_t(size - 1), C.byref(need))
        assert rc == -4 and need.value == size and buf.raw == b"\xAA" * 1024
    rc = binding.lib().ydc_stream_delta_inspect(p._h, d3, C.c_size_t(len(d3)), buf, C.c_size_t(1024), C.byref(need))
    assert rc == 0 and need.value == size and buf.raw[:size] == p.stream_delta_inspect(d3)
    refused(p, "the sidecar of an earlier delta", lambda: p.stream_delta_inspect(d2))
    pair.prev = snapshot.parse(p.stream_snapshot())
    s.stream_delta_apply_inspected(d3, buf.raw[:size])
    same_inspection("after the third pair", I, p, s)
    # ydc_stream_inspect_load on P rewrites a record that exists: the epoch moves, P's delta sidecars are
    # refused by S, and a new base with its full sidecar brings S back.
    tk = I.tasks()
    one = {k: tk[k][:1] for k in ("task_id", "started_at", "env_id", "requestor_ip", "prefetch")}
    one["requestor_ip"] = np.array([0x0A0A0A0A], np.uint32)
    p.stream_inspect_load(**one)
    I.load(one)
    pair.epoch += 1
    run.tick(requests(ls, 2, FAR, 5))
    d4, s4, _ = pair.take()
    assert snapshot.parse_inspect_delta(s4)["epoch"] == 2
    refused(s, "an epoch mismatch after ydc_stream_inspect_load on P", lambda: s.stream_delta_apply_inspected(d4, s4))
    pair.rebase()
    assert inspection_of(s)[0]["requestor_ip"][0] == 0x0A0A0A0A
    run.tick(requests(ls, 2, FAR, 6))
    pair.step(n_ins=2)
    # On P, the sidecar of a delta after a further tick: refused, P as it was.
    d5 = p.stream_delta()
    run.tick(requests(ls, 1, FAR, 7))
    refused(p, "ydc_stream_delta_inspect after a further tick", lambda: p.stream_delta_inspect(d5))
    pair.rebase()
    off.stream_end()
    off.close()
    pair.finish([lambda: requests(ls, 3, FAR, 8)] * 2)


def test_other_modes_and_inspection_off_on_the_primary_are_refused():
    sv = roomy_pool(6, 8)
    ctx = reserve.new_ctx(sv)
    lib = binding.lib()
    need, buf, blob = C.c_size_t(0), C.create_string_buffer(4096), bytes(512)

    def all_three_refuse(what):
        rcs = (lib.ydc_stream_delta_inspect(ctx._h, None, C.c_size_t(0), buf, C.c_size_t(4096), C.byref(need)),
               lib.ydc_stream_inspect_restore(ctx._h, blob, C.c_size_t(512)),
               lib.ydc_stream_delta_apply_inspected(ctx._h, blob, C.c_size_t(512), blob, C.c_size_t(512)))
        assert rcs == (-1, -1, -1), (what, rcs)

    all_three_refuse("no stream")
    ctx.stream_begin(8, 8, 12)
    all_three_refuse("a plain stream")
    ctx.stream_end()
    ctx.stream_begin(8, 8, 12, max_waiting=32)
    all_three_refuse("a waiting-only stream")
    ctx.stream_end()
    ctx.stream_begin_leased(8, 8, 12, 64, 16, 16, 6, 64)
    all_three_refuse("a leased stream without inspection and with bytes that are no blobs")
    ctx.stream_inspect_begin()
    side = ctx.stream_delta_inspect()
    p = snapshot.parse_inspect_delta(side)
    assert (p["kind"], p["n"], p["n_servants"], p["epoch"], len(side)) == (snapshot.INSPECT_FULL, 0, 6, 1, 120 + 96)
    binding.group_init_local([ctx])
    all_three_refuse("a context in a group")
    ctx.group_destroy()
    ctx.stream_inspect_restore(side)  # (onto the very state it describes: accepted, and the epoch stays)
    assert ctx.stream_delta_inspect() == side
    ctx.stream_end()
    ctx.close()

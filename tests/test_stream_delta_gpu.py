"""ydc_stream_delta_base / ydc_stream_delta / ydc_stream_delta_apply / ydc_stream_delta_stop: a standby
that follows the primary delta by delta.

Twins: the primary P ticks against the mode's model (the Run of tests/test_stream_snapshot_gpu.py). The
standby S is restored once from ydc_stream_delta_base's bytes and then only applies deltas. After every
delta: (a) the delta is snapshot.build_delta(S's previous snapshot, P's snapshot now), byte for byte — the
device's two passes and the numpy codec agree; (b) S's snapshot is P's, byte for byte. At the end (c) both
get the same five further ticks and agree with each other and with the model in every output, the grant
ids, ydc_stream_leases_get, ydc_get_running, ydc_stream_book_get and ydc_stream_alive_get (Run.tick).
ydc_get_stats has no capture counter, so that the table's buffers stay where a captured step expects them
is asserted by those ticks themselves running the captured route (stream_graph's default) on S.
Every test fails without the feature: the entry points are missing."""
import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_book_model as BM
from tests import stream_lease_model as L
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_cases as wcases
from tests import stream_wait_lease_model as WM
from tests import test_stream_alive_gpu as alive
from tests import test_stream_reserve_gpu as reserve
from tests import test_stream_rpc_gpu as rpc
from tests.test_stream_reserve_gpu import all_granted, requests, roomy_pool
from tests.test_stream_snapshot_gpu import Run, leased_run, report, wait_leased_run, zombies_of
from yadcc_amd import binding, snapshot, synth

pytestmark = pytest.mark.gpu
INVALID, NO_BASE = "invalid argument", "no delta base"
FAR = 1 << 40


class Pair:
    """P (run.ctxs[0]) with a base taken now, and S restored from the base's bytes."""

    def __init__(self, run):
        self.run, self.p = run, run.ctxs[0]
        blob = self.p.stream_delta_base()
        assert blob == self.p.stream_snapshot(), "ydc_stream_delta_base does not write ydc_stream_snapshot's bytes"
        self.s = binding.Context(device=0)
        self.s.stream_restore(blob)
        self.prev = snapshot.parse(blob)
        self.steps = 0

    def step(self, **want):
        """One delta taken on P and applied on S, with (a) and (b). want: header fields to assert."""
        delta = self.p.stream_delta()
        full = self.p.stream_snapshot()
        now = snapshot.parse(full)
        assert delta == snapshot.build_delta(self.prev, now), "step %d: the delta is not f(before, after)" % self.steps
        self.s.stream_delta_apply(delta)
        assert self.s.stream_snapshot() == full, "step %d: the standby's snapshot is not the primary's" % self.steps
        self.prev = now
        self.steps += 1
        d = snapshot.parse_delta(delta)
        for k, v in want.items():
            assert d[k] == v, "step %d: %s is %d, expected %d" % (self.steps, k, d[k], v)
        return d

    def finish(self, events):
        """(c): the same further ticks on both, each against the model and against the other."""
        self.run.ctxs = [self.p, self.s]
        for ev in events:
            self.run.tick(ev() if callable(ev) else ev)
        assert self.p.stream_snapshot() == self.s.stream_snapshot()
        self.p.stream_delta_stop()
        self.run.end()


def held(ls):
    return np.array(sorted(ls.table.L), np.uint64)


def grant(run, ls, n, seed):
    while n:
        k = min(n, 1000)
        assert all_granted(run.tick(requests(ls, k, FAR, seed)))
        n, seed = n - k, seed + 1


@pytest.mark.parametrize("base_leases,max_leases", [(0, 512), (1, 1024), (63, 2048), (64, 512), (65, 1024),
                                                    ("full", 512), ("full", 1024), ("full", 2048)])
def test_leased_lists_of_every_length(base_leases, max_leases):
    """Tables of 1024, 2048 and 4096 slots (one, two and four workgroups of kLeaseTile); the base taken at
    |L| of 0 (before the first tick), 1, 63, 64, 65 and max_leases; deltas of 0, 1, 63, 64, 65 (and, in
    the largest table, 1000) erases and as many inserts: the lists' last wave empty, one lane, one short
    of full, full, and one over. An empty delta. Every lease erased and as many granted in one delta (the
    slots are used again). Every lease renewed."""
    sv = roomy_pool(40, 64)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 4
    run = leased_run(sv, ls, dict(tasks=1100, leases=max_leases, renewals=2048, frees=2048, reports=40, report_ids=2048))
    n0 = max_leases if base_leases == "full" else base_leases
    grant(run, ls, n0, 100)
    pair = Pair(run)
    assert len(pair.prev["l_id"]) == n0 and pair.prev["lease_tick"] == run.t
    seed = 200
    for k in [0, 1, 63, 64, 65] + ([1000] if max_leases == 2048 else []):
        ids = held(ls)
        f = min(k, len(ids))
        start = (len(ids) - f) // 2  # (out of the middle of the id range)
        pick = ids[start:start + f]
        want = run.tick(requests(ls, 0, 0, seed, free_ids=pick))
        assert want["freed"] == f
        pair.step(n_ins=0, n_era=f, n_upd=0, n_leases=len(ids) - f)
        g = min(k, max_leases - len(ls.table))
        assert all_granted(run.tick(requests(ls, g, FAR, seed + 1)))
        pair.step(n_ins=g, n_era=0, n_upd=0)
        seed += 2
    d = pair.step(n_ins=0, n_era=0, n_upd=0)  # nothing happened since: wholly empty, and applied
    assert (d["base_lease_tick"], d["base_next_id"]) == (d["lease_tick"], d["next_id"])
    # Every lease erased, as many granted, one delta.
    ids = held(ls)
    want = run.tick(requests(ls, 0, 0, seed, free_ids=ids))
    assert want["freed"] == len(ids) and want["n_leases"] == 0
    grant(run, ls, len(ids), seed + 1)
    pair.step(n_ins=len(ids), n_era=len(ids), n_upd=0, n_leases=len(ids))
    # Every lease renewed.
    ids = held(ls)
    want = run.tick(requests(ls, 0, 0, seed + 9, renew_ids=ids, renew_expires_at=np.full(len(ids), FAR + 7, np.int64)))
    assert want["renewed"].all()
    pair.step(n_ins=0, n_era=0, n_upd=len(ids))

    def further(i):
        def ev():
            ids = held(ls)
            return requests(ls, min(20, max_leases - len(ids)), FAR, 900 + i, free_ids=ids[i::7][:30])
        return ev
    pair.finish([further(i) for i in range(5)])


def test_expiry_to_zombie_and_reports_that_stamp_and_sweep():
    """Leases that run out become zombies (updates: the state word); a report that lists a servant's zombies
    stamps them and sweeps nothing (updates: the stamps, and the servant's report tick in the registry
    section); the next report leaves one out: it is swept (an erase) and the others carry the new stamp."""
    sv = roomy_pool(40, 40)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 4
    run = leased_run(sv, ls, dict(tasks=300, leases=1024, renewals=1024, frees=1024, reports=40, report_ids=1024))
    T = ls.table
    exp = np.full(300, FAR, np.int64)
    exp[:90] = 2  # (overdue from now == 3 on)
    assert all_granted(run.tick(requests(ls, 300, exp, 1)))        # now 0
    pair = Pair(run)
    for s in (2, 3):
        run.tick(requests(ls, 0, 0, s))                            # now 1, 2
    pair.step(n_ins=0, n_era=0, n_upd=0)  # (a delta over 2 ticks in which no lease changed)
    want = run.tick(requests(ls, 10, FAR, 4))                      # now 3: 90 overdue
    assert want["expired"] == 90
    d = pair.step(n_ins=10, n_era=0, n_upd=90)
    assert ((d["upd_state"] & np.uint32(snapshot.ZOMBIE)) != 0).all()
    zo = zombies_of(T)
    sa = max(zo, key=lambda s: len(zo[s]))
    assert len(zo[sa]) >= 2
    want = run.tick(requests(ls, 0, 0, 5, **report([(sa, zo[sa])])))          # now 4: stamped, nothing swept
    assert want["swept"] == 0
    d = pair.step(n_ins=0, n_era=0, n_upd=len(zo[sa]))
    assert set((d["upd_state"] & np.uint32(snapshot.STAMP)).tolist()) == {run.t} and d["rep_tick"][sa] == run.t
    want = run.tick(requests(ls, 0, 0, 6, **report([(sa, zo[sa][1:])])))      # now 5: the first one swept
    assert want["swept"] == 1
    d = pair.step(n_ins=0, n_era=1, n_upd=len(zo[sa]) - 1)
    assert list(d["era_id"]) == [zo[sa][0]]
    # The standby sweeps, renews and refuses as the primary does.
    live = [t for t in held(ls).tolist() if not T.L[t][2]][:40]
    others = sorted(s for s in zo if s != sa)[:3]
    pair.finish([lambda: requests(ls, 0, 0, 7, **report([(s, []) for s in others])),
                 lambda: requests(ls, 0, 0, 8, renew_ids=held(ls), renew_expires_at=np.full(len(T), FAR + 1, np.int64)),
                 lambda: requests(ls, 20, FAR, 9, free_ids=np.array(live, np.uint64)),
                 lambda: requests(ls, 0, 0, 10), lambda: requests(ls, 5, FAR, 11)])


def test_a_chain_of_20_deltas_and_a_delta_over_20_ticks():
    """The lease model's own traffic (grants, frees, renewals, reports, expiry): a delta after each of 20
    ticks, then one delta over 20 ticks."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=5)
    ls = L.LeaseStream(sv, 120, 60, 20, L.LeaseTable(), n_envs=2)
    run = leased_run(sv, ls, dict(tasks=120, leases=4096, renewals=4096, frees=8192, reports=ls.n_rep, report_ids=1 << 15))
    run.drive(3)
    pair = Pair(run)
    seen = dict(n_ins=0, n_era=0, n_upd=0)
    for _ in range(20):
        run.drive(1)
        d = pair.step()
        for k in seen:
            seen[k] += d[k]
    assert min(seen.values()) > 0, seen
    rec = run.drive(20)
    assert sum(r["expired"] for r in rec) and sum(r["freed"] for r in rec)
    d = pair.step()
    assert d["lease_tick"] - d["base_lease_tick"] == 20 and d["n_ins"] > 120 and d["n_era"] > 60
    pair.finish([ls.next_tick] * 5)


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_and_leased(stream_graph, monkeypatch):
    """W is carried whole: entries that wait, lapse and are granted between the deltas. With the captured
    step and with the step enqueued kernel by kernel."""
    reserve._graph(monkeypatch, stream_graph)
    sv = wcases.small_stream().es.sv
    ws = WM.new_stream(sv, 48, 0, 0, 64, n_envs=1, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    run = wait_leased_run(ws, 48, 64, 256)
    k = np.arange(48)
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=48, lease_for=20 + 3 * k, wait=2 + k % 5))   # now 0
    assert want["n_waiting"] >= 8
    pair = Pair(run)
    assert len(pair.prev["w_tag"]) == want["n_waiting"]
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=10, lease_for=7 + np.arange(10), wait=3))   # now 1
    d = pair.step(n_waiting=want["n_waiting"])
    assert d["n_waiting"] > d["base_n_waiting"]
    want = run.tick(wcases.scripted(ws, ws.next_tick(), n=5, lease_for=9, wait=2, free=sorted(ws.state.T.L)[:6]))  # now 2
    assert want["w_expired"] >= 1 and want["w_granted"] == 6
    pair.step(n_era=6, n_waiting=want["n_waiting"])
    for _ in range(2):
        run.tick(wcases.scripted(ws, ws.next_tick(), n=0))
    pair.step()
    pair.finish([lambda: wcases.scripted(ws, ws.next_tick(), n=3, lease_for=5, wait=2, free=sorted(ws.state.T.L)[:2])] * 5)


def test_rpc_with_book_aliveness_and_two_mask_words():
    """An rpc stream over 70 digests (env_words == 2) with the running-task book and the servants' expiry
    column: W with its row counts, E (heartbeats move it in every tick) and B, which is carried exactly
    when it changed."""
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
    gen = AM.AliveGen(ws, life=alive.FAR, p_stop=0, p_short=0)
    run.drive(4, gen)
    pair = Pair(run)
    assert pair.prev["env_words"] == 2 and pair.prev["book"] and pair.prev["alive"] and pair.prev["rpc"]
    carried = 0
    for _ in range(6):
        run.drive(1, gen)
        d = pair.step()
        carried += d["book_present"]
        assert d["n_wait_rows"] == ws.state.q.rows() and len(d["e_expires_at"]) == 70
    assert carried > 0 and len(book.B) > 0
    d = pair.step(book_present=0, n_ins=0, n_era=0, n_upd=0)  # (B as in the base: not carried)
    assert d["n_book"] == len(book.B)
    run.drive(3, gen)
    pair.step()
    assert ws.es.n == 70
    pair.finish([gen.next_tick] * 5)


def empty_tick(ctx, now, ip=None, n=0, alive=False):
    """A tick by hand, beside the models: n requests of digest 0 from host `ip`, nothing else."""
    if alive:
        ctx.stream_alive_stage(np.empty(0, np.int64))
    z32, z64, i64 = np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.int64)
    z = np.zeros(n, np.uint32)
    tasks = {"env_id": z, "min_version": z, "requestor_ip": z + np.uint32(ip or 0)}
    return ctx.stream_tick_leased(z32, np.empty(0, binding.ROW_DTYPE), z32, z64, i64, z64, z32, np.zeros(1, np.uint32), z64,
                                  tasks, np.full(n, FAR, np.int64), now)


def test_host_aliases_are_part_of_the_structure():
    """The base carries the aliases; requests from an aliased host are kept off that servant on the standby
    as on the primary; changing the aliases on the primary ends the chain."""
    sv = roomy_pool(6, 8)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 2
    run = leased_run(sv, ls, dict(tasks=8, leases=64, renewals=16, frees=16, reports=6, report_ids=64))
    p = run.ctxs[0]
    alias_ip = (192 << 24) + 77
    p.set_host_aliases(np.array([alias_ip], np.uint32), np.array([3], np.uint32))
    run.aliases = ([alias_ip], [3])
    assert all_granted(run.tick(requests(ls, 8, FAR, 1)))
    pair = Pair(run)
    assert list(pair.prev["alias_servant"]) == [3]
    assert all_granted(run.tick(requests(ls, 6, FAR, 2)))
    pair.step(n_ins=6)
    s = pair.s
    out_p, out_s = empty_tick(p, run.t, alias_ip, 4), empty_tick(s, run.t, alias_ip, 4)
    assert np.array_equal(out_p[0], out_s[0]) and np.array_equal(out_p[1], out_s[1])
    assert 3 not in out_p[0].tolist() and (out_p[0] < 6).all()
    assert p.stream_snapshot() == s.stream_snapshot()
    # (P has ticked beside its standby now; a delta still comes out, and S, which ticked, refuses it)
    delta = p.stream_delta()
    with pytest.raises(binding.YdcError, match=INVALID):
        s.stream_delta_apply(delta)
    p.set_host_aliases(np.empty(0, np.uint32), np.empty(0, np.uint32))
    with pytest.raises(binding.YdcError, match=NO_BASE):
        p.stream_delta()
    for c in (p, s):
        c.stream_end()
        c.close()


def unchanged(ctx, what):
    """Context manager: the refused call inside leaves ctx's snapshot bytes as they were."""
    class Guard:
        def __enter__(self):
            self.before = ctx.stream_snapshot()

        def __exit__(self, *exc):
            if exc[0] is None:
                assert ctx.stream_snapshot() == self.before, "%s changed the stream" % what
    return Guard()


def test_apply_refusals_leave_the_standby_as_it_was():
    sv = roomy_pool(6, 16)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 2
    run = leased_run(sv, ls, dict(tasks=24, leases=64, renewals=16, frees=16, reports=6, report_ids=64))
    p = run.ctxs[0]
    with unchanged(p, "ydc_stream_delta without a base"):
        with pytest.raises(binding.YdcError, match=NO_BASE):
            p.stream_delta()
    run.tick(requests(ls, 12, FAR, 1))                                              # ids 0 .. 11
    run.tick(requests(ls, 0, 0, 2, free_ids=np.array([2, 5], np.uint64)))            # 2 and 5 are gone
    pair = Pair(run)
    s = pair.s
    base_blob = p.stream_snapshot()
    run.tick(requests(ls, 4, FAR, 3, free_ids=np.array([3, 7], np.uint64)))          # ids 12 .. 15
    d1, snap1 = p.stream_delta(), p.stream_snapshot()
    run.tick(requests(ls, 3, FAR, 4, free_ids=np.array([8], np.uint64)))
    d2, snap2 = p.stream_delta(), p.stream_snapshot()
    assert d1 == snapshot.build_delta(snapshot.parse(base_blob), snapshot.parse(snap1))
    assert d2 == snapshot.build_delta(snapshot.parse(snap1), snapshot.parse(snap2))
    h = snapshot.parse_delta(d1)
    assert list(h["era_id"]) == [3, 7] and list(h["ins_id"]) == [12, 13, 14, 15]
    era_off, ins_off = snapshot.DELTA_HEADER.unpack_from(d1)[33], snapshot.DELTA_HEADER.unpack_from(d1)[31]

    def forged(at, value):
        b = bytearray(d1)
        b[at:at + 8] = int(value).to_bytes(8, "little")
        b[24:32] = snapshot.checksum(bytes(b)).to_bytes(8, "little")
        return bytes(b)

    # A twin standby that ticked.
    s2 = binding.Context(device=0)
    s2.stream_restore(base_blob)
    empty_tick(s2, run.t)
    bad = {
        "a delta out of order": (s, d2),
        "an erased id that is not there": (s, forged(era_off, 2)),     # (2 was freed before the base; [2, 7] ascends)
        "a second erased id that is not there": (s, forged(era_off + 8, 5)),  # ([3, 5]: 5 was freed before the base too)
        "an inserted id that is a lease": (s, forged(ins_off, 9)),
        "a flipped byte": (s, d1[:300] + bytes([d1[300] ^ 4]) + d1[301:]),
        "cut short": (s, d1[:-8]),
        "a delta onto a ticked standby": (s2, d1),
    }
    snapshot.parse_delta(bad["an erased id that is not there"][1])  # (well-formed: only the table can tell)
    for name, (ctx, blob) in bad.items():
        with unchanged(ctx, name):
            with pytest.raises(binding.YdcError, match=INVALID):
                ctx.stream_delta_apply(blob)
                pytest.fail("%s was applied" % name)
    s.stream_delta_apply(d1)
    assert s.stream_snapshot() == snap1
    with unchanged(s, "the same delta twice"):
        with pytest.raises(binding.YdcError, match=INVALID):
            s.stream_delta_apply(d1)
    s.stream_delta_apply(d2)
    assert s.stream_snapshot() == snap2
    # A delta of another base: P takes a new base one tick later, S is still at the old one.
    run.tick(requests(ls, 2, FAR, 5))
    assert p.stream_delta_base() == p.stream_snapshot()
    run.tick(requests(ls, 2, FAR, 6))
    d_other = p.stream_delta()
    with unchanged(s, "a delta of another base"):
        with pytest.raises(binding.YdcError, match=INVALID):
            s.stream_delta_apply(d_other)
    # cap too small: the size needed, nothing written, the base not advanced; then the same bytes.
    run.tick(requests(ls, 1, FAR, 7, free_ids=np.array([12], np.uint64)))
    before = snapshot.parse(p.stream_snapshot())
    prev = snapshot.parse_delta(d_other)
    C = binding.C
    need = C.c_size_t(0)
    buf = C.create_string_buffer(b"\xAA" * 4096, 4096)
    rc = binding.lib().ydc_stream_delta(p._h, buf, C.c_size_t(271), C.byref(need))
    assert rc == -4 and need.value >= 272 + 24 + 8 and buf.raw == b"\xAA" * 4096
    rc = binding.lib().ydc_stream_delta(p._h, buf, C.c_size_t(need.value - 1), C.byref(need))
    assert rc == -4 and buf.raw == b"\xAA" * 4096
    size = need.value
    rc = binding.lib().ydc_stream_delta(p._h, buf, C.c_size_t(4096), C.byref(need))
    assert rc == 0 and need.value == size
    d3 = snapshot.parse_delta(buf.raw[:size])
    assert (d3["base_lease_tick"], d3["n_ins"], d3["n_era"]) == (prev["lease_tick"], 1, 1) and d3["lease_tick"] == before["lease_tick"]
    # S missed a delta: it is restored from a new base.
    s.stream_restore(p.stream_delta_base())
    run.ctxs = [p, s]
    run.tick(requests(ls, 3, FAR, 8))
    s2.stream_end()
    s2.close()
    run.end()


def test_the_chain_ends_when_the_structure_changes():
    """ydc_stream_delta returns YDC_ERR_NO_BASE after a structural heartbeat, an effective ydc_stream_reserve,
    ydc_remove_servants and a tick in which a servant expires; the refused call writes nothing and leaves
    the stream ticking; the base is dropped (the next call says NO_BASE too); a new base works."""
    sv = roomy_pool(8, 16)
    ls = L.LeaseStream(sv, 0, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 2
    run = leased_run(sv, ls, dict(tasks=24, leases=64, renewals=16, frees=16, reports=8, report_ids=64))
    p = run.ctxs[0]
    run.tick(requests(ls, 12, FAR, 1))
    now, with_e = [run.t], [False]

    def chain_ended(what):
        with unchanged(p, what):
            for _ in range(2):
                with pytest.raises(binding.YdcError, match=NO_BASE):
                    p.stream_delta()
        before = p.stream_delta_base()
        s = binding.Context(device=0)
        s.stream_restore(before)
        empty_tick(p, now[0], n=2, alive=with_e[0])
        now[0] += 1
        delta, after = p.stream_delta(), p.stream_snapshot()
        assert delta == snapshot.build_delta(snapshot.parse(before), snapshot.parse(after)), what
        s.stream_delta_apply(delta)
        assert s.stream_snapshot() == after, what
        s.stream_end()
        s.close()

    assert p.stream_delta_base() == p.stream_snapshot()
    # A heartbeat that is not structural keeps the chain (current_load alone).
    reg = snapshot.parse(p.stream_snapshot())
    row = {k: int(reg[c][1]) for k, c in (("version", "version"), ("num_processors", "num_processors"), ("current_load", "current_load"),
                                          ("max_tasks", "servant_max_tasks"), ("flags", "flags"), ("ip_id", "ip_id"))}
    row["env_mask"] = int(reg["env_mask"][1][0])
    p.update_servants([1], [dict(row, current_load=row["current_load"] + 3)])
    d = snapshot.parse_delta(p.stream_delta())
    assert d["current_load"][1] == row["current_load"] + 3 and d["n_ins"] == 0
    # A structural one (another environment set, one no request asks for) ends it.
    p.update_servants([1], [dict(row, current_load=row["current_load"] + 3, env_mask=row["env_mask"] | 1 << 40)])
    chain_ended("a structural heartbeat")
    assert p.stream_reserve(max_leases=64)["max_leases"] == 64  # (no effect: the chain goes on)
    p.stream_delta()
    assert p.stream_reserve(max_leases=200)["max_leases"] == 200
    chain_ended("ydc_stream_reserve")
    p.remove_servants([7])
    chain_ended("ydc_remove_servants")
    # A tick in which a servant expires.
    expires = np.full(7, FAR, np.int64)
    expires[6] = now[0]  # (not due in the next tick, whose clock is now[0]; due in the one after)
    p.stream_alive_begin(expires)
    with_e[0] = True
    chain_ended("ydc_stream_alive_begin")  # (the mode gained E)
    assert snapshot.parse(p.stream_snapshot())["n_servants"] == 7
    empty_tick(p, now[0], alive=True)
    now[0] += 1
    assert list(p.stream_alive_removed()[0]) == [6] and snapshot.parse(p.stream_snapshot())["n_servants"] == 6
    chain_ended("a tick that expired a servant")
    p.stream_delta_stop()
    with pytest.raises(binding.YdcError, match=NO_BASE):
        p.stream_delta()
    p.stream_end()
    p.close()


def test_modes_without_a_lease_table_and_groups_are_refused():
    sv = roomy_pool(6, 8)
    ctx = reserve.new_ctx(sv)
    lib, C = binding.lib(), binding.C
    need, buf = C.c_size_t(0), C.create_string_buffer(4096)

    def all_four_refuse(what):
        rcs = (lib.ydc_stream_delta_base(ctx._h, buf, C.c_size_t(4096), C.byref(need)),
               lib.ydc_stream_delta(ctx._h, buf, C.c_size_t(4096), C.byref(need)),
               lib.ydc_stream_delta_apply(ctx._h, bytes(512), C.c_size_t(512)), lib.ydc_stream_delta_stop(ctx._h))
        assert rcs == (-1, -1, -1, -1), (what, rcs)

    all_four_refuse("no stream")
    ctx.stream_begin(8, 8, 12)
    all_four_refuse("a plain stream")
    out = ctx.stream_tick(np.empty(0, np.uint32), np.empty(0, binding.ROW_DTYPE), np.empty(0, np.uint32),
                          synth.make_tasks(4, sv, n_envs=1, seed=1, self_frac=0.0))
    assert len(out) == 4
    ctx.stream_end()
    ctx.stream_begin(8, 8, 12, max_waiting=32)
    all_four_refuse("a waiting-only stream")
    assert len(ctx.stream_snapshot()) > 0  # (its full snapshot is what such a stream has)
    ctx.stream_end()
    ctx.stream_begin_leased(8, 8, 12, 64, 16, 16, 6, 64)
    assert ctx.stream_delta_base() == ctx.stream_snapshot()
    binding.group_init_local([ctx])
    all_four_refuse("a context in a group")
    ctx.group_destroy()
    empty_tick(ctx, 0, n=3)
    assert snapshot.parse_delta(ctx.stream_delta())["n_ins"] == 3  # (the base outlived the refusals)
    ctx.stream_delta_stop()
    ctx.stream_end()
    ctx.close()

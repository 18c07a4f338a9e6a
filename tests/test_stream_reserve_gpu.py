"""ydc_stream_reserve: the capacities of an open stream grow and its device-resident state (the
lease table L with next_id, the waiting queue W, the clock, the tick number behind the report
stamps) is carried over.

Every case is a TWIN RUN: context A is begun with the final bounds, context B is begun small and
reserved in mid-stream; both get identical ticks on the same servant table. Each tick of each
context is compared with the mode's model (tests/stream_lease_model.py, stream_wait_lease_model.py,
stream_rpc_model.py, all pinned against the verbatim reference) on every output, on running_tasks,
on the lease snapshot and on the tick's counts in ydc_get_stats, and A and B are compared with each
other, exactly. The models are made with the final bounds. Every test fails without the feature:
the entry point is missing."""
import numpy as np
import pytest

from tests import stream_lease_model as L
from tests import stream_rpc_cases as rcases
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_cases as wcases
from tests import stream_wait_lease_model as WM
from tests import test_stream_lease_gpu as lease
from tests import test_stream_rpc_gpu as rpc
from tests import test_stream_wait_lease_gpu as wl
from yadcc_amd import binding, pack, streaming, synth

pytestmark = pytest.mark.gpu
TILE = 1024
FAR = 64 * TILE
SNAP = ("ids", "servants", "expires_at", "zombie")
COUNTERS = ("granted", "leases_expired", "leases_swept", "leases_freed", "renewals_refused")


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def new_ctx(sv):
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(sv))
    return ctx


def roomy_pool(n, slots, seed=42):
    """n idle servants of one digest that max_tasks alone bounds: n * slots grants fit."""
    sv = synth.make_servants(n, n_tasks_hint=n * slots, n_envs=1, seed=seed)
    sv["num_processors"][:], sv["current_load"][:] = 4096, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = slots, 0
    return sv


def same_outputs(t, mode, a, b):
    """The outputs of one tick on A and on B, wherever they are defined."""
    if mode == "rpc":
        for k in a:
            if k not in ("servants", "task_ids"):
                assert np.array_equal(a[k], b[k]), "tick %d: %s differs between the twins" % (t, k)
        for i in range(len(a["status"])):
            for x, y in zip(streaming.rpc_grants(a, i), streaming.rpc_grants(b, i)):
                assert np.array_equal(x, y), "tick %d: grants of request %d differ between the twins" % (t, i)
        return
    if mode == "leased":
        (out, ids, *rest), (out_b, ids_b, *rest_b) = a, b
        g = out < L.IDX_ENV_NOT_FOUND
    else:
        (out, ids, ren, unk, n_l, tags, idx, rids, n_w), (out_b, ids_b, ren_b, unk_b, n_lb, tags_b, idx_b, rids_b, n_wb) = a, b
        g, gw = out < WM.IDX_WAITING, idx < WM.IDX_ENV_NOT_FOUND
        assert np.array_equal(idx, idx_b) and np.array_equal(rids[gw], rids_b[gw]), t
        rest, rest_b = (ren, unk, n_l, tags, n_w), (ren_b, unk_b, n_lb, tags_b, n_wb)
    assert np.array_equal(out, out_b) and np.array_equal(ids[g], ids_b[g]), "tick %d: answers differ between the twins" % t
    for x, y in zip(rest, rest_b):
        assert np.array_equal(x, y), "tick %d: outputs differ between the twins" % t


def same_state(t, a, b):
    for name, x, y in zip(SNAP, a.stream_leases(), b.stream_leases()):
        assert np.array_equal(x, y), "tick %d: lease snapshot %s differs between the twins" % (t, name)
    assert np.array_equal(a.get_running(), b.get_running()), "tick %d: running differs between the twins" % t
    sa, sb = a.stats(), b.stats()
    assert [sa[k] for k in COUNTERS] == [sb[k] for k in COUNTERS], (t, sa, sb)


class Twin:
    """A (begun large) and B (begun small) on one stream `ws` of `mode`."""
    MODS = {"leased": (lease, L.model_tick), "wait_leased": (wl, WM.model_tick), "rpc": (rpc, RM.model_tick)}

    def __init__(self, mode, ws, a, b, masks=False):
        self.mode, self.ws, self.a, self.b, self.masks, self.t = mode, ws, a, b, masks, 0
        self.mod, self.model = self.MODS[mode]

    def tick(self, ev):
        """The model's tick, then the same tick on both contexts -> the model's record."""
        want = self.model(self.ws, ev)
        got = [self.mod.gpu_tick(c, self.ws, ev, self.masks) for c in (self.a, self.b)]
        for c, g in zip((self.a, self.b), got):
            self.mod.check_tick(self.t, c, self.ws, g, want)
        same_outputs(self.t, self.mode, *got)
        same_state(self.t, self.a, self.b)
        self.t += 1
        return want

    def drive(self, ticks):
        return [self.tick(self.ws.next_tick()) for _ in range(ticks)]

    def refused_on_b(self, ev, match):
        """B refuses `ev` and nothing of it is applied."""
        before = self.b.stream_leases(), self.b.get_running()
        with pytest.raises(binding.YdcError, match=match):
            self.mod.gpu_tick(self.b, self.ws, ev, self.masks)
        for x, y in zip(before[0], self.b.stream_leases()):
            assert np.array_equal(x, y), "a refused tick changed the lease table"
        assert np.array_equal(before[1], self.b.get_running()), "a refused tick changed running_tasks"

    def end(self):
        if self.mode != "leased":  # W itself, one tag per entry, in queue order
            w = self.ws.state.take()
            assert np.array_equal(self.a.stream_waiting_take(), w) and np.array_equal(self.b.stream_waiting_take(), w)
        for c in (self.a, self.b):
            c.stream_end()
            c.close()


def leased_twin(sv, ls, small, large, masks=False):
    """small / large: dicts of tasks, leases, renewals, frees, reports, report_ids."""
    ctxs = []
    for caps in (large, small):
        ctx = new_ctx(sv)
        ctx.stream_begin_leased(ls.es.hb + 8, 16, caps["tasks"], caps["leases"], caps["renewals"], caps["frees"],
                                caps["reports"], caps["report_ids"])
        ctxs.append(ctx)
    return Twin("leased", ls, ctxs[0], ctxs[1], masks)


def requests(ls, n, expires_at, seed, **over):
    """The stream's next tick with hand-made traffic: n ordinary requests, nothing else unless given."""
    ev = ls.next_tick()
    tk = synth.make_tasks(n, ls.es.sv, n_envs=1, seed=seed, self_frac=0.0)
    return lease.quiet(ev, tasks=tk, release_idx=np.empty(0, np.uint32),
                       lease_expires_at=np.broadcast_to(np.asarray(expires_at, np.int64), (n,)).copy(), **over)


def all_granted(want):
    return bool((want["out"] < L.IDX_ENV_NOT_FOUND).all())


def test_leased_rehash_of_a_full_table():
    """max_leases 600 -> 5000: a table of 2048 slots (two tiles of the rehash grid, above the floor of
    1024) is filed again into one of 16384. It holds exactly 600 leases: 90 zombies, 30 renewed
    expiries, and 100 ids freed out of the middle of the id range. One more request is refused and
    changes nothing, the reserve changes nothing that ydc_stream_leases_get shows, the same tick is
    then accepted; afterwards every old live id renews, every old zombie refuses, and a free of each
    old id gives its servant's slot back."""
    sv = roomy_pool(40, 40)
    ls = L.LeaseStream(sv, 300, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 4
    big = dict(tasks=300, leases=5000, renewals=1024, frees=1024, reports=40, report_ids=1024)
    tw = leased_twin(sv, ls, dict(big, leases=600, renewals=64, frees=128), big)
    T = ls.table
    exp0 = np.full(300, 1000, np.int64)
    exp0[:100] = 2  # (overdue from now == 3 on)
    assert all_granted(tw.tick(requests(ls, 300, exp0, 1)))                 # now 0: ids 0 .. 299
    assert all_granted(tw.tick(requests(ls, 300, 1000, 2)))                 # now 1: ids 300 .. 599
    ren = np.concatenate([np.arange(10), np.arange(250, 270)]).astype(np.uint64)
    want = tw.tick(requests(ls, 0, 0, 3, free_ids=np.arange(150, 250, dtype=np.uint64), renew_ids=ren,
                            renew_expires_at=np.full(30, 5000, np.int64)))  # now 2
    assert want["freed"] == 100 and want["renewed"].all() and len(T) == 500
    want = tw.tick(requests(ls, 100, 1000, 4))                              # now 3: ids 600 .. 699, 10 .. 99 overdue
    assert all_granted(want) and want["expired"] == 90 and len(T) == 600 and T.next_id == 700
    assert tw.b.stream_caps()["max_leases"] == 600
    before = tw.b.stream_leases()
    assert len(before[0]) == 600 and before[3].sum() == 90
    # One request more than B has room for.
    ev = requests(ls, 1, 1000, 5)                                           # now 4
    tw.refused_on_b(ev, "max_leases")
    caps = tw.b.stream_reserve(max_leases=5000, max_renewals=1024, max_frees=1024)
    assert caps == tw.a.stream_caps() and caps["max_leases"] == 5000 and caps["max_renewals"] == 1024
    for name, x, y in zip(SNAP, before, tw.b.stream_leases()):
        assert np.array_equal(x, y), "the reserve changed the lease snapshot's %s" % name
    same_state(tw.t, tw.a, tw.b)
    want = tw.tick(ev)  # the very same tick
    assert all_granted(want) and want["task_id"][0] == 700 and want["n_leases"] == 601
    # Every old id: the live ones renew, the zombies refuse; then each is freed.
    old, zombie = before[0], before[3].astype(bool)
    want = tw.tick(requests(ls, 0, 0, 6, renew_ids=old, renew_expires_at=np.full(600, 7000, np.int64)))
    assert np.array_equal(want["renewed"], (~zombie).astype(np.uint8)) and want["renew_refused"] == 90
    run_before = tw.b.get_running().astype(np.int64)
    want = tw.tick(requests(ls, 0, 0, 7, free_ids=old))
    assert want["freed"] == 600 and want["n_leases"] == 1
    assert np.array_equal(run_before - tw.b.get_running(), np.bincount(before[1], minlength=40))
    tw.end()


def test_report_stamps_and_the_tick_number_survive():
    """In tick k every servant reports all of its zombies: they are kept and carry k's number. Reserve.
    In tick k + 1 one servant reports without one of its ids: exactly that zombie is swept, the ones
    it lists again are kept. Two ticks later another servant reports nothing: its zombies, stamped in
    tick k, are swept (a tick number that had started again at 1 would by then equal their stamp)."""
    sv = roomy_pool(6, 8)
    ls = L.LeaseStream(sv, 12, 0, 0, L.LeaseTable(), n_envs=1)
    ls.es.hb = 2
    big = dict(tasks=12, leases=3000, renewals=16, frees=16, reports=6, report_ids=64)
    tw = leased_twin(sv, ls, dict(big, leases=16), big)
    assert all_granted(tw.tick(requests(ls, 12, 0, 1)))  # now 0: ids 0 .. 11, overdue from now == 1 on
    of = {}
    for t, e in sorted(ls.table.L.items()):
        of.setdefault(e[0], []).append(t)
    servants = sorted(of, key=lambda s: -len(of[s]))
    assert len(servants) >= 2 and len(of[servants[0]]) >= 2, of
    sa, sb = servants[0], servants[1]

    def report(lists):
        off = np.cumsum([0] + [len(ids) for _, ids in lists]).astype(np.uint32)
        return dict(report_servants=np.array([s for s, _ in lists], np.uint32), report_off=off,
                    report_ids=np.array([t for _, ids in lists for t in ids], np.uint64))

    want = tw.tick(requests(ls, 0, 0, 2, **report([(s, of[s]) for s in servants])))  # tick k (now 1)
    assert want["expired"] == 12 and want["swept"] == 0 and want["report_unknown"].all()
    tw.b.stream_reserve(max_leases=3000)
    assert tw.b.stream_caps() == tw.a.stream_caps()
    want = tw.tick(requests(ls, 0, 0, 3, **report([(sa, of[sa][1:])])))              # tick k + 1
    assert want["swept"] == 1 and of[sa][0] not in ls.table.L and all(t in ls.table.L for t in of[sa][1:])
    assert tw.b.stats()["leases_swept"] == 1
    assert tw.tick(requests(ls, 0, 0, 4))["swept"] == 0
    want = tw.tick(requests(ls, 0, 0, 5, **report([(sb, [])])))                      # tick k + 3
    assert want["swept"] == len(of[sb]) and not any(t in ls.table.L for t in of[sb])
    tw.end()


def wait_leased_twin(ws, small, large):
    ctxs = []
    for tasks, waiting, leases in (large, small):
        ctx = new_ctx(ws.es.sv)
        ctx.stream_begin_waiting_leased(ws.es.hb + 8, 16, tasks, waiting, leases, 16, 64, ws.es.n, 64)
        ctxs.append(ctx)
    return Twin("wait_leased", ws, ctxs[0], ctxs[1])


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_queue_and_leases_grow_together(stream_graph, monkeypatch):
    """Three servants with few slots. 48 requests with distinct deadlines, tags and lease durations:
    some are granted, the rest wait. 48 more are refused by B (|W| + 48 > 48); max_waiting, max_leases
    and max_tasks grow; a tick before the last tick's clock is still refused; the same 48 are accepted.
    Then leases are freed: the waiters are granted in queue order, their ids go on from next_id and
    their leases run from the granting tick; the others time out at their own deadlines. With the
    captured step and with the step enqueued kernel by kernel (stream_graph=0)."""
    _graph(monkeypatch, stream_graph)
    sv = wcases.small_stream().es.sv
    ws = WM.new_stream(sv, 100, 0, 0, 200, n_envs=1, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    tw = wait_leased_twin(ws, (48, 48, 64), (100, 200, 2000))
    S = ws.state
    k = np.arange(48)
    want = tw.tick(wcases.scripted(ws, ws.next_tick(), n=48, lease_for=20 + 3 * k, wait=4 + k % 7))  # now 0
    granted0 = int((want["out"] < WM.IDX_WAITING).sum())
    assert granted0 >= 8 and want["n_waiting"] >= 8
    ev = wcases.scripted(ws, ws.next_tick(), n=48, lease_for=50 + k, wait=3 + k % 5)                 # now 1
    tw.refused_on_b(ev, "max_waiting")
    caps = tw.b.stream_reserve(max_waiting=200, max_leases=2000, max_tasks=100)
    assert caps == tw.a.stream_caps() and (caps["max_waiting"], caps["max_leases"], caps["max_tasks"]) == (200, 2000, 100)
    same_state(tw.t, tw.a, tw.b)
    with pytest.raises(binding.YdcError, match="before the previous"):
        wl.gpu_tick(tw.b, ws, dict(ev, now=-1))
    want = tw.tick(ev)
    assert want["n_waiting"] > 48
    # Slots come back: the queue's front is granted, ids from next_id on, in queue order.
    first = S.T.next_id
    held = sorted(S.T.L)[:6]
    want = tw.tick(wcases.scripted(ws, ws.next_tick(), n=100, lease_for=9, wait=2, free=held))       # now 2
    gw = want["res_idx"] < WM.IDX_ENV_NOT_FOUND
    assert gw.sum() == 6 and list(want["res_ids"][gw]) == list(range(first, first + 6))
    assert want["w_granted"] == 6 and want["joined"] > 0
    rec = [tw.tick(wcases.scripted(ws, ws.next_tick(), n=0)) for _ in range(9)]                     # now 3 .. 11
    assert sum(r["w_expired"] for r in rec) > 64 and sum(1 for r in rec if r["w_expired"]) >= 5
    assert rec[-1]["n_waiting"] == 0
    tw.end()


def test_rpc_rows_waiting_and_requests_grow():
    """Blocked RPCs with different n_immediate / n_prefetch wait in W. B (8 requests, 509 rows, 16
    waiting) refuses a tick that A takes; max_requests, max_rows and max_waiting grow; rows(W) is what
    it was; the granted counts and the packed grants of the RPCs resolved later equal the twin's."""
    ws = rcases.small_stream(max_rows=3000, max_waiting=64)
    state = ws.state
    ctxs = []
    for req, rows, waiting in ((24, 3000, 64), (8, 509, 16)):
        ctx = new_ctx(ws.es.sv)
        ctx.stream_begin_rpc(ws.es.hb + 8, 16, req, rows, waiting, 4096, 16, 64, ws.es.n, 64)
        ctxs.append(ctx)
    tw = Twin("rpc", ws, ctxs[0], ctxs[1])
    shapes = [(1, 2), (3, 0), (0, 2), (2, 5), (1, 0), (4, 4), (0, 1)]
    want = tw.tick(rcases.scripted(ws, ws.next_tick(), rpcs=[(200, 100, 30, 5)] +
                                   [(a, b, 10 + a, 20 + b) for a, b in shapes]))                      # now 0
    assert want["status"][0] == 0 and want["n_waiting"] == 7 and want["n_waiting_rows"] == sum(a + b for a, b in shapes)
    want = tw.tick(rcases.scripted(ws, ws.next_tick(), rpcs=[(a + 1, b, 12, 20) for a, b in shapes] + [(2, 2, 5, 3)]))
    assert want["n_waiting"] == 15
    rows_w = want["n_waiting_rows"]
    ev = rcases.scripted(ws, ws.next_tick(), rpcs=[(1, 1, 7, 15)] * 8)                                # now 2
    tw.refused_on_b(ev, "max_waiting")
    caps = tw.b.stream_reserve(max_requests=24, max_rows=3000, max_waiting=64)
    assert caps == tw.a.stream_caps() and (caps["max_tasks"], caps["max_rows"], caps["max_waiting"]) == (24, 3000, 64)
    assert state.q.rows() == rows_w
    want = tw.tick(ev)
    assert want["n_waiting"] == 23 and want["n_waiting_rows"] == rows_w + 16  # rows(W) went on from where it was
    # 24 requests in one tick (more than B began with), and slots given back: waiting RPCs are granted.
    held = sorted(state.T.L)[:20]
    want = tw.tick(rcases.scripted(ws, ws.next_tick(), rpcs=[(1, 0, 7, 9)] * 24, free=held))         # now 3
    assert len(want["res_servants"]) == 20 and (want["res_n_granted"] > 1).any() and want["w_granted"] >= 2
    rec = [tw.tick(rcases.scripted(ws, ws.next_tick(), free=sorted(state.T.L)[:4])) for _ in range(4)]
    assert sum(len(r["res_servants"]) for r in rec) == 16
    tw.end()


def test_look_back_arrays_follow_max_tasks():
    """max_tasks 1000 -> 66 000 (65 tiles of 1024: a second look-back window). After the growth a tick
    of 66 000 requests has its only grants behind position 65 536."""
    n = 66_000
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=1, seed=5)
    ls = L.LeaseStream(sv, n, 0, 0, L.LeaseTable(), n_envs=1)
    big = dict(tasks=n, leases=1 << 17, renewals=16, frees=16, reports=ls.n_rep, report_ids=64)
    tw = leased_twin(sv, ls, dict(big, tasks=1000), big)
    assert all_granted(tw.tick(requests(ls, 700, 100, 40)))
    real = np.array([FAR + 1, FAR + 2, FAR + 300, n - 5, n - 2, n - 1])

    def wide(seed):
        tk = {"env_id": np.full(n, 0xFFFF, np.uint32), "min_version": np.zeros(n, np.uint32),
              "requestor_ip": np.zeros(n, np.uint32)}
        some = synth.make_tasks(len(real), ls.es.sv, n_envs=1, seed=seed, self_frac=0.0)
        for k in tk:
            tk[k][real] = some[k]
        return lease.quiet(ls.next_tick(), tasks=tk, lease_expires_at=np.full(n, 100, np.int64))

    ev = wide(41)
    tw.refused_on_b(ev, "capacity")
    assert tw.b.stream_reserve(max_tasks=n) == tw.a.stream_caps()
    want = tw.tick(ev)
    g = want["out"] < L.IDX_ENV_NOT_FOUND
    assert g[real].all() and g.sum() == len(real) and list(want["task_id"][real]) == list(range(700, 700 + len(real)))
    assert all_granted(tw.tick(requests(ls, 700, 100, 42)))
    want = tw.tick(wide(43))
    assert want["task_id"][n - 1] == 1400 + 2 * len(real) - 1
    tw.end()


def seeded_leased_twin(sv, n_envs, tasks, frees, renewals, small_leases, large_leases, masks=False):
    ls = L.LeaseStream(sv, tasks, frees, renewals, L.LeaseTable(), n_envs=n_envs)
    big = dict(tasks=tasks, leases=large_leases, renewals=4096, frees=8192, reports=ls.n_rep, report_ids=1 << 15)
    return leased_twin(sv, ls, dict(big, leases=small_leases), big, masks)


def test_more_than_256_classes_runs_eagerly():
    """~600 servant classes: every tick is enqueued instead of replayed (eager_only); the seeded lease
    traffic of tests/test_stream_lease_gpu.py, grown after four ticks."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=3000, n_envs=n_envs, seed=23)
    tw = seeded_leased_twin(sv, n_envs, 1000, 500, 100, 5000, 1 << 15, masks=True)
    tw.drive(4)
    assert 0 < len(tw.ws.table) <= 4000
    tw.b.stream_reserve(max_leases=1 << 15)
    rec = tw.drive(8)
    assert len(tw.ws.table) + 1000 > 5000 or sum(r["freed"] for r in rec) > 0
    assert sum(r["expired"] for r in rec) and sum(r["swept"] for r in rec)
    tw.end()


def test_remove_servants_after_a_growth():
    """k_lease_remap over the rehashed table: the leases of removed rows vanish, the others follow the
    compaction of the registry, on B as on A."""
    sv = synth.make_servants(80, n_tasks_hint=3000, n_envs=2, seed=11)
    tw = seeded_leased_twin(sv, 2, 500, 300, 80, 2500, 1 << 15)
    ls = tw.ws
    tw.drive(4)
    tw.b.stream_reserve(max_leases=1 << 15)
    tw.drive(4)
    removed = np.array([3, 17, 40], np.uint32)
    assert sum(1 for e in ls.table.L.values() if e[0] in (3, 17, 40)) and sum(1 for e in ls.table.L.values() if e[0] > 40)
    for c in (tw.a, tw.b):
        c.remove_servants(removed)
    lease.drop_rows(ls, removed)
    for c in (tw.a, tw.b):
        for name, x, y in zip(SNAP, c.stream_leases(), ls.table.snapshot()):
            assert np.array_equal(x, y), name
        assert np.array_equal(c.get_running(), ls.es.running.astype(np.uint32))
    tw.drive(6)
    tw.end()


def test_refusals_and_no_ops():
    sv = roomy_pool(6, 8)
    ls = L.LeaseStream(sv, 12, 0, 0, L.LeaseTable(), n_envs=1)
    ctx = new_ctx(sv)
    invalid = "invalid argument"
    # No stream open; a plain stream.
    with pytest.raises(binding.YdcError, match=invalid):
        ctx.stream_reserve(max_tasks=100)
    with pytest.raises(binding.YdcError, match=invalid):
        ctx.stream_caps()
    ctx.stream_begin(8, 8, 12)
    with pytest.raises(binding.YdcError, match=invalid):
        ctx.stream_reserve(max_tasks=100)
    assert ctx.stream_caps() == dict(max_updates=8, max_releases=8, max_tasks=12, max_rows=0, max_waiting=0,
                                     max_leases=0, max_renewals=0, max_frees=0, max_reports=0, max_report_ids=0)
    out = ctx.stream_tick(np.empty(0, np.uint32), np.empty(0, binding.ROW_DTYPE), np.empty(0, np.uint32),
                          synth.make_tasks(4, sv, n_envs=1, seed=1, self_frac=0.0))
    assert len(out) == 4  # (the plain stream is still usable)
    ctx.stream_end()
    ctx.close()
    # A leased stream: fields of another mode, bounds beyond the limits; it goes on afterwards.
    big = dict(tasks=12, leases=64, renewals=16, frees=16, reports=6, report_ids=64)
    tw = leased_twin(sv, ls, big, big)
    tw.tick(requests(ls, 12, 50, 1))
    caps = tw.b.stream_caps()
    assert caps == dict(max_updates=ls.es.hb + 8, max_releases=16, max_tasks=12, max_rows=0, max_waiting=0,
                        max_leases=64, max_renewals=16, max_frees=16, max_reports=6, max_report_ids=64)
    for bad in (dict(max_waiting=10), dict(max_rows=100), dict(max_leases=(1 << 30) + 1),
                dict(max_tasks=0x80000000), dict(max_report_ids=0x80000000)):
        with pytest.raises(binding.YdcError, match=invalid):
            tw.b.stream_reserve(**bad)
        assert tw.b.stream_caps() == caps
    # Smaller or equal: YDC_OK, nothing changes.
    assert tw.b.stream_reserve() == caps
    assert tw.b.stream_reserve(max_leases=64, max_tasks=3, max_renewals=16, max_updates=1) == caps
    tw.tick(requests(ls, 6, 50, 2))
    tw.end()
    # A waiting stream has no lease table; max_rows needs an rpc stream.
    ws = wcases.small_stream()
    ctx = new_ctx(ws.es.sv)
    ctx.stream_begin(8, 8, 12, max_waiting=32)
    for bad in (dict(max_leases=10), dict(max_frees=10), dict(max_rows=10)):
        with pytest.raises(binding.YdcError, match=invalid):
            ctx.stream_reserve(**bad)
    assert ctx.stream_reserve(max_waiting=100, max_tasks=20)["max_waiting"] == 100
    ctx.stream_end()
    ctx.stream_begin_waiting_leased(8, 8, 12, 32, 64, 8, 8, 3, 16)
    with pytest.raises(binding.YdcError, match=invalid):
        ctx.stream_reserve(max_rows=10)
    ctx.stream_end()
    ctx.stream_begin_rpc(8, 8, 8, 64, 16, 64, 8, 8, 3, 16)
    with pytest.raises(binding.YdcError, match=invalid):
        ctx.stream_reserve(max_requests=100)  # (max_rows 64 < max_requests)
    assert ctx.stream_reserve(max_requests=100, max_rows=400)["max_tasks"] == 100
    ctx.stream_end()
    ctx.close()

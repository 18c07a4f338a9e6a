"""One request row per RPC on the device (ydc_stream_begin_rpc / ydc_stream_tick_rpc): every tick
is compared with the model (tests/stream_rpc_model.py, pinned against the verbatim reference by
tests/test_stream_rpc_model.py) on every output: status and count per request, the granted rows'
servants and ids, the resolved list with its packed grants, |W|, rows(W), |L|, running_tasks, the
lease snapshot, the lease counters, and W itself through ydc_stream_waiting_take at the end."""
import os

import numpy as np
import pytest

from tests import stream_rpc_cases as cases
from tests import stream_rpc_model as M
from tests import stream_wait_lease_model as WL
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, pack, streaming, synth

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ref_stream_rpc_cfg5_ticks.npz")
TILE = 1024      # kRpcTile
FAR = 64 * TILE  # the first row a workgroup's first look-back window cannot cover


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def begin(ws, max_requests, max_leases=1 << 16, renewals=4096, frees=8192, report_ids=1 << 17, reports=None, ctx=None):
    if ctx is None:
        ctx = binding.Context(device=0)
        ctx.upload_servants(pack.to_abi_columns(ws.es.sv))
    ctx.stream_begin_rpc(ws.es.hb + 8, 16, max(max_requests, 1), ws.state.max_rows, ws.state.max_waiting,
                         min(max_leases, ws.state.max_leases), renewals, frees, reports or ws.n_rep, report_ids)
    return ctx


def gpu_tick(ctx, ws, ev, masks=False):
    em = ws.es.abi["env_mask"][ev["upd_idx"]] if masks else None
    return ctx.stream_tick_rpc(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["renew_ids"],
                               ev["renew_expires_at"], ev["free_ids"], ev["report_servants"], ev["report_off"],
                               ev["report_ids"], ev["tasks"], ev["n_immediate"], ev["n_prefetch"], ev["lease_for"],
                               ev["deadlines"], ev["tags"], ev["now"], env_masks=em)


def check_state(t, ctx, ws):
    for name, a, b in zip(("ids", "servants", "expires_at", "zombie"), ctx.stream_leases(), ws.table.snapshot()):
        assert np.array_equal(a, b), "tick %d: lease snapshot %s differs" % (t, name)


def check_tick(t, ctx, ws, got, want, snapshot=True):
    for k in ("status", "n_granted", "renewed", "report_unknown", "res_tags", "res_status", "res_n_granted",
              "res_first", "res_servants", "res_task_ids"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, "tick %d: %s has %s entries, the model %s" % (t, k, a.shape, b.shape)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, "tick %d: %s[%d] gpu %s model %s (%d differ)" % (t, k, bad[0], a[bad[0]], b[bad[0]], bad.size)
    n = len(got["status"])
    parts = [streaming.rpc_grants(got, i) for i in range(n)]
    srv = np.concatenate([p[0] for p in parts] or [np.empty(0, np.uint32)])
    ids = np.concatenate([p[1] for p in parts] or [np.empty(0, np.uint64)])
    assert np.array_equal(srv, want["servants"]), "tick %d: the new requests' servants differ" % t
    assert np.array_equal(ids, want["task_ids"]), "tick %d: the new requests' task ids differ" % t
    for j in range(len(got["res_tags"])):  # the views find each entry's grants behind its `first`
        assert len(streaming.rpc_resolved_grants(got, j)[0]) == want["res_n_granted"][j]
    assert (got["n_waiting"], got["n_waiting_rows"], got["n_leases"]) == (
        want["n_waiting"], want["n_waiting_rows"], want["n_leases"]), (t, got["n_waiting"], got["n_waiting_rows"])
    assert np.array_equal(ctx.get_running(), want["running"]), "tick %d: running differs" % t
    st = ctx.stats()
    assert (st["leases_expired"], st["leases_swept"], st["leases_freed"], st["renewals_refused"]) == (
        want["expired"], want["swept"], want["freed"], want["renew_refused"]), (t, st)
    assert st["granted"] == len(want["servants"]) + len(want["res_servants"]), t
    if snapshot:
        check_state(t, ctx, ws)


def drive(ctx, ws, ticks, masks=False, snapshot_every=1, t0=0):
    rec = []
    for t in range(t0, t0 + ticks):
        ev = ws.next_tick()
        want = M.model_tick(ws, ev)
        check_tick(t, ctx, ws, gpu_tick(ctx, ws, ev, masks), want, snapshot=t % snapshot_every == 0)
        rec.append(want)
    return rec


def end(ctx, ws):
    """W itself: one tag per blocked RPC, in queue order."""
    assert np.array_equal(ctx.stream_waiting_take(), ws.state.take())
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_cfg5_stream_against_the_reference(stream_graph, monkeypatch):
    """cfg5's 2000 servants, the fixture's stream, against the model tick by tick and against what
    the VERBATIM reference answered; with the captured step and with stream_graph=0."""
    _graph(monkeypatch, stream_graph)
    fx = np.load(FIXTURE)
    M.check_conditions(fx)
    ws = M.new_stream(M.cfg5_one_slot(), int(fx["rpcs"]), int(fx["frees"]), int(fx["renewals"]),
                      int(fx["max_waiting"]), int(fx["max_rows"]), **BIG)
    ctx = begin(ws, int(fx["rpcs"]))
    rec = drive(ctx, ws, int(fx["ticks"]), snapshot_every=8)
    for k, v in M.digests(rec).items():
        assert np.array_equal(v, fx[k]), k
    end(ctx, ws)


def test_more_than_256_classes_runs_eagerly():
    """~600 servant classes: the step is enqueued instead of replayed (eager_only), through the same
    kernels."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    ws = M.new_stream(sv, 40, 300, 100, 1000, 1 << 14, n_envs=n_envs, **BIG)
    ctx = begin(ws, 40)
    rec = drive(ctx, ws, 26, masks=True)
    assert sum(r["w_granted"] for r in rec) and sum(r["w_expired"] for r in rec) and sum(r["partial"] for r in rec)
    end(ctx, ws)


@pytest.mark.parametrize("case", cases.CASES, ids=[c.__name__ for c in cases.CASES])
def test_hand_written_ticks(case):
    """tests/stream_rpc_cases.py (each pinned against the verbatim class on the CPU)."""
    ws = cases.small_stream()
    ctx = begin(ws, cases.MAX_REQUESTS, 4096, renewals=16, frees=16, report_ids=64, reports=ws.es.n)
    t = [0]

    def tick(ev):
        want = M.model_tick(ws, ev)
        check_tick(t[0], ctx, ws, gpu_tick(ctx, ws, ev), want)
        t[0] += 1
        return want
    cases.play(ws, case(), tick)
    end(ctx, ws)


def test_refusals_leave_everything_untouched():
    """rows == 0 and each capacity bound, at the bound and one above (tests/stream_rpc_cases.py);
    the other tick calls on an rpc context and this one on another."""
    ctxs = {}

    def ctx_of(ws):
        if id(ws) not in ctxs:  # (the stream is kept alive beside its context: ids are not reused)
            ctxs[id(ws)] = (ws, begin(ws, cases.MAX_REQUESTS, 4096, renewals=16, frees=16, report_ids=64,
                                      reports=ws.es.n))
        return ctxs[id(ws)][1]

    def tick(ws, ev):
        want = M.model_tick(ws, ev)
        check_tick(int(ev["now"]), ctx_of(ws), ws, gpu_tick(ctx_of(ws), ws, ev), want)
        return want

    def refused(ws, ev, what):
        pattern = {"rows == 0": "asks for no grant"}.get(what, what)
        with pytest.raises(binding.YdcError, match=pattern):
            gpu_tick(ctx_of(ws), ws, ev)
        check_state(int(ev["now"]), ctx_of(ws), ws)
        assert np.array_equal(ctx_of(ws).get_running(), ws.es.running.astype(np.uint32))
    cases.refusals(tick, refused)
    ws = cases.small_stream()
    ctx = ctx_of(ws)
    ev = cases.scripted(ws, ws.next_tick(), rpcs=[(1, 1, 9, 5)])
    with pytest.raises(binding.YdcError, match="ydc_stream_tick_rpc"):
        ctx.stream_tick(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["tasks"])
    with pytest.raises(binding.YdcError, match="ydc_stream_tick_rpc"):
        ctx.stream_tick_waiting_leased(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["renew_ids"],
                                       ev["renew_expires_at"], ev["free_ids"], ev["report_servants"],
                                       ev["report_off"], ev["report_ids"], ev["tasks"], ev["lease_for"],
                                       ev["deadlines"], ev["tags"], ev["now"])
    check_tick(0, ctx, ws, gpu_tick(ctx, ws, ev), M.model_tick(ws, ev))
    ctx.stream_end()
    ctx.stream_begin_waiting_leased(ws.es.hb + 8, 16, 8, 16, 4096, 16, 16, ws.es.n, 64)
    ctx._max_rows = 64  # (the binding sizes the packed lists by it)
    with pytest.raises(binding.YdcError, match="ydc_stream_begin_rpc"):
        gpu_tick(ctx, ws, cases.scripted(ws, ws.next_tick(), rpcs=[(1, 1, 9, 5)]))
    for _, c in ctxs.values():
        c.stream_end()
        c.close()


def test_with_every_request_one_plus_zero_it_is_a_waiting_leased_context():
    """Every request 1 + 0: answers, ids, the resolved list, W and L equal those of
    ydc_stream_tick_waiting_leased on a twin context fed the same stream."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=9)
    ws = WL.new_stream(sv, 900, 300, 50, 3000, n_envs=2, rate=lambda now: 1.0 if now % 12 < 8 else 0.125)
    twin, ctx = binding.Context(device=0), binding.Context(device=0)
    for c in (twin, ctx):
        c.upload_servants(pack.to_abi_columns(sv))
    twin.stream_begin_waiting_leased(ws.es.hb + 8, 16, 900, 3000, 1 << 14, 4096, 8192, ws.n_rep, 1 << 17)
    ctx.stream_begin_rpc(ws.es.hb + 8, 16, 900, 3901, 3000, 1 << 14, 4096, 8192, ws.n_rep, 1 << 17)
    waited = 0
    for t in range(20):
        ev = ws.next_tick()
        want = WL.model_tick(ws, ev)
        a = twin.stream_tick_waiting_leased(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["renew_ids"],
                                            ev["renew_expires_at"], ev["free_ids"], ev["report_servants"],
                                            ev["report_off"], ev["report_ids"], ev["tasks"], ev["lease_for"],
                                            ev["deadlines"], ev["tags"], ev["now"])
        one = np.ones(len(ev["tags"]), np.uint32)
        b = gpu_tick(ctx, ws, dict(ev, n_immediate=one, n_prefetch=0 * one))
        out, ids, renewed, unknown, n_leases, res_tags, res_idx, res_ids, n_waiting = a
        assert np.array_equal(out, want["out"]), t
        g = out < WL.IDX_WAITING
        assert np.array_equal(np.where(g, 0, out), b["status"]) and np.array_equal(b["n_granted"], g), t
        assert np.array_equal(b["servants"][g], out[g]) and np.array_equal(b["task_ids"][g], ids[g]), t
        gw = res_idx < WL.IDX_ENV_NOT_FOUND
        assert np.array_equal(b["res_tags"], res_tags) and np.array_equal(b["res_status"], np.where(gw, 0, res_idx)), t
        assert np.array_equal(b["res_servants"], res_idx[gw]) and np.array_equal(b["res_task_ids"], res_ids[gw]), t
        assert np.array_equal(renewed, b["renewed"]) and np.array_equal(unknown, b["report_unknown"]), t
        assert (n_leases, n_waiting, n_waiting) == (b["n_leases"], b["n_waiting"], b["n_waiting_rows"]), t
        for x, y in zip(twin.stream_leases(), ctx.stream_leases()):
            assert np.array_equal(x, y), t
        assert np.array_equal(twin.get_running(), ctx.get_running()), t
        waited += int(gw.sum())
    assert waited > 100
    assert np.array_equal(twin.stream_waiting_take(), ctx.stream_waiting_take())
    for c in (twin, ctx):
        c.stream_end()
        c.close()


def _versions_pool():
    """40 idle servants: 20 of version 10, 19 of version 20 and one of version 30 with a single
    slot; max_tasks alone bounds a servant."""
    sv = synth.make_servants(40, n_tasks_hint=6_000, n_envs=1, seed=42)
    sv["version"][:20], sv["version"][20:39], sv["version"][39], sv["max_tasks"][39] = 10, 20, 30, 1
    sv["num_processors"][:], sv["current_load"][:] = 4096, 0
    return sv


def _scripted_stream(sv, max_requests, max_waiting, max_rows, max_leases=1 << 30):
    ws = M.new_stream(sv, max_requests, 0, 0, max_waiting, max_rows, max_leases=max_leases, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    return ws


def _tick(ctx, ws, t, rpcs, min_version, free=(), snapshot=True):
    ev = cases.scripted(ws, ws.next_tick(), rpcs=rpcs, free=free)
    ev["tasks"]["min_version"][:] = min_version
    ev["tags"] = np.arange(t * 1000, t * 1000 + len(rpcs), dtype=np.uint64)
    want = M.model_tick(ws, ev)
    check_tick(t, ctx, ws, gpu_tick(ctx, ws, ev), want, snapshot=snapshot)
    return want


def test_rows_that_straddle_tiles_and_a_table_filled_to_exactly_max_leases():
    """max_rows = 2051 (not a multiple of 4: the tail takes the scalar stores). An RPC of 250 rows,
    one of 10 that straddles the first 256-thread tile, one of 700 whose owner search crosses tiles,
    one behind it that straddles the 1024-row tile; all are granted, and with them the table holds
    exactly max_leases leases. One more row is refused; a freed id makes room for it."""
    sv = _versions_pool()
    n = 250 + 10 + 700 + 90 + 3
    ws = _scripted_stream(sv, 8, 16, 2051, max_leases=n)
    ctx = begin(ws, 8, n, renewals=16, frees=16, report_ids=64, reports=ws.es.n)
    want = _tick(ctx, ws, 0, [(250, 0, 50, 9), (4, 6, 50, 9), (300, 400, 50, 9), (45, 45, 50, 9), (0, 3, 50, 9)], 0)
    assert list(want["n_granted"]) == [250, 10, 700, 90, 3] and want["n_leases"] == n == len(ctx.stream_leases()[0])
    ev = cases.scripted(ws, ws.next_tick(), rpcs=[(1, 0, 50, 9)])
    with pytest.raises(binding.YdcError, match="max_leases"):
        gpu_tick(ctx, ws, ev)
    want = _tick(ctx, ws, 2, [], 0, free=[7])  # (|L| counts as it is before the tick's frees)
    assert want["n_leases"] == n - 1
    want = _tick(ctx, ws, 3, [(1, 0, 50, 9)], 0)
    assert list(want["n_granted"]) == [1] and want["n_leases"] == n
    end(ctx, ws)


@pytest.mark.parametrize("tiles", [64, 65, 129])
def test_lookback_grid_of(tiles):
    """max_rows = (tiles - 1) * 1024 + 515. First W's front is filled with RPCs of 1000 rows for
    version 30, which one servant with a single slot has (the first row takes it, the RPCs wait):
    66 of them for 129 tiles, so that everything after lies behind row 65 536 (second and third
    look-back window), as many as fit for 64 and 65 tiles. Then RPCs of 100 rows for version 20
    take every slot of the newer servants and the rest of them wait behind. Then two ticks free 500
    of those leases and bring RPCs for any version: grants of W's entries behind the front,
    survivors behind them and grants of new requests in one batch."""
    max_rows = (tiles - 1) * TILE + 515
    sv = _versions_pool()
    ws = _scripted_stream(sv, 128, 512, max_rows)
    ctx = begin(ws, 128, 1 << 18, frees=4096, reports=ws.es.n)
    front = min(66, (max_rows - 24_000) // 1000)
    assert front * 1000 >= FAR or tiles < 129
    want = _tick(ctx, ws, 0, [(1, 0, 100, 1000)] + [(500, 500, 100, 1000)] * front, 30, snapshot=False)
    assert want["n_waiting"] == front and want["n_waiting_rows"] == front * 1000
    want = _tick(ctx, ws, 1, [(60, 40, 100, 1000)] * 100, 20)
    assert 10 < want["n_waiting"] - front < 90 and want["partial"] == 1
    for t in (2, 3):
        newer = [i for i, e in ws.table.L.items() if 20 <= e[0] < 39]
        first = ws.table.next_id
        want = _tick(ctx, ws, t, [(5, 5, 100, 1000)] * 100, np.where(np.arange(100) % 4 == 3, 20, 0),
                     free=newer[::max(1, len(newer) // 500)][:500])
        assert want["freed"] == 500 and want["w_granted"] >= 4 and (want["res_first"] < 500).all()
        assert want["n_waiting"] > front + 5 and int((want["n_granted"] > 0).sum()) >= 50
        assert want["task_ids"][0] == first + len(want["res_task_ids"])  # (W's grants come first)
    end(ctx, ws)


class Picky(M.RpcStream):
    """Every 16th request asks for version 30, which one servant with a single slot has."""

    def next_tick(self):
        ev = super().next_tick()
        ev["tasks"]["min_version"][::16] = 30
        return ev


def test_bin_overflow_with_rpc_traffic():
    """The first eager exit (tests/test_stream_wait_lease_gpu.py): the captured step's gated
    k_rpc_grant and k_rpc_settle returned; the host places the batch again with the radix sort and
    the ungated kernels answer. W is non-empty before and after."""
    from tests.test_binsort_gpu import _context, _crowded_bin_pool
    sv = _crowded_bin_pool()
    sv["max_tasks"][48:] = 0
    sv["version"][47], sv["num_processors"][47], sv["max_tasks"][47] = 30, 1, 1
    ws = Picky(sv, 1200, 1000, 200, M.RpcState(3000, 12_000), rate=lambda now: 1.0)
    c = _context(True)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        c.stream_begin_rpc(4096 + 8, 16, 1200, 12_000, 3000, 1 << 15, 4096, 8192, ws.n_rep, 1 << 17)
        drive(c, ws, 4)
        assert c.stats()["radix_passes"] == 0 and len(ws.state.q) > 50  # (so far the bin sort placed the slots)
        ws.rep_pos = 0
        ev = ws.next_tick()
        es = ws.es
        es.sv["max_tasks"][48:96], es.sv["max_tasks"][96:] = 2047, 1
        es.abi = pack.to_abi_columns(es.sv)
        who = np.union1d(ev["upd_idx"], np.arange(48, 4096)).astype(np.uint32)
        rows = np.zeros(len(who), dtype=binding.ROW_DTYPE)
        for k in ("version", "num_processors", "current_load", "max_tasks"):
            rows[k] = es.sv[k][who]
        rows["flags"], rows["ip_id"], rows["env_mask"] = es.abi["flags"][who], es.abi["ip_id"][who], es.abi["env_mask"][who]
        ev = dict(ev, upd_idx=who, upd_rows=rows)
        want = M.model_tick(ws, ev)
        assert want["freed"] and want["n_waiting"] > 50 and len(want["res_tags"]) and len(ev["tags"])
        check_tick(4, c, ws, gpu_tick(c, ws, ev), want)
        assert c.stats()["radix_passes"] >= 1  # (placed again with the radix sort)
        drive(c, ws, 3, t0=5)
        c.stream_end()
    finally:
        c.close()


def test_captured_passes_run_out_with_rpc_traffic():
    """The second eager exit (tests/test_stream_lease_edges_gpu.py: five huge servants): a tick that
    needs more matching passes than were captured. The host finishes the passes and the ungated
    kernels read clock and tick number from the arena in place."""
    from tests.test_stream_lease_edges_gpu import Exits, _huge_servants
    ws = M.new_stream(_huge_servants(), 60_000, 100_000, 2000, 120_000, 300_000, n_envs=3, rate=lambda now: 1.0,
                      report_frac=0.5)
    ctx = begin(ws, 60_000, 1 << 20, frees=1 << 17, report_ids=1 << 19)
    ex, rec, queued = Exits(), [], []
    for t in range(5):
        queued.append(len(ws.state.q))
        ev = ws.next_tick()
        want = M.model_tick(ws, ev)
        check_tick(t, ctx, ws, gpu_tick(ctx, ws, ev), want, snapshot=t % 2 == 0)
        ex.note(t, ctx)
        rec.append(want)
    print("rounds per tick", ex.rounds, "exit taken in ticks", ex.taken, "|W| before", queued)
    busy = [t for t in ex.taken if rec[t]["freed"] and rec[t]["renewed"].sum()]
    assert busy and busy[0] < 4, (ex.rounds, ex.taken, queued)  # (and at least one tick follows it)
    end(ctx, ws)

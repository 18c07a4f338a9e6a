"""Waiting queue and lease table in one streaming context (ydc_stream_begin_waiting_leased /
ydc_stream_tick_waiting_leased): a queued request is granted in a later tick, takes its task id
then (the queue's grants before the new ones) and its lease runs from that tick. Every tick is
compared with the model (tests/stream_wait_lease_model.py, pinned against the verbatim reference by
tests/test_stream_wait_lease_model.py) on every output: answers, ids of both regions, the resolved
list, |W|, |L|, running_tasks (ydc_get_running), the lease snapshot (ydc_stream_leases_get) and the
tick's counts in ydc_get_stats."""
import os

import numpy as np
import pytest

from tests import stream_lease_model as L
from tests import stream_wait_lease_cases as cases
from tests import stream_wait_lease_model as M
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ref_stream_wait_lease_cfg5_ticks.npz")
TILE = 1024      # kWaitTile
FAR = 64 * TILE  # the first position a workgroup's first look-back window cannot cover


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def begin(ws, max_leases, tasks, renewals=4096, frees=8192, report_ids=1 << 17, ctx=None, reports=None):
    if ctx is None:
        ctx = binding.Context(device=0)
        ctx.upload_servants(pack.to_abi_columns(ws.es.sv))
    ctx.stream_begin_waiting_leased(ws.es.hb + 8, 16, max(tasks, 1), ws.state.max_waiting, max_leases, renewals,
                                    frees, reports or ws.n_rep, report_ids)
    return ctx


def gpu_tick(ctx, ws, ev, masks=False):
    em = ws.es.abi["env_mask"][ev["upd_idx"]] if masks else None
    return ctx.stream_tick_waiting_leased(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["renew_ids"],
                                          ev["renew_expires_at"], ev["free_ids"], ev["report_servants"],
                                          ev["report_off"], ev["report_ids"], ev["tasks"], ev["lease_for"],
                                          ev["deadlines"], ev["tags"], ev["now"], env_masks=em)


def check_state(t, ctx, ws):
    for name, a, b in zip(("ids", "servants", "expires_at", "zombie"), ctx.stream_leases(), ws.table.snapshot()):
        assert np.array_equal(a, b), "tick %d: lease snapshot %s differs" % (t, name)


def check_tick(t, ctx, ws, got, want, snapshot=True):
    out, ids, renewed, unknown, n_leases, res_tags, res_idx, res_ids, n_waiting = got
    bad = np.nonzero(out != want["out"])[0]
    assert bad.size == 0, "tick %d: request %d gpu %x model %x (%d differ)" % (
        t, bad[0], out[bad[0]], want["out"][bad[0]], bad.size)
    g = out < M.IDX_WAITING
    assert np.array_equal(ids[g], want["task_id"][g]), "tick %d: the new requests' task ids differ" % t
    assert np.array_equal(res_tags, want["res_tags"]), "tick %d: resolved tags differ" % t
    assert np.array_equal(res_idx, want["res_idx"]), "tick %d: resolved answers differ" % t
    gw = res_idx < M.IDX_ENV_NOT_FOUND
    assert np.array_equal(res_ids[gw], want["res_ids"][gw]), "tick %d: the queue's task ids differ" % t
    assert np.array_equal(renewed, want["renewed"]), "tick %d: out_renewed differs" % t
    assert np.array_equal(unknown, want["report_unknown"]), "tick %d: out_report_unknown differs" % t
    assert (n_waiting, n_leases) == (want["n_waiting"], want["n_leases"]), (t, n_waiting, n_leases)
    assert np.array_equal(ctx.get_running(), want["running"]), "tick %d: running differs" % t
    st = ctx.stats()
    assert (st["leases_expired"], st["leases_swept"], st["leases_freed"], st["renewals_refused"]) == (
        want["expired"], want["swept"], want["freed"], want["renew_refused"]), (t, st)
    assert st["granted"] == int(g.sum()) + int(gw.sum()), t  # (the queue's grants count too)
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


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_cfg5_stream_against_the_reference(stream_graph, monkeypatch):
    """2000 servants (cfg5), the fixture's stream, against the model tick by tick and against what the
    VERBATIM reference answered (tests/golden/ref_stream_wait_lease_cfg5_ticks.npz); with the captured
    step and with the step enqueued kernel by kernel (stream_graph=0)."""
    _graph(monkeypatch, stream_graph)
    fx = np.load(FIXTURE)
    M.check_conditions(fx)
    sv, _ = synth.make_config("cfg5")
    tasks = int(fx["tasks"])
    ws = M.new_stream(sv, tasks, int(fx["frees"]), int(fx["renewals"]), int(fx["max_waiting"]))
    ctx = begin(ws, 1 << 18, tasks)
    rec = drive(ctx, ws, int(fx["ticks"]), snapshot_every=8)
    for k, v in M.digests(rec).items():
        assert np.array_equal(v, fx[k]), k
    ctx.stream_end()
    ctx.close()


def test_more_than_256_classes_runs_eagerly():
    """~600 servant classes: the step is enqueued instead of replayed (eager_only), through the same
    kernels."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    ws = M.new_stream(sv, 3000, 1500, 300, 8000, n_envs=n_envs, rate=lambda now: 1.0 if now % 12 < 8 else 0.125)
    ctx = begin(ws, 1 << 16, 3000)
    rec = drive(ctx, ws, 26, masks=True)
    assert sum(r["w_granted"] for r in rec) and sum(r["w_expired"] for r in rec) and sum(r["swept"] for r in rec)
    ctx.stream_end()
    ctx.close()


def test_wide_registry():
    """70 digests (env_words == 2): heartbeats carry their masks."""
    n_envs = 70
    sv = synth.make_servants(40, n_tasks_hint=2000, n_envs=n_envs, seed=31)
    ws = M.new_stream(sv, 1500, 900, 200, 4000, n_envs=n_envs, rate=lambda now: 1.0 if now % 12 < 8 else 0.125)
    ctx = begin(ws, 1 << 15, 1500)
    rec = drive(ctx, ws, 26, masks=True)
    assert sum(r["w_granted"] for r in rec) and sum(r["w_expired"] for r in rec) and sum(r["expired"] for r in rec)
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("case", cases.CASES, ids=[c.__name__ for c in cases.CASES])
def test_hand_written_ticks(case):
    """tests/stream_wait_lease_cases.py (each pinned against the verbatim class on the CPU)."""
    ws = cases.small_stream()
    ctx = begin(ws, 4096, cases.MAX_TASKS, renewals=16, frees=16, report_ids=64, reports=ws.es.n)
    t = [0]

    def tick(ev):
        want = M.model_tick(ws, ev)
        check_tick(t[0], ctx, ws, gpu_tick(ctx, ws, ev), want)
        t[0] += 1
        return want
    cases.play(ws, case(), tick)
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("tiles", [64, 65, 129, 167])
def test_lookback_grid_of(tiles):
    """max_waiting + max_tasks = (tiles - 1) * 1024 + 515: the last tile is partial and neither the
    batch nor max_waiting is a multiple of 4 long (the new requests' answers take the scalar stores).
    40 idle servants: 20 of version 10, 19 of version 20 and one of version 30 with a single slot.
    First the queue's front is filled with requests for version 30 (the first takes the slot, the
    others stay until their deadline): 72 000 of them for 129 and
    167 tiles, so that everything after lies behind position 65 536 (second and third look-back
    window), as many as fit for 64 and 65 tiles. Then 8 000 requests for version 20 take every slot
    of the newer servants and the rest of them waits behind. Then two ticks that free 500 of those
    leases (the second also 3 000 of the older servants') and bring 8 000 requests for any version: grants of the queue, survivors behind them and
    grants of new requests (on the older servants) in one batch, each id = next_id + the number of
    ALL grants in front."""
    n = (tiles - 1) * TILE + 515
    tasks = 8_000
    mw = n - tasks
    assert (n + TILE - 1) // TILE == tiles and n % 4 == 3 and mw % 4 == 3
    floods = min((FAR + tasks - 1) // tasks, (mw - 2 * tasks) // tasks)
    front = floods * tasks - 1
    assert front >= FAR or tiles < 129
    sv = synth.make_servants(40, n_tasks_hint=6_000, n_envs=1, seed=42)
    sv["version"][:20], sv["version"][20:39], sv["version"][39], sv["max_tasks"][39] = 10, 20, 30, 1
    sv["num_processors"][:], sv["current_load"][:] = 4096, 0  # (max_tasks alone bounds a servant)
    ws = M.new_stream(sv, tasks, 0, 0, mw, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    ctx = begin(ws, 1 << 18, tasks, frees=4096, reports=ws.es.n)

    def tick(t, min_version, free=()):
        ev = cases.scripted(ws, ws.next_tick(), n=tasks, lease_for=100, wait=1000, free=free)
        ev["tasks"]["min_version"][:] = min_version
        ev["tags"] = np.arange(t * tasks, (t + 1) * tasks, dtype=np.uint64)  # (unique over the run)
        before = ws.state.q.tag.copy()
        want = M.model_tick(ws, ev)
        check_tick(t, ctx, ws, gpu_tick(ctx, ws, ev), want, snapshot=t >= floods)
        granted = want["res_tags"][want["res_idx"] < M.IDX_ENV_NOT_FOUND]
        return (want, np.nonzero(np.isin(before, granted))[0], np.nonzero(~np.isin(before, want["res_tags"]))[0],
                mw + np.nonzero(want["out"] < M.IDX_WAITING)[0])

    for t in range(floods):
        want, _, _, _ = tick(t, 30)
        assert want["n_waiting"] == (t + 1) * tasks - 1
    want, _, _, new_grant = tick(floods, 20)
    assert 1000 < len(new_grant) < tasks - 1000 and want["n_waiting"] == front + tasks - len(new_grant)
    for t in (floods + 1, floods + 2):
        newer = [i for i, e in ws.table.L.items() if 20 <= e[0] < 39]
        any_version = np.where(np.arange(tasks) % 4 == 3, 30, 0)  # (every 4th new request stays behind)
        first = ws.table.next_id
        # (none yet in the first of the two ticks; in the second more than its waiters for any version)
        older = [i for i, e in ws.table.L.items() if e[0] < 20][:3000]
        want, q_grant, q_stay, new_grant = tick(t, any_version, free=newer[::max(1, len(newer) // 500)][:500] + older)
        assert want["freed"] == 500 + len(older) and len(q_grant) >= 500
        assert q_grant[0] >= front and q_grant[-1] > front + 400
        assert q_stay[-1] > q_grant[-1] and (q_stay >= front).sum() > 1000
        assert len(new_grant) >= 300 and new_grant[-1] > mw + 300 and new_grant[0] >= mw > q_stay[-1]
        assert want["task_id"][want["out"] < M.IDX_WAITING][0] == first + len(q_grant)  # (the queue's grants come first)
        assert ws.table.next_id == first + len(q_grant) + len(new_grant)
    ctx.stream_end()
    ctx.close()


class Picky(M.WaitLeaseStream):
    """Every 16th request asks for version 30, which one servant with a single slot has: the first
    takes it, the others wait until their deadlines."""

    def next_tick(self):
        ev = super().next_tick()
        ev["tasks"]["min_version"][::16] = 30
        return ev


def test_bin_overflow_with_a_queue_and_lease_traffic():
    """The first eager exit (tests/test_binsort_gpu.py: the leased form): four ordinary ticks on a
    pool whose bins fit, then the heartbeats of tick 4 bring in 4000 servants whose first slots share
    one key. The captured step has applied the tick's renewals, frees, reports and the sweep and
    gathered the batch; its gated k_wait_lease_commit returned; the host places the batch again with
    the radix sort and the ungated kernel answers. W is non-empty before and after."""
    from tests.test_binsort_gpu import _context, _crowded_bin_pool
    sv = _crowded_bin_pool()
    sv["max_tasks"][48:] = 0
    sv["version"][47], sv["num_processors"][47], sv["max_tasks"][47] = 30, 1, 1
    ws = Picky(sv, 3000, 1000, 200, M.WaitLeaseState(6000), rate=lambda now: 1.0)
    c = _context(True)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        c.stream_begin_waiting_leased(4096 + 8, 16, 3000, 6000, 1 << 15, 4096, 8192, ws.n_rep, 1 << 17)
        drive(c, ws, 4)
        assert c.stats()["radix_passes"] == 0 and len(ws.state.q) > 100  # (so far the bin sort placed the slots)
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
        assert len(ev["renew_ids"]) and len(ev["free_ids"]) and len(ev["report_ids"]) and len(ev["tags"])
        want = M.model_tick(ws, ev)
        assert want["freed"] and want["swept"] and want["expired"] and int(want["renewed"].sum())
        assert want["n_waiting"] > 100 and want["w_expired"] and want["joined"]
        check_tick(4, c, ws, gpu_tick(c, ws, ev), want)
        assert c.stats()["radix_passes"] >= 1  # (placed again with the radix sort)
        drive(c, ws, 3, t0=5)
        c.stream_end()
    finally:
        c.close()


def test_captured_passes_run_out_with_a_queue_and_lease_traffic():
    """The second eager exit (tests/test_stream_lease_edges_gpu.py): a tick that needs more matching
    passes than were captured. The host finishes the passes and the ungated kernel reads clock and
    tick number from the arena in place."""
    from tests.test_stream_lease_edges_gpu import Exits, _huge_servants
    ws = M.new_stream(_huge_servants(), 150_000, 100_000, 2000, 300_000, n_envs=3, rate=lambda now: 1.0,
                      report_frac=0.5)
    ctx = begin(ws, 1 << 20, 150_000, frees=1 << 17, report_ids=1 << 19)
    ex, rec, queued = Exits(), [], []
    for t in range(5):
        queued.append(len(ws.state.q))
        ev = ws.next_tick()
        want = M.model_tick(ws, ev)
        check_tick(t, ctx, ws, gpu_tick(ctx, ws, ev), want, snapshot=t % 2 == 0)
        ex.note(t, ctx)
        rec.append(want)
    print("rounds per tick", ex.rounds, "exit taken in ticks", ex.taken, "|W| before", queued)
    busy = [t for t in ex.taken if queued[t] > 1000 and rec[t]["freed"] and rec[t]["renewed"].sum() and rec[t]["w_granted"]]
    assert busy and busy[0] < 4, (ex.rounds, ex.taken, queued)  # (and at least one tick follows it)
    ctx.stream_end()
    ctx.close()


def test_refusals_leave_everything_untouched():
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=9)
    mw, max_leases = 2000, 3100
    ws = M.new_stream(sv, 1000, 200, 50, mw, n_envs=2, max_leases=max_leases,
                      rate=lambda now: 1.0 if now % 12 < 7 else 0.125)
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(ws.es.sv))
    ctx.stream_begin_waiting_leased(ws.es.hb + 8, 16, 2000, mw, max_leases, 64, 512, ws.n_rep, 4096)
    drive(ctx, ws, 7)
    nw, nl = len(ws.state.q), len(ws.table)
    assert nw > 50 and nl > 200
    ev = ws.next_tick()
    n = len(ev["tags"])

    def with_tasks(k, **over):
        tk = synth.make_tasks(k, ws.es.sv, n_envs=2, seed=901)
        return dict(ev, tasks=tk, lease_for=np.full(k, 9, np.int64), deadlines=np.full(k, 99, np.int64),
                    tags=np.zeros(k, np.uint64), **over)
    # |W| + n_tasks > max_waiting
    with pytest.raises(binding.YdcError, match="max_waiting"):
        gpu_tick(ctx, ws, with_tasks(mw - nw + 1))
    # |L| + |W| + n_tasks > max_leases, although |L| + n_tasks and |W| + n_tasks fit
    k = max_leases - nl - nw + 1
    assert 0 < k <= mw - nw and nl + k <= max_leases
    with pytest.raises(binding.YdcError, match="waiting .* max_leases"):
        gpu_tick(ctx, ws, with_tasks(k))
    with pytest.raises(binding.YdcError, match="before the previous"):
        gpu_tick(ctx, ws, dict(ev, now=ev["now"] - 2))
    with pytest.raises(binding.YdcError, match="capacity"):
        gpu_tick(ctx, ws, dict(ev, renew_ids=np.zeros(65, np.uint64), renew_expires_at=np.zeros(65, np.int64)))
    with pytest.raises(binding.YdcError, match="reports twice"):
        gpu_tick(ctx, ws, dict(ev, report_servants=np.array([5, 7, 5], np.uint32),
                               report_off=np.array([0, 0, 0, 0], np.uint32), report_ids=np.empty(0, np.uint64)))
    # the three other tick calls on this context
    with pytest.raises(binding.YdcError, match="ydc_stream_tick_waiting_leased"):
        ctx.stream_tick(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["tasks"])
    with pytest.raises(binding.YdcError, match="ydc_stream_tick_waiting_leased"):
        ctx.stream_tick_waiting(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["tasks"], ev["deadlines"],
                                ev["tags"], ev["now"])
    with pytest.raises(binding.YdcError, match="ydc_stream_tick_waiting_leased"):
        ctx.stream_tick_leased(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["renew_ids"],
                               ev["renew_expires_at"], ev["free_ids"], ev["report_servants"], ev["report_off"],
                               ev["report_ids"], ev["tasks"], ev["now"] + ev["lease_for"], ev["now"])
    # nothing was applied: W, L, next_id and running_tasks are as they were ...
    check_state(7, ctx, ws)
    assert np.array_equal(ctx.get_running(), ws.es.running.astype(np.uint32)) and nl + nw + n <= max_leases
    # ... and the tick itself and the following ones still match the model
    want = M.model_tick(ws, ev)
    check_tick(7, ctx, ws, gpu_tick(ctx, ws, ev), want)
    drive(ctx, ws, 4, t0=8)
    ctx.stream_end()
    # this tick call on the three other kinds of context
    for open_it in (lambda: ctx.stream_begin(ws.es.hb + 8, 16, 2000),
                    lambda: ctx.stream_begin(ws.es.hb + 8, 16, 2000, max_waiting=mw),
                    lambda: ctx.stream_begin_leased(ws.es.hb + 8, 16, 2000, max_leases, 64, 512, ws.n_rep, 4096)):
        open_it()
        ctx._max_waiting = mw  # (the binding sizes the resolved arrays by it)
        with pytest.raises(binding.YdcError, match="ydc_stream_tick"):
            gpu_tick(ctx, ws, ws.next_tick())
        ctx.stream_end()
    ctx.close()


def test_with_every_deadline_passed_it_is_a_leased_context():
    """Deadlines of `now` and W unused: answers, ids and leases equal those of a leased context fed
    lease_expires_at = now + lease_for. Then waiters are taken (ydc_stream_waiting_take) and the
    stream ended: nothing leaks into the next begin."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=9)
    ws = M.new_stream(sv, 400, 200, 50, 3000, n_envs=2, rate=lambda now: 1.0)
    ls = L.LeaseStream(sv, 400, 200, 50, L.LeaseTable(), n_envs=2)
    ctx = begin(ws, 1 << 14, 400)
    other = binding.Context(device=0)
    other.upload_servants(pack.to_abi_columns(sv))
    other.stream_begin_leased(ls.es.hb + 8, 16, 400, 1 << 14, 4096, 8192, ls.n_rep, 1 << 17)
    timeouts = 0
    for t in range(12):
        ev = ls.next_tick()
        want = L.model_tick(ls, ev)
        a = other.stream_tick_leased(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["renew_ids"],
                                     ev["renew_expires_at"], ev["free_ids"], ev["report_servants"],
                                     ev["report_off"], ev["report_ids"], ev["tasks"], ev["lease_expires_at"],
                                     ev["now"])
        n = len(ev["lease_expires_at"])
        ev2 = dict(ev, lease_for=ev["lease_expires_at"] - ev["now"], deadlines=np.full(n, ev["now"], np.int64),
                   tags=np.arange(n, dtype=np.uint64))
        b = gpu_tick(ctx, ws, ev2)
        g = want["out"] < L.IDX_ENV_NOT_FOUND
        assert np.array_equal(a[0], want["out"]) and np.array_equal(b[0], a[0]), t
        assert np.array_equal(a[1][g], b[1][g]) and a[4] == b[4] and len(b[5]) == 0 and b[8] == 0, t
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), t
        for x, y in zip(other.stream_leases(), ctx.stream_leases()):
            assert np.array_equal(x, y), t
        assert np.array_equal(other.get_running(), ctx.get_running()), t
        timeouts += int((want["out"] == L.IDX_TIMEOUT).sum())
    assert timeouts > 100
    other.stream_end()
    other.close()
    # waiters now: one more tick with deadlines ahead
    ev = ls.next_tick()
    n = len(ev["lease_expires_at"])
    b = gpu_tick(ctx, ws, dict(ev, lease_for=ev["lease_expires_at"] - ev["now"],
                               deadlines=np.full(n, ev["now"] + 50, np.int64), tags=np.arange(100, 100 + n, dtype=np.uint64)))
    waiting = 100 + np.nonzero(b[0] == M.IDX_WAITING)[0]
    assert len(waiting) > 20 and b[8] == len(waiting)
    assert np.array_equal(ctx.stream_waiting_take(), waiting.astype(np.uint64))
    assert len(ctx.stream_waiting_take()) == 0
    ctx.stream_end()
    # a new stream on the same context starts empty: ids from 0, no lease, no waiter
    ws2 = cases.small_stream()
    ctx.upload_servants(pack.to_abi_columns(ws2.es.sv))
    begin(ws2, 4096, cases.MAX_TASKS, renewals=16, frees=16, report_ids=64, ctx=ctx, reports=ws2.es.n)
    assert all(len(c) == 0 for c in ctx.stream_leases())
    t = [0]

    def tick(ev):
        want = M.model_tick(ws2, ev)
        check_tick(t[0], ctx, ws2, gpu_tick(ctx, ws2, ev), want)
        t[0] += 1
        return want
    cases.play(ws2, cases.a_freed_id_lets_a_waiter_in(), tick)
    ctx.stream_end()
    ctx.close()


def test_remove_servants_with_waiters_and_leases_on_the_removed_rows():
    """Servants 3, 17 and 40 leave while W is non-empty and leases are open on them and on later rows:
    their leases vanish, the others follow the compaction, W is untouched and goes on being tried."""
    from tests.test_stream_lease_gpu import drop_rows
    sv = synth.make_servants(80, n_tasks_hint=3000, n_envs=2, seed=11)
    ws = M.new_stream(sv, 1500, 300, 80, 6000, n_envs=2, rate=lambda now: 1.0 if now % 12 < 9 else 0.125)
    ctx = begin(ws, 1 << 15, 1500)
    drive(ctx, ws, 8)
    removed = np.array([3, 17, 40], np.uint32)
    assert sum(1 for e in ws.table.L.values() if e[0] in (3, 17, 40)) and len(ws.state.q) > 20
    assert sum(1 for e in ws.table.L.values() if e[0] > 40)
    ctx.remove_servants(removed)
    drop_rows(ws, removed)
    check_state(8, ctx, ws)
    assert np.array_equal(ctx.get_running(), ws.es.running.astype(np.uint32))
    rec = drive(ctx, ws, 10, t0=8)
    assert sum(r["w_granted"] for r in rec)
    ctx.stream_end()
    ctx.close()

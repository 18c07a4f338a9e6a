"""Streaming leased mode (ydc_stream_begin_leased / ydc_stream_tick_leased): the device remembers
every grant (task id, servant, expiry, zombie flag) and applies renewals, frees by id, expiry and
servant reports inside the tick. Every tick is compared with the model (tests/stream_lease_model.py,
pinned against the verbatim reference by tests/test_stream_lease_model.py) on every output, on
running_tasks (ydc_get_running), on the lease snapshot (ydc_stream_leases_get) and on the tick's
counts in ydc_get_stats."""
import os

import numpy as np
import pytest

from tests import stream_lease_model as M
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ref_stream_lease_cfg5_ticks.npz")


def begin(ls, max_leases, tasks, renewals=4096, frees=8192, report_ids=1 << 17):
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(ls.es.sv))
    ctx.stream_begin_leased(ls.es.hb + 8, 16, max(tasks, 1), max_leases, renewals, frees, ls.n_rep, report_ids)
    return ctx


def gpu_tick(ctx, ls, ev, masks=False):
    em = ls.es.abi["env_mask"][ev["upd_idx"]] if masks else None
    return ctx.stream_tick_leased(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["renew_ids"],
                                  ev["renew_expires_at"], ev["free_ids"], ev["report_servants"],
                                  ev["report_off"], ev["report_ids"], ev["tasks"], ev["lease_expires_at"],
                                  ev["now"], env_masks=em)


def check_tick(t, ctx, ls, got, want, snapshot=True):
    out, ids, renewed, unknown, n_leases = got
    bad = np.nonzero(out != want["out"])[0]
    assert bad.size == 0, "tick %d: request %d gpu %x model %x (%d differ)" % (
        t, bad[0], out[bad[0]], want["out"][bad[0]], bad.size)
    g = out < M.IDX_ENV_NOT_FOUND
    assert np.array_equal(ids[g], want["task_id"][g]), "tick %d: task ids differ" % t
    assert np.array_equal(renewed, want["renewed"]), "tick %d: out_renewed differs" % t
    assert np.array_equal(unknown, want["report_unknown"]), "tick %d: out_report_unknown differs" % t
    assert n_leases == want["n_leases"], (t, n_leases, want["n_leases"])
    assert np.array_equal(ctx.get_running(), want["running"]), "tick %d: running differs" % t
    st = ctx.stats()
    assert (st["leases_expired"], st["leases_swept"], st["leases_freed"], st["renewals_refused"]) == (
        want["expired"], want["swept"], want["freed"], want["renew_refused"]), (t, st)
    assert st["granted"] == int(g.sum()), t
    if snapshot:
        for name, a, b in zip(("ids", "servants", "expires_at", "zombie"), ctx.stream_leases(), ls.table.snapshot()):
            assert np.array_equal(a, b), "tick %d: lease snapshot %s differs" % (t, name)


def drive(ctx, ls, ticks, masks=False, snapshot_every=1, t0=0):
    rec = []
    for t in range(t0, t0 + ticks):
        ev = ls.next_tick()
        want = M.model_tick(ls, ev)
        got = gpu_tick(ctx, ls, ev, masks)
        check_tick(t, ctx, ls, got, want, snapshot=t % snapshot_every == 0)
        rec.append(want)
    return rec


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_leased_cfg5_stream_against_the_reference(stream_graph, monkeypatch):
    """2000 servants (cfg5), the fixture's stream, against the model tick by tick and against what
    the VERBATIM reference answered (tests/golden/ref_stream_lease_cfg5_ticks.npz); with the captured
    step and with the step enqueued kernel by kernel (stream_graph=0)."""
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)
    fx = np.load(FIXTURE)
    M.check_conditions(fx)
    sv, _ = synth.make_config("cfg5")
    tasks = int(fx["tasks"])
    ls = M.LeaseStream(sv, tasks, int(fx["frees"]), int(fx["renewals"]), M.LeaseTable())
    ctx = begin(ls, 1 << 18, tasks)
    rec = drive(ctx, ls, int(fx["ticks"]), snapshot_every=8)
    for k, v in M.digests(rec).items():
        assert np.array_equal(v, fx[k]), k
    ctx.stream_end()
    ctx.close()


def test_leased_more_than_256_classes_runs_eagerly():
    """~600 servant classes: the step is enqueued instead of replayed (eager_only), through the
    same lease kernels."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    ls = M.LeaseStream(sv, 3000, 1500, 300, M.LeaseTable(), n_envs=n_envs)
    ctx = begin(ls, 1 << 16, 3000)
    rec = drive(ctx, ls, 14, masks=True)
    assert sum(r["expired"] for r in rec) and sum(r["swept"] for r in rec)
    ctx.stream_end()
    ctx.close()


def test_leased_wide_registry():
    """70 digests (env_words == 2): heartbeats carry their masks."""
    n_envs = 70
    sv = synth.make_servants(40, n_tasks_hint=2000, n_envs=n_envs, seed=31)
    ls = M.LeaseStream(sv, 1500, 900, 200, M.LeaseTable(), n_envs=n_envs)
    ctx = begin(ls, 1 << 15, 1500)
    rec = drive(ctx, ls, 20, masks=True)
    assert sum(r["expired"] for r in rec) and sum(r["swept"] for r in rec) and sum(r["timeouts"] for r in rec)
    ctx.stream_end()
    ctx.close()


def quiet(ev, **over):
    """The tick's heartbeats and requests with hand-made lease traffic."""
    e = dict(ev)
    e.update(renew_ids=np.empty(0, np.uint64), renew_expires_at=np.empty(0, np.int64),
             free_ids=np.empty(0, np.uint64), report_servants=np.empty(0, np.uint32),
             report_off=np.zeros(1, np.uint32), report_ids=np.empty(0, np.uint64))
    e.update(over)
    return e


def test_leased_long_lived_lease_is_found_past_its_home_slot():
    """max_leases 512: a table of 1024 slots, up to 40 % full. Leases 0 and 1024 live on while more
    than 1024 younger ids come and go (every tick's frees look the previous tick's grants up); the
    two are then renewed, reported, and freed by id. Written for the home slot id & (cap - 1), under
    which 0 and 1024 collide; under the multiplicative home they do not, and a replay of the rule
    (tests/lease_table_cases.py: replay_consecutive) files 1598 of these 1600 ids at their home slot
    and 2 one slot behind it: this is a long-lived pair among short-lived neighbours, not a probe
    past the home slot. Chains, holes inside them and the wrap: tests/test_lease_table_gpu.py."""
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=5)
    ls = M.LeaseStream(sv, 200, 0, 0, M.LeaseTable(512), n_envs=2)
    ctx = begin(ls, 512, 200)
    T = ls.table
    prev = np.empty(0, np.uint64)
    for t in range(8):
        ev = quiet(ls.next_tick(), free_ids=prev)
        ev["lease_expires_at"][:] = 1000
        want = M.model_tick(ls, ev)
        check_tick(t, ctx, ls, gpu_tick(ctx, ls, ev), want)
        g = want["out"] < M.IDX_ENV_NOT_FOUND
        prev = want["task_id"][g]
        prev = prev[(prev != 0) & (prev != 1024)]  # leases 0 and 1024 stay
    assert T.next_id > 1100 and 0 in T.L and 1024 in T.L
    for t, over in enumerate([
            dict(renew_ids=np.array([1024, 0, 1024], np.uint64), renew_expires_at=np.array([7, 2000, 8], np.int64)),
            dict(report_servants=np.array([T.L[0][0]], np.uint32), report_off=np.array([0, 2], np.uint32),
                 report_ids=np.array([0, 1024], np.uint64)),
            dict(free_ids=np.array([1024, 0, 1024], np.uint64))], 8):
        ev = ls.next_tick()
        ev = quiet(ev, tasks={k: v[:0] for k, v in ev["tasks"].items()}, lease_expires_at=np.empty(0, np.int64), **over)
        want = M.model_tick(ls, ev)
        check_tick(t, ctx, ls, gpu_tick(ctx, ls, ev), want)
    assert 0 not in T.L and 1024 not in T.L
    ctx.stream_end()
    ctx.close()


def drop_rows(ls, removed):
    """The stream's own registry after ydc_remove_servants(removed)."""
    es = ls.es
    keep = np.ones(es.n, bool)
    keep[removed] = False
    es.sv = {k: v[keep] for k, v in es.sv.items()}
    es.abi = {k: (v[keep] if isinstance(v, np.ndarray) and len(v) == es.n else v) for k, v in es.abi.items()}
    es.foreign, es.running = es.foreign[keep], es.running[keep]
    es.n = int(keep.sum())
    es.hb_pos %= es.n
    ls.rep_pos %= es.n
    ls.table.remove_servants(removed)


def test_leased_remove_servants_mid_stream():
    """Servants 3, 17 and 40 expire while leases are open on them and on later rows: their leases
    vanish, the others follow the compaction; frees, reports and sweeps go on with the new rows."""
    sv = synth.make_servants(80, n_tasks_hint=3000, n_envs=2, seed=11)
    ls = M.LeaseStream(sv, 500, 300, 80, M.LeaseTable(), n_envs=2)
    ctx = begin(ls, 1 << 15, 500)
    drive(ctx, ls, 8)
    removed = np.array([3, 17, 40], np.uint32)
    on_removed = sum(1 for e in ls.table.L.values() if e[0] in (3, 17, 40))
    later = sum(1 for e in ls.table.L.values() if e[0] > 40)
    assert on_removed and later
    ctx.remove_servants(removed)
    drop_rows(ls, removed)
    for name, a, b in zip(("ids", "servants", "expires_at", "zombie"), ctx.stream_leases(), ls.table.snapshot()):
        assert np.array_equal(a, b), name
    assert np.array_equal(ctx.get_running(), ls.es.running.astype(np.uint32))
    drive(ctx, ls, 10, t0=8)
    ctx.stream_end()
    ctx.close()


def test_leased_refusals_leave_everything_untouched():
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=9)
    ls = M.LeaseStream(sv, 400, 200, 50, M.LeaseTable(3000), n_envs=2)
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(ls.es.sv))
    ctx.stream_begin_leased(ls.es.hb + 8, 16, 3000, 3000, 64, 512, ls.n_rep, 4096)
    drive(ctx, ls, 6)
    ev = ls.next_tick()
    none = quiet(ev)
    # |L| + n_tasks > max_leases
    room = 3000 - len(ls.table)
    many = synth.make_tasks(room + 1, ls.es.sv, n_envs=2, seed=901)
    with pytest.raises(binding.YdcError, match="max_leases"):
        gpu_tick(ctx, ls, dict(none, tasks=many, lease_expires_at=np.full(room + 1, 99, np.int64)))
    # the clock goes backwards
    with pytest.raises(binding.YdcError, match="before the previous"):
        gpu_tick(ctx, ls, dict(ev, now=ev["now"] - 2))
    # counts above the capacities given at begin
    with pytest.raises(binding.YdcError, match="capacity"):
        gpu_tick(ctx, ls, quiet(ev, renew_ids=np.zeros(65, np.uint64), renew_expires_at=np.zeros(65, np.int64)))
    with pytest.raises(binding.YdcError, match="capacity"):
        gpu_tick(ctx, ls, quiet(ev, free_ids=np.zeros(513, np.uint64)))
    with pytest.raises(binding.YdcError, match="max_report_ids"):
        gpu_tick(ctx, ls, quiet(ev, report_servants=np.array([0], np.uint32), report_off=np.array([0, 4097], np.uint32),
                                report_ids=np.zeros(4097, np.uint64)))
    # a servant twice in one tick's reports
    with pytest.raises(binding.YdcError, match="reports twice"):
        gpu_tick(ctx, ls, quiet(ev, report_servants=np.array([5, 7, 5], np.uint32),
                                report_off=np.array([0, 0, 0, 0], np.uint32)))
    # the other tick calls on a leased context
    with pytest.raises(binding.YdcError, match="ydc_stream_tick_leased"):
        ctx.stream_tick(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["tasks"])
    with pytest.raises(binding.YdcError, match="ydc_stream_tick_leased"):
        n = len(ev["tasks"]["env_id"])
        ctx.stream_tick_waiting(ev["upd_idx"], ev["upd_rows"], ev["release_idx"], ev["tasks"],
                                np.zeros(n, np.int64), np.zeros(n, np.uint64), ev["now"])
    # nothing was applied: the tick itself and the following ones still match the model
    want = M.model_tick(ls, ev)
    check_tick(6, ctx, ls, gpu_tick(ctx, ls, ev), want)
    drive(ctx, ls, 4, t0=7)
    ctx.stream_end()
    # ... and the leased tick on a plain context
    ctx.stream_begin(ls.es.hb + 8, 16, 400)
    with pytest.raises(binding.YdcError, match="without a lease table"):
        gpu_tick(ctx, ls, quiet(ls.next_tick()))
    ctx.stream_end()
    ctx.close()

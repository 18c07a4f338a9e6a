"""Streaming waiting mode (ydc_stream_begin_waiting / ydc_stream_tick_waiting): requests that find
no free servant wait in a queue on the device and are tried again at the start of every later
tick until granted, EnvironmentNotFound or past their deadline. Every tick is compared with the
model (tests/stream_wait_model.py, pinned against the verbatim reference by
tests/test_stream_wait_model.py): the new requests' answers, the resolved list (content and
order), the queue's size, running_tasks and the grant count."""
import os

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import stream_wait_model as M
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu


def begin(es, max_waiting, frees, tasks):
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(es.sv))
    ctx.stream_begin(es.hb + 8, max(frees, 1), tasks, max_waiting=max_waiting)
    return ctx


def check_tick(t, ctx, ws, q, tick, got, want):
    now, who, rows, rel, tk, dl, tags = tick
    out, rt, ri, nw = got
    wout, wrt, wri, wnw, batch = want
    bad = np.nonzero(out != wout)[0]
    assert bad.size == 0, "tick %d: request %d gpu %x model %x (%d differ)" % (
        t, bad[0], out[bad[0]], wout[bad[0]], bad.size)
    assert np.array_equal(rt, wrt), "tick %d: resolved tags differ (%d vs %d)" % (t, len(rt), len(wrt))
    assert np.array_equal(ri, wri), "tick %d: resolved answers differ" % t
    assert nw == wnw, (t, nw, wnw)
    # a new request whose deadline has passed is never queued
    assert not ((out == M.IDX_WAITING) & (dl <= now)).any(), t
    ws.commit(out, ri, nw)
    assert np.array_equal(ctx.get_running(), ws.es.running.astype(np.uint32)), "tick %d: running differs" % t
    assert ctx.stats()["granted"] == int((batch < M.IDX_ENV_NOT_FOUND).sum()), t


def drive(ctx, ws, q, ticks, masks=False, before=None):
    for t in range(ticks):
        tick = ws.next_tick()
        now, who, rows, rel, tk, dl, tags = tick
        if before:
            tick = before(t, tick)
            now, who, rows, rel, tk, dl, tags = tick
        want = q.tick(M.oracle_place(ws.es), tk, dl, tags, now)
        em = ws.es.abi["env_mask"][who] if masks else None
        got = ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, now, env_masks=em)
        check_tick(t, ctx, ws, q, tick, got, want)


def saturated(max_waiting=12_000, seed=42):
    sv = synth.make_servants(150, n_tasks_hint=4000 * 6, n_envs=2, seed=seed)
    ws = M.WaitingStream(sv, 4000, 500, max_waiting, n_envs=2)
    return ws, M.WaitQueue(max_waiting)


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_saturated_pool(stream_graph, monkeypatch):
    """150 servants, 4000 requests and 500 frees per tick, 2 digests, deadlines now + {0, 1, 2, 5,
    40}: the queue fills to its bound and is served in arrival order as slots come free; with the
    captured step and with the step enqueued kernel by kernel (stream_graph=0)."""
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    ws, q = saturated()
    ctx = begin(ws.es, 12_000, 500, 4000)
    drive(ctx, ws, q, 32)
    assert ws.n_waiting > 5000
    ctx.stream_end()
    ctx.close()


def test_waiting_cfg5_shape_against_the_reference():
    """2000 servants (cfg5), 10k requests per tick, max_waiting 20k, 60 ticks, against what the
    VERBATIM reference answered on the same stream (tests/golden/ref_stream_wait_cfg5_60_ticks.npz,
    generator tests/golden/make_stream_wait_golden.py)."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_stream_wait_cfg5_60_ticks.npz"))
    sv, _ = synth.make_config("cfg5")
    mw = int(fx["max_waiting"])
    ws = M.WaitingStream(sv, int(fx["tasks"]), int(fx["frees"]), mw)
    ctx = begin(ws.es, mw, int(fx["frees"]), int(fx["tasks"]))
    for t in range(int(fx["ticks"])):
        now, who, rows, rel, tk, dl, tags = ws.next_tick()
        out, rt, ri, nw = ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, now)
        assert synth.placement_hash(out) == int(fx["digest"][t]), "tick %d: answers differ" % t
        assert len(rt) == int(fx["n_resolved"][t]), t
        assert M.hash_u64(rt) == int(fx["res_tag_digest"][t]), "tick %d: resolved tags differ" % t
        assert synth.placement_hash(ri) == int(fx["res_idx_digest"][t]), "tick %d: resolved answers differ" % t
        assert nw == int(fx["n_waiting"][t]), t
        ws.commit(out, ri, nw)
        if t % 10 == 9 or t > 24:
            assert synth.placement_hash(ctx.get_running()) == int(fx["run_digest"][t]), t
    ctx.stream_end()
    ctx.close()


def test_waiting_more_than_256_classes_runs_eagerly():
    """~600 servant classes: the step is enqueued instead of replayed (eager_only) — the same
    gather and compaction kernels around the batch."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    ws = M.WaitingStream(sv, 3000, 300, 9000, n_envs=n_envs)
    q = M.WaitQueue(9000)
    ctx = begin(ws.es, 9000, 300, 3000)
    drive(ctx, ws, q, 12, masks=True)
    assert ctx.stats()["n_classes"] > 256 and ws.n_waiting > 0
    ctx.stream_end()
    ctx.close()


def test_waiting_wide_registry_digest_removed_mid_stream():
    """A registry with 70 digests (two mask words, <= 256 classes: captured). At tick 12 every
    servant that advertises the digest most of the queue waits for drops it in one structural
    heartbeat: the step is captured again and those waiting entries resolve EnvironmentNotFound."""
    n_envs = 70
    sv = synth.make_servants(40, n_tasks_hint=2000, n_envs=n_envs, seed=31)
    ws = M.WaitingStream(sv, 1500, 60, 6000, n_envs=n_envs)
    q = M.WaitQueue(6000)
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(ws.es.sv))
    ctx.stream_begin(ws.es.n + 8, 60, 1500, max_waiting=6000)  # (room for every servant's heartbeat)
    dropped = {}

    def before(t, tick):
        if t != 12:
            return tick
        now, who, rows, rel, tk, dl, tags = tick
        es = ws.es
        d = int(np.bincount(q.cols["env_id"], minlength=n_envs).argmax())
        has = (es.sv["env_mask"][:, d // 64] >> np.uint64(d % 64)) & np.uint64(1)
        idx = np.nonzero(has)[0].astype(np.uint32)
        es.sv["env_mask"][idx, d // 64] &= ~(np.uint64(1) << np.uint64(d % 64))
        es.abi = pack.to_abi_columns(es.sv)
        who2 = np.union1d(who, idx).astype(np.uint32)
        rows2 = np.zeros(len(who2), dtype=binding.ROW_DTYPE)
        for k in ("version", "num_processors", "current_load", "max_tasks"):
            rows2[k] = es.sv[k][who2]
        rows2["flags"], rows2["ip_id"] = es.abi["flags"][who2], es.abi["ip_id"][who2]
        dropped["digest"], dropped["waiting"] = d, int((q.cols["env_id"] == d).sum())
        return now, who2, rows2, rel, tk, dl, tags

    drive(ctx, ws, q, 20, masks=True, before=before)
    assert ctx.stats()["n_classes"] <= 256
    assert dropped["waiting"] > 0
    ctx.stream_end()
    ctx.close()


def test_waiting_refusals_apply_nothing():
    """|W| + n > max_waiting is YDC_ERR_CAPACITY, `now` before the previous tick's and a plain tick
    on a waiting context are YDC_ERR_INVALID_ARGUMENT — and none of them applies anything: the tick
    sent again correctly still matches the model (its frees were not applied twice)."""
    ws, q = saturated(max_waiting=9000, seed=43)
    ctx = begin(ws.es, 9000, 500, 4000)
    drive(ctx, ws, q, 10)
    assert ws.n_waiting > 5000
    for t in range(10, 16):
        tick = ws.next_tick()
        now, who, rows, rel, tk, dl, tags = tick
        room = 9000 - ws.n_waiting
        more = synth.make_tasks(room + 1, ws.es.sv, n_envs=2, seed=900 + t)
        with pytest.raises(binding.YdcError, match="CAPACITY|capacity"):
            ctx.stream_tick_waiting(who, rows, rel, more, np.full(room + 1, now + 5, np.int64),
                                    np.arange(room + 1, dtype=np.uint64), now)
        with pytest.raises(binding.YdcError, match="before the previous"):
            ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, now - 2)  # (the previous tick's: now - 1)
        with pytest.raises(binding.YdcError, match="ydc_stream_tick_waiting"):
            ctx.stream_tick(who, rows, rel, tk)
        want = q.tick(M.oracle_place(ws.es), tk, dl, tags, now)
        got = ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, now)
        check_tick(t, ctx, ws, q, tick, got, want)
    ctx.stream_end()
    ctx.close()


def test_waiting_with_every_deadline_passed_is_a_plain_tick():
    """deadline == now for every request: nothing ever waits, and the answers are exactly those of
    a plain streaming context fed the same stream."""
    ws, _ = saturated(seed=44)
    ws2, _ = saturated(seed=44)
    ctx = begin(ws.es, 4000, 500, 4000)
    plain = binding.Context(device=0)
    plain.upload_servants(pack.to_abi_columns(ws2.es.sv))
    plain.stream_begin(ws2.es.hb + 8, 500, 4000)
    timeouts = 0
    for t in range(12):
        now, who, rows, rel, tk, dl, tags = ws.next_tick()
        _, who2, rows2, rel2, tk2, _, _ = ws2.next_tick()
        out, rt, ri, nw = ctx.stream_tick_waiting(who, rows, rel, tk, np.full(len(dl), now, np.int64), tags, now)
        want = plain.stream_tick(who2, rows2, rel2, tk2)
        assert np.array_equal(out, want) and len(rt) == 0 and nw == 0, t
        g = ctx.stats()["granted"]
        assert g == plain.stats()["granted"] == int((want < O.IDX_ENV_NOT_FOUND).sum())
        timeouts += int((want == O.IDX_TIMEOUT).sum())
        ws.commit(out, ri, nw)
        ws2.es.commit(want)
        assert np.array_equal(ctx.get_running(), plain.get_running())
    assert timeouts > 0
    for c in (ctx, plain):
        c.stream_end()
        c.close()


def test_waiting_take_hands_over_the_queue():
    """stream_waiting_take returns the queue's tags in arrival order and leaves it empty; the
    following ticks go on from an empty queue."""
    ws, q = saturated(seed=45)
    ctx = begin(ws.es, 12_000, 500, 4000)
    drive(ctx, ws, q, 12)
    assert ws.n_waiting > 0
    taken = ctx.stream_waiting_take()
    assert np.array_equal(taken, q.take())
    assert np.all(np.diff(taken.astype(np.int64)) > 0)  # (tags are issued in arrival order)
    ws.n_waiting = 0
    assert len(ctx.stream_waiting_take()) == 0
    drive(ctx, ws, q, 4)
    ctx.stream_end()
    ctx.close()

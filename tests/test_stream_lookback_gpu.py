"""k_wait_compact and k_lease_grant rank their positions with a decoupled look-back over tiles of
1024: wave 0 of a workgroup reads 64 predecessor words at a time and steps back until it meets an
inclusive prefix. These tests give the two kernels grids of more than 64 and more than 128 tiles,
so that a second and a third window exist, with work (survivors, resolved entries, grants) behind
position 65 536, and grids of exactly 64, 65, 128 and 129 tiles whose last tile is partial and
whose size is no multiple of 4. Every tick is compared with the model (tests/stream_wait_model.py,
tests/stream_lease_model.py); each test asserts on the model's side that its stream reached the
positions it is about."""
import numpy as np
import pytest

from tests import stream_lease_model as L
from tests import stream_wait_model as W
from tests import test_stream_lease_gpu as lease
from tests import test_stream_waiting_gpu as waiting
from yadcc_amd import synth

pytestmark = pytest.mark.gpu
TILE = 1024  # kWaitTile, kLeaseTile
FAR = 64 * TILE  # the first position a workgroup's first look-back window cannot cover


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def wait_facts(sv, tasks, frees, max_waiting, ticks, n_envs):
    """The model alone over the stream the GPU is about to get: per tick |W| before the tick, the
    highest queue position resolved, the highest surviving, the survivors' count (queue and new),
    and whether the last new request joined the queue."""
    ws = W.WaitingStream(sv, tasks, frees, max_waiting, n_envs=n_envs)
    q = W.WaitQueue(max_waiting)
    facts = []
    for _ in range(ticks):
        now, who, rows, rel, tk, dl, tags = ws.next_tick()
        before = q.tag.copy()
        out, rt, ri, nw, _ = q.tick(W.oracle_place(ws.es), tk, dl, tags, now)
        ws.commit(out, ri, nw)
        res = np.nonzero(np.isin(before, rt))[0]
        stay = np.nonzero(~np.isin(before, rt))[0]
        facts.append(dict(w=len(before), n=len(out), hi_resolved=int(res[-1]) if len(res) else -1,
                          hi_survivor=int(stay[-1]) if len(stay) else -1, n_resolved=len(rt), n_waiting=nw,
                          last_joined=bool(len(out) and out[-1] == W.IDX_WAITING),
                          first_resolved=bool(len(res) and res[0] == 0)))
    return facts


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_queue_beyond_65536_entries(stream_graph, monkeypatch):
    """150 servants, 30 000 requests and 1 500 frees per tick, max_waiting 140 000: a batch of
    170 000 positions, 167 tiles, three look-back windows. The queue itself grows past 65 536
    entries, so survivors and resolved entries sit behind the first window and the survivors'
    count needs more than 16 of the packed pair's 31 bits."""
    _graph(monkeypatch, stream_graph)
    mw, tasks, frees, ticks = 140_000, 30_000, 1_500, 16
    sv = synth.make_servants(150, n_tasks_hint=24_000, n_envs=2, seed=42)
    facts = wait_facts(sv, tasks, frees, mw, ticks, 2)
    deep = [f for f in facts if f["w"] > FAR]
    assert len(deep) >= 4, [f["w"] for f in facts]
    assert all(f["hi_resolved"] >= FAR and f["hi_survivor"] >= FAR for f in deep), deep
    assert all(f["n_waiting"] > 1 << 16 and f["n_resolved"] > 10_000 for f in deep), deep
    assert (mw + tasks + TILE - 1) // TILE == 167
    ws, q = W.WaitingStream(sv, tasks, frees, mw, n_envs=2), W.WaitQueue(mw)
    ctx = waiting.begin(ws.es, mw, frees, tasks)
    waiting.drive(ctx, ws, q, ticks)
    assert ws.n_waiting == facts[-1]["n_waiting"]
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("tiles", [64, 65, 128, 129])
def test_waiting_grid_of_exactly(tiles):
    """max_waiting + max_tasks = (tiles - 1) * 1024 + 515: the last tile is partial and the batch
    is no multiple of 4 long. A saturated pool: the new requests (the last 8 000 positions) mostly
    join the queue, so their ranks come from the prefix over every tile in front of them; expiries
    and grants resolve entries from the queue's first position on."""
    n = (tiles - 1) * TILE + 515
    tasks, frees, ticks = 8_000, 300, 8
    mw = n - tasks
    sv = synth.make_servants(40, n_tasks_hint=6_000, n_envs=2, seed=42)
    facts = wait_facts(sv, tasks, frees, mw, ticks, 2)
    assert (n + TILE - 1) // TILE == tiles and n % 4 == 3
    assert sum(f["n"] == tasks and f["last_joined"] for f in facts) >= 3, facts
    assert sum(f["first_resolved"] for f in facts) >= 3 and facts[-1]["n_waiting"] > 20_000, facts
    ws, q = W.WaitingStream(sv, tasks, frees, mw, n_envs=2), W.WaitQueue(mw)
    ctx = waiting.begin(ws.es, mw, frees, tasks)
    waiting.drive(ctx, ws, q, ticks)
    ctx.stream_end()
    ctx.close()


class SkewedLeaseStream(L.LeaseStream):
    """A leased stream on a pool with two digests whose requests ask for digest 1 in 15 % of the
    cases and for an unknown one in 2 %: digest 0 runs out of slots early in a tick's batch and
    digest 1 never does, so grants (1), Timeouts (0) and EnvironmentNotFound are interleaved from
    there to the batch's end."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.mix = np.random.default_rng(5)

    def next_tick(self):
        ev = super().next_tick()
        env = ev["tasks"]["env_id"]
        env[:] = self.mix.random(len(env)) < 0.15
        env[self.mix.random(len(env)) < 0.02] = 0xFFFF
        return ev


def test_leased_grants_beyond_position_65536():
    """2000 servants (cfg2's pool with two digests), 72 000 requests, 60 000 frees by id and 2 000
    renewals per tick; max_tasks 132 003: k_lease_grant runs over 129 tiles + 3 positions (three
    windows, the scalar tail). From tick 2 on digest 0 is saturated: hundreds of grants, thousands
    of Timeouts and EnvironmentNotFound alternate behind position 65 536, and every id there is
    next_id + its rank among all the grants in front."""
    max_tasks, tasks, ticks = 132_003, 72_000, 7
    assert (max_tasks + TILE - 1) // TILE == 129 and max_tasks % 4 == 3
    sv, _ = synth.make_config("cfg2", n_envs=2)
    ls = SkewedLeaseStream(sv, tasks, 60_000, 2000, L.LeaseTable(), n_envs=2)
    ctx = lease.begin(ls, 1 << 18, max_tasks, frees=1 << 17, report_ids=1 << 17)
    rec = lease.drive(ctx, ls, ticks, snapshot_every=3)
    far = [r["out"][FAR:] for r in rec]
    mixed = [o for o in far if len(o) and (o < L.IDX_ENV_NOT_FOUND).sum() > 500 and (o == L.IDX_TIMEOUT).sum() > 500
             and (o == L.IDX_ENV_NOT_FOUND).sum() > 50]
    assert len(mixed) >= 4, [(len(o), int((o < L.IDX_ENV_NOT_FOUND).sum())) for o in far]
    assert sum(r["freed"] for r in rec) > 100_000 and sum(r["swept"] for r in rec) and sum(r["expired"] for r in rec)
    ctx.stream_end()
    ctx.close()


def _batch(n, sv, real, seed):
    """n requests for a digest nobody has, except at `real` (ordinary requests)."""
    tk = {"env_id": np.full(n, 0xFFFF, np.uint32), "min_version": np.zeros(n, np.uint32),
          "requestor_ip": np.zeros(n, np.uint32)}
    some = synth.make_tasks(len(real), sv, n_envs=1, seed=seed, self_frac=0.0)
    for k in tk:
        tk[k][real] = some[k]
    return tk


@pytest.mark.parametrize("tiles", [64, 65, 128, 129])
def test_leased_grid_of_exactly(tiles):
    """max_tasks = (tiles - 1) * 1024 + 515: the last tile is partial, the size is no multiple of 4
    (the scalar tail of k_lease_grant's stores). A hand-made batch on 60 servants: requests for an
    unknown digest everywhere except a grant in the first and in the last valid position and
    around every tile boundary a window starts or ends at. Then a tick
    of 700 requests (every tile but the first publishes a zero aggregate), then the wide batch
    again: the ids go on where the previous tick stopped."""
    n = (tiles - 1) * TILE + 515
    assert (n + TILE - 1) // TILE == tiles and n % 4 == 3
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=1, seed=5)
    ls = L.LeaseStream(sv, n, 0, 0, L.LeaseTable(), n_envs=1)
    ctx = lease.begin(ls, 1 << 18, n)  # (|L| + n_tasks <= max_leases is asked of every tick)
    edges = [0, 1, 3, 4, 1023, 1024, n - 1, n - 2, n - 4, n - 5, (tiles - 1) * TILE - 1, (tiles - 1) * TILE]
    for w in range(64 * TILE, n, 64 * TILE):
        edges += [w - TILE - 1, w - TILE, w - 1, w, w + 1, w + TILE - 1, w + TILE]
    real = np.array(sorted(set(e for e in edges if 0 <= e < n)))
    granted = 0
    for t, size in enumerate([n, 700, n]):
        ev = ls.next_tick()
        if size == n:
            tk = _batch(n, ls.es.sv, real, 40 + t)
        else:
            tk = synth.make_tasks(size, ls.es.sv, n_envs=1, seed=40 + t, self_frac=0.0)
        ev = lease.quiet(ev, tasks=tk, lease_expires_at=np.full(size, 100, np.int64))
        first = ls.table.next_id
        want = L.model_tick(ls, ev)
        lease.check_tick(t, ctx, ls, lease.gpu_tick(ctx, ls, ev), want)
        g = want["out"] < L.IDX_ENV_NOT_FOUND
        if size == n:
            assert g[real].all() and g.sum() == len(real), "the pool did not grant the hand-made requests"
            assert want["task_id"][0] == first and want["task_id"][n - 1] == first + len(real) - 1
        else:
            assert g.all()
        granted += int(g.sum())
    assert ls.table.next_id == granted == 2 * len(real) + 700
    ctx.stream_end()
    ctx.close()

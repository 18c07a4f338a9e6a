"""Inspection on the device (ydc_stream_inspect_begin / _load / _servants / _tasks; the detail records
beside the lease table's slots, the servants' discovered_at / ever_assigned columns, k_inspect_pack,
k_inspect_servants): after every tick of a leased, waiting-and-leased or rpc stream with inspection on,
the two get calls are compared with the model (tests/stream_inspect_model.py, pinned against the
verbatim reference's DumpInternals by tests/test_stream_inspect_model.py), beside everything the
modes' own gpu_tick / check_tick compare."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_inspect_model as IM
from tests import stream_lease_model as L
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WM
from tests import test_stream_lease_gpu as lease
from tests import test_stream_rpc_gpu as rpc
from tests import test_stream_wait_lease_gpu as wl
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu
MODS = {"leased": (L, lease), "wait_leased": (WM, wl), "rpc": (RM, rpc)}
TASK_COLS = ("task_id", "servant_idx", "expires_at", "zombie", "started_at", "env_id", "requestor_ip", "prefetch")
SERVANT_COLS = ("discovered_at", "ever_assigned", "running_tasks", "capacity_available")
TILE = 1024  # kLeaseTile / kRpcTile: positions per workgroup of the granting passes


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


def pool(n=160, seed=3, hint=5200):
    return synth.make_servants(n, n_tasks_hint=hint, n_envs=2, seed=seed)


# Per mode the pool the two-tile stream runs on: roomy enough for more than a tile of grants per tick,
# and in the modes with a queue tight enough that requests wait and are granted later.
POOL_HINT = {"leased": 5200, "wait_leased": 600, "rpc": 3600}


def stream(mode, sv):
    """A stream of `mode` whose placed batch has about 1 500 positions: two tiles of the granting
    pass, grants in both (two_tiles() says whether a tick had them)."""
    if mode == "leased":
        ws = L.LeaseStream(sv, 1500, 1300, 120, L.LeaseTable(), n_envs=2, report_frac=0.3)
    elif mode == "wait_leased":
        # (W's region, max_waiting positions, leads the batch: the new requests lie in the second tile)
        ws = WM.new_stream(sv, 400, 300, 120, 1100, n_envs=2, rate=lambda now: 1.0 if now % 12 < 8 else 0.25,
                           report_frac=0.3)
    else:
        ws = RM.new_stream(sv, 40, 600, 120, 400, 1536, n_envs=2, report_frac=0.3,
                           rate=lambda now: 1.0 if now % 12 < 8 else 0.25, **BIG)
    ws.es.hb = 24
    return ws


def begin(mode, ws, ctx=None):
    if mode == "leased":
        assert ctx is None
        return lease.begin(ws, 1 << 14, 1500)
    if mode == "wait_leased":
        return wl.begin(ws, 1 << 14, 400, ctx=ctx)
    return rpc.begin(ws, 40, max_leases=1 << 14, ctx=ctx)


class Inspected:
    """A stream `ws` of `mode` on `ctx` with inspection on, and the model's side of it."""

    def __init__(self, mode, ws, ctx, alive=False, begin_now=True):
        self.mode, (self.M, self.G) = mode, MODS[mode]
        self.ws, self.ctx, self.alive, self.t = ws, ctx, alive, 0
        self.I = None
        if begin_now:
            self.inspect_begin()

    def inspect_begin(self, **cols):
        self.I = IM.attach(self.ws, cols.get("discovered_at"), cols.get("ever_assigned"))
        self.ctx.stream_inspect_begin(**cols)

    def check(self):
        ctx, I, t = self.ctx, self.I, self.t
        got, want = ctx.stream_inspect_tasks(), I.tasks()
        assert len(got["task_id"]) == len(want["task_id"]), "tick %d: |L| gpu %d model %d" % (
            t, len(got["task_id"]), len(want["task_id"]))
        for k in TASK_COLS:
            bad = np.nonzero(got[k] != want[k])[0]
            assert bad.size == 0, "tick %d: tasks %s: lease %d gpu %s model %s (%d differ)" % (
                t, k, got["task_id"][bad[0]], got[k][bad[0]], want[k][bad[0]], bad.size)
        got, want = ctx.stream_inspect_servants(), I.servants()
        for k in SERVANT_COLS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (t, k, got[k].shape, want[k].shape)
            bad = np.nonzero(got[k] != want[k])[0]
            assert bad.size == 0, "tick %d: servants %s: row %d gpu %s model %s (%d differ)" % (
                t, k, bad[0], got[k][bad[0]], want[k][bad[0]], bad.size)
        assert got["totals"] == want["totals"], (t, got["totals"], want["totals"])

    def tick(self, ev, snapshot=True):
        if self.alive:
            self.ctx.stream_alive_stage(ev["upd_expires_at"])
        # (the GPU first: gpu_tick reads the heartbeats' masks by the numbering the tick came with)
        got = self.G.gpu_tick(self.ctx, self.ws, ev)
        if self.I is not None:
            want = IM.model_tick(self.M, self.ws, ev, alive=self.alive)
        elif self.alive:
            want = AM.model_tick(self.M, self.ws, ev)
        else:
            want = self.M.model_tick(self.ws, ev)
        self.G.check_tick(self.t, self.ctx, self.ws, got, want, snapshot=snapshot)
        if self.I is not None:
            self.check()
        self.t += 1
        return got, want

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def two_tiles(mode, ws, ev):
    """Whether the tick's granting pass inserted leases from both of its tiles. The model's batch is
    [W's live entries | the new requests]; the device's positions are the same in leased and rpc mode
    (rows of entries without rows do not exist), and [max_waiting slots of W | the new requests] with
    a waiting queue, where max_waiting >= TILE puts every new request into the second tile."""
    I = ws.table.inspect
    rows = I.last_rows
    if mode == "wait_leased":
        n_live = I.last_n - len(ev["tags"])
        assert ws.state.max_waiting >= TILE and n_live <= TILE
        return bool((rows < n_live).any() and (rows >= n_live).any())
    return bool(len(rows) and rows.min() < TILE <= rows.max())


@pytest.mark.parametrize("mode,stream_graph", [(m, g) for m in MODS for g in ("1", "0")])
def test_every_tick_of_each_mode(mode, stream_graph, monkeypatch):
    """30 ticks, batches of about 1 500 positions: grants fall into two commit tiles, and the second
    tile's ids and records depend on the look-back. Tasks, servants and totals after every tick."""
    _graph(monkeypatch, stream_graph)
    ws = stream(mode, pool(hint=POOL_HINT[mode]))
    x = Inspected(mode, ws, begin(mode, ws))
    both = prefetched = from_w = 0
    for _ in range(30):
        ev = ws.next_tick()
        _, want = x.tick(ev)
        from_w += want.get("w_granted", 0)
        both += two_tiles(mode, ws, ev)
    tk = x.I.tasks()
    prefetched = int(tk["prefetch"].sum())
    assert both >= 3, "only %d ticks granted from both tiles" % both
    assert (mode == "leased" or from_w > 0) and (prefetched > 0) == (mode == "rpc"), (from_w, prefetched)
    assert int(x.I.ever.sum()) > 3000 and len(tk["task_id"]) > 200
    x.close()


def test_rpc_prefetch_follows_rank_and_waiters_start_at_their_grant():
    """A saturated pool of servants with two slots at the most: RPCs wait and are granted ticks later with started_at of
    the granting tick; n_immediate == 0 RPCs hold prefetched leases only; inside an RPC the flag is 0
    for the first n_immediate grants and 1 behind them."""
    sv = pool(64, seed=11)
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 2)
    ws = RM.new_stream(sv, 12, 10, 10, 200, 1200, n_envs=2, report_frac=0.3, rate=lambda now: 1.0 if now % 6 < 4 else 0.0)
    ws.es.hb = 16
    x = Inspected("rpc", ws, rpc.begin(ws, 12))
    submitted, shape, late, only_prefetch, mixed = {}, {}, 0, 0, 0
    for _ in range(20):
        ev = ws.next_tick()
        now = int(ev["now"])
        for tag, a, b in zip(ev["tags"].tolist(), ev["n_immediate"].tolist(), ev["n_prefetch"].tolist()):
            submitted[tag], shape[tag] = now, (a, b)
        got, want = x.tick(ev)
        tk = x.ctx.stream_inspect_tasks()
        row = {int(t): k for k, t in enumerate(tk["task_id"])}
        for j, tag in enumerate(want["res_tags"].tolist()):  # W's entries answered in this tick
            g, first = int(want["res_n_granted"][j]), int(want["res_first"][j])
            ids = want["res_task_ids"][first:first + g].tolist()
            n_imm = shape[tag][0]
            for rank, t in enumerate(ids):
                k = row[int(t)]
                assert tk["started_at"][k] == now > submitted[tag], (tag, now, submitted[tag])
                assert tk["prefetch"][k] == (rank >= n_imm), (tag, rank, n_imm)
                late += 1
                only_prefetch += n_imm == 0
        at = 0
        for i, tag in enumerate(ev["tags"].tolist()):  # the new requests
            g = int(want["n_granted"][i])
            for rank, t in enumerate(want["task_ids"][at:at + g].tolist()):
                k = row[int(t)]
                assert tk["started_at"][k] == now and tk["prefetch"][k] == (rank >= shape[tag][0])
                only_prefetch += shape[tag][0] == 0
                mixed += 0 < shape[tag][0] <= rank
            at += g
    assert late > 0 and only_prefetch > 0 and mixed > 0, (late, only_prefetch, mixed)
    x.close()


@pytest.mark.parametrize("mode", list(MODS))
def test_inspection_begun_late(mode):
    """Leases granted before the begin call carry the sentinels, leases granted after it do not; a
    second begin call replaces the servant columns and leaves the details alone."""
    ws = stream(mode, pool(96, seed=5))
    x = Inspected(mode, ws, begin(mode, ws), begin_now=False)
    for _ in range(4):
        x.tick(ws.next_tick())
    early = set(ws.table.L)
    assert len(early) > 100
    x.inspect_begin()
    assert (x.I.disc == ws.table.last_now).all()  # (NULL: the previous accepted tick's now)
    x.check()
    tk = x.ctx.stream_inspect_tasks()
    assert (tk["env_id"] == binding.INSPECT_NO_ID).all() and (tk["requestor_ip"] == binding.INSPECT_NO_ID).all()
    assert (tk["started_at"] == binding.INSPECT_NO_TIME).all() and not tk["prefetch"].any()
    for _ in range(5):
        x.tick(ws.next_tick())
    tk = x.ctx.stream_inspect_tasks()
    old = np.array([int(t) in early for t in tk["task_id"]], bool)
    assert old.any() and (~old).any()
    assert (tk["env_id"][old] == binding.INSPECT_NO_ID).all() and (tk["env_id"][~old] != binding.INSPECT_NO_ID).all()
    assert (tk["started_at"][~old] >= 4).all()
    # A second call: the columns given, the details as they were.
    disc, ever = np.arange(ws.es.n, dtype=np.int64) + 100, np.arange(ws.es.n, dtype=np.uint64) * 3
    x.I.disc, x.I.ever = disc.copy(), ever.copy()
    x.ctx.stream_inspect_begin(disc, ever)
    x.check()
    x.tick(ws.next_tick())
    x.close()


def test_records_survive_reserve_and_book_begin():
    """ydc_stream_reserve from a table for 64 leases to one for 4 096 files every lease again (other
    home slots): each keeps its record. ydc_stream_book_begin afterwards moves the stream once more."""
    sv = pool(64, seed=7)
    ws = L.LeaseStream(sv, 12, 6, 4, L.LeaseTable(64), n_envs=2, report_frac=0.3)
    ws.es.hb = 16
    ctx = lease.begin(ws, 64, 12)
    x = Inspected("leased", ws, ctx)
    while len(ws.table.L) < 40:
        x.tick(ws.next_tick())
    before = ctx.stream_inspect_tasks()
    assert len(before["task_id"]) >= 40 and (before["env_id"] != binding.INSPECT_NO_ID).all()
    ws.table.max_leases = 4096
    ctx.stream_reserve(max_leases=4096, max_tasks=600)
    x.check()
    after = ctx.stream_inspect_tasks()
    for k in TASK_COLS:
        assert np.array_equal(before[k], after[k]), k
    ctx.stream_book_begin(5000)
    x.check()
    for k in TASK_COLS:
        assert np.array_equal(before[k], ctx.stream_inspect_tasks()[k]), k
    ws.es.tasks_per_tick = 600
    for _ in range(4):  # (the grown stream goes on, past the old table's 64 leases)
        ev = ws.next_tick()
        ctx.stream_book_stage(n_ids=len(ev["report_ids"]))
        x.tick(ev)
    assert len(ws.table.L) > 64
    x.close()


def test_remove_servants_compacts_the_columns():
    """ydc_remove_servants between ticks: discovered_at and ever_assigned follow the compaction in
    order, the removed rows' tasks are gone with their records."""
    ws = stream("leased", pool(96, seed=5))
    x = Inspected("leased", ws, begin("leased", ws))
    for _ in range(4):
        x.tick(ws.next_tick())
    x.I.disc[:] = np.arange(ws.es.n) + 50  # (distinct values: an order that is kept shows)
    x.ctx.stream_inspect_begin(x.I.disc, x.I.ever)
    removed = np.array([0, 17, 63, 64, 95], np.uint32)
    on_removed = sum(1 for e in ws.table.L.values() if e[0] in set(removed.tolist()))
    assert on_removed > 0
    x.ctx.remove_servants(removed)
    lease.drop_rows(ws, removed)
    x.check()
    assert len(x.I.disc) == 91 and x.I.disc[0] == 51 and x.I.disc[-1] == 50 + 94
    for _ in range(3):
        x.tick(ws.next_tick())
    x.close()


@pytest.mark.parametrize("mode", ["leased", "rpc"])
def test_aliveness_removes_and_a_heartbeat_appends(mode):
    """Servants run out inside ticks (the removal route): both columns are compacted in order and the
    orphans' tasks are gone; a servant a tick's heartbeats append has discovered_at == now and
    ever_assigned 0 before the tick's own grants."""
    sv = pool(70, seed=3)
    ws = stream(mode, sv)
    ctx = begin(mode, ws)
    first = AM.first_expiries(70, life=4)
    AM.attach(ws, first)
    ctx.stream_alive_begin(first)
    x = Inspected(mode, ws, ctx, alive=True)
    gen = AM.AliveGen(ws, life=4, p_stop=0.3, p_short=0.3, seed=3)
    removed = orphans = 0
    appended = None
    for t in range(12):
        ev = gen.next_tick()
        if t == 6:
            row, s_new = AM.append_servant(ws, 0, 0x0A636363)
            ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
            ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
            ev["upd_expires_at"] = np.concatenate([ev["upd_expires_at"], [int(ev["now"]) + 100]]).astype(np.int64)
            appended = int(ev["now"])
        _, want = x.tick(ev)
        removed += len(want["removed"])
        orphans += want["orphans"]
        if t == 6:
            assert x.I.disc[-1] == appended and x.ctx.stream_inspect_servants()["discovered_at"][-1] == appended
    assert removed >= 2 and orphans > 0 and appended is not None, (removed, orphans)
    x.close()


def twin(mode, sv):
    ws = stream(mode, sv)
    return Inspected(mode, ws, begin(mode, ws))


@pytest.mark.parametrize("mode", ["leased", "rpc"])
def test_restart_carries_the_details_beside_the_blob(mode):
    """A: the two get calls persisted beside ydc_stream_snapshot's blob. B: ydc_stream_restore,
    ydc_stream_inspect_begin(columns), ydc_stream_inspect_load(columns). Both answer the same, and go on
    doing so over 10 further ticks."""
    a = twin(mode, pool(96, seed=5))
    for _ in range(6):
        a.tick(a.ws.next_tick())
    blob, sv_cols, tk_cols = a.ctx.stream_snapshot(), a.ctx.stream_inspect_servants(), a.ctx.stream_inspect_tasks()
    assert len(tk_cols["task_id"]) > 100
    b = binding.Context(device=0)
    b.stream_restore(blob)
    with pytest.raises(binding.YdcError):  # (the blob says nothing about inspection: off after a restore)
        b.stream_inspect_tasks()
    b.stream_inspect_begin(sv_cols["discovered_at"], sv_cols["ever_assigned"])
    # Refused loads leave the state untouched: an unknown id, a duplicate id, more records than leases.
    state = b.stream_inspect_tasks()
    assert (state["env_id"] == binding.INSPECT_NO_ID).all()
    bad_id = dict(tk_cols, task_id=tk_cols["task_id"].copy())
    bad_id["task_id"][3] = a.ws.table.next_id + 5
    dup = dict(tk_cols, task_id=tk_cols["task_id"].copy())
    dup["task_id"][7] = dup["task_id"][2]
    more = {k: np.concatenate([v, v[:1]]) for k, v in tk_cols.items()}
    more["task_id"][-1] = a.ws.table.next_id + 9
    for cols in (bad_id, dup, more):
        with pytest.raises(binding.YdcError):
            b.stream_inspect_load(**cols)
        for k in TASK_COLS:
            assert np.array_equal(b.stream_inspect_tasks()[k], state[k]), k
    b.stream_inspect_load(**tk_cols)
    for k in TASK_COLS:
        assert np.array_equal(b.stream_inspect_tasks()[k], tk_cols[k]), k
    got = b.stream_inspect_servants()
    assert got["totals"] == sv_cols["totals"] and all(np.array_equal(got[k], sv_cols[k]) for k in SERVANT_COLS)
    G = a.G
    for _ in range(10):
        ev = a.ws.next_tick()
        out_b = G.gpu_tick(b, a.ws, ev)
        a.tick(ev)  # (A against the model, which advances once)
        ta, tb = a.ctx.stream_inspect_tasks(), b.stream_inspect_tasks()
        for k in TASK_COLS:
            assert np.array_equal(ta[k], tb[k]), k
        sa, sb = a.ctx.stream_inspect_servants(), b.stream_inspect_servants()
        assert sa["totals"] == sb["totals"] and all(np.array_equal(sa[k], sb[k]) for k in SERVANT_COLS)
    assert out_b is not None
    b.stream_end()
    b.close()
    a.close()


def pathological(S, seed=1):
    """S servants cycling through every branch of GetCapacityAvailable (the rows of
    test_stream_inspect_model.test_totals_by_hand first), running_tasks given at upload."""
    rng = np.random.default_rng(seed)
    sv = synth.make_servants(S, n_tasks_hint=64, n_envs=2, seed=seed)
    hand = [(8, 2, 4, 1, False), (8, 11, 4, 0, False), (16, 5, 2, 5, True), (8, 6, 1, 3, False), (8, 0, 0, 0, False)]
    for s in range(S):
        if s % 7 < 5:
            nproc, load, maxt, run, low = hand[s % 7]
        else:
            nproc, maxt = int(rng.integers(1, 128)), int(rng.integers(0, 64))
            load, run, low = int(rng.integers(0, 200)), int(rng.integers(0, 80)), bool(rng.integers(2))
        sv["num_processors"][s], sv["current_load"][s], sv["max_tasks"][s], sv["running_tasks"][s] = nproc, load, maxt, run
        sv["total_memory"][s] = 64 << 30
        sv["memory_available"][s] = (1 << 20) if low else (32 << 30)
    return sv


@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1025])
def test_totals_at_the_wave_and_workgroup_edges(S):
    sv = pathological(S)
    abi = pack.to_abi_columns(sv)
    low = (abi["flags"] & IM.LOW_MEMORY) != 0
    assert S < 3 or (low & (sv["running_tasks"] > sv["max_tasks"])).any()
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    ctx.stream_begin_leased(8, 8, 16, 64, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    got = ctx.stream_inspect_servants()
    avail = [IM.capacity(sv["num_processors"][s], sv["current_load"][s], sv["max_tasks"][s], sv["running_tasks"][s], low[s])
             for s in range(S)]
    assert np.array_equal(got["capacity_available"], np.array(avail, np.uint32))
    assert np.array_equal(got["running_tasks"], sv["running_tasks"])
    assert got["totals"] == IM.totals(sv["max_tasks"], sv["running_tasks"], avail)
    assert (got["discovered_at"] == 0).all() and (got["ever_assigned"] == 0).all()  # (before the first tick)
    if S == 65:  # the hand-written case's five rows alone would give (5, 9, 11, 1, 1); here they are part of the sum
        five = IM.totals(sv["max_tasks"][:5], sv["running_tasks"][:5], avail[:5])
        assert five == {"servants_up": 5, "running_tasks": 9, "capacity": 11, "capacity_available": 1, "capacity_unavailable": 1}
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("mode", list(MODS))
def test_off_means_off(mode):
    """A twin stream without inspection gives identical tick outputs and ydc_get_stats over the same ticks."""
    sv = pool(96, seed=5)
    on = twin(mode, sv)
    ws_off = stream(mode, sv)
    off = begin(mode, ws_off)
    for _ in range(8):
        ev = on.ws.next_tick()
        ev_off = ws_off.next_tick()
        got_on, _ = on.tick(ev)
        st_on = on.ctx.stats()
        got_off = on.G.gpu_tick(off, ws_off, ev_off)
        st_off = off.stats()
        on.M.model_tick(ws_off, ev_off)
        if isinstance(got_on, dict):
            assert set(got_on) == set(got_off) and all(np.array_equal(got_on[k], got_off[k]) for k in got_on)
        else:
            assert len(got_on) == len(got_off) and all(np.array_equal(a, b) for a, b in zip(got_on, got_off))
        for k in st_on:
            assert k == "stage_ms" or st_on[k] == st_off[k], k  # (every count; the stage times are measurements)
    with pytest.raises(binding.YdcError):
        off.stream_inspect_tasks()
    with pytest.raises(binding.YdcError):
        off.stream_inspect_servants()
    with pytest.raises(binding.YdcError):
        off.stream_inspect_load(np.zeros(1, np.uint64))
    off.stream_end()
    off.close()
    on.close()


def test_refusals():
    """Wrong contexts and modes; a cap too small sets *out_n and writes nothing."""
    sv = pool(64, seed=5)
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(sv))
    with pytest.raises(binding.YdcError):  # no stream
        ctx.stream_inspect_begin()
    ctx.stream_begin(8, 8, 16)
    with pytest.raises(binding.YdcError):  # a plain stream
        ctx.stream_inspect_begin()
    ctx.stream_end()
    ctx.stream_begin(8, 8, 16, max_waiting=32)
    with pytest.raises(binding.YdcError):  # a waiting stream without leases
        ctx.stream_inspect_begin()
    ctx.stream_end()
    ctx.close()
    ws = stream("leased", sv)
    x = Inspected("leased", ws, begin("leased", ws))
    with pytest.raises(binding.YdcError):  # n is not the registry's servant count
        x.ctx.stream_inspect_begin(np.zeros(10, np.int64))
    x.tick(ws.next_tick())
    L_, h = binding.lib(), x.ctx._h
    n_leases = len(ws.table.L)
    assert n_leases > 4
    ids = np.full(n_leases, 0xABCD, np.uint64)
    n = C.c_uint32(0)
    rc = L_.ydc_stream_inspect_tasks(h, ids.ctypes.data, None, None, None, None, None, None, None, n_leases - 1, C.byref(n))
    assert rc == -4 and n.value == n_leases and (ids == 0xABCD).all()
    disc = np.full(ws.es.n, -7, np.int64)
    rc = L_.ydc_stream_inspect_servants(h, disc.ctypes.data, None, None, None, ws.es.n - 1, C.byref(n), None)
    assert rc == -4 and n.value == ws.es.n and (disc == -7).all()
    # Any output pointer may be NULL.
    only = np.empty(n_leases, np.uint8)
    rc = L_.ydc_stream_inspect_tasks(h, None, None, None, None, None, None, None, only.ctypes.data, n_leases, C.byref(n))
    assert rc == 0 and n.value == n_leases and not only.any()
    # ydc_stream_end switches it off; so does the next begin call.
    x.ctx.stream_end()
    x.ctx.stream_begin_leased(8, 8, 16, 64, 8, 8, 8, 8)
    with pytest.raises(binding.YdcError):
        x.ctx.stream_inspect_servants()
    x.close()


def test_a_refused_tick_counts_and_stores_nothing():
    """A tick refused with YDC_ERR_CAPACITY (more leases than max_leases has room for) leaves
    ever_assigned and the records as they were."""
    sv = pool(64, seed=7)
    ws = L.LeaseStream(sv, 40, 0, 0, L.LeaseTable(64), n_envs=2, report_frac=0.3)
    ws.es.hb = 16
    x = Inspected("leased", ws, lease.begin(ws, 64, 40))
    x.tick(ws.next_tick())
    assert len(ws.table.L) + 40 > 64
    before_t, before_s = x.ctx.stream_inspect_tasks(), x.ctx.stream_inspect_servants()
    state = (ws.es.tick_no, ws.es.hb_pos, ws.rep_pos)
    ev = ws.next_tick()
    with pytest.raises(binding.YdcError, match="max_leases"):
        lease.gpu_tick(x.ctx, ws, ev)
    after_t, after_s = x.ctx.stream_inspect_tasks(), x.ctx.stream_inspect_servants()
    for k in TASK_COLS:
        assert np.array_equal(before_t[k], after_t[k]), k
    assert np.array_equal(before_s["ever_assigned"], after_s["ever_assigned"])
    assert np.array_equal(before_s["discovered_at"], after_s["discovered_at"])
    assert state[0] + 1 == ws.es.tick_no
    x.close()

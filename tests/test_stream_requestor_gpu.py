"""The load per requestor on the device (ydc_stream_requestor_find / ydc_stream_requestor_get;
requestor_index.h: k_requestor_leases, _waiting, _find, _fold) against the model
(tests/stream_requestor_model.py: a NumPy fold of what the existing getters answer, pinned against a
dictionary count by tests/test_stream_requestor_model.py): integer equality on every column, in every
mode, beside a twin context that never asks and must answer every tick identically; and the admission
clip end to end (streaming.admit)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import stream_alive_model as AM
from tests import stream_outlook_model as OM
from tests import stream_requestor_model as QM
from tests import stream_rpc_model as RM
from tests import stream_wait_model as WQ
from tests import test_stream_inspect_gpu as ist
from tests import test_stream_lease_gpu as lease
from tests import test_stream_rpc_gpu as rpc
from tests import test_stream_waiting_gpu as wg
from yadcc_amd import binding, pack, streaming, synth

pytestmark = pytest.mark.gpu
UNKNOWN = binding.REQUESTOR_UNKNOWN
WAITING = binding.IDX_WAITING
NOBODY = np.array([0, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)  # ids nobody has (unless a test says otherwise)
E32, E64, I64 = np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.int64)
NO_ROWS = np.empty(0, binding.ROW_DTYPE)
INVALID, CAPACITY = -1, -4


def same_rows(got, want, what=""):
    assert got.dtype == QM.DTYPE and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for k in QM.DTYPE.names:
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, "%s: %s: row %d (requestor %#x) gpu %s model %s (%d differ)" % (
            what, k, bad[0], int(want["requestor_ip"][bad[0]]), got[k][bad[0]], want[k][bad[0]], bad.size)


def check(ctx, want, want_un, ips=(), what=""):
    """get and find of `ctx` against the model's rows: every requestor of the rows and of `ips`, the
    three ids nobody has, and two repeats."""
    got, un = ctx.stream_requestors()
    same_rows(got, want, what + ": get")
    assert un == want_un, (what, un, want_un)
    q = np.concatenate([want["requestor_ip"], np.asarray(ips, np.uint32), NOBODY]).astype(np.uint32)
    q = np.concatenate([q, q[:2]])
    found, un = ctx.stream_requestor_find(q)
    same_rows(found, QM.find(want, q, lease_columns=want_un != UNKNOWN), what + ": find")
    assert un == want_un, (what, un, want_un)
    return got


def same_answers(a, b, what=""):
    if isinstance(a, dict):
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a), what
    else:
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), what


def uploaded(sv):
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(sv))
    return ctx


def roomy_registry(slots_each=800):
    """8 idle servants that take `slots_each` tasks each, digests 0 - 2 everywhere."""
    sv = synth.make_servants(8, n_tasks_hint=64, n_envs=3, seed=1)
    sv["version"][:], sv["num_processors"][:], sv["current_load"][:] = 20, slots_each, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = slots_each, 0
    sv["memory_available"][:], sv["total_memory"][:] = 32 << 30, 64 << 30
    sv["env_mask"] = np.full(8, 7, np.uint64)
    return sv


def saturated_registry():
    """... and 8 that run all they take: every request waits."""
    sv = roomy_registry(2)
    sv["running_tasks"][:] = 2
    return sv


def leased_tick(ctx, now, ips, lease_for=1000, free_ids=E64):
    ips = np.asarray(ips, np.uint32)
    n = len(ips)
    tk = {"env_id": np.zeros(n, np.uint32), "min_version": np.zeros(n, np.uint32), "requestor_ip": ips}
    out, ids, _, _, n_leases = ctx.stream_tick_leased(E32, NO_ROWS, E32, E64, I64, np.asarray(free_ids, np.uint64), E32,
                                                      np.zeros(1, np.uint32), E64, tk, np.full(n, now + lease_for, np.int64), now)
    assert (out < 8).all()
    return ids, n_leases


def rpc_tick(ctx, now, req):
    return ctx.stream_tick_rpc(E32, NO_ROWS, E32, E64, I64, E64, E32, np.zeros(1, np.uint32), E64, req,
                               req["n_immediate"], req["n_prefetch"], req["lease_for"], req["deadline"], req["tag"], now)


def rpc_requests(ips, first_tag, rng, deadline=1 << 40):
    ips = np.asarray(ips, np.uint32)
    n = len(ips)
    n_imm = rng.choice(RM.NIMM, n)
    n_pre = np.where(n_imm == 0, 1 + rng.integers(0, 3, n), rng.choice(RM.NPRE, n)).astype(np.uint32)
    return {"env_id": rng.integers(0, 3, n).astype(np.uint32), "min_version": np.zeros(n, np.uint32), "requestor_ip": ips,
            "n_immediate": n_imm, "n_prefetch": n_pre, "lease_for": np.full(n, 50, np.int64),
            "deadline": np.full(n, deadline, np.int64), "tag": np.arange(first_tag, first_tag + n, dtype=np.uint64)}


# ---- every mode, every tick, beside a twin that never asks -------------------------------------

@pytest.mark.parametrize("mode,stream_graph", [(m, g) for m in ist.MODS for g in ("1", "0")])
def test_each_lease_mode_after_every_tick_with_a_twin(mode, stream_graph, monkeypatch):
    """12 ticks of a leased, waiting-and-leased or rpc stream with inspection on; find for every
    requestor the pool has used so far plus three ids nobody has, and get, after each. The twin gets
    the same ticks and never asks: identical answers, lease snapshot, running_tasks and, at the end,
    snapshot bytes."""
    ist._graph(monkeypatch, stream_graph)
    ws = ist.stream(mode, ist.pool(96, seed=5, hint=ist.POOL_HINT[mode] // 2))
    x = ist.Inspected(mode, ws, ist.begin(mode, ws))
    twin = ist.begin(mode, ws) if mode == "leased" else ist.begin(mode, ws, ctx=uploaded(ws.es.sv))
    twin.stream_inspect_begin()
    used = np.empty(0, np.uint32)
    seen = dict(zombies=0, waiting=0, expired=0, swept=0, leases=0, prefetch=0)
    for t in range(12):
        ev = ws.next_tick()
        used = np.union1d(used, np.asarray(ev["tasks"]["requestor_ip"], np.uint32))
        got_twin = x.G.gpu_tick(twin, ws, ev)
        got, want = x.tick(ev, snapshot=False)
        same_answers(got, got_twin, "tick %d" % t)
        same_answers(x.ctx.stream_leases(), twin.stream_leases(), "tick %d: lease snapshot" % t)
        assert np.array_equal(x.ctx.get_running(), twin.get_running()), t
        rows, un = QM.stream_fold(ws, x.I)
        g = check(x.ctx, rows, un, used, "tick %d" % t)
        # ... and against the existing getters of the same context
        same_rows(g, QM.fold(x.ctx.stream_inspect_tasks(), x.ctx.stream_waiting() if mode != "leased" else None)[0],
                  "tick %d: the getters" % t)
        assert un == 0
        for k, col in (("zombies", "zombies"), ("waiting", "waiting"), ("leases", "leases"), ("prefetch", "prefetch_leases")):
            seen[k] += int(g[col].sum())
        seen["expired"] += want["expired"]
        seen["swept"] += want["swept"]
        if mode == "rpc":
            assert int(g["waiting_rows"].sum()) == got["n_waiting_rows"], t
        if mode == "leased":
            assert not g["waiting"].any() and not g["waiting_rows"].any()
    assert seen["zombies"] and seen["expired"] and seen["swept"] and seen["leases"], seen
    assert (seen["waiting"] > 0) == (mode != "leased") and (seen["prefetch"] > 0) == (mode == "rpc"), seen
    assert x.ctx.stream_snapshot() == twin.stream_snapshot(), "the calls left a trace in the snapshot"
    twin.stream_end()
    twin.close()
    x.close()


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_mode_after_every_tick_with_a_twin(stream_graph, monkeypatch):
    """A waiting stream (no leases): the lease columns are unknown, the demand columns exact."""
    ist._graph(monkeypatch, stream_graph)
    sv = synth.make_servants(60, n_tasks_hint=600 * 3, n_envs=2, seed=42)
    ws, q = WQ.WaitingStream(sv, 600, 80, 1500, n_envs=2), WQ.WaitQueue(1500)
    ctx, twin = wg.begin(ws.es, 1500, 80, 600), wg.begin(ws.es, 1500, 80, 600)
    waited = 0
    for t in range(8):
        tick = ws.next_tick()
        now, who, rows, rel, tk, dl, tags = tick
        want = q.tick(WQ.oracle_place(ws.es), tk, dl, tags, now)
        got_twin = twin.stream_tick_waiting(who, rows, rel, tk, dl, tags, now)
        got = ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, now)
        wg.check_tick(t, ctx, ws, q, tick, got, want)
        same_answers(got, got_twin, "tick %d" % t)
        assert np.array_equal(ctx.get_running(), twin.get_running()), t
        model, un = QM.fold(None, OM.waiting(q))
        g = check(ctx, model, un, tk["requestor_ip"][:50], "tick %d" % t)
        assert un == UNKNOWN and all((g[k] == UNKNOWN).all() for k in ("leases", "zombies", "prefetch_leases"))
        assert np.array_equal(g["waiting"], g["waiting_rows"]) and int(g["waiting"].sum()) == len(q)
        same_rows(g, QM.fold(None, ctx.stream_waiting())[0], "tick %d: the getter" % t)
        waited += len(q)
    assert waited > 500
    assert ctx.stream_snapshot() == twin.stream_snapshot()
    for c in (ctx, twin):
        c.stream_end()
        c.close()


# ---- the table: sizes, the sentinel, stale records, the hot key ----------------------------------

@pytest.mark.parametrize("R", [511, 512, 513, 5000])
def test_distinct_requestors_around_the_first_growth_of_the_table(R):
    """One lease per requestor: 2 R entries fill the smallest table (1 024 slots) at R = 512 and take
    the next size at 513; 5 000 requestors need 16 384 slots."""
    ctx = uploaded(roomy_registry())
    ctx.stream_begin_leased(8, 8, R, 2 * R, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    rng = np.random.default_rng(R)
    ips = np.unique(np.concatenate([rng.integers(1, 0xFFFFFFFE, R + 64, dtype=np.uint64).astype(np.uint32), [1, 0xFFFFFFFD]]))[:R]
    ips = ips[rng.permutation(R)].astype(np.uint32)
    assert len(ips) == R
    _, n_leases = leased_tick(ctx, 1, ips)
    assert n_leases == R
    want = np.zeros(R, QM.DTYPE)
    want["requestor_ip"], want["leases"] = np.sort(ips), 1
    g = check(ctx, want, 0, what="%d requestors" % R)
    same_rows(g, QM.fold(ctx.stream_inspect_tasks(), None)[0], "the getter")
    ctx.stream_end()
    ctx.close()


def test_the_sentinel_is_a_requestor_and_early_leases_belong_to_nobody():
    """Leases granted before ydc_stream_inspect_begin are counted in `unattributed` alone; a request
    from requestor 0xFFFFFFFF granted afterwards is counted under that key. Both in one stream."""
    ctx = uploaded(roomy_registry())
    ctx.stream_begin_leased(8, 8, 128, 512, 8, 8, 8, 8)
    A, ALL = 0x0A000001, 0xFFFFFFFF
    leased_tick(ctx, 1, [A] * 50)
    got, un = ctx.stream_requestors()  # inspection off: nobody's lease is known
    assert len(got) == 0 and un == UNKNOWN
    f, un = ctx.stream_requestor_find([A, ALL])
    assert un == UNKNOWN and all((f[k] == UNKNOWN).all() for k in ("leases", "zombies", "prefetch_leases"))
    assert not f["waiting"].any() and f["requestor_ip"].tolist() == [A, ALL]
    ctx.stream_inspect_begin()
    got, un = ctx.stream_requestors()
    assert len(got) == 0 and un == 50
    f, un = ctx.stream_requestor_find([ALL, A])
    assert un == 50 and not any(f[k].any() for k in QM.COLUMNS)
    leased_tick(ctx, 2, [ALL] * 30 + [A] * 20)
    want = np.zeros(2, QM.DTYPE)
    want["requestor_ip"], want["leases"] = [A, ALL], [20, 30]
    g = check(ctx, want, 50, what="after the second tick")
    model, model_un = QM.fold(ctx.stream_inspect_tasks(), None)
    same_rows(g, model, "the getter")
    assert model_un == 50
    ctx.stream_end()
    ctx.close()


def test_erased_leases_leave_no_trace():
    """200 leases of one requestor, all freed by id in the next tick: every count is 0 and get has no
    row, although the slots still hold their records. Leases of another requestor then reuse slots:
    only that one appears."""
    ctx = uploaded(roomy_registry())
    ctx.stream_begin_leased(8, 8, 256, 256, 8, 256, 8, 8)
    ctx.stream_inspect_begin()
    A, B = 0x0A000001, 0x0A000002
    ids, n_leases = leased_tick(ctx, 1, [A] * 200)
    assert n_leases == 200
    assert check(ctx, QM.fold(ctx.stream_inspect_tasks(), None)[0], 0, what="granted")["leases"].tolist() == [200]
    _, n_leases = leased_tick(ctx, 2, [], free_ids=ids)
    assert n_leases == 0
    got, un = ctx.stream_requestors()
    assert len(got) == 0 and un == 0
    f, _ = ctx.stream_requestor_find([A, B])
    assert not any(f[k].any() for k in QM.COLUMNS)
    _, n_leases = leased_tick(ctx, 3, [B] * 230)  # (230 of 512 slots: some of the 200 are taken again)
    assert n_leases == 230
    want = np.zeros(1, QM.DTYPE)
    want["requestor_ip"], want["leases"] = [B], [230]
    check(ctx, want, 0, [A], "granted again")
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("combine", [None, "0"])
def test_hot_key_and_the_shapes_of_a_wave(combine, monkeypatch):
    """One requestor holds 4 096 leases and another one 1; in W, where entry i is thread i's, a wave
    of 64 distinct requestors, and one whose requestor changes in mid-wave. With equal requestors
    combined inside the wave (the default) and with an atomic per entry (requestor_combine=0)."""
    if combine is not None:
        monkeypatch.setenv("YDC_REQUESTOR_COMBINE", combine)
    A, B = 0xC0A80001, 0xC0A80002
    ctx = uploaded(roomy_registry())
    ctx.stream_begin_leased(8, 8, 4100, 8192, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    rng = np.random.default_rng(3)
    ips = np.full(4097, A, np.uint32)
    ips[rng.integers(4097)] = B
    leased_tick(ctx, 1, ips, lease_for=5)
    leased_tick(ctx, 20, [])  # (all of them zombies now)
    want = np.zeros(2, QM.DTYPE)
    want["requestor_ip"], want["leases"], want["zombies"] = [A, B], [4096, 1], [4096, 1]
    g = check(ctx, want, 0, what="4 096 + 1")
    same_rows(g, QM.fold(ctx.stream_inspect_tasks(), None)[0], "the getter")
    ctx.stream_end()
    ctx.close()
    # W of a saturated rpc stream: position i of W is lane i % 64 of a wave.
    ctx = uploaded(saturated_registry())
    ctx.stream_begin_rpc(8, 16, 256, 1 << 12, 256, 1 << 12, 8, 8, 8, 8)
    w = rpc_requests(0x0B000000 + rng.permutation(64).astype(np.uint32), 1, rng)  # 64 lanes, 64 requestors
    r = rpc_tick(ctx, 10, w)
    assert (r["status"] == WAITING).all() and r["n_waiting"] == 64
    model, un = QM.fold(None, ctx.stream_waiting())
    assert len(model) == 64 and un == UNKNOWN
    check(ctx, model, un, what="64 distinct requestors in a wave")
    more = rpc_requests([A] * 40 + [B] * 24, 100, rng)  # the second wave: the requestor changes at lane 40
    r = rpc_tick(ctx, 11, more)
    assert (r["status"] == WAITING).all() and r["n_waiting"] == 128
    model, un = QM.fold(None, ctx.stream_waiting())
    g = check(ctx, model, un, what="the requestor changes in mid-wave")
    at = {int(ip): i for i, ip in enumerate(g["requestor_ip"])}
    assert g["waiting"][at[A]] == 40 and g["waiting"][at[B]] == 24 and len(g) == 66
    assert g["waiting_rows"][at[A]] == int(more["n_immediate"][:40].sum() + more["n_prefetch"][:40].sum())
    assert int(g["waiting_rows"].sum()) == r["n_waiting_rows"]
    ctx.stream_end()
    ctx.close()


def test_waiting_queue_edges_on_a_saturated_rpc_stream():
    """|W| = 0, 1, 1023, 1024, 1025 from three requestors with mixed n_immediate / n_prefetch: entries
    and rows per requestor, the rows summed against the tick's own count. The entry whose deadline is
    the nearest is counted as long as ydc_stream_inspect_waiting lists it."""
    ctx = uploaded(saturated_registry())
    ctx.stream_begin_rpc(8, 16, 1100, 1 << 13, 1100, 1 << 14, 8, 8, 8, 8)
    three = np.array([0x0A000001, 0x0A000002, 0xFFFFFFFF], np.uint32)
    rng = np.random.default_rng(7)
    n, rows = 0, 0
    for t, add in enumerate((0, 1, 1022, 1, 1)):
        if add:
            req = rpc_requests(rng.choice(three, add), 1 + n, rng)
            if n == 0:
                req["deadline"][0] = 12  # (one unit ahead of the ticks' clock: about to expire, still in W)
                first = req
            r = rpc_tick(ctx, 11, req)
            assert (r["status"] == WAITING).all() and r["n_waiting"] == n + add
            n, rows = n + add, r["n_waiting_rows"]
        assert n == (0, 1, 1023, 1024, 1025)[t]
        view = ctx.stream_waiting()
        assert len(view["tag"]) == n and (n == 0 or view["deadline"][0] == 12)
        model, un = QM.fold(None, view)
        g = check(ctx, model, un, three, "|W| = %d" % n)
        assert un == UNKNOWN and int(g["waiting"].sum()) == n and int(g["waiting_rows"].sum()) == rows
        assert set(g["requestor_ip"].tolist()) <= set(three.tolist())
    assert len(g) == 3 and int(first["requestor_ip"][0]) in g["requestor_ip"].tolist()
    # Inspection on: the lease columns become known (nobody holds a lease), W's stay.
    ctx.stream_inspect_begin()
    model["leases"] = model["zombies"] = model["prefetch_leases"] = 0
    check(ctx, model, 0, three, "with inspection")
    ctx.stream_end()
    ctx.close()


# ---- the registry changes, the stream grows, the stream moves -------------------------------------

def test_after_removal_reserve_and_restore():
    ws = ist.stream("rpc", ist.pool(96, seed=5, hint=ist.POOL_HINT["rpc"] // 2))
    x = ist.Inspected("rpc", ws, ist.begin("rpc", ws))
    ask = lambda what, ctx=None: check(ctx or x.ctx, *QM.stream_fold(ws, x.I), what=what)
    for _ in range(4):
        x.tick(ws.next_tick(), snapshot=False)
    removed = np.array([0, 17, 63, 64, 95], np.uint32)
    before = int(ask("before")["leases"].sum())
    assert sum(1 for e in ws.table.L.values() if e[0] in set(removed.tolist())) > 0
    x.ctx.remove_servants(removed)
    lease.drop_rows(ws, removed)
    assert int(ask("after ydc_remove_servants")["leases"].sum()) < before
    x.tick(ws.next_tick(), snapshot=False)
    ask("a tick later")
    caps = x.ctx.stream_caps()
    ws.state.max_waiting, ws.state.max_rows = 2 * caps["max_waiting"], 2 * caps["max_rows"]
    x.ctx.stream_reserve(max_waiting=ws.state.max_waiting, max_rows=ws.state.max_rows, max_leases=2 * caps["max_leases"])
    ask("after ydc_stream_reserve")  # (L was filed again into a larger table, the records with it)
    x.tick(ws.next_tick(), snapshot=False)
    g = ask("a tick after it")
    assert len(ws.state.q) and len(ws.table.L) and g["waiting"].any() and g["leases"].any()
    blob, sv_cols, tk_cols = x.ctx.stream_snapshot(), x.ctx.stream_inspect_servants(), x.ctx.stream_inspect_tasks()
    b = binding.Context(device=0)
    b.stream_restore(blob)
    check(b, *QM.stream_fold(ws, None), what="after ydc_stream_restore")  # (inspection is off there)
    b.stream_inspect_begin(sv_cols["discovered_at"], sv_cols["ever_assigned"])
    rows, un = b.stream_requestors()
    assert un == len(ws.table.L) and not (rows["leases"] != 0).any()  # (every lease is without a record)
    b.stream_inspect_load(**tk_cols)
    ask("after ydc_stream_inspect_load", b)
    assert b.stream_snapshot() == blob
    b.stream_end()
    b.close()
    x.close()


def test_after_an_aliveness_expiry():
    """Servants run out inside ticks: the orphans' leases are erased without the zombie stage and
    count for nobody from that tick on."""
    sv = ist.pool(70, seed=3)
    ws = ist.stream("leased", sv)
    ctx = ist.begin("leased", ws)
    first = AM.first_expiries(70, life=4)
    AM.attach(ws, first)
    ctx.stream_alive_begin(first)
    x = ist.Inspected("leased", ws, ctx, alive=True)
    gen = AM.AliveGen(ws, life=4, p_stop=0.3, p_short=0.3, seed=3)
    removed = orphans = 0
    for t in range(10):
        _, want = x.tick(gen.next_tick(), snapshot=False)
        removed += len(want["removed"])
        orphans += want["orphans"]
        check(x.ctx, *QM.stream_fold(ws, x.I), what="tick %d" % t)
    assert removed >= 2 and orphans > 0, (removed, orphans)
    x.close()


# ---- the contract ------------------------------------------------------------------------------

def test_contract_and_refusals():
    sv = ist.pool(64, seed=5)
    ctx = uploaded(sv)
    L_ = binding.lib()
    one, row = np.array([5], np.uint32), np.zeros(1, QM.DTYPE)
    n, un = C.c_uint32(77), C.c_uint32(77)
    for what in ("no stream", "a plain stream"):
        with pytest.raises(binding.YdcError, match="no stream is open" if what == "no stream" else "keeps no state"):
            ctx.stream_requestor_find([1])
        with pytest.raises(binding.YdcError):
            ctx.stream_requestors()
        assert L_.ydc_stream_requestor_find(ctx._h, None, 0, None, None) == INVALID, what  # (even without a query)
        assert L_.ydc_stream_requestor_get(ctx._h, None, 0, C.byref(n), None) == INVALID and n.value == 0, what
        if what == "no stream":
            ctx.stream_begin(8, 8, 16)
    ctx.stream_end()
    ctx.close()
    ctx = uploaded(roomy_registry())
    ctx.stream_begin_leased(8, 8, 64, 256, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    ips = np.array([9, 7, 9, 3, 7, 9, 1, 0xFFFFFFFF], np.uint32)
    leased_tick(ctx, 1, ips)
    h = ctx._h
    # n == 0 is a call like any other; NULL columns are allowed with it.
    assert L_.ydc_stream_requestor_find(h, None, 0, None, None) == 0
    assert L_.ydc_stream_requestor_find(h, None, 0, None, C.byref(un)) == 0 and un.value == 0
    got, _ = ctx.stream_requestor_find([])
    assert len(got) == 0 and got.dtype == QM.DTYPE
    # n > 0 with a NULL column, 2^24 + 1 queries, a NULL out_n.
    assert L_.ydc_stream_requestor_find(h, None, 1, row.ctypes.data, None) == INVALID
    assert L_.ydc_stream_requestor_find(h, one.ctypes.data, 1, None, None) == INVALID
    assert L_.ydc_stream_requestor_find(h, one.ctypes.data, (1 << 24) + 1, row.ctypes.data, None) == INVALID
    assert "2^24" in L_.ydc_last_error(h).decode()
    assert L_.ydc_stream_requestor_get(h, row.ctypes.data, 1, None, None) == INVALID
    # Repeated queries answer alike and echo the query.
    q = np.array([9, 9, 4, 7, 9, 4], np.uint32)
    f, _ = ctx.stream_requestor_find(q)
    assert f["requestor_ip"].tolist() == q.tolist() and f["leases"].tolist() == [3, 3, 0, 2, 3, 0]
    # cap one too small: *out_n is set and nothing is written.
    room = np.full(5, 0xAB, np.uint8).repeat(24).view(QM.DTYPE)
    before = room.tobytes()
    rc = L_.ydc_stream_requestor_get(h, room.ctypes.data, 4, C.byref(n), C.byref(un))
    assert rc == CAPACITY and n.value == 5 and room.tobytes() == before
    rc = L_.ydc_stream_requestor_get(h, room.ctypes.data, 5, C.byref(n), C.byref(un))
    assert rc == 0 and n.value == 5 and un.value == 0
    assert sorted(zip(room["requestor_ip"].tolist(), room["leases"].tolist())) == [(1, 1), (3, 1), (7, 2), (9, 3), (0xFFFFFFFF, 1)]
    assert L_.ydc_stream_requestor_get(h, None, 0, C.byref(n), None) == CAPACITY and n.value == 5  # (how the wrapper asks)
    # Pipelined batches outstanding.
    DA = binding.DeviceArray
    tk = synth.make_tasks(256, sv, n_envs=2)
    cols = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
    d_out = DA.from_numpy(np.zeros(256, np.uint32))
    ctx.dispatch_device_async(*cols, d_out)
    for call in (lambda: ctx.stream_requestor_find([9]), ctx.stream_requestors):
        with pytest.raises(binding.YdcError, match="pipelined"):
            call()
    ctx.dispatch_wait()
    assert ctx.stream_requestor_find([9])[0]["leases"].tolist() == [3]
    ctx.stream_end()
    with pytest.raises(binding.YdcError, match="no stream is open"):
        ctx.stream_requestors()
    ctx.close()
    # The clip itself: an unknown load is refused, NULL prefetch columns mean zeros.
    load = np.zeros(2, QM.DTYPE)
    load["leases"] = [UNKNOWN, 0]
    with pytest.raises(binding.YdcError):
        binding.admit_clip([1, 2], [1, 1], None, load, 4)
    load["leases"] = [3, 3]
    imm, pre = binding.admit_clip([1, 1], [2, 2], None, load, 4)
    assert imm.tolist() == [1, 0] and not pre.any()
    assert L_.ydc_admit_clip(None, None, None, 0, None, 4, None, None) == 0
    assert L_.ydc_admit_clip(None, one.ctypes.data, None, 1, load.ctypes.data, 4, one.ctypes.data, None) == INVALID


def test_calls_between_dispatch_ticks_and_the_resident_kernel():
    """ydc_dispatch_tick leaves its kernel resident only while no stream is open (an open stream
    takes the turn off the one-workgroup kernel), so the read calls, which end a resident kernel first
    as the outlook's do, never meet a live one. Without a stream they are refused and the resident
    sequence goes on, exact; from the begin call on tick_resident_calls stops growing, and every
    ydc_dispatch_tick between the calls stays exact."""
    sv = roomy_registry(40)
    ctx = uploaded(sv)
    sv = {k: np.array(v, copy=True) for k, v in sv.items()}

    def tick(seed):
        tk = synth.make_tasks(1, sv, n_envs=3, seed=seed, self_frac=0.0)
        want, _, wrun = O.dispatch(sv, tk, "scan")
        got, _ = ctx.dispatch_tick(tk, commit=True)
        assert np.array_equal(got, want), seed
        sv["running_tasks"] = wrun
        st = ctx.stats()
        return st["tick_resident_calls"], st["tick_launched_calls"]

    tick(1)
    r1, l1 = tick(2)
    r2, l2 = tick(3)
    assert (r2, l2) == (r1 + 1, l1), "the tick kernel did not stay resident"
    with pytest.raises(binding.YdcError, match="no stream is open"):
        ctx.stream_requestor_find([5])
    r3, l3 = tick(4)
    assert r3 + l3 == r2 + l2 + 1
    ctx.stream_begin_leased(8, 8, 64, 256, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    leased_tick(ctx, 1, [5, 6, 5])
    sv["running_tasks"] = ctx.get_running().astype(sv["running_tasks"].dtype)
    tick(5)
    f, un = ctx.stream_requestor_find([5, 6])
    assert f["leases"].tolist() == [2, 1] and un == 0
    tick(6)
    rows, _ = ctx.stream_requestors()
    assert rows["leases"].tolist() == [2, 1]
    r4, l4 = tick(7)
    assert (r4, l4) == (r3, l3), "a resident tick kernel beside an open stream"
    assert np.array_equal(ctx.get_running(), sv["running_tasks"])
    ctx.stream_end()
    ctx.close()


# ---- end to end: a fair share at the door ---------------------------------------------------------

def test_admit_keeps_a_greedy_requestor_at_its_cap():
    """6 rpc ticks; requestor G asks for 20 grants in each, requestor H for one. With cap = 8 G never has
    more than 8 grants outstanding (leases, zombies included, plus the rows it waits for), H's requests
    are never reduced, and the ticks answer exactly what the model answers for the clipped requests:
    the tick itself is unchanged."""
    G, H, CAP = 0xC0A80A0A, 0xC0A80A0B, 8
    ws = RM.new_stream(ist.pool(64, seed=11, hint=300), 30, 20, 10, 400, 4096, n_envs=2, report_frac=0.3,
                       rate=lambda now: 1.0)
    ws.es.hb = 16
    x = ist.Inspected("rpc", ws, rpc.begin(ws, 40))
    asked = admitted = held_most = 0
    for t in range(6):
        ev = ws.next_tick()
        k = len(ev["tags"])
        assert G not in ev["tasks"]["requestor_ip"] and H not in ev["tasks"]["requestor_ip"]
        at = [k // 2, k]  # (G in the middle of the batch, H at its end)
        ev["tasks"] = {"env_id": np.insert(ev["tasks"]["env_id"], at, [0, 0]).astype(np.uint32),
                       "min_version": np.insert(ev["tasks"]["min_version"], at, [0, 0]).astype(np.uint32),
                       "requestor_ip": np.insert(ev["tasks"]["requestor_ip"], at, [G, H]).astype(np.uint32)}
        ev["n_immediate"] = np.insert(ev["n_immediate"], at, [12, 1]).astype(np.uint32)
        ev["n_prefetch"] = np.insert(ev["n_prefetch"], at, [8, 0]).astype(np.uint32)
        ev["lease_for"] = np.insert(ev["lease_for"], at, [40, 40]).astype(np.int64)
        ev["deadlines"] = np.insert(ev["deadlines"], at, [int(ev["now"]) + 3] * 2).astype(np.int64)
        ev["tags"] = np.insert(ev["tags"], at, [(1 << 40) + 2 * t, (1 << 40) + 2 * t + 1]).astype(np.uint64)
        ips = ev["tasks"]["requestor_ip"]
        before, _ = x.ctx.stream_requestor_find(ips)
        imm, pre, keep = streaming.admit(x.ctx, ev["tasks"], ev["n_immediate"], ev["n_prefetch"], CAP)
        want_imm, want_pre = QM.admit_clip(ips, ev["n_immediate"], ev["n_prefetch"], before, CAP)
        assert np.array_equal(imm, want_imm) and np.array_equal(pre, want_pre) and np.array_equal(keep, imm + pre > 0)
        h = ips == H
        assert imm[h].tolist() == [1] and pre[h].tolist() == [0] and keep[h].all(), "H was reduced"
        g = ips == G
        asked += 20
        admitted += int(imm[g].sum() + pre[g].sum())
        ev["tasks"] = {c: v[keep] for c, v in ev["tasks"].items()}
        ev["n_immediate"], ev["n_prefetch"] = imm[keep], pre[keep]
        for c in ("lease_for", "deadlines", "tags"):
            ev[c] = ev[c][keep]
        x.tick(ev, snapshot=False)  # (the device's answers against stream_rpc_model fed the clipped requests)
        load, _ = x.ctx.stream_requestor_find([G, H])
        held = int(load["leases"][0]) + int(load["waiting_rows"][0])
        assert held <= CAP, "tick %d: G holds %d" % (t, held)
        held_most = max(held_most, held)
        check(x.ctx, *QM.stream_fold(ws, x.I), what="tick %d" % t)
    assert 0 < admitted < asked and held_most == CAP, (admitted, asked, held_most)
    x.close()

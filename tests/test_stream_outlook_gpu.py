"""The outlook per request personality and the view of the waiting queue on the device
(ydc_stream_outlook_get / ydc_stream_inspect_waiting; stream_outlook.h: k_outlook_classes, _queries,
_waiting, _leases) against the model (tests/stream_outlook_model.py, pinned against the verbatim
reference by tests/test_stream_outlook_model.py): integer equality on every column, in every mode,
beside a twin context that never asks and must answer every tick identically."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_outlook_model as OM
from tests import stream_rpc_model as RM
from tests import stream_wait_model as WQ
from tests import test_stream_inspect_gpu as ist
from tests import test_stream_lease_gpu as lease
from tests import test_stream_waiting_gpu as wg
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu
LDS_CLASSES = 256  # kOutlookLdsClasses
LDS_BINS = 2048    # kOutlookLdsBins
WAITING = binding.IDX_WAITING
E32, E64, I64 = np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.int64)
NO_ROWS = np.empty(0, binding.ROW_DTYPE)


def queries(n_envs, versions=(0, 20), extra=()):
    """Every digest x every min_version, plus ids nobody has."""
    env = list(range(n_envs)) + list(extra)
    return (np.repeat(np.array(env, np.uint32), len(versions)), np.tile(np.array(versions, np.uint32), len(env)))


def same(got, want, what=""):
    for k in OM.COLUMNS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, "%s: %s: query %d gpu %s model %s (%d differ)" % (
            what, k, bad[0], got[k][bad[0]], want[k][bad[0]], bad.size)


def same_waiting(got, want, what=""):
    assert set(got) == set(OM.WAITING_COLUMNS)
    for k in OM.WAITING_COLUMNS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])


def same_answers(a, b, what=""):
    if isinstance(a, dict):
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a), what
    else:
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), what


# ---- every mode, every tick, beside a twin that never asks -------------------------------------

@pytest.mark.parametrize("mode,stream_graph", [(m, g) for m in ist.MODS for g in ("1", "0")])
def test_each_lease_mode_after_every_tick_with_a_twin(mode, stream_graph, monkeypatch):
    """12 ticks of a leased, waiting-and-leased or rpc stream with inspection on; the outlook of every
    digest x two min_versions (and of two ids nobody has) and W after each. The twin gets the same
    ticks and never asks: identical answers, lease snapshot and running_tasks."""
    ist._graph(monkeypatch, stream_graph)
    ws = ist.stream(mode, ist.pool(96, seed=5, hint=ist.POOL_HINT[mode] // 2))
    x = ist.Inspected(mode, ws, ist.begin(mode, ws))
    twin = ist.begin(mode, ws) if mode == "leased" else ist.begin(mode, ws, ctx=_uploaded(ws.es.sv))
    twin.stream_inspect_begin()
    env, minv = queries(2, extra=(2, 64, 0xFFFF))
    seen = dict(zombies=0, waiting=0, expired=0, swept=0, leases=0)
    for t in range(12):
        ev = ws.next_tick()
        got_twin = x.G.gpu_tick(twin, ws, ev)
        got, want = x.tick(ev, snapshot=False)
        same_answers(got, got_twin, "tick %d" % t)
        same_answers(x.ctx.stream_leases(), twin.stream_leases(), "tick %d: lease snapshot" % t)
        assert np.array_equal(x.ctx.get_running(), twin.get_running()), t
        o = x.ctx.stream_outlook(env, minv)
        same(o, OM.stream_outlook(ws, env, minv, inspect=x.I), "tick %d" % t)
        same_waiting(x.ctx.stream_waiting(), OM.stream_waiting(ws), "tick %d" % t)
        seen["zombies"] += int(o["zombies"][:4:2].sum())
        seen["leases"] += int(o["leases"][:4:2].sum())
        seen["waiting"] += int(o["waiting"][:4:2].sum())
        seen["expired"] += want["expired"]
        seen["swept"] += want["swept"]
        if mode == "rpc":
            assert int(o["waiting_rows"][:4:2].sum()) == got["n_waiting_rows"], t
    # (a tick that made zombies and one that swept some were among them; the modes with W had waiters)
    assert seen["zombies"] and seen["expired"] and seen["swept"] and seen["leases"], seen
    assert (seen["waiting"] > 0) == (mode != "leased"), seen
    twin.stream_end()
    twin.close()
    x.close()


def _uploaded(sv):
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(sv))
    return ctx


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_waiting_mode_after_every_tick_with_a_twin(stream_graph, monkeypatch):
    """A waiting stream (no leases): supply and W's histogram; leases / zombies are unknown."""
    ist._graph(monkeypatch, stream_graph)
    sv = synth.make_servants(60, n_tasks_hint=600 * 3, n_envs=2, seed=42)
    ws, q = WQ.WaitingStream(sv, 600, 80, 1500, n_envs=2), WQ.WaitQueue(1500)
    ctx, twin = wg.begin(ws.es, 1500, 80, 600), wg.begin(ws.es, 1500, 80, 600)
    env, minv = queries(2, extra=(2, 64))
    waited = 0
    for t in range(12):
        tick = ws.next_tick()
        now, who, rows, rel, tk, dl, tags = tick
        want = q.tick(WQ.oracle_place(ws.es), tk, dl, tags, now)
        got_twin = twin.stream_tick_waiting(who, rows, rel, tk, dl, tags, now)
        got = ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, now)
        wg.check_tick(t, ctx, ws, q, tick, got, want)
        same_answers(got, got_twin, "tick %d" % t)
        assert np.array_equal(ctx.get_running(), twin.get_running()), t
        o = ctx.stream_outlook(env, minv)
        same(o, OM.outlook(ws.es.sv, ws.es.abi["flags"], ws.es.running, env, minv,
                           queue=(q.cols["env_id"], np.ones(len(q), np.int64))), "tick %d" % t)
        assert (o["leases"] == binding.OUTLOOK_UNKNOWN).all() and (o["waiting"] == o["waiting_rows"]).all()
        same_waiting(ctx.stream_waiting(), OM.waiting(q), "tick %d" % t)
        waited += int(o["waiting"][:4:2].sum())
    assert waited > 500
    for c in (ctx, twin):
        c.stream_end()
        c.close()


# ---- the registry pass: wave, workgroup and class-count edges ----------------------------------

def direct(sv, env, minv):
    """The outlook of a registry as uploaded, on a leased stream without a tick -> (gpu, model)."""
    abi = pack.to_abi_columns(sv)
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    ctx.stream_begin_leased(8, 8, 16, 64, 8, 8, 8, 8)
    got = ctx.stream_outlook(env, minv)
    want = OM.outlook(sv, abi["flags"], sv["running_tasks"], env, minv, queue=None, leases=None)
    ctx.stream_end()
    ctx.close()
    return got, want


@pytest.mark.parametrize("S", [0, 1, 63, 64, 65, 257, 1025])
def test_registry_edges(S):
    """Servants cycling through every branch of GetCapacityAvailable, at the edges of a wave and of a
    workgroup, and no servant at all."""
    sv = ist.pathological(max(S, 1))
    sv = {k: v[:S] for k, v in sv.items()}
    env, minv = queries(2, versions=(0, 19, 20, 21), extra=(2, 63, 64))
    got, want = direct(sv, env, minv)
    same(got, want, "S = %d" % S)
    assert (got["leases"] == binding.OUTLOOK_UNKNOWN).all() and not got["waiting"].any()
    if S >= 63:
        assert got["eligible"][0] > got["free_servants"][0] > 0 and got["grants_available"][0] > 0


def test_no_servant_accepts_tasks():
    sv = ist.pathological(200)
    sv["max_tasks"][:] = 0
    env, minv = queries(2)
    got, want = direct(sv, env, minv)
    same(got, want)
    assert not any(got[k].any() for k in OM.COLUMNS[:6])


@pytest.mark.parametrize("n_classes", [1, LDS_CLASSES - 1, LDS_CLASSES, LDS_CLASSES + 1])
def test_class_count_edges(n_classes):
    """One version per servant makes a class each: the per-workgroup table in LDS at its bound, and
    the plain global atomics one class above it."""
    S = n_classes + 300  # (more than one workgroup; the first 300 classes have two members)
    sv = ist.pathological(S, seed=3)
    sv["max_tasks"] = np.maximum(sv["max_tasks"], 1)
    sv["env_mask"][:] = 3
    sv["version"] = (100 + np.arange(S) % n_classes).astype(sv["version"].dtype)
    top = 100 + n_classes
    versions = sorted({0, 100, 101, 100 + n_classes // 2, top - 2, top - 1, top})
    env, minv = queries(2, versions=versions)
    got, want = direct(sv, env, minv)
    same(got, want, "%d classes" % n_classes)
    assert got["eligible"][0] == S and got["eligible"][len(versions) - 1] == 0
    assert got["eligible"][len(versions) - 2] == int((sv["version"] >= versions[-2]).sum()) > 0


def test_wide_masks():
    """150 digests in three mask words: a query in every word, the last bit of the last word, and
    the first id behind the table."""
    sv = synth.make_servants(200, n_tasks_hint=4000, n_envs=150, seed=7)
    assert sv["env_mask"].shape == (200, 3)
    sv["env_mask"][5, 2] |= np.uint64(1) << np.uint64(63)  # digest 191
    sv["max_tasks"][5] = max(int(sv["max_tasks"][5]), 2)
    env, minv = queries(150, extra=(150, 191, 192, 0xFFFF))
    got, want = direct(sv, env, minv)
    same(got, want)
    at = {e: 2 * i for i, e in enumerate(list(range(150)) + [150, 191, 192, 0xFFFF])}  # (its row at min_version 0)
    assert got["eligible"][at[191]] == 1
    assert got["eligible"][at[64]:at[128]].any() and got["eligible"][at[128]:at[150]].any()  # (every word has takers)
    assert not any(got[k][at[192]] for k in OM.COLUMNS[:8]) and not any(got[k][at[150]] for k in OM.COLUMNS[:8])


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_query_counts_duplicates_and_versions_nobody_has(n):
    sv = ist.pathological(65)
    rng = np.random.default_rng(n)
    env = rng.integers(0, 3, n).astype(np.uint32)  # (three values in up to 65 places: duplicates)
    minv = rng.choice(np.array([0, 20, 1000], np.uint32), n)
    got, want = direct(sv, env, minv)
    same(got, want, "n = %d" % n)
    assert all(len(got[k]) == n for k in OM.COLUMNS)
    assert not got["eligible"][minv == 1000].any()
    if n == 65:
        first = {}
        for i, key in enumerate(zip(env.tolist(), minv.tolist())):
            j = first.setdefault(key, i)
            assert all(got[k][i] == got[k][j] for k in OM.COLUMNS)
        assert len(first) < n


def test_sums_are_64_bit():
    sv = ist.pathological(2)
    for k, v in (("num_processors", 0xFFFFFFFF), ("max_tasks", 0xFFFFFFFF), ("current_load", 0), ("version", 20)):
        sv[k][:] = v
    sv["running_tasks"][:] = (0, 1)
    sv["env_mask"][:] = 1
    sv["memory_available"][:] = 32 << 30
    got, want = direct(sv, [0], [0])
    same(got, want)
    assert int(got["max_tasks"][0]) == 2 * 0xFFFFFFFF == int(got["capacity_available"][0])
    assert int(got["grants_available"][0]) == 2 * 0xFFFFFFFF - 1 and got["eligible"][0] == got["free_servants"][0] == 2


# ---- W: a saturated rpc stream, scripted ---------------------------------------------------------

def saturated_registry(words):
    """8 servants that run all they take; digests 0 - 2 everywhere, with `words` > 1 also 64 * words - 1
    (the last bit of the table) and 1000 on servant 0."""
    sv = synth.make_servants(8, n_tasks_hint=64, n_envs=3, seed=1)
    sv["version"][:], sv["num_processors"][:], sv["current_load"][:] = 20, 64, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = 2, 2
    sv["memory_available"][:], sv["total_memory"][:] = 32 << 30, 64 << 30
    mask = np.zeros((8, words), np.uint64)
    mask[:, 0] = 7
    if words > 1:
        mask[0, words - 1] |= np.uint64(1) << np.uint64(63)
        mask[0, 1000 // 64] |= np.uint64(1) << np.uint64(1000 % 64)
    sv["env_mask"] = mask[:, 0].copy() if words == 1 else mask
    return sv


def rpc_tick(ctx, now, req):
    n = len(req["env_id"])
    return ctx.stream_tick_rpc(E32, NO_ROWS, E32, E64, I64, E64, E32, np.zeros(1, np.uint32), E64, req,
                               req["n_immediate"], req["n_prefetch"], req["lease_for"], req["deadline"], req["tag"], now)


def requests(rng, n, envs, first_tag):
    return {"env_id": rng.choice(np.array(envs, np.uint32), n), "min_version": rng.choice(np.array([0, 20], np.uint32), n),
            "requestor_ip": ((172 << 24) + rng.integers(0, 1 << 20, n)).astype(np.uint32),
            "n_immediate": rng.choice(RM.NIMM[1:], n), "n_prefetch": rng.choice(RM.NPRE, n),
            "lease_for": rng.integers(1, 90, n).astype(np.int64), "deadline": np.full(n, 1 << 40, np.int64),
            "tag": np.arange(first_tag, first_tag + n, dtype=np.uint64)}


@pytest.mark.parametrize("words", [1, LDS_BINS // 64 + 1])
def test_waiting_queue_edges_on_a_saturated_rpc_stream(words):
    """|W| = 0, 1, 1024, 1025 with mixed n_immediate / n_prefetch: the histogram per digest (in LDS,
    and with 33 mask words = 2113 bins in global memory), waiting_rows against the tick's own count,
    the view of W column for column, its refusal, and that asking empties nothing."""
    sv = saturated_registry(words)
    last = 64 * words - 1
    envs = [0, 1, 2] + ([last, 1000] if words > 1 else [])
    ctx = _uploaded(sv)
    ctx.stream_begin_rpc(8, 16, 1100, 1 << 13, 1100, 1 << 14, 8, 8, 8, 8)
    flags = pack.to_abi_columns(sv)["flags"]
    env, minv = queries(3, extra=(last, 1000 if words > 1 else 40, 64 * words, 0xFFFF))
    rng = np.random.default_rng(words)
    w = {k: v[:0] for k, v in requests(rng, 0, envs, 0).items()}
    L_, n_out = binding.lib(), C.c_uint32(7)
    for t, add in enumerate((0, 1, 1023, 1)):
        if add:
            req = requests(rng, add, envs, 1 + len(w["tag"]))
            r = rpc_tick(ctx, 10 + t, req)
            assert (r["status"] == WAITING).all() and r["n_waiting"] == len(w["tag"]) + add
            w = {k: np.concatenate([w[k], req[k]]) for k in w}
            rows = int(w["n_immediate"].sum() + w["n_prefetch"].sum())
            assert r["n_waiting_rows"] == rows
        n = len(w["tag"])
        assert n == (0, 1, 1024, 1025)[t]
        o = ctx.stream_outlook(env, minv)
        same(o, OM.outlook(sv, flags, sv["running_tasks"], env, minv,
                           queue=(w["env_id"], w["n_immediate"].astype(np.int64) + w["n_prefetch"])), "|W| = %d" % n)
        assert int(o["waiting"][::2].sum()) == n and (o["free_servants"] == 0).all()
        assert n == 0 or int(o["waiting_rows"][::2].sum()) == rows
        view = ctx.stream_waiting()
        for k, col in (("tag", "tag"), ("env_id", "env_id"), ("min_version", "min_version"), ("requestor_ip", "requestor_ip"),
                       ("deadline", "deadline"), ("lease_for", "lease_for"), ("n_immediate", "n_immediate"),
                       ("n_prefetch", "n_prefetch")):
            assert np.array_equal(view[k], w[col]), ("|W| = %d" % n, k)
        if n:  # cap = |W| - 1: the count, and nothing written
            tags = np.full(n, 0xABCD, np.uint64)
            rc = L_.ydc_stream_inspect_waiting(ctx._h, tags.ctypes.data, None, None, None, None, None, None, None, n - 1,
                                               C.byref(n_out))
            assert rc == -4 and n_out.value == n and (tags == 0xABCD).all()
            only = np.zeros(n, np.uint32)  # any output pointer may be NULL
            rc = L_.ydc_stream_inspect_waiting(ctx._h, None, None, None, None, None, None, None, only.ctypes.data, n,
                                               C.byref(n_out))
            assert rc == 0 and n_out.value == n and np.array_equal(only, w["n_prefetch"])
    assert len(set(w["env_id"].tolist())) == len(envs)
    # W is intact: a tick that frees every slot grants the queue's head and whoever else finds a slot,
    # in queue order, and the others stay as they stood.
    r = ctx.stream_tick_rpc(E32, NO_ROWS, np.repeat(np.arange(8, dtype=np.uint32), 2), E64, I64, E64, E32,
                            np.zeros(1, np.uint32), E64, {"env_id": E32, "min_version": E32, "requestor_ip": E32},
                            E32, E32, I64, I64, E64, 20)
    gone = np.isin(w["tag"], r["res_tags"])
    assert gone[0] and np.array_equal(r["res_tags"], w["tag"][gone]) and r["n_waiting"] == 1025 - int(gone.sum())
    assert np.array_equal(ctx.stream_waiting()["tag"], w["tag"][~gone])
    ctx.stream_end()
    ctx.close()


# ---- L: the histograms over the inspection records ------------------------------------------------

@pytest.mark.parametrize("words", [1, LDS_BINS // 64 + 1])
def test_lease_histograms_over_filed_records(words):
    """1 500 leases in two tiles of the pass, a third of them zombies, their records filed with
    ydc_stream_inspect_load: digests of every mask word, ids behind the table and leases without a
    record, which count for no digest."""
    sv = saturated_registry(words)
    sv["running_tasks"][:], sv["max_tasks"][:], sv["num_processors"][:] = 0, 400, 400
    ctx = _uploaded(sv)
    ctx.stream_begin_leased(8, 8, 1600, 4096, 8, 8, 8, 8)
    n = 1500
    rng = np.random.default_rng(5)
    tk = {"env_id": np.zeros(n, np.uint32), "min_version": np.zeros(n, np.uint32),
          "requestor_ip": np.full(n, (172 << 24) + 5, np.uint32)}
    out, ids, _, _, n_leases = ctx.stream_tick_leased(E32, NO_ROWS, E32, E64, I64, E64, E32, np.zeros(1, np.uint32), E64, tk,
                                                      np.where(np.arange(n) % 3 == 0, 5, 500).astype(np.int64), 1)
    assert n_leases == n and (out < 8).all()
    env, minv = queries(3, extra=(64 * words - 1, 1000, 64 * words, 5000))
    same(ctx.stream_outlook(env, minv), OM.outlook(sv, pack.to_abi_columns(sv)["flags"], np.bincount(out, minlength=8),
                                                   env, minv, None, None), "inspection off")
    none = {"env_id": E32, "min_version": E32, "requestor_ip": E32}
    ctx.stream_tick_leased(E32, NO_ROWS, E32, E64, I64, E64, E32, np.zeros(1, np.uint32), E64, none, I64, 100)
    lid, _, _, zombie = ctx.stream_leases()
    assert len(lid) == n and zombie.sum() == 500
    ctx.stream_inspect_begin()
    o = ctx.stream_outlook(env, minv)
    assert not o["leases"].any() and not o["zombies"].any()  # (granted before inspection: no digest)
    rec = rng.choice(np.array([0, 1, 2, 64 * words - 1, 1000, 64 * words, 5000, binding.INSPECT_NO_ID], np.uint32), n)
    rec[:8] = [0, 1, 2, 64 * words - 1, 1000, 64 * words, 5000, binding.INSPECT_NO_ID]
    ctx.stream_inspect_load(lid[100:], env_id=rec[100:])  # (the first hundred keep the sentinel)
    rec[:100] = binding.INSPECT_NO_ID
    o = ctx.stream_outlook(env, minv)
    same(o, OM.outlook(sv, pack.to_abi_columns(sv)["flags"], np.bincount(out, minlength=8), env, minv, None, (rec, zombie)))
    assert 0 < int(o["leases"][::2].sum()) < n and 0 < int(o["zombies"][::2].sum()) < 500
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("mode", ["leased", "rpc"])
def test_inspection_begun_late(mode):
    """Unknown before the begin call; afterwards the earlier leases count for no digest."""
    ws = ist.stream(mode, ist.pool(96, seed=5, hint=ist.POOL_HINT[mode] // 2))
    x = ist.Inspected(mode, ws, ist.begin(mode, ws), begin_now=False)
    env, minv = queries(2)
    for _ in range(3):
        x.tick(ws.next_tick(), snapshot=False)
    o = x.ctx.stream_outlook(env, minv)
    same(o, OM.stream_outlook(ws, env, minv, inspect=None), "before")
    assert (o["leases"] == binding.OUTLOOK_UNKNOWN).all() and (o["zombies"] == binding.OUTLOOK_UNKNOWN).all()
    x.inspect_begin()
    assert len(ws.table.L) > 50 and not x.ctx.stream_outlook(env, minv)["leases"].any()
    for _ in range(3):
        x.tick(ws.next_tick(), snapshot=False)
    o = x.ctx.stream_outlook(env, minv)
    same(o, OM.stream_outlook(ws, env, minv, inspect=x.I), "after")
    assert 0 < int(o["leases"][::2].sum()) < len(ws.table.L)
    x.close()


# ---- the prediction held against the tick ----------------------------------------------------------

def test_the_next_tick_grants_exactly_grants_available():
    """40 servants with load of their own and tasks running; for three personalities from a host
    that owns no servant, one RPC asking for grants_available + 3 rows with its deadline at now is
    granted exactly grants_available."""
    sv = synth.make_servants(40, n_tasks_hint=400, n_envs=3, seed=9)
    rng = np.random.default_rng(9)
    sv["running_tasks"] = (rng.random(40) * (sv["max_tasks"] + 1)).astype(sv["running_tasks"].dtype)
    sv["current_load"] = np.minimum(sv["current_load"], sv["num_processors"] - 1).astype(sv["current_load"].dtype)
    sv["current_load"][:4] = sv["num_processors"][:4] + 2
    abi = pack.to_abi_columns(sv)
    slots = int(np.minimum(sv["max_tasks"], sv["num_processors"]).sum())
    ctx = _uploaded(sv)
    ctx.stream_begin_rpc(8, 8, 4, slots + 8, 8, 2 * slots + 16, 8, 8, 8, 8)  # (max_rows has room for the largest ask)
    asked = 0
    for t, (env, minv) in enumerate(((0, 20), (1, 0), (2, 20), (0, 0))):
        o = ctx.stream_outlook([env], [minv])
        same(o, OM.outlook(sv, abi["flags"], ctx.get_running(), [env], [minv], queue=(E32, E32), leases=None), "personality %d" % t)
        g = int(o["grants_available"][0])
        assert t > 0 or g > 0
        split = g // 2  # (immediate and prefetch rows alike)
        req = {"env_id": np.array([env], np.uint32), "min_version": np.array([minv], np.uint32),
               "requestor_ip": np.array([(172 << 24) + 77], np.uint32), "n_immediate": np.array([split + 1], np.uint32),
               "n_prefetch": np.array([g + 3 - split - 1], np.uint32), "lease_for": np.array([50], np.int64),
               "deadline": np.array([t], np.int64), "tag": np.array([t], np.uint64)}
        r = rpc_tick(ctx, t, req)
        assert int(r["n_granted"][0]) == g and r["n_waiting"] == 0, (t, g, r["n_granted"])
        if g == 0:
            assert r["status"][0] == (binding.IDX_TIMEOUT if o["eligible"][0] else binding.IDX_ENV_NOT_FOUND)
        asked += g
        after = ctx.stream_outlook([env], [minv])
        assert int(after["grants_available"][0]) == 0 and int(after["free_servants"][0]) == 0
        assert int(after["running_tasks"][0]) == int(o["running_tasks"][0]) + g
    assert asked > 50
    ctx.stream_end()
    ctx.close()


# ---- the registry changes, the stream grows, the stream moves -------------------------------------

def test_after_removal_a_new_digest_reserve_and_restore():
    ws = ist.stream("rpc", ist.pool(96, seed=5, hint=ist.POOL_HINT["rpc"] // 2))
    x = ist.Inspected("rpc", ws, ist.begin("rpc", ws))
    env, minv = queries(3, extra=(64,))
    check = lambda what: (same(x.ctx.stream_outlook(env, minv), OM.stream_outlook(ws, env, minv, inspect=x.I), what),
                          same_waiting(x.ctx.stream_waiting(), OM.stream_waiting(ws), what))
    for _ in range(4):
        x.tick(ws.next_tick(), snapshot=False)
    removed = np.array([0, 17, 63, 64, 95], np.uint32)
    x.ctx.remove_servants(removed)
    lease.drop_rows(ws, removed)
    check("after ydc_remove_servants")
    x.tick(ws.next_tick(), snapshot=False)
    check("a tick later")
    # A heartbeat appends a servant with a digest nobody had: the tables are rebuilt inside the tick.
    ev = ws.next_tick()
    like = int(np.nonzero(ws.es.sv["max_tasks"] > 0)[0][0])
    row, s_new = AM.append_servant(ws, like, 0x0A636363)
    ws.es.sv["env_mask"][s_new] |= np.uint64(4)
    ws.es.abi["env_mask"][s_new] |= np.uint64(4)
    row["env_mask"] = ws.es.abi["env_mask"][s_new]
    ev["upd_idx"] = np.concatenate([ev["upd_idx"], [s_new]]).astype(np.uint32)
    ev["upd_rows"] = np.concatenate([ev["upd_rows"], row])
    assert not x.ctx.stream_outlook([2], [0])["eligible"][0]
    x.tick(ev, snapshot=False)
    check("after a structural heartbeat")
    assert x.ctx.stream_outlook([2], [0])["eligible"][0] == 1
    caps = x.ctx.stream_caps()
    ws.state.max_waiting, ws.state.max_rows = 2 * caps["max_waiting"], 2 * caps["max_rows"]
    x.ctx.stream_reserve(max_waiting=ws.state.max_waiting, max_rows=ws.state.max_rows, max_leases=2 * caps["max_leases"])
    check("after ydc_stream_reserve")
    x.tick(ws.next_tick(), snapshot=False)
    check("a tick after it")
    assert len(ws.state.q) and len(ws.table.L)
    b = binding.Context(device=0)
    b.stream_restore(x.ctx.stream_snapshot())
    same(b.stream_outlook(env, minv), OM.stream_outlook(ws, env, minv, inspect=None), "after ydc_stream_restore")
    same_waiting(b.stream_waiting(), OM.stream_waiting(ws), "after ydc_stream_restore")
    b.stream_end()
    b.close()
    x.close()


# ---- refusals ----------------------------------------------------------------------------------

def test_refusals():
    sv = ist.pool(64, seed=5)
    ctx = _uploaded(sv)
    L_ = binding.lib()
    one, out, n = np.zeros(1, np.uint32), np.zeros(1, binding.OUTLOOK_DTYPE), C.c_uint32(7)
    for what in ("no stream", "a plain stream"):
        with pytest.raises(binding.YdcError):
            ctx.stream_outlook([0], [0])
        with pytest.raises(binding.YdcError):
            ctx.stream_waiting()
        assert L_.ydc_stream_outlook_get(ctx._h, None, None, 0, None) == -1, what  # (even without a query)
        if what == "no stream":
            ctx.stream_begin(8, 8, 16)
    ctx.stream_end()
    ctx.stream_begin_leased(8, 8, 16, 64, 8, 8, 8, 8)
    assert L_.ydc_stream_outlook_get(ctx._h, None, None, 0, None) == 0  # n == 0
    assert len(ctx.stream_outlook([], [])["eligible"]) == 0
    assert L_.ydc_stream_outlook_get(ctx._h, one.ctypes.data, one.ctypes.data, 1, None) == -1  # NULL out
    assert L_.ydc_stream_outlook_get(ctx._h, None, one.ctypes.data, 1, out.ctypes.data) == -1
    assert L_.ydc_stream_inspect_waiting(ctx._h, None, None, None, None, None, None, None, None, 0, None) == -1
    # A leased stream has no W: 0 entries, whatever the room.
    assert L_.ydc_stream_inspect_waiting(ctx._h, None, None, None, None, None, None, None, None, 0, C.byref(n)) == 0
    assert n.value == 0 and len(ctx.stream_waiting()["tag"]) == 0
    # Pipelined batches outstanding.
    DA = binding.DeviceArray
    tk = synth.make_tasks(256, sv, n_envs=2)
    cols = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
    d_out = DA.from_numpy(np.zeros(256, np.uint32))
    ctx.dispatch_device_async(*cols, d_out)
    with pytest.raises(binding.YdcError, match="pipelined"):
        ctx.stream_outlook([0], [0])
    with pytest.raises(binding.YdcError, match="pipelined"):
        ctx.stream_waiting()
    ctx.dispatch_wait()
    abi = pack.to_abi_columns(sv)
    same(ctx.stream_outlook([0, 1], [0, 20]), OM.outlook(sv, abi["flags"], sv["running_tasks"], [0, 1], [0, 20]))
    ctx.stream_end()
    ctx.close()

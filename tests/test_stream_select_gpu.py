"""The lease table filtered, counted and paged on the device (ydc_stream_inspect_select /
ydc_stream_inspect_count; stream_select.h: k_select_count, k_select_hist, k_select_digit, k_select_pack)
against the model (tests/stream_select_model.py, with hand cases of its own in
tests/test_stream_select_model.py): integer for integer on every column, the number of matches and the
number of rows. T, the table the model filters, is the lease models' (tests/stream_inspect_model.py's
Inspect.tasks(), or a ledger kept from the ticks' own answers where a test grants by hand);
ydc_stream_inspect_tasks of the same context is looked at as a second witness only."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_select_model as SM
from tests import test_stream_inspect_gpu as ist
from tests import test_stream_lease_gpu as lease
from tests import test_stream_requestor_gpu as rq
from tests.test_stream_select_model import differential_filters
from yadcc_amd import binding, snapshot, streaming, synth

pytestmark = pytest.mark.gpu
INVALID = -1
E32, E64, I64 = rq.E32, rq.E64, rq.I64
NO_ID, NO_TIME = SM.NO_ID, SM.NO_TIME
CAPS = (0, 1, 63, 64, 65)


def ask(ctx, T, cap, what="", **f):
    """One select against the model. -> matches."""
    got, m = ctx.stream_inspect_select(cap, **f)
    want, wm = SM.select(T, cap, **f)
    assert m == wm, "%s: %r: matches gpu %d model %d" % (what, f, m, wm)
    SM.same(got, want, "%s: %r cap %d" % (what, f, cap))
    return m


def ask_caps(ctx, T, what="", **f):
    """... with every cap around the filter's M matches and the fixed ones."""
    m = SM.select(T, 0, **f)[1]
    for cap in sorted(set(CAPS + tuple(c for c in (m - 1, m, m + 1) if c >= 0))):
        assert ask(ctx, T, cap, what, **f) == m
    return m


def witness(ctx, T):
    got = ctx.stream_inspect_tasks()
    SM.same({k: got[k] for k in SM.COLS}, T, "ydc_stream_inspect_tasks")


class Ledger:
    """T of a leased stream that is granted by hand: a row per grant, from the tick's own answers."""

    def __init__(self, ctx):
        self.ctx, self.rows = ctx, []

    def grant(self, now, ips, lease_for=1000, env=0, attributed=True):
        ips = np.asarray(ips, np.uint32)
        n = len(ips)
        tk = {"env_id": np.full(n, env, np.uint32), "min_version": np.zeros(n, np.uint32), "requestor_ip": ips}
        out, ids, _, _, n_leases = self.ctx.stream_tick_leased(E32, rq.NO_ROWS, E32, E64, I64, E64, E32, np.zeros(1, np.uint32),
                                                               E64, tk, np.full(n, now + lease_for, np.int64), now)
        assert (out < 8).all()
        for i in range(n):
            self.rows.append((int(ids[i]), int(out[i]), now + lease_for, 0) + (
                (now, env, int(ips[i]), 0) if attributed else (NO_TIME, NO_ID, NO_ID, 0)))
        assert n_leases == len(self.rows)
        return ids

    @property
    def T(self):
        return SM.rows(self.rows)


# ---- table sizes, |L|, caps ------------------------------------------------------------------------

@pytest.mark.parametrize("max_leases,sizes", [(512, (0, 1, 511)), (2048, (0, 1, 511, 1500, 2048))])
def test_table_sizes_and_caps(max_leases, sizes):
    """Tables of 1 024 and 4 096 slots at |L| = 0, 1, 511, 1 500, 2 048 (= max_leases): a filter that
    matches everything, one that matches nothing, one per requestor, every cap around M; at |L| = 2 048
    cursors that leave M = 1 023, 1 024 and 1 025 matches (a tile of the pack)."""
    A, B = 0x0A000001, 0xFFFFFFFF
    ctx = rq.uploaded(rq.roomy_registry())
    ctx.stream_begin_leased(8, 8, 1024, max_leases, 8, 8, 8, 8)
    assert ctx.stream_caps()["max_leases"] == max_leases
    ctx.stream_inspect_begin()
    led = Ledger(ctx)
    rng = np.random.default_rng(max_leases)
    for t, size in enumerate(sizes):
        add = size - len(led.rows)
        if add:
            led.grant(10 + t, np.where(rng.random(add) < 0.9, A, B), lease_for=100 * (t + 1))
        T = led.T
        assert len(T["task_id"]) == size
        witness(ctx, T)
        what = "%d slots, |L| = %d" % (2 * max(max_leases, 512), size)
        assert ask_caps(ctx, T, what) == size
        assert ask_caps(ctx, T, what, servant=4000) == 0
        assert ask_caps(ctx, T, what, requestor_ip=7) == 0
        m = ask_caps(ctx, T, what, requestor_ip=A) + ask_caps(ctx, T, what, requestor_ip=B)
        assert m == size
        ask_caps(ctx, T, what, expires_before=10 + t + 100 * t + 1)  # (the leases of the earlier ticks)
        ask(ctx, T, size, what, servant=int(T["servant_idx"][0]) if size else 0, zombie=0)
    if max_leases == 2048:
        ids = T["task_id"]
        for M in (1023, 1024, 1025):
            assert ask_caps(ctx, T, "M = %d" % M, after_id=int(ids[-M - 1])) == M
        assert ask(ctx, T, 2048, requestor_ip=A) > 1025  # (the hot requestor, whole)
    ctx.stream_end()
    ctx.close()


# ---- ids that make the radix select work ------------------------------------------------------------

def id_sets():
    around = lambda k: [(1 << k) + d for d in range(-3, 4)]
    base = 0x00AB_CDEF_0123_4500
    return {
        "straddling 2^8, 2^16, 2^32 and 2^56": (around(8) + around(16) + around(32) + around(56), None),
        "2^8 alone": (around(8), None),
        "2^32 alone": (around(32), None),
        "2^56 alone": (around(56), None),
        "the top byte only": ([(b << 56) | 0x00AB_CDEF_0123_45 for b in range(0, 255, 3)], None),
        "the bottom byte only": ([base | b for b in range(256)], None),
        "a threshold bin of many": ([(5 << 56) | j for j in range(300)] + [(9 << 56) | j for j in range(300)] + [3], None),
        "two bytes apart": ([(j << 40) | (j * 37 % 251) for j in range(1, 400)], None),
        "the largest next_id": ([(1 << 64) - 2 - 5 * j for j in range(200)] + [1, 2], (1 << 64) - 1),
    }


@pytest.fixture(scope="module")
def seed_blob():
    """A leased stream's snapshot to rewrite: 8 roomy servants, room for 2 048 leases, one lease."""
    ctx = rq.uploaded(rq.roomy_registry())
    ctx.stream_begin_leased(8, 8, 64, 2048, 8, 8, 8, 8)
    rq.leased_tick(ctx, 1, [5])
    blob = ctx.stream_snapshot()
    ctx.stream_end()
    ctx.close()
    return blob


@pytest.mark.parametrize("name", list(id_sets()))
def test_ids_that_exercise_the_radix_select(name, seed_blob):
    """Lease tables written through the snapshot codec and ydc_stream_restore, details filed by
    ydc_stream_inspect_load: every cap from 1 to 5, around the middle and up to |L| + 1, with the empty
    filter, a requestor (a third of the leases), a zombie filter and a cursor."""
    ids, next_id = id_sets()[name]
    ids = np.array(sorted(ids), np.uint64)
    n = len(ids)
    rng = np.random.default_rng(n)
    d = snapshot.parse(seed_blob)
    srv = rng.integers(0, 8, n).astype(np.uint32)
    d.update(l_id=ids, l_expires_at=rng.integers(50, 5000, n).astype(np.int64), l_servant=srv,
             l_zombie=(rng.random(n) < 0.3).astype(np.uint8), l_stamp=np.zeros(n, np.uint32),
             next_id=next_id if next_id is not None else int(ids[-1]) + 1,
             running_tasks=np.bincount(srv, minlength=8).astype(np.uint32))
    d.pop("l_state")
    ctx = binding.Context(device=0)
    ctx.stream_restore(snapshot.build(d))
    T = {"task_id": ids, "servant_idx": srv, "expires_at": d["l_expires_at"], "zombie": d["l_zombie"],
         "started_at": np.full(n, NO_TIME, np.int64), "env_id": np.full(n, NO_ID, np.uint32),
         "requestor_ip": np.full(n, NO_ID, np.uint32), "prefetch": np.zeros(n, np.uint8)}
    caps = sorted(set([1, 2, 3, 4, 5, n // 3, n // 2 - 1, n // 2, n // 2 + 1, n - 1, n, n + 1]) - {0})
    for cap in caps:  # inspection off: the table predicates, the sentinels beside the rows
        ask(ctx, T, cap, name)
        ask(ctx, T, cap, name, zombie=0)
    ctx.stream_inspect_begin()
    ask(ctx, T, n, name, unattributed=True)
    known = rng.random(n) < 0.8
    T["started_at"] = np.where(known, rng.integers(0, 40, n), NO_TIME).astype(np.int64)
    T["env_id"] = np.where(known, rng.integers(0, 3, n), NO_ID).astype(np.uint32)
    T["requestor_ip"] = np.where(known, rng.choice([0, 7, 0xFFFFFFFF], n), NO_ID).astype(np.uint32)
    T["prefetch"] = np.where(known, rng.integers(0, 2, n), 0).astype(np.uint8)
    ctx.stream_inspect_load(**{k: v[known] for k, v in T.items()})
    witness(ctx, T)
    for cap in caps:
        ask(ctx, T, cap, name)
        ask(ctx, T, cap, name, requestor_ip=0xFFFFFFFF)
        ask(ctx, T, cap, name, zombie=1, expires_before=3000)
        ask(ctx, T, cap, name, after_id=int(ids[n // 4]), prefetch=0)
    for page in (1, 7):
        got = SM.concat(list(streaming.iter_tasks(ctx, page, requestor_ip=7)))
        SM.same(got, SM.select(T, n, requestor_ip=7)[0], "%s: pages of %d" % (name, page))
    ctx.stream_end()
    ctx.close()


# ---- every predicate, alone and in conjunctions, in every mode -------------------------------------

def conjunctions(T, rng):
    """Each predicate alone with a value of T's, then pairs and triples of them."""
    n = len(T["task_id"])
    assert n
    pick = lambda ok=None: int(rng.choice(np.nonzero(ok)[0] if ok is not None else n))
    att = T["started_at"] != NO_TIME
    i = pick(att) if att.any() else pick()
    z = pick(T["zombie"] == 1) if T["zombie"].any() else i
    one = [{"servant": int(T["servant_idx"][i])}, {"zombie": 1}, {"zombie": 0},
           {"expires_before": int(np.median(T["expires_at"]))}, {"after_id": int(T["task_id"][n // 2])}]
    if att.any():
        one += [{"env_id": int(T["env_id"][i])}, {"requestor_ip": int(T["requestor_ip"][i])}, {"prefetch": 1}, {"prefetch": 0},
                {"started_before": int(T["started_at"][i]) + 1}, {"unattributed": True}]
    out = list(one)
    for _ in range(12):
        k = int(rng.choice([2, 2, 3]))
        f = {}
        for j in rng.permutation(len(one))[:k]:
            f.update(one[j])
        out.append(f)
    out += [{"servant": int(T["servant_idx"][z]), "zombie": 1}, {"zombie": 1, "expires_before": int(T["expires_at"][z]) + 1}]
    return out


@pytest.mark.parametrize("mode", list(ist.MODS))
def test_each_predicate_alone_and_in_conjunctions(mode):
    """Inspection begun late, so that about half the leases are unattributed; zombies after expiry
    ticks; prefetch = 1 in rpc mode. Before the begin call: the four table predicates work, the detail
    columns are the sentinels, a record predicate is refused."""
    ws = ist.stream(mode, ist.pool(96, seed=5, hint=ist.POOL_HINT[mode] // 2))
    x = ist.Inspected(mode, ws, ist.begin(mode, ws), begin_now=False)
    rng = np.random.default_rng(7)
    for _ in range(5):
        x.tick(ws.next_tick(), snapshot=False)
    T = SM.table(ws)
    assert len(T["task_id"]) > 100 and T["zombie"].any()
    for f in conjunctions(T, rng):
        ask(x.ctx, T, 50, mode + ", inspection off", **f)
        ask(x.ctx, T, len(T["task_id"]), mode + ", inspection off", **f)
    for f in ({"env_id": 0}, {"requestor_ip": 5}, {"prefetch": 0}, {"started_before": 9}, {"unattributed": True},
              {"servant": 1, "env_id": 0}):
        with pytest.raises(binding.YdcError, match="inspection is off"):
            x.ctx.stream_inspect_select(10, **f)
        with pytest.raises(binding.YdcError, match="inspection is off"):
            x.ctx.stream_inspect_count([{}, f])
    x.inspect_begin()
    seen = dict(zombies=0, unattributed=0, prefetch=0, cut=0)
    for t in range(6):
        x.tick(ws.next_tick(), snapshot=False)
        T = SM.table(ws, x.I)
        fs = conjunctions(T, rng)
        for f in fs:
            m = ask(x.ctx, T, 40, "%s, tick %d" % (mode, t), **f)
            seen["cut"] += m > 40
        counts = x.ctx.stream_inspect_count(fs[:64])
        assert np.array_equal(counts, SM.count(T, fs[:64])), t
        seen["zombies"] += ask(x.ctx, T, 1 << 20, mode, zombie=1)
        seen["unattributed"] += ask(x.ctx, T, 1 << 20, mode, unattributed=True)
        seen["prefetch"] += ask(x.ctx, T, 1 << 20, mode, prefetch=1)
    witness(x.ctx, T)
    assert seen["zombies"] and seen["unattributed"] and seen["cut"] and (seen["prefetch"] > 0) == (mode == "rpc"), seen
    x.close()


# ---- stale records, rehash, renumbering -------------------------------------------------------------

def test_a_freed_leases_requestor_is_no_longer_found():
    """200 leases of one requestor, all freed by id: their slots keep the records, nothing matches; 230
    leases of another requestor then reuse some of the slots."""
    ctx = rq.uploaded(rq.roomy_registry())
    ctx.stream_begin_leased(8, 8, 256, 256, 8, 256, 8, 8)
    ctx.stream_inspect_begin()
    A, B = 0x0A000001, 0x0A000002
    led = Ledger(ctx)
    ids = led.grant(1, [A] * 200)
    assert ask(ctx, led.T, 300, requestor_ip=A) == 200
    _, n_leases = rq.leased_tick(ctx, 2, [], free_ids=ids)
    assert n_leases == 0
    led.rows = []
    for f in ({}, {"requestor_ip": A}, {"env_id": 0}, {"started_before": 5}, {"unattributed": True}):
        assert ask(ctx, led.T, 300, "all freed", **f) == 0
    led.grant(3, [B] * 230)
    assert ask(ctx, led.T, 300, requestor_ip=A) == 0 and ask(ctx, led.T, 300, requestor_ip=B) == 230
    assert ask(ctx, led.T, 100, started_before=4) == 230
    ctx.stream_end()
    ctx.close()


def test_the_same_answers_after_reserve_and_remove_servants():
    ws = ist.stream("rpc", ist.pool(96, seed=5, hint=ist.POOL_HINT["rpc"] // 2))
    x = ist.Inspected("rpc", ws, ist.begin("rpc", ws))
    rng = np.random.default_rng(3)
    for _ in range(4):
        x.tick(ws.next_tick(), snapshot=False)

    def every(what):
        T = SM.table(ws, x.I)
        fs = conjunctions(T, rng)
        for f in fs:
            ask(x.ctx, T, 30, what, **f)
        assert np.array_equal(x.ctx.stream_inspect_count(fs[:64]), SM.count(T, fs[:64])), what
        return T

    T = every("before")
    removed = np.array([0, 17, 63, 64, 95], np.uint32)
    kept = T["servant_idx"][~np.isin(T["servant_idx"], removed) & (T["servant_idx"] > 17)]
    s = int(np.bincount(kept).argmax())  # a servant that stays, holds leases and is renumbered
    held = ask(x.ctx, T, 1 << 20, servant=s)
    assert sum(1 for e in ws.table.L.values() if e[0] in set(removed.tolist())) > 0 and held > 0
    x.ctx.remove_servants(removed)
    lease.drop_rows(ws, removed)
    T = every("after ydc_remove_servants")
    renumbered = s - int((removed < s).sum())
    assert renumbered < s
    assert ask(x.ctx, T, 1 << 20, "the filter in the new numbering", servant=renumbered) == held
    x.tick(ws.next_tick(), snapshot=False)
    caps = x.ctx.stream_caps()
    ws.state.max_waiting, ws.state.max_rows = 2 * caps["max_waiting"], 2 * caps["max_rows"]
    before = x.ctx.stream_inspect_select(1 << 20, zombie=0)
    x.ctx.stream_reserve(max_waiting=ws.state.max_waiting, max_rows=ws.state.max_rows, max_leases=2 * caps["max_leases"])
    after = x.ctx.stream_inspect_select(1 << 20, zombie=0)  # (L filed again into a larger table)
    assert before[1] == after[1] and before[1] > 0
    SM.same(after[0], before[0], "after ydc_stream_reserve")
    every("after ydc_stream_reserve")
    x.tick(ws.next_tick(), snapshot=False)
    every("a tick after it")
    x.close()


def test_the_same_answers_after_an_aliveness_expiry():
    sv = ist.pool(70, seed=3)
    ws = ist.stream("leased", sv)
    ctx = ist.begin("leased", ws)
    first = AM.first_expiries(70, life=4)
    AM.attach(ws, first)
    ctx.stream_alive_begin(first)
    x = ist.Inspected("leased", ws, ctx, alive=True)
    gen = AM.AliveGen(ws, life=4, p_stop=0.3, p_short=0.3, seed=3)
    rng = np.random.default_rng(5)
    removed = orphans = 0
    for t in range(10):
        _, want = x.tick(gen.next_tick(), snapshot=False)
        removed += len(want["removed"])
        orphans += want["orphans"]
        T = SM.table(ws, x.I)
        if len(T["task_id"]):
            for f in conjunctions(T, rng)[:12]:
                ask(x.ctx, T, 25, "tick %d" % t, **f)
        ask(x.ctx, T, 1 << 20, "tick %d" % t)
    assert removed >= 2 and orphans > 0, (removed, orphans)
    x.close()


# ---- the count ---------------------------------------------------------------------------------------

def test_count_of_0_1_63_64_filters_and_65_refused():
    ctx = rq.uploaded(rq.roomy_registry())
    ctx.stream_begin_leased(8, 8, 2048, 2048, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    led = Ledger(ctx)
    rng = np.random.default_rng(1)
    led.grant(5, rng.integers(0, 40, 1500), lease_for=50)
    led.grant(9, rng.integers(30, 70, 300), lease_for=10, env=1)
    T = led.T
    ids = T["task_id"]
    filters = [{}] + [{"requestor_ip": r} for r in range(0, 70, 2)] + [{"servant": s} for s in range(9)] + [
        {"env_id": 1, "requestor_ip": 35}, {"after_id": int(ids[700])}, {"after_id": int(ids[700]), "env_id": 0},
        {"expires_before": 20}, {"expires_before": 19}, {"started_before": 9}, {"unattributed": True}, {"zombie": 1},
        {"prefetch": 0}, {"prefetch": 1, "servant": 2}] + [{"requestor_ip": 200 + r} for r in range(20)]
    assert len(filters) >= 65
    for n in (0, 1, 63, 64):
        got = ctx.stream_inspect_count(filters[:n])
        assert got.dtype == np.uint32 and np.array_equal(got, SM.count(T, filters[:n])), n
        for f, c in list(zip(filters[:n], got))[::7]:
            assert ctx.stream_inspect_select(3, **f)[1] == c, f  # (the select's matches for the same filter)
    assert int(ctx.stream_inspect_count(filters[:64])[0]) == 1800
    out = np.full(65, 0xABABABAB, np.uint32)
    arr = (binding.LeaseFilter * 65)(*[binding.lease_filter(**f) for f in filters[:65]])
    assert binding.lib().ydc_stream_inspect_count(ctx._h, arr, 65, out.ctypes.data) == INVALID
    assert (out == 0xABABABAB).all() and "65 filters" in binding.lib().ydc_last_error(ctx._h).decode()
    assert binding.lib().ydc_stream_inspect_count(ctx._h, None, 0, None) == 0
    ctx.stream_end()
    ctx.close()


# ---- paging ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [1, 7, 64, 1000])
def test_iter_tasks_pages_equal_the_filtered_table(page):
    ctx = rq.uploaded(rq.roomy_registry())
    ctx.stream_begin_leased(8, 8, 2048, 2048, 8, 8, 8, 8)
    led = Ledger(ctx)
    rng = np.random.default_rng(page)
    led.grant(3, rng.integers(0, 6, 400), attributed=False)
    ctx.stream_inspect_begin()
    led.grant(5, rng.integers(0, 6, 1300), lease_for=50)
    T = led.T
    for f in ({"requestor_ip": 2}, {"unattributed": True}, {"servant": int(T["servant_idx"][0]), "expires_before": 60},
              {"requestor_ip": 77}) + (({},) if page > 1 else ()):
        want = SM.pages(T, page, **dict(f))
        got = list(streaming.iter_tasks(ctx, page, **dict(f)))
        assert len(got) == len(want) and [len(p["task_id"]) for p in got] == [len(p["task_id"]) for p in want], f
        SM.same(SM.concat(got), SM.select(T, len(T["task_id"]), **f)[0], "pages of %d, %r" % (page, f))
    ctx.stream_end()
    ctx.close()


# ---- it changes nothing -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(ist.MODS))
def test_a_twin_that_never_selects_answers_alike(mode):
    ws = ist.stream(mode, ist.pool(96, seed=5, hint=ist.POOL_HINT[mode] // 2))
    x = ist.Inspected(mode, ws, ist.begin(mode, ws))
    twin = ist.begin(mode, ws) if mode == "leased" else ist.begin(mode, ws, ctx=rq.uploaded(ws.es.sv))
    twin.stream_inspect_begin()
    rng = np.random.default_rng(2)
    for t in range(20):
        ev = ws.next_tick()
        got_twin = x.G.gpu_tick(twin, ws, ev)
        got, _ = x.tick(ev, snapshot=False)
        rq.same_answers(got, got_twin, "tick %d" % t)
        T = SM.table(ws, x.I)
        for cap, f in differential_filters(ws, x.I, rng, int(ev["now"]), k=3, caps=(0, 5, 100))[1]:
            ask(x.ctx, T, cap, "tick %d" % t, **f)
        x.ctx.stream_inspect_count([{}, {"zombie": 1}])
        rq.same_answers(x.ctx.stream_leases(), twin.stream_leases(), "tick %d: lease snapshot" % t)
        assert np.array_equal(x.ctx.get_running(), twin.get_running()), t
    assert x.ctx.stream_snapshot() == twin.stream_snapshot(), "the calls left a trace in the snapshot"
    twin.stream_end()
    twin.close()
    x.close()


def test_between_dispatch_ticks_and_the_resident_kernel():
    """ydc_dispatch_tick leaves its kernel resident while no stream is open; the select, like the
    outlook, ends a resident kernel before it reads. Refused without a stream (the resident sequence
    goes on), exact between ydc_dispatch_tick calls beside an open stream."""
    sv = rq.roomy_registry(40)
    ctx = rq.uploaded(sv)
    tick = lambda seed: ctx.dispatch_tick(synth.make_tasks(1, sv, n_envs=3, seed=seed, self_frac=0.0), commit=True)
    tick(1), tick(2)
    r1 = ctx.stats()["tick_resident_calls"]
    tick(3)
    assert ctx.stats()["tick_resident_calls"] == r1 + 1, "the tick kernel did not stay resident"
    with pytest.raises(binding.YdcError, match="no stream is open"):
        ctx.stream_inspect_select(4)
    tick(4)
    ctx.stream_begin_leased(8, 8, 64, 256, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    led = Ledger(ctx)
    led.grant(1, [5, 6, 5])
    tick(5)
    assert ask(ctx, led.T, 8, requestor_ip=5) == 2
    tick(6)
    assert ctx.stream_inspect_count([{"requestor_ip": 6}, {}]).tolist() == [1, 3]
    tick(7)
    assert ask(ctx, led.T, 1) == 3
    ctx.stream_end()
    ctx.close()


# ---- every refusal, with the outputs untouched ---------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    L_ = binding.lib()
    ids = np.full(4, 0xAB, np.uint64)
    n, m = C.c_uint32(77), C.c_uint32(78)

    def refused(ctx, f, out_n=True, out_m=True, count=True):
        rc = L_.ydc_stream_inspect_select(ctx._h, C.byref(f) if f is not None else None, ids.ctypes.data, *([None] * 7), 4,
                                          C.byref(n) if out_n else None, C.byref(m) if out_m else None)
        assert rc == INVALID and (n.value, m.value) == (77, 78) and (ids == 0xAB).all(), (rc, n.value, m.value)
        one = np.full(1, 0xCD, np.uint32)
        if f is not None and count:  # (the count refuses what the select refuses for its filter or its stream)
            assert L_.ydc_stream_inspect_count(ctx._h, C.byref(f), 1, one.ctypes.data) == INVALID and one[0] == 0xCD
        return L_.ydc_last_error(ctx._h).decode()

    every = binding.lease_filter()
    sv = ist.pool(64, seed=5)
    ctx = rq.uploaded(sv)
    assert "no stream is open" in refused(ctx, every)
    ctx.stream_begin(8, 8, 16)
    assert "keeps no state" in refused(ctx, every)
    ctx.stream_end()
    ctx.stream_begin(8, 8, 16, max_waiting=64)
    assert "keeps no leases" in refused(ctx, every)
    ctx.stream_end()
    ctx.close()
    ctx = rq.uploaded(rq.roomy_registry())
    ctx.stream_begin_leased(8, 8, 64, 256, 8, 8, 8, 8)
    led = Ledger(ctx)
    led.grant(1, [9, 7, 9], attributed=False)
    assert "inspection is off" in refused(ctx, binding.lease_filter(requestor_ip=9))
    assert "inspection is off" in refused(ctx, binding.lease_filter(unattributed=True))
    ctx.stream_inspect_begin()
    for bad in (0x200, 0x80000000, 0x1FF | 0x400):
        f = binding.lease_filter()
        f.fields = bad
        assert "selects" in refused(ctx, f)
    assert "zombie 2" in refused(ctx, binding.lease_filter(zombie=2))
    assert "prefetch 2" in refused(ctx, binding.lease_filter(prefetch=2))
    f = binding.lease_filter(servant=1)
    f.zombie = f.prefetch = 9  # (not selected: not looked at)
    assert L_.ydc_stream_inspect_select(ctx._h, C.byref(f), *([None] * 8), 4, C.byref(n), C.byref(m)) == 0
    n.value, m.value = 77, 78
    refused(ctx, None)
    refused(ctx, every, out_n=False, count=False)
    refused(ctx, every, out_m=False, count=False)
    assert L_.ydc_stream_inspect_count(ctx._h, C.byref(every), 1, None) == INVALID
    assert L_.ydc_stream_inspect_count(ctx._h, None, 1, ids.ctypes.data) == INVALID and (ids == 0xAB).all()
    # Pipelined batches outstanding.
    DA = binding.DeviceArray
    tk = synth.make_tasks(256, sv, n_envs=2)
    cols = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
    d_out = DA.from_numpy(np.zeros(256, np.uint32))
    ctx.dispatch_device_async(*cols, d_out)
    assert "pipelined" in refused(ctx, every)
    ctx.dispatch_wait()
    # ... and what is no refusal: every column NULL, cap 0, a servant the registry does not have.
    assert L_.ydc_stream_inspect_select(ctx._h, C.byref(every), *([None] * 8), 2, C.byref(n), C.byref(m)) == 0
    assert (n.value, m.value) == (2, 3)
    assert L_.ydc_stream_inspect_select(ctx._h, C.byref(every), *([None] * 8), 0, C.byref(n), C.byref(m)) == 0
    assert (n.value, m.value) == (0, 3)
    assert ask(ctx, led.T, 1 << 31, servant=0xFFFFFFFF) == 0 and ask(ctx, led.T, 0xFFFFFFFF) == 3
    ctx.stream_end()
    ctx.close()


# ---- a randomised differential -------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(ist.MODS))
def test_randomised_differential(mode):
    """60 ticks with 5 random filters between ticks (drawn from the model's T, caps 1 / 7 / 64). The two
    conditions on the inputs are the model's alone: at least 90 % of the filters match a lease, at
    least 30 % match more than their cap."""
    ws = ist.stream(mode, ist.pool(96, seed=5, hint=ist.POOL_HINT[mode] // 2))
    x = ist.Inspected(mode, ws, ist.begin(mode, ws))
    x.check = lambda: None  # (the getters are test_stream_inspect_gpu's to compare; here: the select)
    rng = np.random.default_rng(11)
    asked = some = over = 0
    for t in range(60):
        ev = ws.next_tick()
        x.tick(ev, snapshot=False)
        T, qs = differential_filters(ws, x.I, rng, int(ev["now"]))
        for cap, f in qs:
            m = ask(x.ctx, T, cap, "%s, tick %d" % (mode, t), **f)
            asked, some, over = asked + 1, some + (m >= 1), over + (m > cap)
        if t % 10 == 9:
            fs = [f for _, f in qs]
            assert np.array_equal(x.ctx.stream_inspect_count(fs), SM.count(T, fs)), t
    assert asked == 300 and some >= 0.9 * asked and over >= 0.3 * asked, (mode, asked, some, over)
    x.close()

"""The book by digest on the device (ydc_stream_book_find / ydc_stream_book_distinct;
k_book_index_build, k_book_index_find, k_book_distinct): every answer is compared with the model
(tests/stream_book_find_model.py, the reference daemon's one pass over the list, pinned against a scan
by tests/test_stream_book_find_model.py) on all five fields of a hit and all five columns of the fold,
with integer equality; `rebuilt` is asserted wherever the header fixes it; and a twin context that
gets the same ticks and never asks shows that the calls leave the stream alone."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_alive_cases as acases
from tests import stream_book_find_model as FM
from tests import stream_book_model as BM
from tests import stream_lease_cases as cases
from tests import stream_lease_model as L
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WM
from tests import test_stream_lease_gpu as lease
from tests import test_stream_rpc_gpu as rpc
from tests import test_stream_wait_lease_gpu as wl
from tests.test_stream_alive_gpu import GpuPlayer
from tests.test_stream_book_gpu import Booked, _graph
from tests.test_stream_reserve_gpu import new_ctx
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, streaming, synth

pytestmark = pytest.mark.gpu
ALL = (1 << 64) - 1  # the index's free-slot mark, and an ordinary key
ABSENT = [3, 5, 1 << 32, (1 << 63) + 12345, ALL - 1, 0x9E3779B97F4A7C15, 77, 1 << 40, 6, 12]
DISTINCT = ("servant_idx", "task_grant_id", "servant_task_id", "digest_key", "count")
INVALID, CAPACITY = -1, -4  # YDC_ERR_INVALID_ARGUMENT, YDC_ERR_CAPACITY


def same_hits(what, got, want):
    assert got.dtype == FM.HIT and len(got) == len(want), what
    for f in FM.HIT.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s: %s[%d] gpu %d model %d (%d of %d differ)" % (
            what, f, bad[0], got[f][bad[0]], want[f][bad[0]], bad.size, len(want))


def same_fold(what, got, want):
    assert len(got) == len(want) == 5
    for name, a, b in zip(DISTINCT, got, want):
        assert a.dtype == b.dtype and len(a) == len(b), "%s: %d rows of %s, model %d" % (what, len(a), name, len(b))
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, "%s: distinct %s[%d] gpu %d model %d (%d differ)" % (
            what, name, bad[0], a[bad[0]], b[bad[0]], bad.size)


def ask(ctx, book, what, rebuilt=None, extra=()):
    """Every distinct key of the model's B, five absent ones, 0 and all-ones (and `extra`): find, find
    again in another order, distinct. rebuilt: what the first call must report (None: either); the
    two behind it never build."""
    cols = book.columns()
    present = sorted(set(cols[3].tolist()))
    absent = [k for k in ABSENT if k not in set(present)][:5]
    assert len(absent) == 5
    keys = np.concatenate([np.array(present + absent + [0, ALL], np.uint64), np.asarray(extra, np.uint64)])
    got, built = ctx.stream_book_find(keys)
    same_hits(what, got, FM.find(cols, keys))
    if rebuilt is not None:
        assert built == rebuilt, "%s: rebuilt %d, expected %d" % (what, built, rebuilt)
    got, built = ctx.stream_book_find(keys[::-1])
    same_hits(what + " (again)", got, FM.find(cols, keys[::-1]))
    assert not built, "%s: a find right behind a find built the index again" % what
    got, built = ctx.stream_book_distinct()
    same_fold(what, got, FM.distinct(cols))
    assert not built, "%s: distinct right behind a find built the index again" % what
    return got


def keyed(ev, t):
    """Payload columns of a tick's reports whose keys collide: on even ticks task_grant_id % 7 (6 as
    all-ones), on odd ticks one key per id with bits above 2^32 set."""
    ids = np.asarray(ev["report_ids"], np.uint64)
    if t % 2 == 0:
        dkey = ids % np.uint64(7)
        dkey[dkey == 6] = np.uint64(ALL)
    else:
        dkey = ids * np.uint64(0x100000001) + np.uint64(t)
    return BM.payload(ev)[0], dkey


class Pair:
    """A context that asks (a Booked, with the model beside it) and a twin that gets the same ticks and
    never asks."""

    def __init__(self, mode, ws, make_ctx, max_book, masks=False):
        self.b = Booked(mode, ws, make_ctx(), max_book, masks)
        self.twin = make_ctx()
        self.twin.stream_book_begin(max_book)

    def tick(self, ev, stid, dkey, snapshot=True):
        b = self.b
        for c in (b.ctx, self.twin):
            c.stream_book_stage(stid, dkey)
        b.book.stage(stid, dkey)
        want = b.tick(ev, stage=False, snapshot=snapshot)  # (the asker against the model, B included)
        got = b.G.gpu_tick(self.twin, b.ws, ev, b.masks)
        b.G.check_tick(b.t - 1, self.twin, b.ws, got, want, snapshot=snapshot)  # (answers, leases, running_tasks)
        for name, x, y in zip(DISTINCT, b.ctx.stream_book(), self.twin.stream_book()):
            assert np.array_equal(x, y), "tick %d: book %s differs between the twins" % (b.t - 1, name)
        return want

    def close(self):
        assert self.b.ctx.stream_snapshot() == self.twin.stream_snapshot(), "the calls left a trace in the snapshot"
        self.b.close()
        self.twin.stream_end()
        self.twin.close()


def seeded(mode):
    """The pools and streams of tests/test_stream_book_gpu.py's three mode tests."""
    if mode == "leased":
        sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
        ws = L.LeaseStream(sv, 400, 250, 60, L.LeaseTable(), n_envs=2, report_frac=0.3)
        return ws, lambda: lease.begin(ws, 1 << 14, 400)
    if mode == "wait_leased":
        sv = synth.make_servants(40, n_tasks_hint=2000, n_envs=2, seed=31)
        ws = WM.new_stream(sv, 600, 350, 80, 3000, n_envs=2, rate=lambda now: 1.0 if now % 12 < 8 else 0.125,
                           report_frac=0.3)
        return ws, lambda: wl.begin(ws, 1 << 14, 600)
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=8)
    ws = RM.new_stream(sv, 40, 300, 100, 1000, 1 << 12, n_envs=2, report_frac=0.3, **BIG)
    return ws, lambda: rpc.begin(ws, 40)


@pytest.mark.parametrize("stream_graph", ["1", "0"])
@pytest.mark.parametrize("mode", ["leased", "wait_leased", "rpc"])
def test_every_mode_beside_a_twin_that_never_asks(mode, stream_graph, monkeypatch):
    """10 ticks with colliding keys; after each one every key of B, absent ones, 0 and all-ones. The
    twin agrees on every tick, on B and, at the end, on the bytes of ydc_stream_snapshot."""
    _graph(monkeypatch, stream_graph)
    ws, make_ctx = seeded(mode)
    p = Pair(mode, ws, make_ctx, 6000)
    hits = collide = 0
    for t in range(10):
        ev = ws.next_tick()
        p.tick(ev, *keyed(ev, t))
        fold = ask(p.b.ctx, p.b.book, "%s tick %d" % (mode, t), rebuilt=len(ev["report_servants"]) > 0)
        hits, collide = hits + len(fold[0]), collide + int((fold[4] > 1).sum())
    assert hits > 50 and collide > 5, (hits, collide)
    p.close()


SIZES = [0, 167, 507, 1060, 1386, 1465, 1711, 1990, 2296, 2188, 2208, 2285]


def test_book_across_the_tile_and_table_edges():
    """|B| grows through 1024 and 2048 entries: two tiles, then three, of k_book_distinct, and an index
    of 1024, 4096 and 8192 slots. |B| + 300 queries after every tick."""
    sv = synth.make_servants(200, n_tasks_hint=9000, n_envs=2, seed=3)
    ls = L.LeaseStream(sv, 1500, 600, 100, L.LeaseTable(), n_envs=2, report_frac=0.5)
    b = Booked("leased", ls, lease.begin(ls, 1 << 15, 1500, report_ids=1 << 13), 1 << 13)
    rng = np.random.default_rng(5)
    sizes = []
    for t in range(12):
        ev = ls.next_tick()
        stid, dkey = keyed(ev, t)
        b.ctx.stream_book_stage(stid, dkey)
        b.book.stage(stid, dkey)
        b.tick(ev, stage=False, snapshot=False)
        sizes.append(len(b.book))
        held = b.book.columns()[3]
        pool = np.concatenate([held, np.array(ABSENT + [0, ALL], np.uint64)])
        ask(b.ctx, b.book, "tick %d" % t, rebuilt=len(ev["report_servants"]) > 0,
            extra=np.concatenate([held, pool[rng.integers(0, len(pool), 300)]]))
    assert sizes == SIZES, sizes
    b.close()


def column(pattern, m, i):
    """The key column of m entries; i: the number of the size (patterns that need a key draw it by i)."""
    k = np.arange(m, dtype=np.uint64)
    if pattern == "sequential":  # all ones, 0, 1, 2, ...
        return k - np.uint64(1)
    if pattern == "multiples_of_2_32":  # 0, 2^32, 2 * 2^32, ...
        return k << np.uint64(32)
    if pattern == "one_key":
        return np.full(m, [0, ALL, 0xDEADBEEF00000001][i % 3], np.uint64)
    if pattern == "two_keys":
        return np.where(k % np.uint64(2) == 0, np.uint64(0), np.uint64(ALL))
    assert pattern == "last_repeats_first"
    col = k - np.uint64(1)
    if m:
        col[-1] = col[0]
    return col


EDGES = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 2049]


@pytest.mark.parametrize("pattern", ["sequential", "multiples_of_2_32", "one_key", "two_keys", "last_repeats_first"])
def test_exact_sizes_with_hand_made_keys(pattern):
    """B is exactly a key column of m entries: tick 0 grants one task, then its servant lists that id
    m times (an id listed k times gives k entries) with the column staged; the next report replaces
    it. m: the workgroup's edge, the tile's, both sides of the index's first two doublings. Every
    size is asked 0, 1, 255, 256, 257 and 5000 queries."""
    ls = cases.small_stream()
    ctx = new_ctx(ls.es.sv)
    ctx.stream_begin_leased(ls.es.hb + 8, 16, cases.MAX_TASKS, 64, 64, 64, ls.es.n, 2049)
    b = Booked("leased", ls, ctx, 2 * 2049)
    r = b.tick(cases.scripted(ls, ls.next_tick(), n=1, lease=[10 ** 6]))
    assert int((r["out"] < L.IDX_ENV_NOT_FOUND).sum()) == 1
    (s, (tid,)), = cases.held(ls.table).items()
    rng = np.random.default_rng(9)
    for i, m in enumerate(EDGES):
        col = column(pattern, m, i)
        ev = cases.scripted(ls, ls.next_tick(), reports=[(s, [tid] * m)])
        stid = np.arange(m, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 40)
        ctx.stream_book_stage(stid, col)
        b.book.stage(stid, col)
        r = b.tick(ev, stage=False)
        assert r["unknown_reported"] == 0 and len(b.book) == m
        cols = b.book.columns()
        assert np.array_equal(cols[3], col)
        what = "%s, m = %d" % (pattern, m)
        fold = ask(ctx, b.book, what, rebuilt=True)
        assert len(fold[0]) == len(set(col.tolist())) and int(fold[4].sum()) == m
        pool = np.concatenate([col, np.array(ABSENT + [0, ALL], np.uint64)])
        for n in (0, 1, 255, 256, 257, 5000):
            q = pool[rng.integers(0, len(pool), n)]
            got, built = ctx.stream_book_find(q)
            same_hits("%s, %d queries" % (what, n), got, FM.find(cols, q))
            assert not built
    b.close()


def hand(max_book=256, max_leases=64):
    ls = cases.small_stream(max_leases)
    ctx = new_ctx(ls.es.sv)
    ctx.stream_begin_leased(ls.es.hb + 8, 16, cases.MAX_TASKS, max_leases, 64, 64, ls.es.n, 64)
    return Booked("leased", ls, ctx, max_book)


def test_staleness_and_renumbering():
    """`rebuilt` as the header fixes it, and the answers against the model every time: find after find;
    ticks without reports; a report that replaces its servant's entries; an empty report; the caller's
    ydc_remove_servants of a row with entries and of a lower row without; a larger book; a reserve;
    snapshot and restore into a fresh context."""
    b = hand()
    ls, ctx, book = b.ws, b.ctx, b.book

    def tick(what, rebuilt, reports=(), key=lambda ids: ids % np.uint64(3), **kw):
        ev = cases.scripted(ls, ls.next_tick(), reports=list(reports), **kw)
        stid, dkey = BM.payload(ev)[0], key(np.asarray(ev["report_ids"], np.uint64))
        ctx.stream_book_stage(stid, dkey)
        book.stage(stid, dkey)
        r = b.tick(ev, stage=False)
        ask(ctx, book, what, rebuilt=rebuilt)
        return r

    tick("the first call of the stream", True, n=6, lease=[100] * 6)
    assert len(book) == 0
    tick("everybody reports", True, reports=cases.every_servant_lists_everything(ls.table))
    assert len(book) == 6 and max(FM.refresh(book.columns())[1].values()) > 1
    tick("a tick without reports", False)
    tick("requests and no report", False, n=2, lease=[100] * 2)
    of = list(cases.held(ls.table).items())
    assert len(of) >= 3
    (s0, ids0), (s1, ids1) = of[0], of[1]
    before = len(book)
    tick("one servant's report replaces its entries", True, reports=[(s0, ids0[::-1] + ids0[:1])],
         key=lambda ids: ids * np.uint64(1 << 32) + np.uint64(9))
    assert len(book) > before and book.B[-1][1] == ids0[0]
    before = len(book)
    tick("an empty report only clears", True, reports=[(s1, [])])
    assert 0 < len(book) < before
    tick("a tick without reports", False)
    # ydc_remove_servants: a row with entries (positions shift, servant_idx follows) ...
    on = sorted({e[0] for e in book.B})
    idle = [s for s in range(ls.es.n) if s not in cases.held(ls.table)]
    assert len(on) >= 2 and idle and idle[0] < on[-1]
    gone = on[0]
    for what, row in (("ydc_remove_servants of a row with entries", gone),
                      ("ydc_remove_servants of a lower row without", min(s - (s > gone) for s in idle if s != gone))):
        n_before, removed = len(book), np.array([row], np.uint32)
        ctx.remove_servants(removed)
        lease.drop_rows(ls, removed)
        book.remove_servants(removed)
        assert len(book) < n_before if row == gone else (len(book) == n_before and row < max(e[0] for e in book.B) + 1)
        b.check_book()
        ask(ctx, book, what, rebuilt=True)
    assert len(book)
    tick("a tick without reports, behind the removals", False)
    ctx.stream_book_begin(512)
    book.grow(512)
    ask(ctx, book, "ydc_stream_book_begin with a larger bound")  # (either value)
    ctx.stream_book_begin(300)  # (smaller: nothing happens)
    ask(ctx, book, "ydc_stream_book_begin that does nothing", rebuilt=False)
    ctx.stream_reserve(max_leases=256, max_report_ids=128)
    ask(ctx, book, "ydc_stream_reserve")  # (either value)
    ctx.stream_reserve(max_leases=256)  # (nothing to do)
    ask(ctx, book, "ydc_stream_reserve that does nothing", rebuilt=False)
    tick("the grown stream reports", True, reports=cases.every_servant_lists_everything(ls.table))
    blob = ctx.stream_snapshot()
    ask(ctx, book, "behind ydc_stream_snapshot", rebuilt=False)
    fresh = binding.Context(device=0)
    fresh.stream_restore(blob)
    ask(fresh, book, "the restored context", rebuilt=True)
    where = ["row %d" % s for s in range(ls.es.n)]
    found = streaming.find_running(fresh, where, [e[3] for e in book.B] + [ABSENT[1]])
    m = {e[3]: (where[e[0]], e[2]) for e in book.B}  # the daemon's map: the last entry wins
    assert found == [m[e[3]] for e in book.B] + [None]
    assert fresh.stream_snapshot() == blob
    fresh.stream_end()
    fresh.close()
    b.close()


class KeyedPlayer(GpuPlayer):
    """tests/test_stream_alive_gpu.py's player with digest keys that collide (task_grant_id % 3)."""

    def tick(self, beat=acases.FAR, append=None, tasks=None, **kw):
        ev = self.make_ev(self.ls, beat, append, tasks, kw)
        x = self.x
        stid, dkey = ev["stid"], np.asarray(ev["report_ids"], np.uint64) % np.uint64(3)
        x.ctx.stream_book_stage(stid, dkey)
        self.book.stage(stid, dkey)
        x.ctx.stream_alive_stage(ev["upd_expires_at"])
        got = lease.gpu_tick(x.ctx, self.ls, ev)
        want = acases.AM.model_tick(L, self.ls, ev)
        lease.check_tick(x.t, x.ctx, self.ls, got, want)
        x.check_alive(want)
        x.t += 1
        return want


def test_a_servant_erased_by_aliveness_inside_a_tick():
    """A tick without any report in which the expiry timer erases a servant that has entries: the
    index is stale, positions shift and servant_idx follows; the next tick erases nobody and it stays."""
    p = KeyedPlayer(cases.small_stream, True)
    acases.victim(p)  # tick 0 grants 8, in tick 1 every holder reports
    of = cases.held(p.T)
    v = sorted(of)[1]  # (entries in front of its own and behind them, on a lower row and on a higher one)
    ids = of[v]
    assert len(of) >= 3 and v != p.next_beater(), "the next heartbeat would extend its life again"
    ctx = p.x.ctx
    ask(ctx, p.book, "behind the reports", rebuilt=True)
    n_before = len(p.book)
    p.set_expiry(v, 0)  # (the column replaced: B untouched)
    ask(ctx, p.book, "behind ydc_stream_alive_begin", rebuilt=False)
    r = p.tick()
    assert list(r["removed"]) == [v] and len(p.book) == n_before - len(ids) and len(p.book)
    assert any(e[0] >= v for e in p.book.B), "no entry on a row behind the erased one"
    ask(ctx, p.book, "behind the tick that erased a servant", rebuilt=True)
    r = p.tick()
    assert len(r["removed"]) == 0
    ask(ctx, p.book, "behind a tick that erased nobody", rebuilt=False)
    p.x.close()


def test_refusals_leave_the_stream_ticking():
    """No book, a plain stream, no stream; n > 0 with NULL columns, 2^24 + 1 queries, too small a cap
    for distinct, pipelined batches outstanding. After each one the stream answers its next tick as
    its twin does."""
    L_ = binding.lib()
    one, hit = np.array([1], np.uint64), np.zeros(1, binding.HIT_DTYPE)
    n, built = C.c_uint32(77), C.c_uint32(77)
    sv = cases.small_stream().es.sv
    ctx = new_ctx(sv)
    with pytest.raises(binding.YdcError, match="no stream is open"):
        ctx.stream_book_find([1])
    plain = new_ctx(sv)
    for c in (ctx, plain):
        c.stream_begin(16, 16, 8)
    for call in (lambda: ctx.stream_book_find([1]), ctx.stream_book_distinct):
        with pytest.raises(binding.YdcError, match="keeps no state"):
            call()
    tk = synth.make_tasks(8, sv, n_envs=1, seed=4, self_frac=0.0)
    none, rows = np.empty(0, np.uint32), np.zeros(0, binding.ROW_DTYPE)
    got = [c.stream_tick(none, rows, none, tk) for c in (ctx, plain)]
    assert np.array_equal(*got) and (got[0] < L.IDX_ENV_NOT_FOUND).any()
    assert np.array_equal(ctx.get_running(), plain.get_running())
    for c in (ctx, plain):
        c.stream_end()
        c.close()

    ls = cases.small_stream()

    def make_ctx():
        c = new_ctx(ls.es.sv)
        c.stream_begin_leased(ls.es.hb + 8, 16, cases.MAX_TASKS, 64, 64, 64, ls.es.n, 64)
        return c

    # No book yet: refused, and the tick behind it is the model's.
    a, twin = make_ctx(), make_ctx()
    for call in (lambda: a.stream_book_find([1]), a.stream_book_distinct):
        with pytest.raises(binding.YdcError, match="no running-task book"):
            call()
    ev = cases.scripted(ls, ls.next_tick(), n=6, lease=[100] * 6)
    want = L.model_tick(ls, ev)
    for c in (a, twin):
        lease.check_tick(0, c, ls, lease.gpu_tick(c, ls, ev), want)
    a.stream_end()
    with pytest.raises(binding.YdcError, match="no stream is open"):
        a.stream_book_distinct()
    a.close()
    twin.stream_end()
    twin.close()

    ls = cases.small_stream()
    p = Pair("leased", ls, make_ctx, 256)
    a = p.b.ctx
    t = [0]

    def tick(**kw):
        ev = cases.scripted(ls, ls.next_tick(), **kw)
        p.tick(ev, *keyed(ev, t[0]))
        t[0] += 1

    tick(n=6, lease=[100] * 6)
    tick(reports=cases.every_servant_lists_everything(ls.table))
    assert len(p.b.book) == 6
    # n == 0 is a call like any other; NULL columns are allowed with it.
    assert L_.ydc_stream_book_find(a._h, None, 0, None, None) == 0
    assert L_.ydc_stream_book_find(a._h, None, 0, None, C.byref(built)) == 0 and built.value == 0
    # n > 0 with NULL columns.
    assert L_.ydc_stream_book_find(a._h, None, 1, hit.ctypes.data, None) == INVALID
    assert L_.ydc_stream_book_find(a._h, one.ctypes.data, 1, None, C.byref(built)) == INVALID and built.value == 0
    assert L_.ydc_stream_book_distinct(a._h, None, None, None, None, None, 0, None, None) == INVALID  # NULL out_n
    tick()
    # 2^24 + 1 queries: refused before a single one is read.
    assert L_.ydc_stream_book_find(a._h, one.ctypes.data, (1 << 24) + 1, hit.ctypes.data, None) == INVALID
    assert "2^24" in L_.ydc_last_error(a._h).decode()
    tick(reports=cases.every_servant_lists_everything(ls.table)[:1])
    # Too small a cap for distinct: *out_n is set and nothing is written.
    want = FM.distinct(p.b.book.columns())
    k = len(want[0])
    assert k >= 2
    room = [np.full(k, 0xAB, d) for d in (np.uint32, np.uint64, np.uint64, np.uint64, np.uint32)]
    rc = L_.ydc_stream_book_distinct(a._h, *[r.ctypes.data for r in room], k - 1, C.byref(n), C.byref(built))
    assert rc == CAPACITY and n.value == k and built.value == 1
    assert all((r == 0xAB).all() for r in room)
    # ... with exactly enough, and with columns left out.
    rc = L_.ydc_stream_book_distinct(a._h, None, room[1].ctypes.data, None, None, room[4].ctypes.data, k, C.byref(n),
                                     C.byref(built))
    assert rc == 0 and n.value == k and built.value == 0
    assert np.array_equal(room[1], want[1]) and np.array_equal(room[4], want[4]) and (room[0] == 0xAB).all()
    tick()
    # Pipelined batches outstanding.
    DA = binding.DeviceArray
    tk = synth.make_tasks(256, ls.es.sv, n_envs=1)
    cols = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
    d_out = DA.from_numpy(np.zeros(256, np.uint32))
    for c in (a, p.twin):  # (the twin gets the batch too: it differs in the asking alone)
        c.dispatch_device_async(*cols, d_out)
    for call in (lambda: a.stream_book_find([1]), a.stream_book_distinct):
        with pytest.raises(binding.YdcError, match="pipelined"):
            call()
    for c in (a, p.twin):
        c.dispatch_wait()
    ask(a, p.b.book, "behind the refusals", rebuilt=False)
    tick(reports=cases.every_servant_lists_everything(ls.table))
    ask(a, p.b.book, "behind the last tick", rebuilt=True)
    p.close()

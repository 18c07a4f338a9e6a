"""The running-task book on the device (ydc_stream_book_begin / _stage / _get; k_book_commit,
k_book_remap): every tick of a leased, waiting-and-leased or rpc stream with a book is compared with
the model (tests/stream_book_model.py, pinned against the verbatim reference's bookkeeper by
tests/test_stream_book_model.py) on B exactly, order included, and — through the modes' own
check_tick — on the tick's outputs, running_tasks and the lease snapshot."""
import numpy as np
import pytest

from tests import stream_book_cases as bcases
from tests import stream_book_model as BM
from tests import stream_lease_cases as cases
from tests import stream_lease_model as L
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WM
from tests import test_stream_lease_gpu as lease
from tests import test_stream_rpc_gpu as rpc
from tests import test_stream_wait_lease_gpu as wl
from tests.test_stream_reserve_gpu import new_ctx, roomy_pool
from tests.test_stream_rpc_model import BIG
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu
MODS = {"leased": (L, lease), "wait_leased": (WM, wl), "rpc": (RM, rpc)}
COLS = ("servant_idx", "task_grant_id", "servant_task_id", "digest_key")
TILE = 1024  # kBookTile


def _graph(monkeypatch, stream_graph):
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    monkeypatch.setenv("YDC_TUNE", "stream_graph=" + stream_graph)  # (what ydc_create reads)


class Booked:
    """A stream `ws` of `mode` on `ctx` with a book of max_book entries, and the model's book."""

    def __init__(self, mode, ws, ctx, max_book, masks=False):
        self.M, self.G = MODS[mode]
        self.ws, self.ctx, self.masks, self.t = ws, ctx, masks, 0
        ctx.stream_book_begin(max_book)
        self.book = BM.Book(max_book)

    def check_book(self):
        got, want = self.ctx.stream_book(), self.book.columns()
        assert len(got[0]) == len(want[0]), "tick %d: |B| gpu %d model %d" % (self.t, len(got[0]), len(want[0]))
        for name, a, b in zip(COLS, got, want):
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, "tick %d: book %s[%d] gpu %d model %d (%d differ)" % (
                self.t, name, bad[0], a[bad[0]], b[bad[0]], bad.size)

    def tick(self, ev, stage=True, snapshot=True):
        if stage:
            p = BM.payload(ev)
            self.ctx.stream_book_stage(*p)
            self.book.stage(*p)
        want = BM.model_tick(self.M, self.ws, self.book, ev)
        got = self.G.gpu_tick(self.ctx, self.ws, ev, self.masks)
        self.G.check_tick(self.t, self.ctx, self.ws, got, want, snapshot=snapshot)
        self.check_book()
        self.t += 1
        return want

    def drive(self, ticks, stage=lambda t: True):
        return [self.tick(self.ws.next_tick(), stage(self.t)) for _ in range(ticks)]

    def refused(self, ev, match, stage=None):
        """The library refuses `ev`; B, L and running_tasks stay."""
        before = self.ctx.stream_book(), self.ctx.stream_leases(), self.ctx.get_running()
        with pytest.raises(binding.YdcError, match=match):
            self.G.gpu_tick(self.ctx, self.ws, ev, self.masks)
        after = self.ctx.stream_book(), self.ctx.stream_leases(), self.ctx.get_running()
        for x, y in zip(before[0] + before[1] + (before[2],), after[0] + after[1] + (after[2],)):
            assert np.array_equal(x, y), "a refused tick changed something"

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def seen(rec, book):
    known = sum(int((r["report_unknown"] == 0).sum()) for r in rec)
    unknown = sum(int(r["report_unknown"].sum()) for r in rec)
    assert known > 20 and unknown > 5 and len(book), (known, unknown, len(book))


@pytest.mark.parametrize("stream_graph", ["1", "0"])
def test_leased_stream_with_a_book(stream_graph, monkeypatch):
    """70 servants, seeded lease traffic with mixed reports, with the captured step and with the
    step enqueued kernel by kernel; every fifth tick stages nothing (zeros)."""
    _graph(monkeypatch, stream_graph)
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    ls = L.LeaseStream(sv, 400, 250, 60, L.LeaseTable(), n_envs=2, report_frac=0.3)
    b = Booked("leased", ls, lease.begin(ls, 1 << 14, 400), 6000)
    seen(b.drive(10, stage=lambda t: t % 5 != 4), b.book)
    b.close()


def test_waiting_leased_stream_with_a_book():
    sv = synth.make_servants(40, n_tasks_hint=2000, n_envs=2, seed=31)
    ws = WM.new_stream(sv, 600, 350, 80, 3000, n_envs=2, rate=lambda now: 1.0 if now % 12 < 8 else 0.125,
                       report_frac=0.3)
    b = Booked("wait_leased", ws, wl.begin(ws, 1 << 14, 600), 6000)
    seen(b.drive(10), b.book)
    b.close()


def test_rpc_stream_with_a_book():
    sv = synth.make_servants(60, n_tasks_hint=2000, n_envs=2, seed=8)
    ws = RM.new_stream(sv, 40, 300, 100, 1000, 1 << 12, n_envs=2, report_frac=0.3, **BIG)
    b = Booked("rpc", ws, rpc.begin(ws, 40), 6000)
    seen(b.drive(10), b.book)
    assert np.array_equal(b.ctx.stream_waiting_take(), ws.state.take())
    b.close()


def test_more_than_256_classes_runs_eagerly():
    """~600 servant classes: every tick is enqueued (eager_only), k_book_commit with it."""
    n_envs = 150
    sv = synth.make_servants(700, n_tasks_hint=9000, n_envs=n_envs, seed=23)
    ls = L.LeaseStream(sv, 1000, 500, 100, L.LeaseTable(), n_envs=n_envs)
    b = Booked("leased", ls, lease.begin(ls, 1 << 15, 1000), 1 << 14, masks=True)
    seen(b.drive(8), b.book)
    b.close()


def hand(max_book=256, max_leases=64):
    ls = cases.small_stream(max_leases)
    ctx = new_ctx(ls.es.sv)
    ctx.stream_begin_leased(ls.es.hb + 8, 16, cases.MAX_TASKS, max_leases, 64, 64, ls.es.n, 64)
    return Booked("leased", ls, ctx, max_book)


@pytest.mark.parametrize("case", bcases.CASES, ids=[c.__name__ for c in bcases.CASES])
def test_hand_written_same_tick_edges(case):
    """tests/stream_book_cases.py: an id freed and reported in one tick, an id of another servant's
    lease, zombies, ids >= next_id, an id twice in one report, empty reports, a servant reporting in
    consecutive ticks, nothing staged."""
    b = hand()
    bcases.play(b.ws, b.book, case(), b.tick)
    assert b.t == len(case())
    b.close()


def test_staged_count_that_does_not_match_is_refused_and_kept():
    b = hand()
    ls = b.ws
    b.tick(cases.scripted(ls, ls.next_tick(), n=6, lease=[100] * 6))
    reports = cases.every_servant_lists_everything(ls.table)
    ev = cases.scripted(ls, ls.next_tick(), reports=reports)
    p = BM.payload(ev)
    b.ctx.stream_book_stage(p[0][:-1], p[1][:-1])
    b.refused(ev, "staged")
    # the staging is still there: it serves a tick of its own count ...
    short = cases.scripted(ls, ev, reports=[(s, ids) for s, ids in reports[:-1]] + [(reports[-1][0], reports[-1][1][:-1])])
    b.book.stage(p[0][:-1], p[1][:-1])
    b.tick(short, stage=False)
    assert len(b.book) == 5 and b.book.B[0][2] == int(p[0][0]) != 0
    # ... and is consumed by it: the next tick's payload is zeros.
    b.tick(cases.scripted(ls, ls.next_tick(), reports=reports), stage=False)
    assert len(b.book) == 6 and all(e[2] == 0 and e[3] == 0 for e in b.book.B)
    b.close()


def test_capacity_bound_and_growth_in_mid_stream():
    """|B| + n_ids == max_book is accepted, one more is refused with everything unchanged, and after
    ydc_stream_book_begin with a larger bound the refused tick is accepted, entries and order kept."""
    b = hand(max_book=10)
    ls = b.ws
    b.tick(cases.scripted(ls, ls.next_tick(), n=6, lease=[100] * 6))
    of = cases.held(ls.table)
    (sa, ia), rest = list(of.items())[0], list(of.items())[1:]
    b.tick(cases.scripted(ls, ls.next_tick(), reports=rest))
    n_b = len(b.book)
    assert n_b == 6 - len(ia) and n_b >= 1
    fill = [ia[0]] * (10 - n_b)  # (an id may be listed any number of times)
    ev = cases.scripted(ls, ls.next_tick(), reports=[(sa, fill + [ia[0]])])
    with pytest.raises(OverflowError):
        b.book.check(ev)
    b.ctx.stream_book_stage(*BM.payload(ev))
    b.refused(ev, "max_book")
    b.ctx.stream_book_begin(5)  # (smaller: nothing happens)
    b.refused(ev, "max_book")
    b.ctx.stream_book_begin(11)
    b.book.grow(11)
    b.check_book()
    b.book.stage(*BM.payload(ev))  # (the library still holds the refused tick's staging)
    b.tick(ev, stage=False)
    assert len(b.book) == 11 and b.book.B[-1][2] != 0
    # exactly full: a tick whose servant is replaced by as many ids is refused all the same
    # (conservative), an empty report is not.
    ev = ls.next_tick()
    b.refused(cases.scripted(ls, ev, reports=[(sa, [ia[0]])]), "max_book")
    b.tick(cases.scripted(ls, ev, reports=[(sa, [])]))
    assert len(b.book) == n_b
    b.tick(cases.scripted(ls, ls.next_tick(), reports=[(sa, [ia[0]] * (11 - n_b))]))
    assert len(b.book) == 11
    b.close()


@pytest.mark.parametrize("tiles", [2, 64, 65, 129])
def test_book_pass_over_a_grid_of(tiles):
    """max_book + max_report_ids = (tiles - 1) * 1024 + 515 positions (a partial last tile, no
    multiple of 4), B nearly as long as max_book. Two ticks fill B from the id region (every entry
    moves left by about max_book positions; with 129 tiles the second half looks back over more
    than 64 tiles and B ends behind position 65 536); then the servants at B's head report empty
    lists and are dropped while the tail is kept (the largest left shift inside B); then the tail's
    servants are dropped while the head stays; then the first servants list theirs again."""
    P = (tiles - 1) * TILE + 515
    max_book = P // 2 + 30
    max_ids = P - max_book
    G = max_book - 40
    assert (max_book + max_ids + TILE - 1) // TILE == tiles and P % 4 == 3 and (tiles < 129 or G > 65536)
    n_sv = 64
    sv = roomy_pool(n_sv, G // n_sv + 8)
    ls = L.LeaseStream(sv, G, 0, 0, L.LeaseTable(), n_envs=1)
    ctx = new_ctx(sv)
    ctx.stream_begin_leased(ls.es.hb + 8, 16, G, 1 << 18, 16, 16, n_sv, max_ids)
    b = Booked("leased", ls, ctx, max_book)

    def tick(**kw):
        n = kw.get("n", 0)
        ev = ls.next_tick()
        ev = lease.quiet(ev, tasks=synth.make_tasks(n, ls.es.sv, n_envs=1, seed=7, self_frac=0.0),
                         release_idx=np.empty(0, np.uint32), lease_expires_at=np.full(n, 1000, np.int64))
        if "reports" in kw:
            rep = kw["reports"]
            ev.update(report_servants=np.array([s for s, _ in rep], np.uint32),
                      report_off=np.cumsum([0] + [len(i) for _, i in rep]).astype(np.uint32),
                      report_ids=np.array([t for _, i in rep for t in i], np.uint64))
        return b.tick(ev, snapshot=False)

    r = tick(n=G)
    assert (r["out"] < L.IDX_ENV_NOT_FOUND).all()
    of = list(cases.held(ls.table).items())
    assert len(of) >= 16
    half = len(of) // 2
    assert max(sum(len(i) for _, i in of[:half]), sum(len(i) for _, i in of[half:])) <= max_ids
    tick(reports=of[:half])
    tick(reports=of[half:])
    assert len(b.book) == G and [e[1] for e in b.book.B[:3]] == of[0][1][:3]
    tick(reports=[(s, []) for s, _ in of[:half]])
    assert 0 < len(b.book) < G and b.book.B[0][0] == of[half][0]
    quarter = half + (len(of) - half) // 2
    tick(reports=[(s, []) for s, _ in of[quarter:]])
    assert b.book.B[0][0] == of[half][0] and b.book.B[-1][0] == of[quarter - 1][0]
    tick(reports=[(s, ids[::-1]) for s, ids in of[:half]])
    assert b.book.B[0][0] == of[half][0] and b.book.B[-1][1] == of[half - 1][1][0]
    b.close()


def test_captured_passes_run_out_with_a_book():
    """The second eager exit (tests/test_stream_lease_edges_gpu.py) with report traffic in the tick:
    k_book_commit ran once, in the captured step; what the host places again leaves B alone."""
    from tests.test_stream_lease_edges_gpu import Exits, _huge_servants
    ls = L.LeaseStream(_huge_servants(), 150_000, 100_000, 2000, L.LeaseTable(), n_envs=3, report_frac=0.5)
    b = Booked("leased", ls, lease.begin(ls, 1 << 20, 150_000, frees=1 << 17, report_ids=1 << 19), 1 << 20)
    ex, reported = Exits(), []
    for t in range(5):
        ev = ls.next_tick()
        b.tick(ev, snapshot=False)
        ex.note(t, b.ctx)
        reported.append(len(ev["report_ids"]))
    assert [t for t in ex.taken if reported[t] and t < 4], (ex.rounds, ex.taken, reported)
    assert len(b.book) > 1000
    b.close()


def test_bin_overflow_with_a_book():
    """The first eager exit (tests/test_stream_wait_lease_gpu.py: the registry that overflows a bin
    in tick 4) on a waiting-and-leased stream with a book."""
    from tests.test_binsort_gpu import _context, _crowded_bin_pool
    sv = _crowded_bin_pool()
    sv["max_tasks"][48:] = 0
    sv["version"][47], sv["num_processors"][47], sv["max_tasks"][47] = 30, 1, 1
    ws = wl.Picky(sv, 3000, 1000, 200, WM.WaitLeaseState(6000), rate=lambda now: 1.0)
    c = _context(True)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        c.stream_begin_waiting_leased(4096 + 8, 16, 3000, 6000, 1 << 15, 4096, 8192, ws.n_rep, 1 << 17)
        b = Booked("wait_leased", ws, c, 1 << 17)
        b.drive(2)
        ws.rep_pos = 0  # (the servants that hold the leases report: B is not empty when the exit comes)
        b.drive(2)
        assert c.stats()["radix_passes"] == 0 and len(b.book)
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
        assert len(ev["report_ids"])
        n_before = len(b.book)
        b.tick(ev)
        assert c.stats()["radix_passes"] >= 1 and len(b.book) and n_before
        b.drive(2)
        c.stream_end()
    finally:
        c.close()


def test_remove_servants_with_entries_on_removed_and_surviving_rows():
    sv = synth.make_servants(80, n_tasks_hint=3000, n_envs=2, seed=11)
    ls = L.LeaseStream(sv, 500, 300, 80, L.LeaseTable(), n_envs=2, report_frac=0.4)
    b = Booked("leased", ls, lease.begin(ls, 1 << 15, 500), 1 << 13)
    b.drive(6)
    on = {e[0] for e in b.book.B}
    removed = np.array(sorted(on)[1:8:3], np.uint32)
    assert len(removed) == 3 and any(s > removed[-1] for s in on) and any(s < removed[0] for s in on)
    b.ctx.remove_servants(removed)
    lease.drop_rows(ls, removed)
    n_before = len(b.book)
    b.book.remove_servants(removed)
    assert 0 < len(b.book) < n_before
    b.check_book()
    b.drive(5)
    b.close()


def test_reserve_carries_the_book():
    """Twins as in tests/test_stream_reserve_gpu.py: A begun large, B begun small and reserved in
    mid-stream with a non-empty book and a staging pending; both equal the model afterwards."""
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    streams = [L.LeaseStream(sv, 400, 250, 60, L.LeaseTable(), n_envs=2, report_frac=0.3) for _ in range(2)]
    a = Booked("leased", streams[0], lease.begin(streams[0], 1 << 14, 400), 6000)
    small = new_ctx(sv)
    small.stream_begin_leased(streams[1].es.hb + 8, 16, 400, 3000, 4096, 8192, streams[1].n_rep, 1 << 17)
    s = Booked("leased", streams[1], small, 6000)
    for x in (a, s):
        x.drive(5)
    assert len(s.book) > 20 and s.book.B == a.book.B
    ev = s.ws.next_tick()
    p = BM.payload(ev)
    s.ctx.stream_book_stage(*p)
    s.ctx.stream_reserve(max_leases=1 << 14, max_tasks=500, max_report_ids=1 << 18)
    s.check_book()
    s.book.stage(*p)
    s.tick(ev, stage=False)
    a.tick(a.ws.next_tick())
    for x in (a, s):
        x.drive(4)
    assert s.book.B == a.book.B and len(s.book)
    for x, y in zip(a.ctx.stream_book(), s.ctx.stream_book()):
        assert np.array_equal(x, y)
    a.close()
    s.close()


def test_calls_on_the_wrong_context_or_with_the_book_off():
    sv = roomy_pool(8, 8)
    ctx = new_ctx(sv)
    with pytest.raises(binding.YdcError, match="ydc_stream_book_begin"):
        ctx.stream_book_begin(16)  # no stream
    ctx.stream_begin(16, 16, 8)
    with pytest.raises(binding.YdcError, match="ydc_stream_book_begin"):
        ctx.stream_book_begin(16)  # a plain stream
    ctx.stream_end()
    ctx.stream_begin(16, 16, 8, max_waiting=8)
    with pytest.raises(binding.YdcError, match="ydc_stream_book_begin"):
        ctx.stream_book_begin(16)  # a waiting stream without leases
    ctx.stream_end()
    ctx.stream_begin_leased(16, 16, 8, 64, 8, 8, 8, 64)
    with pytest.raises(binding.YdcError, match="ydc_stream_book_get"):
        ctx.stream_book()  # the book is off
    with pytest.raises(binding.YdcError, match="ydc_stream_book_stage"):
        ctx.stream_book_stage([1], [2])
    with pytest.raises(binding.YdcError, match="ydc_stream_book_begin"):
        ctx.stream_book_begin(0)
    with pytest.raises(binding.YdcError, match="max_book"):
        ctx.stream_book_begin((1 << 30) + 1)
    ctx.stream_book_begin(16)
    assert all(len(c) == 0 for c in ctx.stream_book())
    with pytest.raises(binding.YdcError, match="max_report_ids"):
        ctx.stream_book_stage(np.zeros(65, np.uint64), None)
    caps = ctx.stream_caps()
    assert "max_book" not in caps and len(caps) == 10
    # the next begin call switches the book off
    ctx.stream_begin_leased(16, 16, 8, 64, 8, 8, 8, 64)
    with pytest.raises(binding.YdcError, match="ydc_stream_book_get"):
        ctx.stream_book()
    ctx.stream_end()
    ctx.close()

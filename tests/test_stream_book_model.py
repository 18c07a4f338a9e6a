"""The running-task book's model (tests/stream_book_model.py) against the verbatim reference class:
seeded lease streams and the hand-written ticks of tests/stream_book_cases.py go tick by tick through
NotifyServantRunningTasks and GetRunningTasks of oracle/_ref, and after every tick the multiset of
(task_grant_id, servant_task_id) the reference holds is the model's (the reference's own order is
that of an unordered_map). Hand cases with literal values pin the order and the refusals; the ABI
carries the three calls."""
import os
import re

import numpy as np
import pytest

from oracle import refbind as R
from tests import stream_book_cases as bcases
from tests import stream_book_model as BM
from tests import stream_lease_cases as cases
from tests import stream_lease_model as M
from tests.conftest import ROOT
from yadcc_amd import binding, synth

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")


class BookReplay(M.ReferenceReplay):
    """ReferenceReplay whose reports carry servant_task_id, and the reference's GetRunningTasks."""

    def tick(self, ev, stid):
        off, calls = ev["report_off"], iter(range(len(ev["report_servants"])))
        plain = self.ref.notify_servant_running_tasks

        def notify(location, grant_ids, servant_task_ids=None):
            r = next(calls)
            return plain(location, grant_ids, stid[off[r]:off[r + 1]])

        self.ref.notify_servant_running_tasks = notify
        try:
            return super().tick(ev)
        finally:
            del self.ref.notify_servant_running_tasks

    def pairs(self):
        """(task_grant_id as the stream numbers it, servant_task_id), sorted."""
        return sorted((g - self.base, st) for st, g in self.ref.get_running_tasks())


def both(ls_model, ls_ref, book, ref, ev_of, stage, t):
    """One tick through the model (on ls_model) and the reference (on ls_ref's shadow table)."""
    ev = ev_of(ls_model)
    ev_ref = ev_of(ls_ref)
    stid, dkey = BM.payload(ev) if stage else (np.zeros(len(ev["report_ids"]), np.uint64),) * 2
    if stage:
        book.stage(stid, dkey)
    want = BM.model_tick(M, ls_model, book, ev)
    got = ref.tick(ev_ref, stid)
    assert np.array_equal(want["report_unknown"], got["report_unknown"]), t
    assert book.pairs() == ref.pairs(), "tick %d: the book differs from the reference's" % t
    return want


@needs_ref
@pytest.mark.parametrize("shape", [
    # servants, requests / tick, frees / tick, renewals / tick, ticks, digests, servant seed, stream seed
    (60, 300, 200, 60, 30, 2, 3, 83),
    (150, 600, 400, 100, 30, 2, 42, 7),
    (90, 400, 250, 80, 30, 3, 8, 19),
])
def test_seeded_streams_against_the_reference_bookkeeper(shape):
    n_sv, tasks, frees, renewals, ticks, n_envs, seed, sseed = shape
    sv = synth.make_servants(n_sv, n_tasks_hint=tasks * 6, n_envs=n_envs, seed=seed)
    a = M.LeaseStream(sv, tasks, frees, renewals, M.LeaseTable(), n_envs=n_envs, seed=sseed)
    b = M.LeaseStream(sv, tasks, frees, renewals, M.LeaseTable(), n_envs=n_envs, seed=sseed)
    book, ref = BM.Book(), BookReplay(b)
    seen = dropped = 0
    try:
        for t in range(ticks):
            before = len(book)
            want = both(a, b, book, ref, lambda ls: ls.next_tick(), t % 5 != 4, t)
            seen += int((want["report_unknown"] == 0).sum())
            dropped += len(book) < before
    finally:
        ref.close()
    assert seen > 100 and dropped and len(book), (seen, dropped, len(book))


@needs_ref
@pytest.mark.parametrize("case", bcases.CASES, ids=[c.__name__ for c in bcases.CASES])
def test_hand_written_ticks_against_the_reference_bookkeeper(case):
    a, b = cases.small_stream(), cases.small_stream()
    book, ref = BM.Book(), BookReplay(b)
    try:
        steps, step_b = case(), iter(case())
        t = [0]

        def tick(ev, stage):
            make_b, _ = next(step_b)
            ev_b = b.next_tick()
            kw = make_b(b.table, int(ev_b["now"]))
            kw.pop("stage", None)
            stid, dkey = BM.payload(ev) if stage else (np.zeros(len(ev["report_ids"]), np.uint64),) * 2
            if stage:
                book.stage(stid, dkey)
            want = BM.model_tick(M, a, book, ev)
            got = ref.tick(cases.scripted(b, ev_b, **kw), stid)
            assert np.array_equal(want["report_unknown"], got["report_unknown"]), t[0]
            assert book.pairs() == ref.pairs(), "tick %d: the book differs from the reference's" % t[0]
            t[0] += 1
            return want

        bcases.play(a, book, steps, tick)
        assert t[0] == len(steps)
    finally:
        ref.close()


def test_hand_written_ticks_on_the_model_alone():
    for case in bcases.CASES:
        ls, book = cases.small_stream(), BM.Book()
        bcases.play(ls, book, case(), bcases.tick_on_model(ls, book))


def _ev(reports, now=0):
    off = np.cumsum([0] + [len(ids) for _, ids in reports]).astype(np.uint32)
    return {"now": now, "report_servants": np.array([s for s, _ in reports], np.uint32), "report_off": off,
            "report_ids": np.array([t for _, ids in reports for t in ids], np.uint64)}


def test_order_staging_and_refusals_by_hand():
    B = BM.Book(max_book=6)
    ev = _ev([(2, [10, 11]), (0, [12])])
    B.stage([1, 2, 3], [7, 8, 9])
    B.check(ev)
    B.apply(ev, [0, 0, 0])
    assert B.B == [(2, 10, 1, 7), (2, 11, 2, 8), (0, 12, 3, 9)]
    # servant 2 reports again: its entries go, the survivor first, then the permitted ids in report
    # order; an id twice gives two entries; nothing staged: zeros.
    ev = _ev([(2, [11, 11, 99])])
    B.check(ev)
    B.apply(ev, [0, 0, 1])
    assert B.B == [(0, 12, 3, 9), (2, 11, 0, 0), (2, 11, 0, 0)]
    # a staged count that does not match: refused, the staging stays and serves the right tick.
    B.stage([5], None)
    with pytest.raises(ValueError):
        B.check(_ev([(1, [40, 41])]))
    assert B.B == [(0, 12, 3, 9), (2, 11, 0, 0), (2, 11, 0, 0)] and B.staged is not None
    ev = _ev([(1, [40])])
    B.check(ev)
    B.apply(ev, [0])
    assert B.B[-1] == (1, 40, 5, 0) and B.staged is None
    # |B| + n_ids == max_book is accepted (conservative: the ids count whether permitted or not) ...
    ev = _ev([(3, [50, 51])])
    B.check(ev)
    # ... one more is refused, until the book grows.
    ev3 = _ev([(3, [50, 51, 52])])
    with pytest.raises(OverflowError):
        B.check(ev3)
    B.grow(7)
    B.check(ev3)
    # an empty report only clears; removal drops and renumbers.
    B.apply(_ev([(2, [])]), [])
    assert B.B == [(0, 12, 3, 9), (1, 40, 5, 0)]
    B.remove_servants([0])
    assert B.B == [(0, 40, 5, 0)]
    assert [list(c) for c in B.columns()] == [[0], [40], [5], [0]]


def test_abi_carries_the_book():
    assert binding.ABI_VERSION == 8
    src = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define YDC_ABI_VERSION 8u", src)
    for name in ("ydc_stream_book_begin", "ydc_stream_book_stage", "ydc_stream_book_get"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.ABI_SYMBOLS
    assert [k for k, _ in binding.StreamCaps._fields_][-1] == "max_report_ids" and len(binding.StreamCaps._fields_) == 10

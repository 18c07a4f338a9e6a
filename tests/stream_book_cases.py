"""Hand-written ticks for the running-task book (tests/stream_book_model.py), on the small pool and
with the helpers of tests/stream_lease_cases.py. Played through the model and the verbatim
reference class (tests/test_stream_book_model.py) and on the GPU (tests/test_stream_book_gpu.py).

A step is (make, expect): make(T, now) -> the tick's lease traffic as in stream_lease_cases, plus
"stage": True (payload columns staged, the default) or False (nothing staged: zeros);
expect(r, T, book) asserts that the step met its situation.
"""
from tests import stream_book_model as BM
from tests import stream_lease_cases as cases
from tests.stream_lease_cases import held, idle_servants


def play(ls, book, steps, tick):
    """tick(ev, stage) -> the tick's record; it advances ls.table and book."""
    for make, expect in steps:
        ev = ls.next_tick()
        kw = make(ls.table, int(ev["now"]))
        stage = kw.pop("stage", True)
        r = tick(cases.scripted(ls, ev, **kw), stage)
        if expect:
            expect(r, ls.table, book)


def grant(n, lease):
    make, expect = cases.grant(n, lease)
    return make, (lambda r, T, book: expect(r, T))


def everything(T, now):
    return dict(reports=cases.every_servant_lists_everything(T))


def all_listed(r, T, book):
    assert not r["report_unknown"].any() and len(book) == len(T.L) == len(r["report_unknown"])
    assert sorted(e[1] for e in book.B) == sorted(T.L)


def freed_and_reported():
    """An id freed by id and listed by its servant in the same tick is unknown: no entry; the
    servant's other ids are entries."""
    def make(T, now):
        sa, ia = max(held(T).items(), key=lambda kv: len(kv[1]))
        assert len(ia) >= 2
        return dict(free=[ia[0]], reports=[(sa, ia)])

    def expect(r, T, book):
        assert list(r["report_unknown"])[0] == 1 and not r["report_unknown"][1:].any() and r["freed"] == 1
        assert len(book) == len(r["report_unknown"]) - 1

    return [grant(8, 100), (make, expect)]


def report_oddities():
    """Six leases, two of them zombies from now == 2 on. All listed and known at now == 1. At now == 2
    servant a lists its first id twice, an id of servant b, ids not handed out and its own (perhaps
    zombie) ids; an idle servant lists a's id; another idle one reports nothing; nothing is staged.
    At now == 3 servant a reports again (replaced once more) and servant b reports an empty list
    (cleared); the others keep theirs."""
    mem = {}

    def at2(T, now):
        assert now == 2
        (sa, ia), (sb, ib) = mem["ab"] = list(held(T).items())[:2]
        z, w = idle_servants(T)[:2]
        return dict(stage=False, reports=[(sa, [ia[0], ia[0], ib[0], T.next_id, T.next_id + 5] + ia),
                                          (z, [ia[0]]), (w, [])])

    def second(r, T, book):
        (sa, ia), (sb, ib) = mem["ab"]
        assert r["expired"] == 2 and r["unknown_reported"] >= 4
        mine = [e for e in book.B if e[0] == sa]
        live = [t for t in ia if not T.L[t][2]]
        want = ([ia[0]] * 2 if ia[0] in live else []) + live
        assert [e[1] for e in mine] == want and all(e[2] == 0 and e[3] == 0 for e in mine)
        assert book.B[-len(mine):] == mine or not mine  # (this tick's ids stand behind the survivors)
        assert any(e[0] == sb for e in book.B)  # (b did not report: kept, zombies included)

    def at3(T, now):
        (sa, ia), (sb, ib) = mem["ab"]
        return dict(reports=[(sb, []), (sa, ia[::-1])])

    def third(r, T, book):
        (sa, ia), (sb, ib) = mem["ab"]
        assert not any(e[0] == sb for e in book.B)
        assert [e[1] for e in book.B if e[0] == sa] == [t for t in ia[::-1] if not T.L[t][2]]
        assert all(e[2] != 0 for e in book.B if e[0] == sa)

    return [grant(6, [1, 1, 100, 100, 100, 100]), (everything, all_listed), (at2, second), (at3, third)]


def zombie_listed_then_swept():
    """Every lease turns zombie while in the book; their servants list them again: all unknown, the
    book empties although the leases stay; then empty reports sweep them."""
    def gone(r, T, book):
        assert r["report_unknown"].all() and len(book) == 0 and r["n_leases"] == 4 and r["swept"] == 0

    def swept(r, T, book):
        assert r["swept"] == 4 and len(book) == 0

    return [grant(4, 1), (everything, all_listed), (everything, gone),
            ((lambda T, now: dict(reports=[(s, []) for s in held(T)])), swept)]


CASES = [freed_and_reported, report_oddities, zombie_listed_then_swept]


def tick_on_model(ls, book):
    from tests import stream_lease_model as M

    def tick(ev, stage):
        if stage:
            book.stage(*BM.payload(ev))
        return BM.model_tick(M, ls, book, ev)
    return tick

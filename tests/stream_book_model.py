"""The running-task book B of a leased stream (ydc_stream_book_begin / _stage / _get) as a plain
list: the yardstick of tests/test_stream_book_gpu.py, pinned against the verbatim reference's
RunningTaskBookkeeper by tests/test_stream_book_model.py.

It wraps the lease models (tests/stream_lease_model.py and the two built on it) and changes nothing
in them: a tick's report_unknown is theirs. Step 6 of a leased tick, for B
(task_dispatcher.cc:222-277, running_task_bookkeeper.cc:24-43):
  - every entry of a servant that reports in the tick is dropped (SetServantRunningTasks replaces
    the servant's list);
  - every reported id k with report_unknown[k] == 0 becomes an entry (servant, id,
    servant_task_id[k], digest_key[k]); an id listed twice gives two; an empty report only clears;
  - servants that do not report keep theirs.
B's order is defined where the reference's (an unordered_map of vectors) is not: the survivors in
their previous order, then the tick's permitted ids in report order.
"""
import numpy as np


class Book:
    def __init__(self, max_book=1 << 30):
        self.max_book = max_book
        self.B = []  # (servant, task_grant_id, servant_task_id, digest_key)
        self.staged = None  # (servant_task_id, digest_key) for the next accepted tick

    def __len__(self):
        return len(self.B)

    def grow(self, max_book):
        """ydc_stream_book_begin on a stream that has a book: larger or nothing."""
        self.max_book = max(self.max_book, max_book)

    def stage(self, servant_task_id=None, digest_key=None, n_ids=None):
        if n_ids is None:
            n_ids = len(servant_task_id if servant_task_id is not None else digest_key)
        z = np.zeros(n_ids, np.uint64)
        self.staged = (z if servant_task_id is None else np.asarray(servant_task_id, np.uint64),
                       z if digest_key is None else np.asarray(digest_key, np.uint64))
        assert len(self.staged[0]) == len(self.staged[1]) == n_ids

    def check(self, ev):
        """The refusals that leave everything untouched, the staging included."""
        n_ids = len(ev["report_ids"])
        if self.staged is not None and len(self.staged[0]) != n_ids:
            raise ValueError("staged count differs from the tick's")
        if len(self.B) + n_ids > self.max_book:
            raise OverflowError("max_book")

    def apply(self, ev, report_unknown):
        """The accepted tick's reports with the lease model's answers; consumes the staging."""
        n_ids = len(ev["report_ids"])
        stid, dkey = self.staged if self.staged is not None else (np.zeros(n_ids, np.uint64),) * 2
        self.staged = None
        reporting = set(ev["report_servants"].tolist())
        B = [e for e in self.B if e[0] not in reporting]
        off, ids = ev["report_off"], ev["report_ids"]
        for r, s in enumerate(ev["report_servants"].tolist()):
            for k in range(int(off[r]), int(off[r + 1])):
                if not report_unknown[k]:
                    B.append((s, int(ids[k]), int(stid[k]), int(dkey[k])))
        self.B = B

    def remove_servants(self, removed):
        """ydc_remove_servants (DropServant): entries of removed rows vanish, the others follow the
        registry's compaction."""
        removed = np.asarray(removed, np.int64)
        gone = set(removed.tolist())
        self.B = [(e[0] - int(np.searchsorted(removed, e[0])),) + e[1:] for e in self.B if e[0] not in gone]

    def columns(self):
        """As ydc_stream_book_get: (servant_idx, task_grant_id, servant_task_id, digest_key)."""
        return (np.array([e[0] for e in self.B], np.uint32), np.array([e[1] for e in self.B], np.uint64),
                np.array([e[2] for e in self.B], np.uint64), np.array([e[3] for e in self.B], np.uint64))

    def pairs(self):
        """The multiset of (task_grant_id, servant_task_id), sorted."""
        return sorted((e[1], e[2]) for e in self.B)


def payload(ev, salt=0):
    """Payload columns for a tick's reports: distinct per position, so that a misplaced entry shows."""
    ids = np.asarray(ev["report_ids"], np.uint64)
    k = np.arange(len(ids), dtype=np.uint64)
    now = np.uint64(int(ev["now"]) + salt)
    return ((ids * np.uint64(1000003) + k * np.uint64(7) + now) & np.uint64((1 << 63) - 1),
            (k * np.uint64(0x9E3779B97F4A7C15) + now * np.uint64(31) + np.uint64(5)))


def model_tick(M, ws, book, ev, place=None):
    """One tick of the lease model M (its model_tick) with the book behind it: refusals first, then
    the lease model's tick, then B from its report_unknown. -> M's record."""
    book.check(ev)
    r = M.model_tick(ws, ev, place) if place else M.model_tick(ws, ev)
    book.apply(ev, r["report_unknown"])
    return r

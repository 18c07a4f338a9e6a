"""Withdrawal by tag (ydc_stream_withdraw_begin / _stage / _result) as a plain model: the yardstick of
tests/test_stream_withdraw_gpu.py. A thin wrapper over the waiting queue's, the waiting + leased and
the rpc models (tests/stream_wait_model.WaitQueue, tests/stream_wait_lease_model.WaitLeaseState,
tests/stream_rpc_model.RpcState), none of which is edited:

  - before a tick, the deadline of every entry of W whose tag is staged becomes the smallest int64;
  - the base tick runs: the entry is expired, so it resolves as Timeout at its queue position,
    untried, and consumes nothing;
  - resolved entries whose tag is staged are relabelled IDX_WITHDRAWN (every entry of W with a
    staged tag was withdrawn, and a new request never enters the resolved list);
  - the entries removed are counted per staged tag, in the caller's order.

A refused tick leaves W and the staging as they were; an accepted tick consumes the staging.
"""
import numpy as np

from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WL

IDX_WITHDRAWN = 0xFFFFFFFC
IDX_TIMEOUT = WL.IDX_TIMEOUT
I64_MIN = np.iinfo(np.int64).min


class Withdrawal:
    """The capability of one stream. queue(): the model's W (an object with .tag and .deadline)."""

    def __init__(self, queue, max_withdraw):
        self.queue, self.max_withdraw = queue, max_withdraw
        self.staged = None  # the caller's tags for the next accepted tick
        self.result = (np.empty(0, np.uint32), 0)  # of the most recent accepted tick

    def begin(self, max_withdraw):
        if max_withdraw == 0 or max_withdraw > 1 << 30:
            raise ValueError("max_withdraw")
        self.max_withdraw = max(self.max_withdraw, max_withdraw)

    def stage(self, tags):
        tags = np.asarray(tags, np.uint64).copy()
        if len(tags) > self.max_withdraw:
            raise OverflowError("max_withdraw")
        self.staged = tags if len(tags) else None

    def tick(self, base, label):
        """base() runs the base model's tick -> its record; label: the record's key (or tuple index) of
        the resolved answers, "res_tags" / index 1 holding their tags. -> the record, relabelled."""
        q = self.queue()
        tags = self.staged if self.staged is not None else np.empty(0, np.uint64)
        hit = np.isin(q.tag, tags)
        before_tag, before_dl = q.tag.copy(), q.deadline
        q.deadline = np.where(hit, I64_MIN, q.deadline)
        try:
            r = base()
        except Exception:
            self.queue().deadline = before_dl  # (refused: nothing applied, the staging kept)
            raise
        self.staged = None
        self.result = (np.array([int((before_tag[hit] == t).sum()) for t in tags], np.uint32), int(hit.sum()))
        if isinstance(r, tuple):  # WaitQueue.tick: (out, resolved_tags, resolved_idx, n_waiting, got)
            r = list(r)
            r[label] = np.where(np.isin(r[1], tags), np.uint32(IDX_WITHDRAWN), r[label]).astype(np.uint32)
            return tuple(r)
        r[label] = np.where(np.isin(r["res_tags"], tags), np.uint32(IDX_WITHDRAWN), r[label]).astype(np.uint32)
        return r


def waiting(q, max_withdraw):
    """A WaitQueue with the capability: tick(place, tasks, deadlines, tags, now) as WaitQueue.tick."""
    w = Withdrawal(lambda: q, max_withdraw)
    w.run = lambda place, tasks, deadlines, tags, now: w.tick(lambda: q.tick(place, tasks, deadlines, tags, now), 2)
    return w


def wait_lease(ws, max_withdraw):
    """A WaitLeaseStream with the capability: run(ev, place=None) as stream_wait_lease_model.model_tick."""
    w = Withdrawal(lambda: ws.state.q, max_withdraw)
    w.run = lambda ev, place=None: w.tick(lambda: WL.model_tick(ws, ev, place), "res_idx")
    return w


def rpc(ws, max_withdraw):
    """An RpcStream with the capability: run(ev, place=None) as stream_rpc_model.model_tick."""
    w = Withdrawal(lambda: ws.state.q, max_withdraw)
    w.run = lambda ev, place=None: w.tick(lambda: RM.model_tick(ws, ev, place), "res_status")
    return w


def unlabelled(a):
    """A resolved answer column with the label taken back: what the base model says of a stream in
    which the withdrawn entries' deadlines had passed."""
    a = np.asarray(a, np.uint32)
    return np.where(a == IDX_WITHDRAWN, np.uint32(IDX_TIMEOUT), a)

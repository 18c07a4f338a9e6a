"""Departure of requestors (ydc_stream_depart_begin / _stage / _result) as a plain model: the yardstick of
tests/test_stream_depart_gpu.py. A thin wrapper over the leased, the waiting + leased and the rpc models
with inspection attached (tests/stream_lease_model, tests/stream_wait_lease_model, tests/stream_rpc_model,
tests/stream_inspect_model); it composes with tests/stream_withdraw_model, tests/stream_quota_model and
tests/stream_alive_model, and edits none of them. With the set R staged:

  - before the base tick, the ids that Inspect.tasks() attributes to a requestor in R (a lease without
    details belongs to nobody) and that the caller's own frees leave in L are appended to the event's
    free_ids: one FreeTask each, behind the caller's;
  - the deadline of every entry of W whose requestor is in R becomes the smallest int64, unless it is
    that already (withdrawal's mark of the same tick: Withdrawal.tick runs OUTSIDE this wrapper, so
    its mark is there first and the entry is withdrawal's);
  - the base tick runs on that event: this IS the defining property, the model has no other semantics;
  - the counts per staged requestor, in the caller's order, come from the state before and after.

A refused tick leaves W and the staging as they were; an accepted tick consumes the staging.

Composition, outermost first: Withdrawal.tick(lambda: Departure.tick(ev, base), label), with
base = Quota.tick where the stream has a quota (its probe then sees the appended frees and the marked
entries, so a requestor at its cap that departs and asks again in one tick is admitted).
"""
import numpy as np

from tests import stream_inspect_model as IM

I64_MIN = np.iinfo(np.int64).min
NO_TIME = IM.NO_TIME
COLUMNS = ("requestor_ip", "leases", "zombies", "waiting", "waiting_rows")


class Departure:
    """The capability of one stream `ws` (of any of the three lease models, inspection attached)."""

    def __init__(self, ws, max_depart):
        self.ws, self.max_depart = ws, 0
        self.begin(max_depart)
        self.staged = None  # the caller's requestors for the next accepted tick
        self.result = ({k: np.empty(0, np.uint32) for k in COLUMNS}, 0, 0)  # of the most recent accepted tick
        self.freed_ids = np.empty(0, np.uint64)  # ... and the leases it freed beyond the caller's own

    def begin(self, max_depart):
        if getattr(self.ws.table, "inspect", None) is None:
            raise ValueError("inspection is off")
        if max_depart == 0 or max_depart > 1 << 24:
            raise ValueError("max_depart")
        self.max_depart = max(self.max_depart, max_depart)

    def stage(self, requestors):
        r = np.asarray(requestors, np.uint32).copy()
        if len(r) > self.max_depart:
            raise OverflowError("max_depart")
        self.staged = r if len(r) else None

    def queue(self):
        st = getattr(self.ws, "state", None)
        return None if st is None else st.q

    def tick(self, ev, base):
        """base(ev) runs the base model's tick on the event it is given -> its record, returned as it is."""
        R = self.staged if self.staged is not None else np.empty(0, np.uint32)
        tk = self.ws.table.inspect.tasks()
        own = np.asarray(ev["free_ids"], np.uint64)
        mine = (tk["started_at"] != NO_TIME) & np.isin(tk["requestor_ip"], R) & ~np.isin(tk["task_id"], own)
        ids, l_ip, l_zombie = tk["task_id"][mine], tk["requestor_ip"][mine], tk["zombie"][mine] != 0
        ev2 = dict(ev, free_ids=np.concatenate([own, ids]).astype(np.uint64))
        q = self.queue()
        if q is not None:
            before_dl = q.deadline
            hit = np.isin(q.cols["requestor_ip"], R) & (q.deadline != I64_MIN)
            w_ip = q.cols["requestor_ip"][hit]
            w_rows = (q.cols["n_imm"][hit].astype(np.int64) + q.cols["n_pre"][hit] if "n_imm" in q.cols
                      else np.ones(int(hit.sum()), np.int64))
            q.deadline = np.where(hit, I64_MIN, q.deadline)
        else:
            w_ip, w_rows = np.empty(0, np.uint32), np.empty(0, np.int64)
        try:
            r = base(ev2)
        except Exception:
            if q is not None:
                self.queue().deadline = before_dl  # (refused: nothing applied, the staging kept)
            raise
        self.staged = None
        rows = {"requestor_ip": R.copy(),
                "leases": np.array([int((l_ip == x).sum()) for x in R], np.uint32),
                "zombies": np.array([int(l_zombie[l_ip == x].sum()) for x in R], np.uint32),
                "waiting": np.array([int((w_ip == x).sum()) for x in R], np.uint32),
                "waiting_rows": np.array([int(w_rows[w_ip == x].sum()) for x in R], np.uint32)}
        self.result = (rows, len(ids), len(w_ip))
        self.freed_ids = ids
        return r


def held_by(ws, requestor):
    """(ids of the leases the model's inspection dump attributes to `requestor`, tags of its entries of W)."""
    tk = ws.table.inspect.tasks()
    mine = (tk["started_at"] != NO_TIME) & (tk["requestor_ip"] == np.uint32(requestor))
    st = getattr(ws, "state", None)
    tags = st.q.tag[st.q.cols["requestor_ip"] == np.uint32(requestor)] if st is not None else np.empty(0, np.uint64)
    return tk["task_id"][mine], tags

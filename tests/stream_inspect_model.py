"""Inspection of a leased stream (ydc_stream_inspect_begin / _load / _servants / _tasks) as a plain
model: the yardstick of tests/test_stream_inspect_gpu.py, pinned against the verbatim reference's
DumpInternals by tests/test_stream_inspect_model.py.

It sits on top of the lease models (tests/stream_lease_model.py and the two built on it, with or
without tests/stream_alive_model.py's aliveness) and edits none of them: every one of them ends a
tick in the table's tick, and attach() turns the stream's table into a subclass of whatever it is
whose tick also keeps what the reference keeps for its dump:
  - per grant of the batch (task_dispatcher.cc:124, :133): started_at = the tick's now (the clock at
    the grant: a request granted out of W starts in the tick that grants it), the request's env_id and
    requestor_ip, prefetch = the row's rank inside its RPC >= n_immediate (rpc mode; 0 elsewhere), and
    ever_assigned[servant] += 1;
  - per servant a tick appends (:208): discovered_at = the tick's now, ever_assigned = 0; removed rows
    leave both columns, order kept; a servant that returns is a new row;
  - a lease that leaves L (free, sweep, orphan) takes its details along.
The batch's columns do not reach the table in every mode (the waiting-and-leased state hands it a
batch of zeros), so stage(ev) computes them from the stream's state before the tick, as Alive.stage
takes the heartbeats' expiries.

capacity() is GetCapacityAvailable (:283-313) and totals() the five numbers of :541-612, in Python
integers reduced modulo 2^64 where the reference's std::uint64_t wraps.
"""
import numpy as np

from tests import stream_lease_model as L

NO_ID = 0xFFFFFFFF
NO_TIME = -(1 << 63)
LOW_MEMORY = 2  # YDC_SERVANT_LOW_MEMORY
M64 = (1 << 64) - 1


def capacity(nproc, load, max_tasks, running, low_memory):
    """GetCapacityAvailable (:283-313) for one servant."""
    if low_memory:
        return int(running)
    foreign = max(int(load) - int(running), 0)
    return min(int(max_tasks), max(int(nproc) - foreign, 0))


def totals(max_tasks, running, avail):
    """:541-612: the sums in u64 arithmetic, the difference read as int64 and clamped at 0."""
    cap = sum(int(m) for m in max_tasks) & M64
    run = sum(int(r) for r in running) & M64
    unav = sum((int(m) - int(a)) & M64 for m, a in zip(max_tasks, avail)) & M64
    left = (cap - run - unav) & M64
    if left >> 63:
        left = 0
    return {"servants_up": len(max_tasks), "running_tasks": run, "capacity": cap, "capacity_available": left,
            "capacity_unavailable": unav}


class Inspect:
    """The details per lease, the two servant columns and the staging of the next tick's batch."""

    def __init__(self, ls, discovered_at=None, ever_assigned=None, last_now=None):
        self.ls = ls
        n = ls.es.n
        self.disc = (np.full(n, 0 if last_now is None else last_now, np.int64) if discovered_at is None
                     else np.array(discovered_at, np.int64))
        self.ever = np.zeros(n, np.uint64) if ever_assigned is None else np.array(ever_assigned, np.uint64)
        self.details = {}  # task id -> (started_at, env_id, requestor_ip, prefetch); absent: the sentinels
        self.last_rows, self.last_n = np.empty(0, np.int64), 0  # the last tick's granted rows of its placed batch
        self.staged = None

    def stage(self, ev):
        """The batch the tick `ev` will place, row by row: (env_id, requestor_ip, prefetch)."""
        now = int(ev["now"])
        st = getattr(self.ls, "state", None)
        new = ev["tasks"]
        if st is None:  # leased: the requests themselves
            env, ip = np.asarray(new["env_id"], np.uint32), np.asarray(new["requestor_ip"], np.uint32)
            pre = np.zeros(len(env), np.uint8)
        else:
            q = st.q
            live = q.deadline > now
            env = np.concatenate([q.cols["env_id"][live], np.asarray(new["env_id"], np.uint32)])
            ip = np.concatenate([q.cols["requestor_ip"][live], np.asarray(new["requestor_ip"], np.uint32)])
            pre = np.zeros(len(env), np.uint8)
            if "n_imm" in q.cols:  # rpc: every position expands into its rows
                ni = np.concatenate([q.cols["n_imm"][live], np.asarray(ev["n_immediate"], np.uint32)]).astype(np.int64)
                rows = ni + np.concatenate([q.cols["n_pre"][live], np.asarray(ev["n_prefetch"], np.uint32)])
                start = np.concatenate([[0], np.cumsum(rows)])[:-1]
                rank = np.arange(int(rows.sum())) - np.repeat(start, rows)
                env, ip = np.repeat(env, rows), np.repeat(ip, rows)
                pre = (rank >= np.repeat(ni, rows)).astype(np.uint8)
        self.staged = (env, ip, pre)

    def grow(self, n, now):
        k = n - len(self.disc)
        if k > 0:
            self.disc = np.concatenate([self.disc, np.full(k, now, np.int64)])
            self.ever = np.concatenate([self.ever, np.zeros(k, np.uint64)])

    def remove(self, removed):
        keep = np.ones(len(self.disc), bool)
        keep[np.asarray(removed, np.int64)] = False
        self.disc, self.ever = self.disc[keep], self.ever[keep]

    def load(self, cols):
        """ydc_stream_inspect_load: the refusals first, then the details filed by id."""
        ids = [int(t) for t in cols["task_id"]]
        T = self.ls.table
        if len(ids) > len(T.L) or len(set(ids)) != len(ids) or any(t not in T.L for t in ids):
            raise ValueError("inspect_load refused")
        for k, t in enumerate(ids):
            self.details[t] = (int(cols["started_at"][k]), int(cols["env_id"][k]), int(cols["requestor_ip"][k]),
                               int(cols["prefetch"][k]))

    def tasks(self):
        """As binding.Context.stream_inspect_tasks: L in id order with the details beside it."""
        ids, srv, exp, zom = self.ls.table.snapshot()
        d = [self.details.get(int(t), (NO_TIME, NO_ID, NO_ID, 0)) for t in ids]
        col = lambda k, t: np.array([x[k] for x in d], t)
        return {"task_id": ids, "servant_idx": srv, "expires_at": exp, "zombie": zom, "started_at": col(0, np.int64),
                "env_id": col(1, np.uint32), "requestor_ip": col(2, np.uint32), "prefetch": col(3, np.uint8)}

    def servants(self):
        """As binding.Context.stream_inspect_servants, from the stream's registry as it is now."""
        es = self.ls.es
        self.grow(es.n, 0 if self.ls.table.last_now is None else self.ls.table.last_now)
        sv, run = es.sv, es.running.astype(np.int64)
        low = (np.asarray(es.abi["flags"]) & LOW_MEMORY) != 0
        avail = [capacity(sv["num_processors"][s], sv["current_load"][s], sv["max_tasks"][s], run[s], low[s])
                 for s in range(es.n)]
        return {"discovered_at": self.disc.copy(), "ever_assigned": self.ever.copy(), "running_tasks": run.astype(np.uint32),
                "capacity_available": np.array(avail, np.uint32), "totals": totals(sv["max_tasks"], run, avail)}


class _InspectTick:
    """Mixed in front of the stream's table class. `inspect`: its Inspect."""

    def tick(self, running, ev, place):
        I = self.inspect
        now = int(ev["now"])
        self.check(len(ev["tasks"]["env_id"]), now)  # (a refused tick files and counts nothing)
        env, ip, pre = I.staged
        I.staged = None
        I.grow(I.ls.es.n, now)
        r = super().tick(running, ev, place)
        got, ids = r["out"], r["task_id"]
        assert len(got) == len(env), "the staged batch is not the batch the tick placed"
        I.last_rows, I.last_n = np.nonzero(got < L.IDX_ENV_NOT_FOUND)[0], len(got)  # (what a test may ask about)
        for i in np.nonzero(got < L.IDX_ENV_NOT_FOUND)[0].tolist():
            I.details[int(ids[i])] = (now, int(env[i]), int(ip[i]), int(pre[i]))
            I.ever[int(got[i])] += np.uint64(1)
        I.details = {t: d for t, d in I.details.items() if t in self.L}
        return r

    def remove_servants(self, removed):
        """ydc_remove_servants and aliveness's removal alike (both end here)."""
        self.inspect.grow(len(self.inspect.ls.es.running) + len(removed), self.last_now or 0)
        super().remove_servants(removed)
        self.inspect.remove(removed)
        self.inspect.details = {t: d for t, d in self.inspect.details.items() if t in self.L}


def attach(ls, discovered_at=None, ever_assigned=None):
    """Inspection for the stream `ls` (of any of the three lease models, with aliveness attached or
    not): its table's class gains the tick above, in place. -> its Inspect."""
    T = ls.table
    T.__class__ = type("Inspect" + T.__class__.__name__, (_InspectTick, T.__class__), {})
    T.inspect = Inspect(ls, discovered_at, ever_assigned, T.last_now)
    return T.inspect


def model_tick(M, ws, ev, place=None, alive=False):
    """One tick of the lease model M on a stream with inspection: the batch is staged here, then M's
    model_tick (through stream_alive_model's where the stream has aliveness too)."""
    ws.table.inspect.stage(ev)
    if alive:
        from tests import stream_alive_model as AM
        return AM.model_tick(M, ws, ev, place)
    return M.model_tick(ws, ev, place) if place else M.model_tick(ws, ev)

"""Usage per requestor (ydc_stream_usage_begin / _get / _find / _load) as a plain model: the yardstick of
tests/test_stream_usage_gpu.py. A thin wrapper over the leased, the waiting + leased and the rpc models
with inspection attached (tests/stream_lease_model, tests/stream_wait_lease_model, tests/stream_rpc_model,
tests/stream_inspect_model), as tests/stream_depart_model wraps them; it edits none of them.

Before the base tick, with the tick's clock `now` and `last` the clock of the previous accepted tick (or
of the begin call: the stream's last now, or, before its first tick, this tick's own now):

    dq = now // quantum - last // quantum          (Python integers: // floors), masked to 64 bits

  - every lease of Inspect.tasks() adds dq to its requestor's slot_time, to zombie_time too if it is a
    zombie, to prefetch_time too if its prefetch byte is set; a lease without details (started_at ==
    NO_TIME) adds dq to unattributed_time and to no row;
  - every entry of the queue (ws.state.q), expired or not, adds dq to its requestor's wait_time and
    rows x dq to wait_row_time (rows = n_imm + n_pre in rpc mode, 1 elsewhere);
  - quanta += dq, ticks += 1.
Every sum is masked to 64 bits. dq == 0 files no key. Then the base tick runs; a refused tick (the base
raises) adds nothing and keeps `last`. The model has no other semantics.
"""
import numpy as np

from tests import stream_inspect_model as IM

M64 = (1 << 64) - 1
NO_TIME = IM.NO_TIME
COLUMNS = ("slot_time", "zombie_time", "prefetch_time", "wait_time", "wait_row_time")
DTYPE = np.dtype([("requestor_ip", "<u4"), ("pad", "<u4")] + [(k, "<u8") for k in COLUMNS])
MIN_SLOTS = 1024


def quanta(last, now, quantum):
    """floor(now / quantum) - floor(last / quantum) modulo 2^64."""
    return (int(now) // int(quantum) - int(last) // int(quantum)) & M64


def slots_for(keys):
    """The table's slots for `keys` requestors: a power of two, at least MIN_SLOTS, at most half full."""
    s = MIN_SLOTS
    while s < 2 * keys:
        s *= 2
    return s


class Usage:
    """The capability of one stream `ws` (of any of the three lease models, inspection attached)."""

    def __init__(self, ws, quantum):
        if getattr(ws.table, "inspect", None) is None:
            raise ValueError("inspection is off")
        if int(quantum) <= 0:
            raise ValueError("quantum")
        self.ws, self.quantum = ws, int(quantum)
        self.last = ws.table.last_now  # None: the stream has not ticked yet
        self.rows = {}  # requestor -> [slot, zombie, prefetch, wait, wait_row]
        self.unattributed = self.quanta = self.ticks = 0
        self.dq = None  # of the most recent accepted tick

    def begin(self, quantum):
        if int(quantum) != self.quantum:
            raise ValueError("another quantum")

    def queue(self):
        st = getattr(self.ws, "state", None)
        return None if st is None else st.q

    def charge(self, now):
        """What a tick at `now` adds, from the state as it is: (dq, {requestor: five sums}, unattributed)."""
        last = now if self.last is None else self.last
        dq = quanta(last, now, self.quantum)
        add, un = {}, 0
        if dq == 0:
            return dq, add, un
        tk = self.ws.table.inspect.tasks()
        for at, ip, z, p in zip(tk["started_at"].tolist(), tk["requestor_ip"].tolist(), tk["zombie"].tolist(),
                                tk["prefetch"].tolist()):
            if at == NO_TIME:
                un += dq
                continue
            r = add.setdefault(ip, [0] * 5)
            r[0] += dq
            r[1] += dq if z else 0
            r[2] += dq if p else 0
        q = self.queue()
        if q is not None and len(q):
            ips = q.cols["requestor_ip"].tolist()
            rows = ((q.cols["n_imm"].astype(np.int64) + q.cols["n_pre"]).tolist() if "n_imm" in q.cols else [1] * len(ips))
            for ip, k in zip(ips, rows):
                r = add.setdefault(ip, [0] * 5)
                r[3] += dq
                r[4] += int(k) * dq
        return dq, add, un

    def tick(self, ev, base):
        """base(ev) runs the tick below this wrapper -> its record, returned as it is."""
        now = int(ev["now"])
        dq, add, un = self.charge(now)
        r = base(ev)  # (refused: it raises, and nothing below happens)
        for ip, v in add.items():
            row = self.rows.setdefault(ip, [0] * 5)
            for k in range(5):
                row[k] = (row[k] + v[k]) & M64
        self.unattributed = (self.unattributed + un) & M64
        self.quanta = (self.quanta + dq) & M64
        self.ticks = (self.ticks + 1) & M64
        self.last, self.dq = now, dq
        return r

    def totals(self):
        return {"unattributed_time": self.unattributed, "quanta": self.quanta, "ticks": self.ticks,
                "n_keys": len(self.rows)}

    def get(self, reset=False):
        """(rows sorted by requestor, the totals); reset: the table and the totals emptied behind the copy."""
        out = np.zeros(len(self.rows), DTYPE)
        for i, ip in enumerate(sorted(self.rows)):
            out[i] = (ip, 0) + tuple(self.rows[ip])
        tot = self.totals()
        if reset:
            self.rows = {}
            self.unattributed = self.quanta = self.ticks = 0
        return out, tot

    def find(self, ips):
        out = np.zeros(len(ips), DTYPE)
        for i, ip in enumerate(int(x) for x in ips):
            out[i] = (ip, 0) + tuple(self.rows.get(ip, [0] * 5))
        return out

    def load(self, rows, totals=None):
        """Adds the rows, duplicates together (a row of zeros still files its key), and the three totals."""
        for r in np.asarray(rows, DTYPE):
            row = self.rows.setdefault(int(r["requestor_ip"]), [0] * 5)
            for k, name in enumerate(COLUMNS):
                row[k] = (row[k] + int(r[name])) & M64
        if totals:
            self.unattributed = (self.unattributed + int(totals.get("unattributed_time", 0))) & M64
            self.quanta = (self.quanta + int(totals.get("quanta", 0))) & M64
            self.ticks = (self.ticks + int(totals.get("ticks", 0))) & M64

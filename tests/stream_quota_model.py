"""The cap per requestor inside the tick (ydc_stream_quota_begin / _set / _result) as a plain model: the
yardstick of tests/test_stream_quota_gpu.py. A wrapper over the waiting + leased and the rpc models
with inspection attached (tests/stream_wait_lease_model, tests/stream_rpc_model,
tests/stream_inspect_model, with or without tests/stream_alive_model's aliveness), none of which is
edited:

  - the base models run steps 1 - 6 (and the servants' expiry) and then call place(batch). So a PROBE
    run of the tick on a deep copy of the stream, whose place reads L with the inspection details and W
    and then aborts, yields the loads at the clip point: held(r) = r's attributed leases (zombies
    included) + the rows of r's entries of W with deadline > now (withdrawal has set the deadline of a
    withdrawn entry to the smallest int64 before). A tick the base model refuses is refused there, on
    the SUBMITTED counts, and nothing of the real stream has changed;
  - the clip: a_i = min(pre_i + want_i, room) - min(pre_i, room), prefetch clipped first;
  - the base tick on the clipped requests (counts a_imm / a_pre, requests with a_i == 0 left out): this
    IS the defining property, the model has no other semantics;
  - the label: the base record expanded to the caller's requests, a request with a_i == 0 answered
    IDX_OVER_QUOTA (no id; rpc: n_granted 0).
"""
import copy

import numpy as np

from tests import stream_inspect_model as IM
from tests import stream_outlook_model as OM
from tests import stream_rpc_model as RM

IDX_OVER_QUOTA = 0xFFFFFFFB
UNLIMITED = 0xFFFFFFFF
NO_TIME = IM.NO_TIME
NO_ID = RM.NO_ID
PER_REQUEST = ("lease_for", "deadlines", "tags")


class _Probed(Exception):
    pass


def held_of(tasks, waiting, now):
    """requestor -> leases + live waiting rows, from the dicts of Inspect.tasks() and stream_waiting()."""
    held = {}
    known = np.asarray(tasks["started_at"], np.int64) != NO_TIME
    for ip in np.asarray(tasks["requestor_ip"], np.uint32)[known].tolist():
        held[ip] = held.get(ip, 0) + 1
    live = np.asarray(waiting["deadline"], np.int64) > now
    rows = np.asarray(waiting["n_immediate"], np.int64) + np.asarray(waiting["n_prefetch"], np.int64)
    for ip, r in zip(np.asarray(waiting["requestor_ip"], np.uint32)[live].tolist(), rows[live].tolist()):
        held[ip] = held.get(ip, 0) + r
    return held


def clip(ips, n_imm, n_pre, held, cap_of):
    """The closed form of include/yadcc_dispatch.h. -> (adm_immediate, adm_prefetch)."""
    asked, a_imm, a_pre = {}, [], []
    for ip, imm, pre in zip((int(x) for x in ips), (int(x) for x in n_imm), (int(x) for x in n_pre)):
        cap = cap_of(ip)
        room = cap - min(cap, held.get(ip, 0))
        p, want = asked.get(ip, 0), imm + pre
        a = min(p + want, room) - min(p, room)
        asked[ip] = p + want
        a_imm.append(min(imm, a))
        a_pre.append(a - min(imm, a))
    return np.array(a_imm, np.uint32), np.array(a_pre, np.uint32)


class Quota:
    """The capability of one stream `ws` of the lease model M (stream_wait_lease_model or
    stream_rpc_model) with inspection attached; alive: aliveness attached too."""

    def __init__(self, M, ws, alive=False):
        self.M, self.ws, self.alive = M, ws, alive
        self.rpc = M is RM
        self.max_overrides = 0
        self.default, self.over = UNLIMITED, {}
        e = np.empty(0, np.uint32)
        self.result = (e, e, 0, 0)  # adm_immediate, adm_prefetch, rows clipped, requests refused
        self.held = {}              # the loads of the most recent tick's new requestors, at its clip point
        self.base = None            # the record of the stream that was given the clipped requests

    def begin(self, max_overrides):
        if max_overrides > 1 << 24:
            raise ValueError("max_overrides")
        self.max_overrides = max(self.max_overrides, max_overrides)

    def set(self, default_cap, overrides=()):
        pairs = list(overrides.items()) if isinstance(overrides, dict) else list(overrides)
        if len(pairs) > self.max_overrides:
            raise OverflowError("max_overrides")
        if len({int(p[0]) for p in pairs}) != len(pairs):
            raise ValueError("a requestor named twice")
        self.default, self.over = int(default_cap), {int(k): int(v) for k, v in pairs}

    def cap_of(self, ip):
        return self.over.get(int(ip), self.default)

    def _base_tick(self, ws, ev, place):
        if ws.table.inspect is None:
            raise ValueError("inspection is off")
        return IM.model_tick(self.M, ws, ev, place, alive=self.alive)

    def loads(self, ev):
        """The probe: requestor -> held at the clip point of the tick `ev`, the stream untouched."""
        ws2, ev2 = copy.deepcopy(self.ws), copy.deepcopy(ev)
        now, box = int(ev["now"]), {}

        def probe(batch):
            box["held"] = held_of(ws2.table.inspect.tasks(), OM.stream_waiting(ws2), now)
            raise _Probed()
        try:
            self._base_tick(ws2, ev2, probe)
        except _Probed:
            return box["held"]
        raise AssertionError("a tick with new requests placed no batch")

    def requests(self, ev):
        n = len(ev["tags"])
        ips = np.asarray(ev["tasks"]["requestor_ip"], np.uint32)
        imm = np.asarray(ev["n_immediate"], np.uint32) if self.rpc else np.ones(n, np.uint32)
        pre = np.asarray(ev["n_prefetch"], np.uint32) if self.rpc else np.zeros(n, np.uint32)
        return ips, imm, pre

    def clipped(self, ev, a_imm, a_pre):
        """The tick a stream without the capability would be given instead."""
        keep = (a_imm.astype(np.int64) + a_pre) > 0
        ev2 = dict(ev, tasks={k: np.asarray(v)[keep] for k, v in ev["tasks"].items()})
        for k in PER_REQUEST:
            ev2[k] = np.asarray(ev[k])[keep]
        if self.rpc:
            ev2["n_immediate"], ev2["n_prefetch"] = a_imm[keep], a_pre[keep]
        return ev2, keep

    def tick(self, ev, place=None):
        """One tick; feeds the answers back like the base model_tick. -> the labelled record (the base
        model's fields, per-request ones by the caller's requests)."""
        ips, imm, pre = self.requests(ev)
        held = self.loads(ev) if len(ips) else {}
        a_imm, a_pre = clip(ips, imm, pre, held, self.cap_of)
        ev2, keep = self.clipped(ev, a_imm, a_pre)
        r = self._base_tick(self.ws, ev2, place)
        want = imm.astype(np.int64) + pre
        adm = a_imm.astype(np.int64) + a_pre
        self.result = (a_imm, a_pre, int((want - adm).sum()), int((~keep).sum()))
        self.held, self.base = {ip: held.get(ip, 0) for ip in set(ips.tolist())}, r
        return label(self.rpc, r, keep)


def label(rpc, r, keep):
    """The base record of the clipped tick as the stream with the capability answers the caller."""
    out = dict(r)
    n = len(keep)

    def spread(a, fill):
        full = np.full(n, fill, np.asarray(a).dtype)
        full[keep] = a
        return full
    if rpc:
        out["status"] = spread(r["status"], IDX_OVER_QUOTA)
        out["n_granted"] = spread(r["n_granted"], 0)
    else:
        out["out"] = spread(r["out"], IDX_OVER_QUOTA)
        out["task_id"] = spread(r["task_id"], NO_ID)
    return out


def unlabelled(rpc, got, a_imm, a_pre):
    """What a device tick answered (binding.Context.stream_tick_rpc's dict, or
    stream_tick_waiting_leased's tuple) with the label taken back: the answers of the stream that was
    given the clipped requests, in the form the modes' own check_tick compares. The refused requests
    (all of them labelled, asserted by the caller) drop out; an rpc tick's expanded outputs are read
    by admitted rows."""
    a_imm, a_pre = np.asarray(a_imm, np.int64), np.asarray(a_pre, np.int64)
    keep = (a_imm + a_pre) > 0
    if not rpc:
        g = list(got)
        g[0], g[1] = got[0][keep], got[1][keep]
        return tuple(g)
    rows = (a_imm + a_pre)[keep]
    g = dict(got)
    g["status"], g["n_granted"] = got["status"][keep], got["n_granted"][keep]
    g["row_off"] = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    g["servants"] = got["servants"][:int(rows.sum())]
    g["task_ids"] = got["task_ids"][:int(rows.sum())]
    return g


def literal(ips, n_imm, n_pre, held, cap_of):
    """The literal loop the closed form stands for: the requests in order, one row at a time while the
    requestor holds less than its cap, an RPC's prefetch rows after its immediate rows."""
    have = dict(held)
    a_imm, a_pre = [], []
    for ip, imm, pre in zip((int(x) for x in ips), (int(x) for x in n_imm), (int(x) for x in n_pre)):
        got = [0, 0]
        for kind, rows in ((0, imm), (1, pre)):
            for _ in range(rows):
                if have.get(ip, 0) < cap_of(ip):
                    have[ip] = have.get(ip, 0) + 1
                    got[kind] += 1
        a_imm.append(got[0])
        a_pre.append(got[1])
    return np.array(a_imm, np.uint32), np.array(a_pre, np.uint32)

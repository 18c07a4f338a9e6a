"""The fair-share level per tick (ydc_stream_quota_fair / _fair_result, ydc_fair_level) as a plain model:
the yardstick of tests/test_stream_fair_gpu.py. A wrapper over tests/stream_quota_model.Quota, which is
not edited:

  - per tick a PROBE run on a deep copy of the stream (as Quota.loads does) reads the registry's columns,
    L and W at the clip point: behind steps 1 - 6, the servants' expiry, the tick's heartbeats and
    withdrawal's mark;
  - from them P, T, O and the level, by the LITERAL rule of include/yadcc_dispatch.h (level() below is
    the closed form by bisection, fill() the progressive fill it stands for);
  - the effective default goes into the quota model as its default for this one tick (cap_of), and
    Quota.tick runs: this IS the defining property, the model has no other semantics.
"""
import copy

import numpy as np

from tests import stream_outlook_model as OM
from tests import stream_quota_model as Q

OFF, REGISTRY, FIXED = 0, 1, 2
UNLIMITED = Q.UNLIMITED
POOL_MAX = (1 << 32) - 2
LOW_MEMORY = 2
RESULT_FIELDS = ("level", "cap_default_effective", "n_askers", "n_override_askers", "pool", "held_total", "held_others",
                 "asked_rows", "capacity_now", "tick_no", "mode")


def top(nproc, load, max_tasks, flags):
    if (int(flags) & LOW_MEMORY) or int(max_tasks) == 0 or int(load) >= int(nproc):
        return 0
    return min(int(max_tasks), int(nproc))


def pool_of(cap_now, percent):
    return min(cap_now * percent // 100, POOL_MAX)


def term(h, a, level):
    return max(h, min(h + a, level))


def f_at(askers, others, level):
    """askers: (h, a, cap) with cap None for a requestor inside the fair share."""
    return others + sum(term(h, a, level if cap is None else cap) for h, a, cap in askers)


def level(askers, others, pool):
    """The written rule, the largest integer found by bisection (f is non-decreasing)."""
    pool = min(pool, POOL_MAX)
    fair = [x for x in askers if x[2] is None]
    if not fair:
        return UNLIMITED
    D = max(h + a for h, a, _ in fair)
    if f_at(askers, others, D) <= pool:
        return UNLIMITED
    if f_at(askers, others, 0) > pool:
        return 0
    lo, hi = 0, D
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f_at(askers, others, mid) <= pool:
            lo = mid
        else:
            hi = mid
    return lo


def fill(askers, others, pool):
    """The literal progressive fill: raise the level by one while f(level + 1) <= P."""
    pool = min(pool, POOL_MAX)
    fair = [x for x in askers if x[2] is None]
    if not fair:
        return UNLIMITED
    D = max(h + a for h, a, _ in fair)
    if f_at(askers, others, 0) > pool:
        return 0
    lv = 0
    while lv < D and f_at(askers, others, lv + 1) <= pool:
        lv += 1
    return UNLIMITED if lv >= D else lv


def cap_default(lv, floor, default):
    return min(default, max(lv, floor))


class Fair:
    """The setting on top of one Quota `q` (whose stream, mode and settings it reads). Everything a
    caller asks that this class does not have is the Quota's."""

    def __init__(self, q):
        self.q = q
        self.mode, self.pool, self.floor = OFF, 0, 0
        self.level_result = dict.fromkeys(RESULT_FIELDS, 0)
        self.effective = None  # the default of the most recent tick, where the mode was on

    def __getattr__(self, k):
        return getattr(self.q, k)

    def fair(self, mode, pool=0, floor=0):
        if mode not in (OFF, REGISTRY, FIXED) or (mode == REGISTRY and pool == 0):
            raise ValueError("fair")
        self.mode, self.pool, self.floor = mode, int(pool), int(floor)

    def cap_of(self, ip):
        """The cap the most recent tick gave the requestor."""
        if self.effective is None:
            return self.q.cap_of(ip)
        return self.q.over.get(int(ip), self.effective)

    def probe(self, ev):
        """-> (held per requestor, T, cap_now) at the clip point of the tick `ev`, the stream untouched; None
        where the tick places no batch (no new request and nothing live in W: the base model never gets there)."""
        q = self.q
        ws2, ev2 = copy.deepcopy(q.ws), copy.deepcopy(ev)
        now, box = int(ev["now"]), {}

        def probe(batch):
            tasks, waiting = ws2.table.inspect.tasks(), OM.stream_waiting(ws2)
            live = np.asarray(waiting["deadline"], np.int64) > now
            rows = np.asarray(waiting["n_immediate"], np.int64) + np.asarray(waiting["n_prefetch"], np.int64)
            es = ws2.es
            box["held"] = Q.held_of(tasks, waiting, now)
            box["T"] = len(tasks["task_id"]) + int(rows[live].sum())
            box["cap_now"] = sum(top(es.sv["num_processors"][s], es.sv["current_load"][s], es.sv["max_tasks"][s],
                                     es.abi["flags"][s]) for s in range(es.n))
            raise Q._Probed()
        try:
            q._base_tick(ws2, ev2, probe)
        except Q._Probed:
            return box["held"], box["T"], box["cap_now"]
        assert not len(ev["tags"]), "a tick with new requests placed no batch"
        return None

    def evaluate(self, held, T, cap_now, ips, want):
        """-> the result block (without tick_no) from the loads and the tick's requests."""
        q = self.q
        asked = {}
        for ip, w in zip((int(x) for x in ips), (int(x) for x in want)):
            asked[ip] = asked.get(ip, 0) + w
        askers = [(held.get(ip, 0), a, q.over.get(ip)) for ip, a in asked.items()]
        others = T - sum(h for h, _, _ in askers)
        assert others >= 0
        P = pool_of(cap_now, self.pool) if self.mode == REGISTRY else min(self.pool, POOL_MAX)
        lv = level(askers, others, P)
        return {"level": lv, "cap_default_effective": cap_default(lv, self.floor, q.default), "n_askers": len(askers),
                "n_override_askers": sum(1 for x in askers if x[2] is not None), "pool": P, "held_total": T,
                "held_others": others, "asked_rows": sum(asked.values()), "capacity_now": cap_now, "mode": self.mode,
                "askers": askers}

    def tick(self, ev, place=None):
        q = self.q
        if self.mode == OFF:
            self.effective = None
            self.level_result = dict.fromkeys(RESULT_FIELDS, 0)
            return q.tick(ev, place)
        ips, imm, pre = q.requests(ev)
        at = self.probe(ev)
        if at is None:  # (nobody asks: the level is unlimited; the totals are those fields' that the model has not got)
            res = {"level": UNLIMITED, "cap_default_effective": q.default, "n_askers": 0, "n_override_askers": 0,
                   "asked_rows": 0, "askers": [], "mode": self.mode}
        else:
            res = self.evaluate(*at, ips, imm.astype(np.int64) + pre)
        self.last_ips = ips
        self.effective = res["cap_default_effective"]
        static = q.default
        q.default = self.effective  # the stream with the static quota whose default_cap is that value for this tick
        try:
            r = q.tick(ev, place)
        finally:
            q.default = static
        self.level_result = res
        return r

    def invariant(self):
        """With floor 0, after the clip of the most recent tick: O + sum (h + admitted) <= max(P, T) where no
        asker has an override. An override is outside the fair share and keeps its own cap, so what the
        overrides were admitted stands on top of T: O + sum (h + admitted) <= max(P, T + sum over the
        overrides of admitted), which is the same statement where there is none."""
        res, q = self.level_result, self.q
        if self.mode == OFF or "held_total" not in res:
            return True
        adm = {}
        for ip, a in zip(self.last_ips.tolist(), (q.result[0].astype(np.int64) + q.result[1]).tolist()):
            adm[ip] = adm.get(ip, 0) + a
        total = res["held_others"] + sum(q.held.get(ip, 0) + a for ip, a in adm.items())
        over = sum(a for ip, a in adm.items() if ip in q.over)
        return total <= max(res["pool"], res["held_total"] + over)

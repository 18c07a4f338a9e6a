"""Cost of the departure of requestors (ydc_stream_depart_begin / _stage / _result).

1. The idle price (--idle): two waiting + leased contexts with inspection on at the cfg5 registry with one
   slot per servant, ticking in turn in one process as tests/tools/withdraw_cost.py's do (2 500 requests a
   tick that wait 4 ticks, |W| about 10 000): (a) the capability off, (b) on with nothing staged, and (c) on
   with one requestor of 16 staged per tick. Median wall time per tick, host call to host return.
2. A departing tick (--leases N, default 100 000): a leased stream with inspection on that holds N leases of
   1 000 requestors, one of them holding 90 % ("hot": that one departs) or uniformly mixed ("uniform": 100
   of the 1 000 depart). Three contexts in the same state:
     depart     the capability on (max_frees 16): ydc_stream_depart_stage, then the tick;
     by_hand    what a scheduler does without it (max_frees = N): ydc_stream_inspect_tasks copies all of L
                out, a numpy filter by requestor_ip, and the ids through free_task_id of the next tick;
     off        no capability (max_frees 16): its empty tick beside `depart`'s empty tick with nothing
                staged shows whether the idle price depends on |L|.
   Per repeat the departed leases are granted again, so every repeat finds |L| = N. Medians and min / max
   of --repeats, microseconds of wall time from host call to host return (every tick ends in a device
   synchronise).
    python tests/tools/depart_cost.py --idle --ticks 300
    python tests/tools/depart_cost.py --leases 1000000
One JSON line per measurement. Under `rocprofv3 --kernel-trace --stats -- python tests/tools/depart_cost.py
--leases ...` the kernel table gives k_depart_leases beside k_lease_sweep, which reads the same table.
Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

E32, E64, Z1 = np.empty(0, np.uint32), np.empty(0, np.uint64), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)
NO_ROWS = np.empty(0, binding.ROW_DTYPE)
FAR = 1 << 40
# the idle legs (withdraw_cost.py's shape)
N, WAIT, MAX_WAITING, WARM, IDLE_REQUESTORS = 2_500, 4, 20_000, 20, 16
# the departing tick (requestor_cost.py's shape)
SERVANTS, SLOTS, PER_TICK, REQUESTORS = 2048, 640, 50_000, 1000


def us(v):
    return round(float(np.median(v)) * 1e6, 1)


def spread(v):
    return [round(float(min(v)) * 1e6, 1), round(float(max(v)) * 1e6, 1)]


# ---- 1. the idle price -----------------------------------------------------------------------------

class IdleLeg:
    def __init__(self, sv, abi, on, staged):
        self.ctx = binding.Context(device=0)
        self.ctx.upload_servants(abi)
        self.es = streaming.EventStream(sv, N, 0)
        self.ctx.stream_begin_waiting_leased(self.es.hb + 8, 16, N, MAX_WAITING, 1 << 16, 16, 16, 16, 16)
        self.ctx.stream_inspect_begin()
        if on:
            self.ctx.stream_depart_begin(64)
        self.staged, self.tick_s, self.stage_s, self.w, self.dismissed = staged, [], [], [], 0

    def tick(self, t):
        who, rows, _, tk = self.es.next_tick()
        tk = dict(tk, requestor_ip=((10 << 24) + (np.arange(N) + t) % IDLE_REQUESTORS).astype(np.uint32))
        tags = t * N + np.arange(N, dtype=np.uint64)
        t0 = time.perf_counter()
        if self.staged and t >= 5:
            self.ctx.stream_depart_stage([(10 << 24) + t % IDLE_REQUESTORS])
        t1 = time.perf_counter()
        r = self.ctx.stream_tick_waiting_leased(who, rows, E32, E64, I64, E64, E32, Z1, E64, tk, np.full(N, FAR, np.int64),
                                                np.full(N, t + WAIT, np.int64), tags, t)
        t2 = time.perf_counter()
        self.tick_s.append(t2 - t1)
        self.stage_s.append(t1 - t0)
        self.w.append(r[8] + int(len(r[5])) - int((r[0] == binding.IDX_WAITING).sum()))  # |W| as the tick found it
        if self.staged and t >= 5:
            self.dismissed += self.ctx.stream_depart_result()[2]
        self.es.commit(r[0][r[0] < binding.IDX_WAITING])

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def idle(ticks):
    sv, _ = synth.make_config("cfg5")
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 1)
    abi = pack.to_abi_columns(sv)
    legs = {"off": IdleLeg(sv, abi, False, False), "on_nothing_staged": IdleLeg(sv, abi, True, False),
            "on_one_of_16_staged": IdleLeg(sv, abi, True, True)}
    for t in range(ticks + WARM):
        for leg in legs.values():
            leg.tick(t)
    out = {"what": "idle", "ticks": ticks, "requests_per_tick": N, "max_waiting": MAX_WAITING}
    for name, leg in legs.items():
        v = leg.tick_s[WARM:]
        out[name] = {"tick_us": us(v), "p10_us": round(float(np.percentile(v, 10)) * 1e6, 1),
                     "p90_us": round(float(np.percentile(v, 90)) * 1e6, 1), "stage_call_us": us(leg.stage_s[WARM:]),
                     "w_median": int(np.median(leg.w[WARM:])), "dismissed_per_tick": round(leg.dismissed / (ticks + WARM), 1)}
        leg.close()
    print(json.dumps(out), flush=True)


# ---- 2. a departing tick ---------------------------------------------------------------------------

def registry():
    sv = synth.make_servants(SERVANTS, n_tasks_hint=64, n_envs=1, seed=1)
    sv["version"][:], sv["num_processors"][:], sv["current_load"][:] = 20, SLOTS, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = SLOTS, 0
    sv["memory_available"][:], sv["total_memory"][:] = 32 << 30, 64 << 30
    sv["env_mask"] = np.ones(SERVANTS, np.uint64)
    return sv


class Holder:
    """A leased context with inspection on; grant() files leases for a column of requestors."""

    def __init__(self, abi, leases, max_frees, depart):
        self.ctx = binding.Context(device=0)
        self.ctx.upload_servants(abi)
        self.ctx.stream_begin_leased(8, 8, PER_TICK, leases + PER_TICK, 8, max_frees, 8, 8)
        self.ctx.stream_inspect_begin()
        if depart:
            self.ctx.stream_depart_begin(128)
        self.now, self.n_leases = 0, 0

    def tick(self, ips=E32, free=E64):
        self.now += 1
        tk = {"env_id": np.zeros(len(ips), np.uint32), "min_version": np.zeros(len(ips), np.uint32), "requestor_ip": ips}
        out, _, _, _, self.n_leases = self.ctx.stream_tick_leased(E32, NO_ROWS, E32, E64, I64, free, E32, Z1, E64, tk,
                                                                  np.full(len(ips), FAR, np.int64), self.now)
        assert (out < SERVANTS).all()

    def grant(self, who):
        for at in range(0, len(who), PER_TICK):
            self.tick(who[at:at + PER_TICK])

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def departing(leases, mix, repeats):
    abi = pack.to_abi_columns(registry())
    rng = np.random.default_rng(5)
    ids = ((10 << 24) + 1 + np.arange(REQUESTORS)).astype(np.uint32)
    if mix == "uniform":
        who, gone = rng.choice(ids, leases), ids[::10].copy()
    else:
        who, gone = rng.choice(ids[1:], leases), ids[:1].copy()
        who[rng.random(leases) < 0.9] = ids[0]
    again = who[np.isin(who, gone)]
    legs = {"depart": Holder(abi, leases, 16, True), "by_hand": Holder(abi, leases, leases, False),
            "off": Holder(abi, leases, 16, False)}
    for h in legs.values():
        h.grant(who)
        assert h.n_leases == leases
    T = {k: [] for k in ("depart_stage", "depart_tick", "by_hand_inspect", "by_hand_filter", "by_hand_tick", "idle_on", "idle_off")}
    clock = time.perf_counter
    for r in range(repeats + 1):
        d, b, o = legs["depart"], legs["by_hand"], legs["off"]
        t0 = clock(); d.tick(); t1 = clock(); o.tick(); t2 = clock()  # noqa: E702
        T["idle_on"].append(t1 - t0)
        T["idle_off"].append(t2 - t1)
        t0 = clock(); d.ctx.stream_depart_stage(gone); t1 = clock(); d.tick(); t2 = clock()  # noqa: E702
        T["depart_stage"].append(t1 - t0)
        T["depart_tick"].append(t2 - t1)
        rows, freed, _ = d.ctx.stream_depart_result()
        t0 = clock(); tasks = b.ctx.stream_inspect_tasks(); t1 = clock()  # noqa: E702
        mine = tasks["task_id"][(tasks["started_at"] != binding.INSPECT_NO_TIME) & np.isin(tasks["requestor_ip"], gone)]
        t2 = clock(); b.tick(free=mine); t3 = clock()  # noqa: E702
        T["by_hand_inspect"].append(t1 - t0)
        T["by_hand_filter"].append(t2 - t1)
        T["by_hand_tick"].append(t3 - t2)
        assert freed == len(mine) == len(again) and d.n_leases == b.n_leases == leases - len(again), (freed, len(mine))
        d.grant(again)
        b.grant(again)
    res = {"what": "departing", "leases": leases, "mix": mix, "repeats": repeats, "departed_leases": int(len(again)),
           "staged_requestors": int(len(gone))}
    for k, v in T.items():
        res[k + "_us"], res[k + "_min_max_us"] = us(v[1:]), spread(v[1:])
    res["depart_total_us"] = us(np.add(T["depart_stage"][1:], T["depart_tick"][1:]))
    res["by_hand_total_us"] = us(np.add(np.add(T["by_hand_inspect"][1:], T["by_hand_filter"][1:]), T["by_hand_tick"][1:]))
    print(json.dumps(res), flush=True)
    for h in legs.values():
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--idle", action="store_true")
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--leases", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.idle:
        idle(a.ticks)
        return
    assert a.leases % PER_TICK == 0 and a.leases + PER_TICK <= SERVANTS * SLOTS
    for mix in ("hot", "uniform"):
        departing(a.leases, mix, a.repeats)


if __name__ == "__main__":
    main()

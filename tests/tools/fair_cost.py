"""Cost of the fair-share level per tick (ydc_stream_quota_fair), three legs alternating tick by tick in one
process, at the cfg5 registry, in waiting-and-leased and in rpc mode, as tests/tools/quota_cost.py measures
the quota itself. Every tick brings 2 400 grants' worth of requests from 16 requestors (2 400 requests, or
800 RPCs of 2 + 1 rows) and frees by id what the tick `--hold` ticks earlier was granted, so L holds about
2 400 x hold leases as far as the pool has slots (--hold 4: 10^4; --hold 420 --pool-scale 10: 10^6, the cfg5
registry's max_tasks and num_processors times ten, because cfg5 itself has 126 010 slots).
    python tests/tools/fair_cost.py --ticks 300 --hold 4
prints one JSON line per mode: median and p10 - p90 wall time per tick (host call to host return) of
  (a) the quota with a static cap that clips about a tenth of the rows,
  (b) the level on, the pool a percent of the registry's capacity,
  (c) the level on, the pool a fixed number of rows,
both pools chosen so that the level clips about as much as (a) does, with the share of the rows each leg's
ticks clipped and the level of the last tick. Under `rocprofv3 --kernel-trace --stats -- python
tests/tools/fair_cost.py ...` the kernel table gives k_fair_sums, k_fair_level and k_fair_done beside
k_quota_loads, k_quota_clip and k_lease_sweep. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

GRANTS, REQUESTORS = 2_400, 16
E64, E32, Z1 = np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)
FAR = 1 << 40


class Leg:
    def __init__(self, sv, abi, rpc, how, hold, cap, pool):
        self.rpc, self.how, self.hold = rpc, how, hold
        self.n = GRANTS // 3 if rpc else GRANTS
        self.ctx = binding.Context(device=0, max_servants=1 << 20)
        self.ctx.upload_servants(abi)
        self.es = streaming.EventStream(sv, self.n, 0)
        hb = self.es.hb + 8
        max_leases = 1 << 16
        while max_leases < 2 * GRANTS * (hold + 1):
            max_leases <<= 1
        if rpc:
            self.ctx.stream_begin_rpc(hb, 16, self.n, 2 * GRANTS, 4096, max_leases, 16, 4096, 16, 16)
        else:
            self.ctx.stream_begin_waiting_leased(hb, 16, self.n, 4096, max_leases, 16, 4096, 16, 16)
        self.ctx.stream_inspect_begin()
        self.ctx.stream_quota_begin(4)
        if how == "static":
            self.ctx.stream_quota_set(cap)
        else:
            self.ctx.stream_quota_fair(binding.FAIR_REGISTRY if how == "registry" else binding.FAIR_FIXED, pool, 0)
        self.ips = (0x0A000000 + np.arange(self.n) % REQUESTORS).astype(np.uint32)
        self.imm = np.full(self.n, 2 if rpc else 1, np.uint32)
        self.pre = np.full(self.n, 1 if rpc else 0, np.uint32)
        self.next_id, self.n_leases, self.granted, self.tick_s, self.asked, self.got = 0, 0, [], [], 0, 0

    def tick(self, t, timed):
        who, rows, _, tk = self.es.next_tick()
        tk = dict(tk, requestor_ip=self.ips)
        free = self.granted.pop(0) if len(self.granted) >= self.hold else E64
        n = self.n
        tags = t * n + np.arange(n, dtype=np.uint64)
        lease_for, dl = np.full(n, FAR, np.int64), np.full(n, t, np.int64)
        t0 = time.perf_counter()
        if self.rpc:
            r = self.ctx.stream_tick_rpc(who, rows, E32, E64, I64, free, E32, Z1, E64, tk, self.imm, self.pre, lease_for, dl,
                                         tags, t)
            n_leases = r["n_leases"]
        else:
            r = self.ctx.stream_tick_waiting_leased(who, rows, E32, E64, I64, free, E32, Z1, E64, tk, lease_for, dl, tags, t)
            n_leases = r[4]
        dt = time.perf_counter() - t0
        got = n_leases - self.n_leases + len(free)  # (ids are handed out in sequence: the tick's are the next `got`)
        self.granted.append(np.arange(self.next_id, self.next_id + got, dtype=np.uint64))
        self.next_id, self.n_leases = self.next_id + got, n_leases
        if timed:
            self.tick_s.append(dt)
            self.asked += GRANTS
            self.got += got

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--hold", type=int, default=4)
    ap.add_argument("--modes", default="waiting_leased,rpc")
    ap.add_argument("--pool-scale", type=int, default=1)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    sv["max_tasks"] = (sv["max_tasks"].astype(np.uint64) * a.pool_scale).astype(sv["max_tasks"].dtype)
    sv["num_processors"] = (sv["num_processors"].astype(np.uint64) * a.pool_scale).astype(sv["num_processors"].dtype)
    abi = pack.to_abi_columns(sv)
    # A requestor asks for GRANTS / REQUESTORS a tick and holds them `hold` ticks: at nine tenths of that it is at its
    # cap; the same for all sixteen together is the fixed pool, and that over the registry's capacity the percent.
    cap = int(0.9 * a.hold * GRANTS / REQUESTORS)
    fixed = cap * REQUESTORS
    top = np.where((abi["flags"] & pack.SERVANT_LOW_MEMORY) | (abi["max_tasks"] == 0) |
                   (abi["current_load"] >= abi["num_processors"]), 0, np.minimum(abi["max_tasks"], abi["num_processors"]))
    percent = max(1, int(round(100.0 * fixed / max(int(top.sum()), 1))))
    warm = a.hold + 20
    for mode in a.modes.split(","):
        rpc = mode == "rpc"
        legs = {"a_quota_static": Leg(sv, abi, rpc, "static", a.hold, cap, 0),
                "b_fair_registry": Leg(sv, abi, rpc, "registry", a.hold, cap, percent),
                "c_fair_fixed": Leg(sv, abi, rpc, "fixed", a.hold, cap, fixed)}
        for t in range(a.ticks + warm):
            for leg in legs.values():
                leg.tick(t, t >= warm)
        out = {"mode": mode, "ticks": a.ticks, "hold": a.hold, "pool_scale": a.pool_scale, "grants_asked_per_tick": GRANTS, "requestors": REQUESTORS,
               "cap": cap, "fixed_pool": fixed, "percent": percent, "capacity_at_upload": int(top.sum())}
        for name, leg in legs.items():
            v = np.array(leg.tick_s) * 1e6
            out[name] = {"tick_us": round(float(np.median(v)), 1), "p10_us": round(float(np.percentile(v, 10)), 1),
                         "p90_us": round(float(np.percentile(v, 90)), 1), "leases": int(leg.n_leases),
                         "clipped_share": round(1 - leg.got / max(leg.asked, 1), 3)}
            if name != "a_quota_static":
                f = leg.ctx.stream_quota_fair_result()
                out[name].update(level=f["level"], pool=f["pool"], held_total=f["held_total"])
            leg.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the cap per requestor inside the tick (ydc_stream_quota_begin / _set), four legs alternating
tick by tick in one process, at the cfg5 registry, in waiting-and-leased and in rpc mode. Every tick
brings 2 400 grants' worth of requests from 16 requestors (2 400 requests, or 800 RPCs of 2 + 1 rows),
all of which the pool can take, and frees by id what the tick four ticks earlier was granted, so L holds
about 10 000 leases.
    python tests/tools/quota_cost.py --ticks 300
prints one JSON line per mode: median wall time per tick (host call to host return) of
  (a) the capability off,
  (b) on, every cap unlimited,
  (c) on, a cap that clips about a tenth of the rows,
  (d) the way without it to the same admission: streaming.admit (ydc_stream_requestor_find +
      ydc_admit_clip) and the tick with the kept rows, timed together,
and the share of the rows each leg's ticks clipped. Under `rocprofv3 --kernel-trace --stats -- python
tests/tools/quota_cost.py ...` the kernel table gives k_quota_claim, k_quota_loads, k_quota_clip and
k_quota_label beside the gather and the commit pass. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

GRANTS, REQUESTORS, HOLD, WARM = 2_400, 16, 4, 20
E64, E32, Z1 = np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)
FAR = 1 << 40


class Leg:
    def __init__(self, sv, abi, rpc, how, cap):
        self.rpc, self.how, self.cap = rpc, how, cap
        self.n = GRANTS // 3 if rpc else GRANTS
        self.ctx = binding.Context(device=0, max_servants=1 << 20)
        self.ctx.upload_servants(abi)
        self.es = streaming.EventStream(sv, self.n, 0)
        hb = self.es.hb + 8
        if rpc:
            self.ctx.stream_begin_rpc(hb, 16, self.n, 2 * GRANTS, 4096, 1 << 16, 16, 4096, 16, 16)
        else:
            self.ctx.stream_begin_waiting_leased(hb, 16, self.n, 4096, 1 << 16, 16, 4096, 16, 16)
        self.ctx.stream_inspect_begin()
        if how in ("unlimited", "clipping"):
            self.ctx.stream_quota_begin(4)
            if how == "clipping":
                self.ctx.stream_quota_set(cap)
        self.ips = (0x0A000000 + np.arange(self.n) % REQUESTORS).astype(np.uint32)
        self.imm = np.full(self.n, 2 if rpc else 1, np.uint32)
        self.pre = np.full(self.n, 1 if rpc else 0, np.uint32)
        self.next_id, self.n_leases, self.granted, self.tick_s, self.asked, self.got = 0, 0, [], [], 0, 0

    def tick(self, t):
        who, rows, _, tk = self.es.next_tick()
        tk = dict(tk, requestor_ip=self.ips)
        free = self.granted.pop(0) if len(self.granted) >= HOLD else E64
        imm, pre, keep = self.imm, self.pre, slice(None)
        t0 = time.perf_counter()
        if self.how == "at_the_door":
            imm, pre, keep = streaming.admit(self.ctx, tk, imm, pre if self.rpc else None, self.cap)
            tk = {k: v[keep] for k, v in tk.items()}
            imm, pre = imm[keep], pre[keep]
        n = len(imm)
        tags = t * self.n + np.arange(n, dtype=np.uint64)
        lease_for, dl = np.full(n, FAR, np.int64), np.full(n, t, np.int64)
        if self.rpc:
            r = self.ctx.stream_tick_rpc(who, rows, E32, E64, I64, free, E32, Z1, E64, tk, imm, pre, lease_for, dl, tags, t)
            n_leases = r["n_leases"]
        else:
            r = self.ctx.stream_tick_waiting_leased(who, rows, E32, E64, I64, free, E32, Z1, E64, tk, lease_for, dl, tags, t)
            n_leases = r[4]
        self.tick_s.append(time.perf_counter() - t0)
        got = n_leases - self.n_leases + len(free)  # (ids are handed out in sequence: the tick's are the next `got`)
        self.granted.append(np.arange(self.next_id, self.next_id + got, dtype=np.uint64))
        self.next_id, self.n_leases = self.next_id + got, n_leases
        if t >= WARM:
            self.asked += GRANTS
            self.got += got

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=300)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    # A requestor asks for GRANTS / REQUESTORS a tick and holds them HOLD ticks: at nine tenths of that it is at its cap.
    cap = int(0.9 * HOLD * GRANTS / REQUESTORS)
    for rpc in (False, True):
        legs = {"a_off": Leg(sv, abi, rpc, "off", 0), "b_on_unlimited": Leg(sv, abi, rpc, "unlimited", 0),
                "c_on_clipping": Leg(sv, abi, rpc, "clipping", cap), "d_find_clip_tick": Leg(sv, abi, rpc, "at_the_door", cap)}
        for t in range(a.ticks + WARM):
            for leg in legs.values():
                leg.tick(t)
        out = {"mode": "rpc" if rpc else "waiting_leased", "ticks": a.ticks, "grants_asked_per_tick": GRANTS,
               "requestors": REQUESTORS, "cap": cap}
        for name, leg in legs.items():
            v = np.array(leg.tick_s[WARM:]) * 1e6
            out[name] = {"tick_us": round(float(np.median(v)), 1), "p10_us": round(float(np.percentile(v, 10)), 1),
                         "p90_us": round(float(np.percentile(v, 90)), 1), "leases": int(leg.n_leases),
                         "clipped_share": round(1 - leg.got / max(leg.asked, 1), 3)}
            leg.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Cost of withdrawal by tag (ydc_stream_withdraw_begin / _stage) in a waiting + leased tick, four legs
alternating tick by tick in one process, at the cfg5 registry with one slot per servant: the pool is
saturated by the first tick, every tick brings 2500 requests that wait 4 ticks, so W holds about
10k entries (max_waiting 20k) and nothing is granted.
    python tests/tools/withdraw_cost.py --ticks 300
prints one JSON line: median wall time per tick (host call to host return; for the staging legs the
ydc_stream_withdraw_stage call apart) of
  (a) the capability off,
  (b) on, nothing staged,
  (c) on, 100 tags of W staged per tick,
  (d) on, max_withdraw = 4096 tags staged per tick, half of them in W,
and the median |W| each leg's ticks found. Under `rocprofv3 --kernel-trace --stats -- python
tests/tools/withdraw_cost.py ...` the kernel table gives k_withdraw_load, k_withdraw_mark and
k_withdraw_label beside k_wait_gather and k_wait_lease_commit. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, WAIT, MAX_WAITING, MAX_WITHDRAW, WARM = 2_500, 4, 20_000, 4096, 20
E64, E32, Z1 = np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)
FAR = 1 << 40


class Leg:
    def __init__(self, sv, abi, on, n_staged):
        self.ctx = binding.Context(device=0)
        self.ctx.upload_servants(abi)
        self.es = streaming.EventStream(sv, N, 0)
        self.ctx.stream_begin_waiting_leased(self.es.hb + 8, 16, N, MAX_WAITING, 1 << 16, 16, 16, 16, 16)
        if on:
            self.ctx.stream_withdraw_begin(MAX_WITHDRAW)
        self.n_staged, self.tick_s, self.stage_s, self.w, self.withdrawn = n_staged, [], [], [], 0

    def staged(self, t):
        """Tags of requests that queued two ticks ago (so none is staged twice); for the large list as
        many again that nobody has."""
        k = self.n_staged if self.n_staged <= 100 else self.n_staged // 2
        tags = (t - 2) * N + np.arange(k, dtype=np.uint64)
        if self.n_staged > 100:
            tags = np.concatenate([tags, (1 << 50) + np.arange(self.n_staged - k, dtype=np.uint64)])
        return tags[::-1].copy()  # (unsorted)

    def tick(self, t):
        who, rows, _, tk = self.es.next_tick()
        tags = t * N + np.arange(N, dtype=np.uint64)
        t0 = time.perf_counter()
        if self.n_staged and t >= 5:
            self.ctx.stream_withdraw_stage(self.staged(t))
        t1 = time.perf_counter()
        r = self.ctx.stream_tick_waiting_leased(who, rows, E32, E64, I64, E64, E32, Z1, E64, tk, np.full(N, FAR, np.int64),
                                                np.full(N, t + WAIT, np.int64), tags, t)
        t2 = time.perf_counter()
        self.tick_s.append(t2 - t1)
        self.stage_s.append(t1 - t0)
        self.w.append(r[8] + int(len(r[5])) - int((r[0] == binding.IDX_WAITING).sum()))  # |W| as the tick found it
        self.withdrawn += int((r[6] == binding.IDX_WITHDRAWN).sum())
        g = r[0][r[0] < binding.IDX_WAITING]
        self.es.commit(g)

    def close(self):
        self.ctx.stream_end()
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=300)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    sv["max_tasks"] = np.minimum(sv["max_tasks"], 1)
    abi = pack.to_abi_columns(sv)
    legs = {"off": Leg(sv, abi, False, 0), "on_nothing_staged": Leg(sv, abi, True, 0),
            "on_100_staged": Leg(sv, abi, True, 100), "on_4096_staged_half_present": Leg(sv, abi, True, MAX_WITHDRAW)}
    for t in range(a.ticks + WARM):
        for leg in legs.values():
            leg.tick(t)
    us = lambda v: round(float(np.median(v[WARM:])) * 1e6, 1)
    out = {"ticks": a.ticks, "requests_per_tick": N, "max_waiting": MAX_WAITING, "max_withdraw": MAX_WITHDRAW}
    for name, leg in legs.items():
        out[name] = {"tick_us": us(leg.tick_s), "stage_call_us": us(leg.stage_s), "w_median": int(np.median(leg.w[WARM:])),
                     "withdrawn_per_tick": round(leg.withdrawn / (a.ticks + WARM), 1)}
        leg.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Cost of ydc_stream_reserve, and the tick of a grown stream beside the tick of a stream begun at
the final size, at lease_tick_cost.py's shape: 2000 servants (cfg5), 10k requests, 10k frees by id,
200 heartbeats, 200 reports and 2k renewals per tick over about --leases ballast leases.
    python tests/tools/stream_reserve_cost.py --leases 100000 --ticks 300
Three leased streams in one process, one after another: two begun with max_leases = leases + 40k
(their difference is the spread a comparison has to beat), one begun with leases + 10k — just room
for the ballast ticks — and grown to leases + 40k by one timed ydc_stream_reserve once the ballast is
in. Prints one JSON line: the reserve's wall time, the table sizes it moved between, and the median
wall time per tick (host call to host return) of the three. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS = 10_000, 200, 2_000
E64, E32 = np.empty(0, np.uint64), np.empty(0, np.uint32)
FAR = 1 << 40


def slots(max_leases):
    return max(1024, 1 << int(np.ceil(np.log2(2 * max_leases))))


def leg(sv, abi, leases, ticks, begin_leases, final_leases):
    """One stream: ballast, the reserve if it was begun smaller, the measured ticks."""
    rng = np.random.default_rng(5)
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    ctx.stream_begin_leased(es.hb + 8, N, N, begin_leases, RENEWALS, N, HB_REPORTS, 1 << 16)
    held = 0
    while held < leases:  # ballast: leases nobody frees; their slots go back by servant index
        who, rows, _, tk = es.next_tick()
        n = min(N, leases - held)
        tk = {k: v[:n] for k, v in tk.items()}
        out, ids, _, _, held = ctx.stream_tick_leased(who, rows, E32, E64, E64.view(np.int64), E64, E32,
                                                      np.zeros(1, np.uint32), E64, tk, np.full(n, FAR, np.int64), 0)
        g = out[out < binding.IDX_ENV_NOT_FOUND]
        ctx.stream_tick_leased(E32, rows[:0], g, E64, E64.view(np.int64), E64, E32, np.zeros(1, np.uint32), E64,
                               {k: v[:0] for k, v in tk.items()}, E64.view(np.int64), 0)
    reserve_ms = None
    if begin_leases < final_leases:
        t0 = time.perf_counter()
        ctx.stream_reserve(max_leases=final_leases)
        reserve_ms = round((time.perf_counter() - t0) * 1e3, 3)
    live_ids, live_srv = E64, E32
    wall = []
    for t in range(ticks + 20):
        now = t + 1
        who, rows, _, tk = es.next_tick()
        ren = rng.integers(0, max(held, 1), RENEWALS).astype(np.uint64)  # ballast ids: live, never freed
        rs = ((t * HB_REPORTS + np.arange(HB_REPORTS)) % es.n).astype(np.uint32)
        order = np.argsort(live_srv, kind="stable")
        srt = live_srv[order]
        lo, hi = np.searchsorted(srt, rs), np.searchsorted(srt, rs, side="right")
        rid = np.concatenate([live_ids[order[l:h]] for l, h in zip(lo, hi)]) if len(order) else E64
        off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint32)
        lex = np.full(len(tk["env_id"]), now + 5, np.int64)
        t0 = time.perf_counter()
        out, ids, _, _, n_l = ctx.stream_tick_leased(who, rows, E32, ren, np.full(RENEWALS, FAR, np.int64), live_ids,
                                                     rs, off, rid, tk, lex, now)
        wall.append(time.perf_counter() - t0)
        g = out < binding.IDX_ENV_NOT_FOUND
        live_ids, live_srv = ids[g], out[g]
    ctx.stream_end()
    ctx.close()
    return round(float(np.median(wall[20:])) * 1e6, 1), reserve_ms, int(n_l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=20_000)
    ap.add_argument("--ticks", type=int, default=300)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    small, final = a.leases + N, a.leases + 4 * N
    begun_1, _, _ = leg(sv, abi, a.leases, a.ticks, final, final)
    grown, reserve_ms, n_l = leg(sv, abi, a.leases, a.ticks, small, final)
    begun_2, _, _ = leg(sv, abi, a.leases, a.ticks, final, final)
    print(json.dumps({"leases": a.leases, "leases_at_end": n_l, "ticks": a.ticks, "reserve_ms": reserve_ms,
                      "slots_before": slots(small), "slots_after": slots(final),
                      "begun_tick_us": [begun_1, begun_2], "grown_tick_us": grown}))


if __name__ == "__main__":
    main()

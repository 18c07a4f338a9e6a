"""Cost of the usage accounting (ydc_stream_usage_begin; stream_usage.h) in a leased streaming tick, at
lease_tick_cost.py's shape: 2000 servants, 10k requests, 10k frees by id, 200 heartbeats, 200 reports, 2k
renewals per tick, inspection on, about |L| ballast leases in the table. The same ticks are run twice in
one process: without the capability and with it (quantum 1, the clock advancing by one per tick, so every
tick accrues).
    python tests/tools/usage_cost.py --leases 1000000 --pattern hot --ticks 300
--pattern hot: one requestor owns 90 % of the requests (and so of L), the others are spread over 1000;
--pattern spread: 10^4 distinct requestors. Prints one JSON line: median wall time per tick (host call
to host return) of both runs, and the table's keys and slots at the end. Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/usage_cost.py ...` the kernel table gives
k_usage_accrue's own duration. Needs the GPU."""
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


def requestors(rng, n, pattern):
    if pattern == "hot":
        return np.where(rng.random(n) < 0.9, 0x0A000001, 0x0B000000 + rng.integers(0, 1000, n)).astype(np.uint32)
    return (0x0B000000 + rng.integers(0, 10_000, n)).astype(np.uint32)


def run(a, sv, abi, with_usage):
    rng = np.random.default_rng(5)
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    max_leases = a.leases + 4 * N
    ctx.stream_begin_leased(es.hb + 8, N, N, max_leases, RENEWALS, N, HB_REPORTS, 1 << 16)
    ctx.stream_inspect_begin()
    if with_usage:
        ctx.stream_usage_begin(1, 20_000)
    far = 1 << 40
    held = n_l = 0
    while held < a.leases:  # ballast: leases nobody frees; their slots go back by servant index
        who, rows, _, tk = es.next_tick()
        tk = dict(tk, requestor_ip=requestors(rng, len(tk["env_id"]), a.pattern))
        out, ids, _, _, n_l = ctx.stream_tick_leased(who, rows, E32, E64, E64.view(np.int64), E64, E32,
                                                     np.zeros(1, np.uint32), E64, tk, np.full(N, far, np.int64), 0)
        g = out[out < binding.IDX_ENV_NOT_FOUND]
        ctx.stream_tick_leased(E32, rows[:0], g, E64, E64.view(np.int64), E64, E32, np.zeros(1, np.uint32), E64,
                               {k: v[:0] for k, v in tk.items()}, E64.view(np.int64), 0)
        held = n_l
    live_ids, live_srv = E64, E32
    took = []
    for t in range(a.ticks + 20):
        now = t + 1
        who, rows, _, tk = es.next_tick()
        tk = dict(tk, requestor_ip=requestors(rng, len(tk["env_id"]), a.pattern))
        ren = rng.integers(0, max(held, 1), RENEWALS).astype(np.uint64)
        rs = ((t * HB_REPORTS + np.arange(HB_REPORTS)) % es.n).astype(np.uint32)
        order = np.argsort(live_srv, kind="stable")
        srt = live_srv[order]
        lo, hi = np.searchsorted(srt, rs), np.searchsorted(srt, rs, side="right")
        rid = np.concatenate([live_ids[order[l:h]] for l, h in zip(lo, hi)]) if len(order) else E64
        off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint32)
        lex = np.full(len(tk["env_id"]), now + 5, np.int64)
        t0 = time.perf_counter()
        out, ids, _, _, n_l = ctx.stream_tick_leased(who, rows, E32, ren, np.full(RENEWALS, far, np.int64), live_ids, rs,
                                                     off, rid, tk, lex, now)
        took.append(time.perf_counter() - t0)
        g = out < binding.IDX_ENV_NOT_FOUND
        live_ids, live_srv = ids[g], out[g]
    totals = ctx.stream_usage_get()[1] if with_usage else None
    ctx.stream_end()
    ctx.close()
    return round(float(np.median(took[20:])) * 1e6, 1), int(n_l), totals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=30_000)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--pattern", choices=("hot", "spread"), default="hot")
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    off_us, n_l, _ = run(a, sv, abi, False)
    on_us, _, totals = run(a, sv, abi, True)
    print(json.dumps({"leases": n_l, "pattern": a.pattern, "ticks": a.ticks, "tick_us": off_us, "tick_with_usage_us": on_us,
                      "usage": totals}))


if __name__ == "__main__":
    main()
